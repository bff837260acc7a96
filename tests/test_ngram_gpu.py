"""GPU: the n-gram LM step kernel (csrc/ngram.hip, asrk_ngram_step_f32) against its numpy float32 restatement
(tests/ngram_reference.py: emulate_f32) - log-probability rows and output states bit for bit.

The kernel has ONE variant (rows are written in place in global memory: no staging limit), with two fill paths: 16-byte
accesses when the row starts on a 16-byte boundary, 4-byte accesses otherwise - V = 64 with stride 64 takes the first
for every row, V = 37 / a stride of V + 3 mix both, V = 333 holds the context with 300 children (more than the
workgroup's 256 threads).  Shapes are the smallest at which it can go wrong; expected rows are computed once per
model and shared."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import ngram_cases as NC
import ngram_reference as NR
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda"
NG = NC.ngram_mod()
R_MAX = 257
PAD_BITS = 0x7FC12345                  # a NaN payload no computation produces: padding columns must keep it

_cache = {}


def _model(V, order):
    """(module on the device, image, states [257], tokens [257], expected states, expected rows) - once per model"""
    if (V, order) not in _cache:
        image = NG.build_image(order, NC.kernel_fixture(V, order), V)
        ctx = NR.image_contexts(image)
        states, tokens = NC.kernel_rows(image, ctx, R_MAX)
        want = [NR.emulate_f32(image, int(s), int(t)) for s, t in zip(states, tokens)]
        w_state = np.array([w[0] for w in want], np.int32)
        w_rows = np.stack([w[1] for w in want])
        depth = {len(ctx[int(s)]) for s in w_state}
        assert depth == set(range(order)), depth                       # a new state at every depth
        kids = np.diff(image["child_off"])
        if order > 1:
            assert (kids[1:] == 0).any() and (image["bo"] > 0).any()
            assert kids.max() == min(300, V - 8)
        assert (tokens == NC.NO_UNIGRAM[0]).any() and (w_rows[:, V - 1] < -200).all()
        _cache[(V, order)] = (NG.NGramLM(image).to(DEV), image, states, tokens, w_state, w_rows)
    return _cache[(V, order)]


def _step(lm, state_in, tokens, parent, ld):
    """the ABI entry with a row stride of its own; the output is pre-filled with PAD_BITS"""
    L = importlib.import_module(PKG_NAME + "._lib")
    ops = importlib.import_module(PKG_NAME + ".ops")
    R = len(tokens)
    out = torch.full((R, ld), PAD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    st = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    p = ops._p
    L.check(L.load().asrk_ngram_step_f32(
        lm.order, lm.vocab_size, lm.img_bo.numel(), lm.img_word.numel(), p(lm.img_uni_logp), p(lm.img_uni_next),
        p(lm.img_bo), p(lm.img_fail), p(lm.img_child_off), p(lm.img_word), p(lm.img_logp), p(lm.img_next),
        p(state_in), 0 if state_in is None else state_in.numel(), p(tokens), p(parent),
        int(parent is not None and parent.dtype == torch.int64), p(st), p(out), ld, R, ops._stream()), "ngram_step")
    return st.cpu().numpy(), out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("order", [1, 2, 4])
@pytest.mark.parametrize("V", [37, 64, 333])
def test_step_kernel_equals_emulate_f32_bit_for_bit(ops, V, order):
    lm, image, states, tokens, w_state, w_rows = _model(V, order)
    pool = np.unique(states)                                           # `repeats`: many rows share a pool entry
    where = np.searchsorted(pool, states)
    for R in (1, 33, R_MAX):
        tok = torch.from_numpy(tokens[:R]).to(DEV)
        own = torch.from_numpy(states[:R]).to(DEV)
        variants = {"absent": (own, None),
                    "identity": (own, torch.arange(R, dtype=torch.int64, device=DEV)),
                    "repeats": (torch.from_numpy(pool).to(DEV), torch.from_numpy(where[:R].astype(np.int32)).to(DEV))}
        for ld in (V, V + 3):
            for name, (st_in, parent) in variants.items():
                st, out = _step(lm, st_in, tok, parent, ld)
                tag = (V, order, R, ld, name)
                assert (st == w_state[:R]).all(), tag
                assert (_bits(out[:, :V]) == _bits(w_rows[:R])).all(), tag
                assert (_bits(out[:, V:]) == PAD_BITS).all(), tag       # padding columns untouched
    ops.check_errors()


def test_rows_of_a_large_launch_equal_the_same_rows_launched_alone(ops):
    lm, image, states, tokens, w_state, w_rows = _model(333, 4)
    tok = torch.from_numpy(tokens).to(DEV)
    own = torch.from_numpy(states).to(DEV)
    st_all, out_all = _step(lm, own, tok, None, 333)
    for r in (0, 1, 100, 255, 256):
        st, out = _step(lm, own[r:r + 1].clone(), tok[r:r + 1].clone(), None, 333 + 3)
        assert st[0] == st_all[r] and (_bits(out[0, :333]) == _bits(out_all[r])).all(), r
    rev = torch.arange(R_MAX - 1, -1, -1, dtype=torch.int32, device=DEV)    # the same rows at other positions
    st_rev, out_rev = _step(lm, own, tok.flip(0), rev, 333)
    assert (st_rev == st_all[::-1]).all() and (_bits(out_rev) == _bits(out_all[::-1])).all()
    ops.check_errors()


def test_module_forward_contract(ops):
    lm, image, states, tokens, w_state, w_rows = _model(37, 4)
    V, B = 37, 5
    assert lm.returns_logp and lm.vocab_size == V and lm.order == 4 and "4-gram" in lm.create_msg()[0]
    x = torch.tensor([[0], [9], [5], [36], [1]], dtype=torch.int64, device=DEV)
    logp, st = lm(x, torch.ones(B, dtype=torch.long), None)            # hidden=None: the empty context
    assert logp.shape == (B, 1, V) and logp.dtype == torch.float32 and logp.device.type == "cuda"
    assert st.shape == (1, B, 1) and st.dtype == torch.int32
    for b in range(B):
        ns, row = NR.emulate_f32(image, 0, int(x[b, 0]))
        assert int(st[0, b, 0]) == ns and (_bits(logp[b, 0].cpu().numpy()) == _bits(row)).all(), b
    assert int(st[0, 2, 0]) == 0 and int(st[0, 3, 0]) == 0             # tokens without a unigram: empty context
    # a second step from the carried state, through the decoders' own gather and through `parent`
    x2 = torch.tensor([[10], [10], [7], [9], [3]], dtype=torch.int64, device=DEV)
    parent = torch.tensor([1, 1, 0, 4, 2], dtype=torch.int64, device=DEV)
    a_logp, a_st = lm(x2, None, hidden=st.index_select(1, parent))
    b_logp, b_st = lm(x2, None, hidden=st, parent=parent)
    assert torch.equal(a_st, b_st) and torch.equal(a_logp.view(torch.int32), b_logp.view(torch.int32))
    for b in range(B):
        ns, row = NR.emulate_f32(image, int(st[0, int(parent[b]), 0]), int(x2[b, 0]))
        assert int(a_st[0, b, 0]) == ns and (_bits(a_logp[b, 0].cpu().numpy()) == _bits(row)).all(), b
    ops.check_errors()
