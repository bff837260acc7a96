"""GPU: the contextual-biasing kernels (csrc/ctx_bias.hip) against their numpy float32 restatement
(tests/bias_reference.py) - rows, states, totals and residuals bit for bit.

asrk_bias_step_f32 and asrk_ngram_bias_step_f32 have ONE variant each (rows are written in place: no staging limit)
with two fill paths: 16-byte accesses when the row and the tables start on a 16-byte boundary, 4-byte accesses
otherwise - V = 64 with stride 64 takes the first for every row, V = 37 / a stride of V + 3 mix both, V = 333 holds
the node with 300 merged entries (more than the workgroup's 256 lanes); R = 257 leaves the last workgroup alone.
The fused entry is compared against the n-gram's own restatement (ngram_reference.emulate_f32) plus one float32 add.
Expected rows are computed once per model and shared."""
import importlib

import numpy as np
import pytest
import torch

import bias_cases as BC
import bias_reference as BR
import ngram_cases as NC
import ngram_reference as NR
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda"
CB = BC.bias_mod()
NG = NC.ngram_mod()
R_MAX = 257
PAD_BITS = 0x7FC12345                  # a NaN payload no computation produces: padding columns must keep it
LM_W = 0.3                             # the fused scorer's image holds every bonus divided by it

_cache = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _model(V):
    """bias alone: (module, image, states [257], tokens [257], expected states, expected rows) - once per V"""
    if V not in _cache:
        image = CB.build_image(BC.kernel_phrases(V), V, BC.KERNEL_WEIGHT)
        paths = BR.image_nodes(image)
        states, tokens = BC.kernel_rows(image, paths, R_MAX)
        want = [BR.emulate_step(image, int(s), int(t)) for s, t in zip(states, tokens)]
        w_state = np.array([w[0] for w in want], np.int32)
        w_rows = np.stack([w[1] for w in want])
        assert {len(paths[int(s)]) for s in w_state} == set(range(13))        # a new state at every depth 0 .. 12
        assert np.diff(image["ext_off"]).max() == min(300, V - 8)
        assert ((tokens < 0) | (tokens >= V)).sum() >= 5
        _cache[V] = (CB.ContextBias(image).to(DEV), image, states, tokens, w_state, w_rows)
    return _cache[V]


def _fused_model(V, order):
    """n-gram + bias: (module, states [257, 2], tokens, expected states [257, 2], expected rows)"""
    key = (V, order)
    if key not in _cache:
        cb, b_img, b_states, tokens, _, _ = _model(V)
        g_img = NG.build_image(order, NC.kernel_fixture(V, order), V)
        g_states, g_tokens = NC.kernel_rows(g_img, NR.image_contexts(g_img), R_MAX)
        tokens = tokens.copy()
        tokens[1::2] = g_tokens[1::2]                                          # half the rows move the n-gram's way
        s_img = CB.build_image(BC.kernel_phrases(V), V, BC.KERNEL_WEIGHT, 1.0 / LM_W)
        want = [BR.emulate_fused(NR, g_img, s_img, sn, sb, t) for sn, sb, t in zip(g_states, b_states, tokens)]
        w_state = np.array([w[0] for w in want], np.int32)
        w_rows = np.stack([w[1] for w in want])
        # rows in which an n-gram entry and a bias entry meet on one word, and rows in which they do not
        both = CB.BiasedNGram.pair(NG.NGramLM(g_img), CB.ContextBias(b_img), LM_W).to(DEV)
        assert np.array_equal(both.bias.image()["phi"], s_img["phi"])
        states = np.stack([g_states, b_states], 1).astype(np.int32)
        _cache[key] = (both, states, tokens, w_state, w_rows)
    return _cache[key]


def _step(mod, state_in, tokens, parent, ld, shift=0):
    """the ABI entries with a row stride of their own; the output is pre-filled with PAD_BITS.  shift: floats by which
    the output's base is moved off its 16-byte boundary"""
    L = importlib.import_module(PKG_NAME + "._lib")
    ops = importlib.import_module(PKG_NAME + ".ops")
    fused = isinstance(mod, CB.BiasedNGram)
    width = 2 if fused else 1
    R = len(tokens)
    buf = torch.full((R * ld + 4,), PAD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    out = buf[shift:shift + R * ld].view(R, ld)
    st = torch.full((R, width), -7, dtype=torch.int32, device=DEV)
    p = ops._p
    n_state = 0 if state_in is None else state_in.numel() // width
    tail = (p(state_in), n_state, p(tokens), p(parent), int(parent is not None and parent.dtype == torch.int64), p(st),
            p(out), ld, R, ops._stream())
    if fused:
        g = mod.ngram
        L.check(L.load().asrk_ngram_bias_step_f32(
            g.order, g.vocab_size, g.img_bo.numel(), g.img_word.numel(), p(g.img_uni_logp), p(g.img_uni_next),
            p(g.img_bo), p(g.img_fail), p(g.img_child_off), p(g.img_word), p(g.img_logp), p(g.img_next),
            *mod.bias._tables(), *tail), "ngram_bias_step")
    else:
        L.check(L.load().asrk_bias_step_f32(mod.vocab_size, *mod._tables(), *tail), "bias_step")
    pad = torch.cat([buf[:shift], buf[shift + R * ld:]]).cpu().numpy()
    assert (_bits(pad) == PAD_BITS).all()
    return st.cpu().numpy().reshape(R, width), out.cpu().numpy()


def _variants(states, tokens, R):
    """state_in / parent forms that must all give the same rows: own states, an int64 identity, an int32 gather from
    the pool of distinct states"""
    tok = torch.from_numpy(tokens[:R]).to(DEV)
    own = torch.from_numpy(np.ascontiguousarray(states[:R])).to(DEV)
    pool, where = np.unique(states.reshape(len(states), -1), axis=0, return_inverse=True)
    where = where.reshape(-1)
    return tok, {"absent": (own, None),
                 "identity": (own, torch.arange(R, dtype=torch.int64, device=DEV)),
                 "repeats": (torch.from_numpy(np.ascontiguousarray(pool)).to(DEV),
                             torch.from_numpy(where[:R].astype(np.int32)).to(DEV))}


@pytest.mark.parametrize("V", [37, 64, 333])
def test_bias_step_equals_the_restatement_bit_for_bit(ops, V):
    cb, image, states, tokens, w_state, w_rows = _model(V)
    for R in (1, 33, R_MAX):
        tok, variants = _variants(states, tokens, R)
        for ld, shift in ((V, 0), (V + 3, 0), (V + 3, 1)):
            for name, (st_in, parent) in variants.items():
                st, out = _step(cb, st_in, tok, parent, ld, shift)
                tag = (V, R, ld, shift, name)
                assert (st[:, 0] == w_state[:R]).all(), tag
                assert (_bits(out[:, :V]) == _bits(w_rows[:R])).all(), tag
                assert (_bits(out[:, V:]) == PAD_BITS).all(), tag               # padding columns untouched
    ops.check_errors()


@pytest.mark.parametrize("order", [1, 4])
@pytest.mark.parametrize("V", [37, 64, 333])
def test_fused_step_equals_ngram_row_plus_one_add_bit_for_bit(ops, V, order):
    both, states, tokens, w_state, w_rows = _fused_model(V, order)
    for R in (1, R_MAX):
        tok, variants = _variants(states, tokens, R)
        for ld, shift in ((V, 0), (V + 3, 0), (V + 3, 1)):
            for name, (st_in, parent) in variants.items():
                st, out = _step(both, st_in, tok, parent, ld, shift)
                tag = (V, order, R, ld, shift, name)
                assert (st == w_state[:R]).all(), tag
                assert (_bits(out[:, :V]) == _bits(w_rows[:R])).all(), tag
                assert (_bits(out[:, V:]) == PAD_BITS).all(), tag
    ops.check_errors()


def test_fused_rows_hold_words_both_automata_overwrite(ops):
    """the fixture reaches what the fused kernel's last pass is for: a word with an n-gram entry above the unigram
    level AND a bias entry in one row, and its value is L(w) + delta, not the fill's"""
    both, states, tokens, w_state, w_rows = _fused_model(333, 4)
    g, b = both.ngram.image(), both.bias.image()
    met = 0
    for sn, sb in w_state:
        if sn == 0 or sb == 0:
            continue
        gw = set(g["word"][g["child_off"][sn]:g["child_off"][sn + 1]].tolist())
        bw = set(b["ext_word"][b["ext_off"][sb]:b["ext_off"][sb + 1]].tolist())
        met += len(gw & bw) > 0
    assert met >= 1


def test_parents_out_of_range_and_absent_state_mean_the_root(ops):
    for mod, states, tokens, width in ((_model(37)[0], _model(37)[2].reshape(-1, 1), _model(37)[3], 1),
                                       (_fused_model(37, 4)[0],) + _fused_model(37, 4)[1:3] + (2,)):
        R = 33
        tok = torch.from_numpy(tokens[:R]).to(DEV)
        st0, out0 = _step(mod, None, tok, None, 37)                             # state_in = None: every row at the root
        zeros = torch.zeros((R, width), dtype=torch.int32, device=DEV)
        st1, out1 = _step(mod, zeros, tok, None, 37)
        assert (st0 == st1).all() and (_bits(out0) == _bits(out1)).all()
        own = torch.from_numpy(np.ascontiguousarray(states[:R])).to(DEV)
        for dtype, bad in ((torch.int32, [-1, R, 2 ** 31 - 1, -2 ** 31]), (torch.int64, [-1, R, 2 ** 40, -2 ** 40])):
            parent = torch.arange(R, dtype=dtype, device=DEV)
            rows = [3, 8, 20, 32]
            parent[rows] = torch.tensor(bad, dtype=dtype, device=DEV)
            st, out = _step(mod, own, tok, parent, 37)
            ref_st, ref_out = _step(mod, own, tok, None, 37)
            keep = np.ones(R, bool)
            keep[rows] = False
            assert (st[keep] == ref_st[keep]).all() and (_bits(out[keep]) == _bits(ref_out[keep])).all()
            assert (st[rows] == st0[rows]).all() and (_bits(out[rows]) == _bits(out0[rows])).all()
    ops.check_errors()


def test_rows_of_a_large_launch_equal_the_same_rows_launched_alone_and_two_runs_agree(ops):
    for mod, states, tokens in ((_model(333)[0], _model(333)[2].reshape(-1, 1), _model(333)[3]),
                                _fused_model(333, 4)[:3]):
        tok = torch.from_numpy(tokens).to(DEV)
        own = torch.from_numpy(np.ascontiguousarray(states)).to(DEV)
        st_all, out_all = _step(mod, own, tok, None, 333)
        st_again, out_again = _step(mod, own, tok, None, 333)
        assert (st_all == st_again).all() and (_bits(out_all) == _bits(out_again)).all()
        for r in (0, 1, 100, 255, 256):
            st, out = _step(mod, own[r:r + 1].clone(), tok[r:r + 1].clone(), None, 333 + 3)
            assert (st[0] == st_all[r]).all() and (_bits(out[0, :333]) == _bits(out_all[r])).all(), r
        rev = torch.arange(R_MAX - 1, -1, -1, dtype=torch.int32, device=DEV)    # the same rows at other positions
        st_rev, out_rev = _step(mod, own, tok.flip(0), rev, 333)
        assert (st_rev == st_all[::-1]).all() and (_bits(out_rev) == _bits(out_all[::-1])).all()
    ops.check_errors()


def test_walk_equals_the_sum_of_the_step_kernels_own_deltas(ops):
    V = 64
    cb, image, *_ = _model(V)
    tok_h, n_h = BC.walk_sequences(V)
    assert {0, 1, 40} <= set(n_h.tolist())
    H, L = tok_h.shape
    tok = torch.from_numpy(tok_h).to(DEV)
    state, total, residual = cb.walk(tok, torch.from_numpy(n_h).to(DEV))
    again = cb.walk(tok, torch.from_numpy(n_h.astype(np.int64)).to(DEV))        # n_tok of another integer type
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((state, total, residual), again))
    state, total, residual = state.cpu().numpy(), total.cpu().numpy(), residual.cpu().numpy()
    # the numpy restatement
    for h in range(H):
        s, tot, res = BR.emulate_walk(image, tok_h[h, :n_h[h]])
        assert state[h] == s and _bits(total[h]) == _bits(tot) and _bits(residual[h]) == _bits(res), h
    # the step kernel's own rows along the same sequences: the row written when token i was consumed holds the delta
    # of token i + 1; a step from no state on a token outside [0, V) leaves the root's row.  Sequences that hold a token
    # outside [0, V) are compared with the restatement only (no row has a column for such a token).
    clean = np.array([((tok_h[h, :n_h[h]] >= 0) & (tok_h[h, :n_h[h]] < V)).all() for h in range(H)])
    assert clean.sum() >= H - 1 and not clean.all()
    acc = np.zeros(H, np.float32)
    rows, st = cb(torch.full((H, 1), -1, dtype=torch.int64, device=DEV), None, None)
    assert int(st.abs().max()) == 0
    for i in range(L):
        rows_h = rows[:, 0].cpu().numpy()
        delta = rows_h[np.arange(H), np.clip(tok_h[:, i], 0, V - 1)]
        acc = np.where(i < n_h, (acc + delta).astype(np.float32), acc)
        rows, st = cb(tok[:, i:i + 1], None, hidden=st)
    assert (_bits(acc[clean]) == _bits(total[clean])).all()
    ops.check_errors()


def test_module_forward_contract(ops):
    cb, image, *_ = _model(37)
    V, B = 37, 5
    x = torch.tensor([[0], [10], [3], [35], [1]], dtype=torch.int64, device=DEV)
    delta, st = cb(x, torch.ones(B, dtype=torch.long), None)
    assert delta.shape == (B, 1, V) and delta.dtype == torch.float32 and st.shape == (1, B, 1) and st.dtype == torch.int32
    x2 = torch.tensor([[11], [11], [4], [3], [3]], dtype=torch.int64, device=DEV)
    parent = torch.tensor([1, 1, 2, 4, 2], dtype=torch.int64, device=DEV)
    a_d, a_st = cb(x2, None, hidden=st.index_select(1, parent))
    out = torch.empty(B * V, dtype=torch.float32, device=DEV)
    st_out = torch.empty(B, dtype=torch.int32, device=DEV)
    b_d, b_st = cb(x2, None, hidden=st, parent=parent, out=out, state_out=st_out)
    assert b_d.data_ptr() == out.data_ptr() and b_st.data_ptr() == st_out.data_ptr()
    assert torch.equal(a_st, b_st) and torch.equal(a_d.view(torch.int32), b_d.view(torch.int32))
    for b in range(B):
        ns, row = BR.emulate_step(image, int(st[0, int(parent[b]), 0]), int(x2[b, 0]))
        assert int(a_st[0, b, 0]) == ns and (_bits(a_d[b, 0].cpu().numpy()) == _bits(row)).all(), b
    both = _fused_model(37, 4)[0]
    d2, st2 = both(x, None, None)
    assert d2.shape == (B, 1, V) and st2.shape == (1, B, 2) and st2.dtype == torch.int32
    c_d, c_st = both(x2, None, hidden=st2.index_select(1, parent))
    e_d, e_st = both(x2, None, hidden=st2, parent=parent)
    assert torch.equal(c_st, e_st) and torch.equal(c_d.view(torch.int32), e_d.view(torch.int32))
    ops.check_errors()
