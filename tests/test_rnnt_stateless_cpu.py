"""CPU: the stateless prediction network of the transducer head - everything that needs no GPU.

 * the two float64 mirrors of the kernels (tests/rnnt_stateless_reference.py: plain loops, conv1d with autograd) agree to
   1e-12 on every kernel shape, on the exact and on the random inputs; the step mirror is a row of the sequence mirror;
   the inputs hold what they were seeded for (pre-activations that are exactly 0 and negative ones; under 1 % of the
   random pre-activations within 1e-5 of 0);
 * the head's configuration: every ValueError of `pred: {module: stateless, ...}`, the state_dict keys of a stateless
   head, the unchanged keys of an LSTM head, the parameter holder's init; check_exclusive and take_decode_block as before;
 * the argument errors of the four new entry points, before any HIP call;
 * the reference side of every search case of tests/test_rnnt_stateless_model_gpu.py, asserted here on float64 alone."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import ngram_reference as NR
import rnnt_beam_reference as BR
import rnnt_reference as RR
import rnnt_stateless_reference as SR
from conftest import PKG_NAME


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


# ---- the mirrors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SR.KERNEL_SHAPES)
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_the_two_mirrors_agree(shape, kind):
    X, w, dY = SR.exact_case(shape) if kind == "exact" else SR.random_case(shape)
    assert X.shape == shape[:3] and w.shape == (shape[2], 1, shape[3]) and X.dtype == np.float32
    Y1, (dX1, dw1) = SR.fwd_loops(X, w), SR.bwd_loops(X, w, dY)
    Y2, dX2, dw2 = SR.bwd_conv(X, w, dY)
    assert np.abs(Y1 - SR.fwd_conv(X, w)).max() <= 1e-12 and np.abs(Y1 - Y2).max() <= 1e-12
    assert np.abs(dX1 - dX2).max() <= 1e-12
    assert np.abs(dw1 - dw2).max() <= 1e-12 * max(1.0, np.abs(dw1).max())
    A = SR.pre_loops(X, w)
    if kind == "exact":
        # every value is on the grid, so f32 holds the float64 results exactly
        for a in (Y1, dX1, dw1):
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
        if A.size > 1:
            assert (A == 0).any() and (A < 0).any() and (A > 0).any(), shape
    else:
        assert SR.near_zero_mask(X, w).mean() < 0.01, shape


def test_exact_zero_has_derivative_zero_in_both_mirrors():
    """a channel with zero weights: pre-activation exactly 0 everywhere, no gradient to X through it, dw = 0"""
    X, w, dY = SR.exact_case((3, 7, 4, 2))
    w = w.copy()
    w[1] = 0
    dX1, dw1 = SR.bwd_loops(X, w, dY)
    _, dX2, dw2 = SR.bwd_conv(X, w, dY)
    for dX, dw in ((dX1, dw1), (dX2, dw2)):
        assert not dX[:, :, 1].any() and not dw[1].any() and dX[:, :, 0].any()


@pytest.mark.parametrize("C,Lc", [(1, 1), (2, 6), (3, 2), (8, 5), (8, 12)])
def test_step_mirror_is_a_row_of_the_sequence_mirror(C, Lc):
    tokens, n_tok, emb, w = SR.step_case(C, Lc)
    assert {int(v) for v in n_tok} == {min(max(v, 0), Lc) for v in (0, 1, C - 1, C, Lc)}
    for r in range(tokens.shape[0]):
        n = int(n_tok[r])
        seq = np.concatenate([[0], tokens[r, :n]])
        want = SR.fwd_loops(emb.astype(np.float64)[seq][None], w)[0, n]
        got = SR.step_loops(tokens[r], n, emb, w)
        assert np.abs(got - want).max() <= 1e-12
        # labels behind position n are never read
        other = tokens[r].copy()
        other[n:] = 10 ** 6
        assert np.array_equal(SR.step_loops(other, n, emb, w), got)
    bad = tokens[1].copy()
    n = int(n_tok[-1])                                 # Lc labels: every one of the last min(C, Lc) is read
    bad[n - 1] = emb.shape[0]
    assert np.isnan(SR.step_loops(bad, n, emb, w)).all()
    bad[n - 1] = -1
    assert np.isnan(SR.step_loops(bad, n, emb, w)).all()


@torch.no_grad()
def test_reference_head_stepwise_equals_the_sequence():
    """StatelessHeadRef.rnn, the one-label-at-a-time form the beam reference drives, equals `predict` on the sequence"""
    torch.manual_seed(1)
    for C in (1, 2, 4):
        ref = SR.StatelessHeadRef(7, 5, 6, C, 8)
        txt = torch.tensor([[3, 1, 6, 6, 2]])
        want = ref.predict(txt)[0]
        state, inp = None, [0] + txt[0].tolist()
        for u, y in enumerate(inp):
            out, state = ref.rnn(ref.emb(torch.tensor([[y]])), state)
            assert out.shape == (1, 1, 6) and state.shape[0] == min(u + 1, C - 1)
            assert float((out[0, 0] - want[u]).abs().max()) <= 1e-12
        assert float((want - torch.as_tensor(SR.fwd_loops(ref.emb(torch.tensor([inp])).detach().numpy(),
                                                          ref.conv.weight.detach().numpy()))[0]).abs().max()) <= 1e-12


# ---- configuration -----------------------------------------------------------------------------------------------------------
def _head(pred, prune=None, V=7, enc_dim=5, joint=8):
    return _mod("src.transducer").TransducerHead(V, enc_dim, pred, joint, prune=prune)


def test_pred_block_validation():
    tr = _mod("src.transducer")
    assert "context" in tr.PRED_KEYS
    h = _head(dict(module="stateless", dim=6))
    assert h.context == 2 and h.stateless and h.dim == h.emb_dim == 6 and h.layer == 1
    h = _head(dict(module="Stateless", dim=6, context=8, emb_dim=6, layer=1, dropout=0.1))
    assert h.context == 8 and tuple(h.ctx.weight.shape) == (6, 1, 8)
    assert _head(dict(module="stateless", dim=6, context=1.0)).context == 1
    for bad in (dict(context=0), dict(context=9), dict(context=2.5), dict(context=True), dict(context="2"),
                dict(context=float("nan")), dict(context=-1), dict(emb_dim=5), dict(layer=2), dict(layer=0),
                dict(contexts=2), dict(kernel=3)):
        with pytest.raises(ValueError):
            _head(dict(dict(module="stateless", dim=6), **bad))
    # `context` belongs to the stateless predictor alone
    for module in ("LSTM", "GRU"):
        with pytest.raises(ValueError, match="unknown pred keys"):
            _head(dict(module=module, dim=6, layer=1, emb_dim=4, context=2))
    with pytest.raises(ValueError, match="unknown pred keys"):
        _head(dict(dim=6, context=2))                                     # the default module is LSTM
    with pytest.raises(NotImplementedError):
        _head(dict(module="transformer", dim=6))
    assert "stateless" in h.create_msg() and "context 8" in h.create_msg()


def test_state_dict_keys():
    lin = ["lin_enc.weight", "lin_enc.bias", "lin_pred.weight", "lin_pred.bias", "lin_out.weight", "lin_out.bias"]
    h = _head(dict(module="stateless", dim=6, context=3))
    assert sorted(h.state_dict()) == sorted(["emb.weight", "ctx.weight"] + lin)
    assert not any(k.startswith("pred.") for k in h.state_dict()) and not hasattr(h, "pred")
    assert tuple(h.emb.weight.shape) == (7, 6) and tuple(h.ctx.weight.shape) == (6, 1, 3)
    hp = _head(dict(module="stateless", dim=6, context=3), prune={'range': 3, 'simple_weight': 0.5})
    assert sorted(hp.state_dict()) == sorted(["emb.weight", "ctx.weight"] + lin + [
        "lin_am.weight", "lin_am.bias", "lin_lm.weight", "lin_lm.bias"])
    assert tuple(hp.lin_lm.weight.shape) == (7, 6)
    # an LSTM / GRU head: the keys it always had
    rnn = ["pred.%s_l%d" % (k, l) for l in range(2) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    for module in ("LSTM", "GRU"):
        h = _head(dict(module=module, dim=6, layer=2, emb_dim=4, dropout=0))
        assert sorted(h.state_dict()) == sorted(["emb.weight"] + rnn + lin)
        assert not hasattr(h, "ctx") and not h.stateless


def test_context_weight_init_is_conv1d_s():
    """the same point of the random stream gives nn.Conv1d's values: the mirror module is a drop-in"""
    tr = _mod("src.transducer")
    torch.manual_seed(11)
    mine = tr.ContextParams(6, 3).weight.detach().clone()
    torch.manual_seed(11)
    conv = torch.nn.Conv1d(6, 6, 3, groups=6, bias=False)
    assert torch.equal(mine, conv.weight.detach()) and float(mine.abs().max()) <= 1 / 3 ** 0.5
    ref = SR.StatelessHeadRef.of(_head(dict(module="stateless", dim=6, context=3)), 5)     # load: strict, complete
    assert set(ref.param_map()) == set(_head(dict(module="stateless", dim=6, context=3)).state_dict())


def test_blocks_outside_pred_behave_as_before():
    tr = _mod("src.transducer")
    head = {'enable': True, 'pred': {'module': 'stateless', 'dim': 6, 'context': 2}}
    tr.check_exclusive({'model': {'transducer': head}})
    tr.check_exclusive({'model': {'transducer': dict(head, enable=False)}, 'mwer': {'enable': True}})
    with pytest.raises(ValueError, match="mwer"):
        tr.check_exclusive({'model': {'transducer': head}, 'mwer': {'enable': True}})
    with pytest.raises(ValueError, match="emb"):
        tr.check_exclusive({'model': {'transducer': head}, 'emb': {'enable': True}})
    d = {'beam_size': 7, 'transducer': {'enable': True, 'max_symbols': 2, 'max_len_ratio': 0.25, 'beam_size': 4, 'nbest': 3}}
    assert tr.take_decode_block(d) == {'max_symbols': 2, 'max_len_ratio': 0.25, 'beam_size': 4, 'nbest': 3}
    assert d == {'beam_size': 7}
    with pytest.raises(ValueError, match="unknown"):
        tr.take_decode_block({'transducer': {'enable': True, 'context': 2}})
    assert tr.take_decode_block({'transducer': {'enable': False, 'beam_size': 99}}) is None
    # RNN-LM fusion stays refused for the stateless head as for the others
    h = _head(dict(module="stateless", dim=4), V=5, enc_dim=4, joint=4)
    with pytest.raises(NotImplementedError, match="NGramLM"):
        h.beam_search(torch.zeros((1, 2, 4)), torch.tensor([2]), 2, 2, 3, lm=torch.nn.Linear(2, 2), lm_weight=0.3)


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_without_gpu():
    """null pointers and impossible sizes are ASRK_EINVAL (-1) / ASRK_ESHAPE (-2) before any HIP call; a missing or short
    workspace is ASRK_EWORKSPACE (-3); B == 0 / R == 0 is ASRK_OK"""
    _mod("build").build(verbose=False)
    L = _mod("_lib").load()
    z, f = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    # forward: X, ldx, w, B, U1, D, C, Y, ldy
    fs = [f, 8, f, 2, 3, 8, 2, f, 8, z]
    for pos, bad in ((0, z), (2, z), (7, z), (1, 7), (8, 7), (3, -1), (4, 0), (5, 0)):
        a = list(fs)
        a[pos] = bad
        assert L.asrk_rnnt_ctx_fwd_f32(*a) == -1, pos
    for bad in (0, 9, -1):
        a = list(fs)
        a[6] = bad
        assert L.asrk_rnnt_ctx_fwd_f32(*a) == -2, bad
    assert L.asrk_rnnt_ctx_fwd_f32(f, 8, f, 2 ** 30, 4, 8, 2, f, 8, z) == -2
    assert L.asrk_rnnt_ctx_fwd_f32(z, 8, z, 0, 3, 8, 2, z, 8, z) == 0
    # workspace size: one [C, D] partial sum per 32 rows of [B*U1]
    ws = L.asrk_rnnt_ctx_bwd_ws_bytes
    assert ws(2, 3, 8, 2) == 1 * 2 * 8 * 4 and ws(4, 65, 512, 2) == 9 * 2 * 512 * 4 and ws(1, 33, 5, 8) == 2 * 8 * 5 * 4
    assert ws(0, 3, 8, 2) == 0 and ws(2, 3, 8, 9) == 0 and ws(2, 3, 8, 0) == 0
    # backward: X, w, Y, dY, B, U1, D, C, dX, dw, ws, ws_bytes
    need = ws(2, 3, 8, 2)
    bs = [f, f, f, f, 2, 3, 8, 2, f, f, f, need, z]
    for pos, bad in ((0, z), (1, z), (2, z), (3, z), (8, z), (9, z), (4, -1), (5, 0), (6, 0)):
        a = list(bs)
        a[pos] = bad
        assert L.asrk_rnnt_ctx_bwd_f32(*a) == -1, pos
    for bad in (0, 9):
        a = list(bs)
        a[7] = bad
        assert L.asrk_rnnt_ctx_bwd_f32(*a) == -2, bad
    for pos, bad in ((10, z), (11, need - 1), (11, 0), (10, ctypes.c_void_p(4098))):
        a = list(bs)
        a[pos] = bad
        assert L.asrk_rnnt_ctx_bwd_f32(*a) == -3, (pos, bad)
    a = list(bs)
    a[4] = 0
    assert L.asrk_rnnt_ctx_bwd_f32(*a) == 0
    # step: tokens, tok_bytes, ldt, n_tok, R, Lc, emb, V, D, w, C, Y, ldy
    ss = [f, 4, 6, f, 5, 6, f, 11, 8, f, 2, f, 8, z]
    for pos, bad in ((0, z), (3, z), (6, z), (9, z), (11, z), (2, 5), (12, 7), (4, -1), (5, 0), (7, 0), (8, 0)):
        a = list(ss)
        a[pos] = bad
        assert L.asrk_rnnt_ctx_step_f32(*a) == -1, pos
    for pos, bad in ((1, 2), (1, 0), (1, 16), (10, 0), (10, 9)):
        a = list(ss)
        a[pos] = bad
        assert L.asrk_rnnt_ctx_step_f32(*a) == -2, (pos, bad)
    a = list(ss)
    a[0], a[3], a[4] = z, z, 0
    assert L.asrk_rnnt_ctx_step_f32(*a) == 0
    a = list(ss)
    a[1] = 8
    a[4] = 0
    assert L.asrk_rnnt_ctx_step_f32(*a) == 0


def test_ops_refuse_host_tensors_and_bad_shapes():
    """host tensors are refused whether or not a GPU is present: there is no eager fall-back"""
    ops = _mod("ops")
    with pytest.raises(RuntimeError):
        ops.RNNTContextFn.apply(torch.zeros(2, 3, 4), torch.zeros(4, 1, 2))
    with pytest.raises(RuntimeError):
        ops.rnnt_ctx_step(torch.zeros((2, 3), dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(5, 4),
                          torch.zeros(4, 1, 2))


# ---- the reference side of the search cases ----------------------------------------------------------------------------------
@pytest.mark.parametrize("context,seed,bias", SR.GREEDY_CASES)
def test_greedy_cases_meet_the_reference_conditions(context, seed, bias):
    """margins >= MIN_MARGIN, blanks and labels, the max_symbols cap, rows finishing at different iterations
    (rnnt_reference.check_greedy_case), and the margins of the max_symbols = 1, max_len = 2 run"""
    tr = _mod("src.transducer")
    head, enc, lens = SR.head_case(tr.TransducerHead, context, seed, bias)
    ref = SR.StatelessHeadRef.of(head, RR.GREEDY_ENC_DIM)
    want = RR.check_greedy_case(ref, enc, lens)
    assert any(want)
    for b in range(3):
        e = enc[b, :int(lens[b])].double()
        tokens, trace = ref.greedy(e, 1, 2)
        assert min(t[2] for t in trace) >= RR.MIN_MARGIN and len(tokens) <= 2
        # one slot of the beam reference is the greedy loop
        for ms, ml, toks in ((RR.GREEDY_MAX_SYMBOLS, RR.GREEDY_MAX_LEN, want[b]), (1, 2, tokens)):
            fin, _ = BR.beam_search(ref, e, 1, ms, ml)
            assert len(fin) == 1 and list(fin[0][0]) == toks


@pytest.mark.parametrize("context,seed,bias", SR.BEAM_CASES)
def test_beam_cases_meet_the_reference_conditions(context, seed, bias):
    """per setting: rnnt_beam_reference.min_margin >= 1e-3 and at least one merge of equal label sequences; the corner
    shapes of the GPU test (enc_len = 1, max_len = 0) have their margins too"""
    tr, ng = _mod("src.transducer"), _mod("src.ngram")
    head, enc, lens = SR.head_case(tr.TransducerHead, context, seed, bias)
    ref = SR.StatelessHeadRef.of(head, RR.GREEDY_ENC_DIM)
    _, lm_row = BR.planted_lm_model(ng, NR, RR.GREEDY_V, seed)
    ms, ml = RR.GREEDY_MAX_SYMBOLS, RR.GREEDY_MAX_LEN
    best = {}
    for W in BR.BEAM_WIDTHS:
        for with_lm in (False, True):
            runs = BR.run_case(ref, enc, lens, W, ms, ml, lm_row if with_lm else None,
                               BR.BEAM_LM_WEIGHT if with_lm else 0.0)
            facts = SR.check_beam_case(runs)
            assert facts["capped"], "the max_symbols cap never binds"
            best[(W, with_lm)] = facts["best"]
    assert any(best[(W, True)] != best[(W, False)] for W in BR.BEAM_WIDTHS), "the LM changes no 1-best"
    for args in ((enc[:1, :1].contiguous(), torch.tensor([1]), 4, ms, ml), (enc, lens, 4, ms, 0)):
        runs = BR.run_case(ref, *args)
        assert min(BR.min_margin(t) for _, t in runs) >= BR.MIN_MARGIN
