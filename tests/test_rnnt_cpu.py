"""CPU: the RNN-transducer head without a GPU.

 * the float64 reference (tests/rnnt_reference.py) is self-consistent: alpha-side and beta-side ln P agree and the
   closed-form gradient equals autograd, both to 1e-12;
 * csrc/rnnt.inc built for the host (tests/native/rnnt_host.cpp) against the reference on the lattice shapes of the GPU
   test, with one lane per direction and with the kernel's 128;
 * config handling: no block / enable: false add no parameter and a reference state_dict loads strict; the mwer / emb
   conflicts; the decode block is taken out of `decode:`;
 * the ABI's argument checks return before any HIP call.

The host build can be run once as a stand-alone sanitizer program: g++ -fsanitize=address,undefined -DRNNT_HOST_MAIN
tests/native/rnnt_host.cpp."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import rnnt_reference as RR
from conftest import PKG_NAME
from helpers import CASES, load_golden, golden_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = [(1, 0), (1, 1), (1, 5), (5, 0), (2, 1), (7, 3), (3, 7)]
LATTICES = SMALL + [(64, 63), (65, 64), (9, 300)]


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,U", SMALL)
def test_reference_is_self_consistent(T, U):
    g = torch.Generator().manual_seed(100 * T + U)
    V = 5
    z = (torch.randn((T, U + 1, V), generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    y = torch.randint(1, V, (U,), generator=g)
    if U >= 2:
        y[1] = y[0]                                    # a repeated label
    lp = RR.log_probs(z)
    la, lb = RR.alpha_lnp(lp, y), RR.beta_lnp(lp, y)
    assert abs(float(la.detach()) - float(lb.detach())) <= 1e-12
    (-la).backward()
    cf = RR.closed_form(z.detach(), y)
    assert float((cf - z.grad).abs().max()) <= 1e-12
    # the gradient of a log-softmax output sums to zero over v
    assert float(cf.sum(-1).abs().max()) <= 1e-12


def test_reference_batch_pads_with_zeros():
    g = torch.Generator().manual_seed(1)
    z = torch.randn((2, 4, 3, 6), generator=g, dtype=torch.float64)
    txt = torch.tensor([[2, 2], [3, 0]])
    nll, grad = RR.batch_nll_grad(z, txt, [4, 2], [2, 0])
    nll2, grad2 = RR.batch_nll_grad(z, txt, [4, 2], [2, 0], use_autograd=False)
    assert float((nll - nll2).abs().max()) <= 1e-12 and float((grad - grad2).abs().max()) <= 1e-12
    assert bool((grad[1, 2:] == 0).all()) and bool((grad[1, :, 1:] == 0).all()) and bool((grad[0] != 0).any())
    # txt_len = 0: the only path is T blanks
    assert abs(float(nll[1]) + float(RR.log_probs(z[1, :2, 0])[:, 0].sum())) <= 1e-12


# ---- host build of csrc/rnnt.inc -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rnh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rnh") / "librnh.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "native", "rnnt_host.cpp")])
    L = ctypes.CDLL(so)
    L.rnnth_lattice.restype = None
    L.rnnth_lattice.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 4
    return L


def _lattice_inputs(T, U, seed):
    """blank / label log-probabilities of a random V = 4 head, float64 and their float32 roundings"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((T, U + 1, 4), generator=g, dtype=torch.float64) * 2
    y = torch.randint(1, 4, (U,), generator=g)
    lp = RR.log_probs(z)
    lpb, lpl = RR._lpb_lpl(lp, y, 0)
    lpl_full = torch.zeros((T, U + 1), dtype=torch.float64)
    lpl_full[:, :U] = lpl
    return z, y, lpb.contiguous(), lpl_full


@pytest.mark.parametrize("nthr", [1, 128])
@pytest.mark.parametrize("T,U", LATTICES)
def test_host_lattice_against_reference(rnh, T, U, nthr):
    """alpha, beta, nll and the gradient coefficients of rnnt.inc in f32 against float64.  Bound: a cell is reached by
    at most T + U additions of rounded terms, each logaddexp adds a few ulps of its result, and every partial result is
    bounded by |ln P|: (T + U + 2) * 8 * 2^-24 * max(1, |ln P|), from the operation count, not from what the code
    gives."""
    z, y, lpb, lpl = _lattice_inputs(T, U, 7 * T + U)
    U1 = U + 1
    f = lambda a: np.ascontiguousarray(a.numpy().astype(np.float32))
    lpb32, lpl32 = f(lpb), f(lpl)
    alpha, beta = np.full((T, U1), np.nan, np.float32), np.full((T, U1), np.nan, np.float32)
    coef = np.full((T, U1, 3), np.nan, np.float32)
    nll = np.zeros(1, np.float32)
    el, tl = np.array([T], np.int64), np.array([U], np.int64)
    p = lambda a: a.ctypes.data
    rnh.rnnth_lattice(p(lpb32), p(lpl32), p(el), p(tl), 1, T, U1, nthr, p(alpha), p(beta), p(nll), p(coef))
    lp = RR.log_probs(z)
    a_ref, lnp = RR.alpha_lattice(lp, y)
    b_ref, lnp_b = RR.beta_lattice(lp, y)
    a_ref = np.array([[float(v) for v in row] for row in a_ref])
    b_ref = np.array([[float(v) for v in row] for row in b_ref])
    tol = (T + U + 2) * 8 * 2.0 ** -24 * max(1.0, abs(float(lnp)))
    assert abs(float(nll[0]) + float(lnp)) <= tol
    assert float(np.abs(alpha - a_ref).max()) <= tol and float(np.abs(beta - b_ref).max()) <= tol
    # the coefficients against the closed form's: gamma and the two transition posteriors, all in [0, 1]
    gam = np.exp(a_ref + b_ref - float(lnp))
    assert float(np.abs(np.exp(coef[:, :, 0].astype(np.float64)) - gam).max()) <= 3 * tol
    bt = np.full((T, U1), -np.inf)
    bt[:-1] = b_ref[1:]
    bt[T - 1, U] = 0.0
    eb = np.exp(a_ref + lpb.numpy() + bt - float(lnp))
    assert float(np.abs(coef[:, :, 1] - eb).max()) <= 3 * tol
    bu = np.full((T, U1), -np.inf)
    bu[:, :-1] = b_ref[:, 1:]
    el_ref = np.exp(a_ref + lpl.numpy() + bu - float(lnp))
    assert float(np.abs(coef[:, :, 2] - el_ref).max()) <= 3 * tol


def test_host_lattice_ragged_batch_and_bad_lengths(rnh):
    """B = 3 with lengths below the padded sizes (one txt_len = 0) and lengths outside [1, T] x [0, U]: clamped, cells
    outside every lattice untouched, each utterance equal to the same utterance walked alone"""
    T, U1 = 6, 5
    rng = np.random.RandomState(3)
    lpb = np.log(rng.uniform(0.1, 0.6, (3, T, U1))).astype(np.float32)
    lpl = np.log(rng.uniform(0.1, 0.4, (3, T, U1))).astype(np.float32)
    p = lambda a: a.ctypes.data
    for lens in (([6, 3, 4], [4, 0, 2]), ([99, 0, -5], [77, -1, 4])):
        el, tl = np.array(lens[0], np.int64), np.array(lens[1], np.int64)
        alpha, beta = np.full((3, T, U1), 7.0, np.float32), np.full((3, T, U1), 7.0, np.float32)
        nll = np.zeros(3, np.float32)
        rnh.rnnth_lattice(p(lpb), p(lpl), p(el), p(tl), 3, T, U1, 128, p(alpha), p(beta), p(nll), None)
        for b in range(3):
            Tb, Ub = min(max(int(el[b]), 1), T), min(max(int(tl[b]), 0), U1 - 1)
            inside = np.zeros((T, U1), bool)
            inside[:Tb, :Ub + 1] = True
            assert (alpha[b][~inside] == 7.0).all() and (beta[b][~inside] == 7.0).all()
            assert np.isfinite(alpha[b][inside]).all() and np.isfinite(nll[b])
            a1, b1 = np.full((1, T, U1), 7.0, np.float32), np.full((1, T, U1), 7.0, np.float32)
            n1 = np.zeros(1, np.float32)
            el1, tl1 = el[b:b + 1].copy(), tl[b:b + 1].copy()
            rnh.rnnth_lattice(p(lpb[b]), p(lpl[b]), p(el1), p(tl1), 1, T, U1, 1, p(a1), p(b1), p(n1), None)
            assert np.array_equal(a1[0], alpha[b]) and np.array_equal(b1[0], beta[b]) and n1[0] == nll[b]
            assert abs(float(beta[b, 0, 0]) + float(nll[b])) <= 1e-4 * (1 + abs(float(nll[b])))


# ---- config handling ------------------------------------------------------------------------------------------------------
HEAD = {'enable': True, 'weight': 0.3, 'joint_dim': 16,
        'pred': {'module': 'LSTM', 'dim': 12, 'layer': 1, 'emb_dim': 20, 'dropout': 0}}


def _tiny_model_cfg():
    return dict(ctc_weight=0.5,
                encoder=dict(prenet='', module='LSTM', bidirection=True, dim=[16, 16], dropout=[0, 0],
                             layer_norm=[False, False], proj=[True, True], sample_rate=[1, 1], sample_style='drop'),
                attention=dict(mode='loc', dim=12, num_head=1, v_proj=False, temperature=0.5, loc_kernel_size=5,
                               loc_kernel_num=2),
                decoder=dict(module='LSTM', dim=16, layer=1, dropout=0))


def test_absent_and_disabled_block_add_no_parameters():
    asr = _mod("src.asr")
    torch.manual_seed(0)
    plain = asr.ASR(13, 11, True, **_tiny_model_cfg())
    torch.manual_seed(0)
    off = asr.ASR(13, 11, True, transducer=dict(HEAD, enable=False), **_tiny_model_cfg())
    torch.manual_seed(0)
    none = asr.ASR(13, 11, True, transducer=None, **_tiny_model_cfg())
    keys = list(plain.state_dict())
    assert list(off.state_dict()) == keys and list(none.state_dict()) == keys
    for k in keys:                                   # the same draws from the same seed
        assert torch.equal(plain.state_dict()[k], off.state_dict()[k])
    assert not plain.enable_rnnt and not off.enable_rnnt and not any("transducer" in k for k in keys)
    assert plain.create_msg() == off.create_msg()
    with pytest.raises(RuntimeError, match="transducer"):
        plain.transducer_logits(None, None, None, None)
    with pytest.raises(RuntimeError, match="transducer"):
        plain.transducer_greedy(None, None)
    on = asr.ASR(13, 11, True, transducer=dict(HEAD), **_tiny_model_cfg())
    new = [k for k in on.state_dict() if k not in keys]
    assert new and all(k.startswith("transducer.") for k in new) and on.enable_rnnt and on.rnnt_weight == 0.3
    assert set(new) == {"transducer." + k for k in
                        ("emb.weight", "pred.weight_ih_l0", "pred.weight_hh_l0", "pred.bias_ih_l0", "pred.bias_hh_l0",
                         "lin_enc.weight", "lin_enc.bias", "lin_pred.weight", "lin_pred.bias", "lin_out.weight",
                         "lin_out.bias")}
    assert len(on.create_msg()) == len(plain.create_msg()) + 1 and "ransducer" in on.create_msg()[-1]
    with pytest.raises(ValueError, match="unknown"):
        asr.ASR(13, 11, True, transducer=dict(HEAD, beam=4), **_tiny_model_cfg())
    # a transducer-only model: CTC is the auxiliary loss, there is no attention decoder
    only = asr.ASR(13, 11, True, transducer=dict(HEAD), **dict(_tiny_model_cfg(), ctc_weight=1))
    assert only.enable_rnnt and only.enable_ctc and not only.enable_att


def test_reference_state_dict_still_loads_strict():
    """a checkpoint of the reference implementation (the golden case's parameters) into a model built with the block
    absent and with enable: false"""
    asr = _mod("src.asr")
    name = "las_hybrid_loc"
    cfg, D, V = CASES[name][:3]
    sd = golden_state_dict(load_golden(name))
    for extra in ({}, {'transducer': None}, {'transducer': dict(HEAD, enable=False)}):
        m = asr.ASR(D, V, False, **dict(cfg, **extra))
        m.load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError):
        asr.ASR(D, V, False, **dict(cfg, transducer=dict(HEAD))).load_state_dict(sd, strict=True)


def test_conflicting_blocks_are_refused():
    tr = _mod("src.transducer")
    base = {'model': {'transducer': dict(HEAD)}}
    tr.check_exclusive(base)
    tr.check_exclusive({'model': {}, 'mwer': {'enable': True}, 'emb': {'enable': True}})
    tr.check_exclusive(dict(base, mwer={'enable': False}, emb={'enable': False}))
    tr.check_exclusive({'model': {'transducer': dict(HEAD, enable=False)}, 'mwer': {'enable': True}})
    with pytest.raises(ValueError) as e:
        tr.check_exclusive(dict(base, mwer={'enable': True, 'nbest': 4}))
    assert "transducer" in str(e.value) and "mwer" in str(e.value)
    with pytest.raises(ValueError) as e:
        tr.check_exclusive(dict(base, mwer={'nbest': 4}))            # mwer's enable defaults to true
    assert "transducer" in str(e.value) and "mwer" in str(e.value)
    with pytest.raises(ValueError) as e:
        tr.check_exclusive(dict(base, emb={'enable': True}))
    assert "transducer" in str(e.value) and "emb" in str(e.value)


def test_decode_block_is_taken_out():
    tr = _mod("src.transducer")
    d = {'beam_size': 4, 'transducer': {'enable': True, 'max_symbols': 2, 'max_len_ratio': 0.25}}
    assert tr.take_decode_block(d) == {'max_symbols': 2, 'max_len_ratio': 0.25} and d == {'beam_size': 4}
    d = {'beam_size': 4, 'transducer': {'enable': True}}
    assert tr.take_decode_block(d) == {'max_symbols': 3, 'max_len_ratio': 0.5} and d == {'beam_size': 4}
    d = {'beam_size': 4, 'transducer': {'enable': False, 'max_symbols': 2}}
    assert tr.take_decode_block(d) is None and d == {'beam_size': 4}
    d = {'beam_size': 4}
    assert tr.take_decode_block(d) is None and d == {'beam_size': 4}
    with pytest.raises(ValueError, match="unknown"):
        tr.take_decode_block({'transducer': {'enable': True, 'beam': 2}})
    with pytest.raises(ValueError, match="align"):
        tr.take_decode_block({'align': True, 'transducer': {'enable': True}})
    with pytest.raises(ValueError, match="rescore"):
        tr.take_decode_block({'rescore': {'enable': True}, 'transducer': {'enable': True}})
    with pytest.raises(ValueError):
        tr.take_decode_block({'transducer': {'enable': True, 'max_symbols': 0}})


@pytest.mark.parametrize("module,layer,seed,bias", RR.GREEDY_CASES)
def test_greedy_cases_meet_the_reference_conditions(module, layer, seed, bias):
    """the cases of the GPU greedy comparison, on the float64 reference alone: every decision's margin is at least 1e-3,
    blanks and non-blanks occur, the max_symbols cap is hit, the rows finish at different iterations; and the mirror
    reproduces the head's teacher-forced contract (<sos> first)"""
    tr = _mod("src.transducer")
    head, enc, lens = RR.greedy_case(tr.TransducerHead, module, layer, seed, bias)
    ref = RR.HeadRef.of(head, RR.GREEDY_ENC_DIM)
    tokens = RR.check_greedy_case(ref, enc, lens)
    assert all(0 < len(t) <= RR.GREEDY_MAX_LEN and all(0 < k < RR.GREEDY_V for k in t) for t in tokens)
    assert set(ref.param_map()) == set(head.state_dict())
    for b in range(3):                               # the second setting of the GPU test: one symbol per frame, two in all
        _, trace = ref.greedy(enc[b, :int(lens[b])].double(), 1, 2)
        assert min(tr[2] for tr in trace) >= RR.MIN_MARGIN
    # greedy decisions are the teacher-forced logits' argmax along the path the search took
    b = 0
    t64 = torch.tensor([tokens[b]])
    z = ref.logits(enc[b:b + 1, :int(lens[b])].double(), t64)[0]
    assert int(z[0, 0].argmax()) in (0, tokens[b][0])


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_without_gpu():
    """null pointers and impossible sizes are ASRK_EINVAL (-1) / ASRK_ESHAPE (-2) before any HIP call; B == 0 is ASRK_OK"""
    _mod("build").build(verbose=False)
    L = _mod("_lib").load()
    z, f = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    # joint
    assert L.asrk_rnnt_joint_f32(z, 8, f, 8, z, 2, 3, 4, 8, f, 8, z) == -1
    assert L.asrk_rnnt_joint_f32(f, 8, f, 8, z, 2, 3, 4, 8, z, 8, z) == -1
    assert L.asrk_rnnt_joint_f32(f, 7, f, 8, z, 2, 3, 4, 8, f, 8, z) == -1          # row stride below J
    assert L.asrk_rnnt_joint_f32(f, 8, f, 8, z, 2, 0, 4, 8, f, 8, z) == -1
    assert L.asrk_rnnt_joint_f32(f, 8, f, 8, z, -1, 3, 4, 8, f, 8, z) == -1
    assert L.asrk_rnnt_joint_f32(z, 8, z, 8, z, 0, 3, 4, 8, z, 8, z) == 0
    assert L.asrk_rnnt_joint_bwd_f32(f, 8, z, 8, 2, 3, 4, 8, f, 8, f, 8, z) == -1
    assert L.asrk_rnnt_joint_bwd_f32(f, 8, f, 8, 2, 3, 4, 8, f, 8, f, 7, z) == -1
    assert L.asrk_rnnt_joint_bwd_f32(z, 8, z, 8, 0, 3, 4, 8, z, 8, z, 8, z) == 0
    # rows: z, ldz, txt, txt_stride, enc_len, txt_len, B, T, U1, V, blank, lse, lpb, lpl
    assert L.asrk_rnnt_rows_f32(z, 5, f, 3, f, f, 2, 3, 4, 5, 0, f, f, f, z) == -1
    assert L.asrk_rnnt_rows_f32(f, 5, z, 3, f, f, 2, 3, 4, 5, 0, f, f, f, z) == -1    # labels needed when U > 0
    assert L.asrk_rnnt_rows_f32(f, 4, f, 3, f, f, 2, 3, 4, 5, 0, f, f, f, z) == -1    # ldz < V
    assert L.asrk_rnnt_rows_f32(f, 5, f, 2, f, f, 2, 3, 4, 5, 0, f, f, f, z) == -1    # txt_stride < U
    assert L.asrk_rnnt_rows_f32(f, 5, f, 3, f, f, 2, 3, 4, 5, 5, f, f, f, z) == -1    # blank outside [0, V)
    assert L.asrk_rnnt_rows_f32(f, 5, f, 3, f, f, 2, 3, 4, 0, 0, f, f, f, z) == -1
    assert L.asrk_rnnt_rows_f32(f, 5, f, 3, f, f, 2 ** 20, 2 ** 10, 4, 5, 0, f, f, f, z) == -2   # B*T*U1 > INT32_MAX
    assert L.asrk_rnnt_rows_f32(z, 5, z, 3, z, z, 0, 3, 4, 5, 0, z, z, z, z) == 0
    # lattice: lpb, lpl, enc_len, txt_len, B, T, U1, alpha, beta, nll
    assert L.asrk_rnnt_lattice_f32(f, f, f, f, 2, 3, 4, z, f, f, z) == -1
    assert L.asrk_rnnt_lattice_f32(f, f, z, f, 2, 3, 4, f, z, f, z) == -1
    assert L.asrk_rnnt_lattice_f32(f, f, f, f, 2, 3, 0, f, f, f, z) == -1
    assert L.asrk_rnnt_lattice_f32(f, f, f, f, 2, 3, 2049, f, f, f, z) == -2
    assert L.asrk_rnnt_lattice_f32(z, z, z, z, 0, 3, 4, z, z, z, z) == 0
    # grad
    ga = [f, 5, f, 3, f, f, 2, 3, 4, 5, 0, f, f, f, f, f, f, f, f, 5, z]
    for pos, bad in ((0, z), (15, z), (17, z), (18, z), (19, 4), (1, 4), (3, 2), (10, -1), (9, 0)):
        a = list(ga)
        a[pos] = bad
        assert L.asrk_rnnt_grad_f32(*a) == -1, pos
    a = list(ga)
    a[18], a[19] = f, 6                              # in place means the same stride
    assert L.asrk_rnnt_grad_f32(*a) == -1
    a = list(ga)
    a[6] = 0
    assert L.asrk_rnnt_grad_f32(*a) == 0
    # greedy step: logits, ld, enc_len, B, T, V, blank, max_symbols, max_len, t_ptr, n_sym, n_tok, tokens, tok_stride,
    # last_tok, emit, done
    gs = [f, 5, f, 2, 3, 5, 0, 3, 4, f, f, f, f, 4, f, f, f, z]
    for pos, bad in ((0, z), (2, z), (9, z), (12, z), (14, z), (15, z), (16, z), (1, 4), (6, 5), (7, -1), (13, 3)):
        a = list(gs)
        a[pos] = bad
        assert L.asrk_rnnt_greedy_step_f32(*a) == -1, pos
    a = list(gs)
    a[3] = 0
    assert L.asrk_rnnt_greedy_step_f32(*a) == 0
