"""CPU: pruned transducer training without a GPU.

 * config handling of `model: transducer: prune:`: bad values and unknown keys raise, the block absent or off leaves the
   state_dict keys as they were, the block on adds exactly the simple joiner's four;
 * the pruning rule of csrc/rnnt_prune.inc built for the host (tests/native/rnnt_prune_host.cpp) against the numpy mirror
   (tests/rnnt_prune_reference.py), exact integer equality.  The occupations are multiples of 2^-10 (or 2^-16) below 1, so
   every window sum is exact in f32 and in float64 and no case needs excluding;
 * the float64 mirror of the band loss against the dense reference with -inf outside the band;
 * the ABI's argument checks return before any HIP call.

The host build can be run once as a stand-alone sanitizer program: g++ -fsanitize=address,undefined
-DRNNT_PRUNE_HOST_MAIN tests/native/rnnt_prune_host.cpp."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import rnnt_reference as RR
import rnnt_prune_reference as PR
from conftest import PKG_NAME

HERE = os.path.dirname(os.path.abspath(__file__))
HEAD = {'enable': True, 'weight': 0.3, 'joint_dim': 16,
        'pred': {'module': 'LSTM', 'dim': 12, 'layer': 1, 'emb_dim': 20, 'dropout': 0}}


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


def _tiny_model_cfg():
    return dict(ctc_weight=0.5,
                encoder=dict(prenet='', module='LSTM', bidirection=True, dim=[16, 16], dropout=[0, 0],
                             layer_norm=[False, False], proj=[True, True], sample_rate=[1, 1], sample_style='drop'),
                attention=dict(mode='loc', dim=12, num_head=1, v_proj=False, temperature=0.5, loc_kernel_size=5,
                               loc_kernel_num=2),
                decoder=dict(module='LSTM', dim=16, layer=1, dropout=0))


# ---- config -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [{'range': 1}, {'range': 33}, {'range': 2.5}, {'range': True}, {'range': '5'},
                                   {'range': float('nan')}, {'simple_weight': -0.1}, {'simple_weight': float('inf')},
                                   {'simple_weight': 'x'}, {'ranges': 5}, {'enable': True, 'weight': 1.0}, 5, [5]])
def test_bad_prune_blocks_raise(block):
    tr, asr = _mod("src.transducer"), _mod("src.asr")
    with pytest.raises(ValueError, match="prune"):
        tr.take_prune_block(block)
    with pytest.raises(ValueError, match="prune"):
        asr.ASR(13, 11, True, transducer=dict(HEAD, prune=block), **_tiny_model_cfg())


def test_prune_block_defaults_and_values():
    tr = _mod("src.transducer")
    assert tr.take_prune_block(None) is None
    assert tr.take_prune_block({}) == {'range': 5, 'simple_weight': 0.5}
    assert tr.take_prune_block({'enable': True, 'range': 2, 'simple_weight': 0}) == {'range': 2, 'simple_weight': 0.0}
    assert tr.take_prune_block({'enable': False, 'range': 32}) is None
    assert tr.take_prune_block({'range': 7.0}) == {'range': 7, 'simple_weight': 0.5}
    with pytest.raises(ValueError, match="range"):
        tr.take_prune_block({'enable': False, 'range': 40})          # validated even when switched off


def test_state_dict_keys_with_and_without_the_block():
    asr = _mod("src.asr")
    torch.manual_seed(0)
    today = asr.ASR(13, 11, True, transducer=dict(HEAD), **_tiny_model_cfg())
    keys = list(today.state_dict())
    for prune in (None, {'enable': False}, {'enable': False, 'range': 3}):
        torch.manual_seed(0)
        m = asr.ASR(13, 11, True, transducer=dict(HEAD, prune=prune), **_tiny_model_cfg())
        assert list(m.state_dict()) == keys and m.rnnt_prune is None
        assert all(torch.equal(m.state_dict()[k], today.state_dict()[k]) for k in keys)   # the same draws
        assert m.create_msg() == today.create_msg()
        with pytest.raises(RuntimeError, match="prune"):
            m.transducer_loss_pruned(None, None, None, None)
    on = asr.ASR(13, 11, True, transducer=dict(HEAD, prune={'enable': True, 'range': 3}), **_tiny_model_cfg())
    new = [k for k in on.state_dict() if k not in keys]
    assert sorted(new) == sorted("transducer." + k for k in ("lin_am.weight", "lin_am.bias", "lin_lm.weight",
                                                             "lin_lm.bias"))
    assert [k for k in on.state_dict() if k in keys] == keys
    assert on.rnnt_prune == {'range': 3, 'simple_weight': 0.5}
    assert tuple(on.transducer.lin_am.weight.shape) == (11, on.encoder.out_dim)
    assert tuple(on.transducer.lin_lm.weight.shape) == (11, 12)
    assert "runed" in on.create_msg()[-1]
    # without a head the block is nobody's: today's whitelist, extended by `prune` only
    with pytest.raises(ValueError, match="unknown"):
        asr.ASR(13, 11, True, transducer=dict(HEAD, pruned={'enable': True}), **_tiny_model_cfg())
    plain = asr.ASR(13, 11, True, **_tiny_model_cfg())
    assert plain.rnnt_prune is None and not any("lin_am" in k for k in plain.state_dict())


def test_infeasible_lengths_raise_from_host_tensors():
    tr = _mod("src.transducer")
    assert tr.infeasible_utterances([2, 5, 1, 1], [10, 10, 2, 3], 3) == [0, 3]
    head = tr.TransducerHead(11, 16, dict(HEAD['pred']), 16, prune={'range': 3, 'simple_weight': 0.5})
    enc = torch.zeros((2, 5, 16))
    with pytest.raises(ValueError) as e:
        head.forward_pruned(enc, torch.tensor([2, 5]), torch.zeros((2, 10), dtype=torch.int64), torch.tensor([10, 10]))
    assert "[0]" in str(e.value) and "[2]" in str(e.value) and "[10]" in str(e.value)
    plain = tr.TransducerHead(11, 16, dict(HEAD['pred']), 16)
    with pytest.raises(RuntimeError, match="prune"):
        plain.forward_pruned(enc, torch.tensor([2, 5]), torch.zeros((2, 10), dtype=torch.int64), torch.tensor([1, 1]))


# ---- the range rule: host build against the mirror ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rph(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rph") / "librph.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "native", "rnnt_prune_host.cpp")])
    L = ctypes.CDLL(so)
    L.rnntph_ranges.restype = None
    L.rnntph_ranges.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    L.rnntph_feasible.restype = ctypes.c_int
    L.rnntph_feasible.argtypes = [ctypes.c_int] * 3
    return L


def _host_ranges(rph, occ, enc_len, txt_len, S, nthr):
    occ = np.ascontiguousarray(occ, np.float32)
    B, T, U1 = occ.shape
    el, tl = np.array(enc_len, np.int64), np.array(txt_len, np.int64)
    s = np.full((B, T), -7, np.int32)
    rph.rnntph_ranges(occ.ctypes.data, el.ctypes.data, tl.ctypes.data, B, T, U1, S, nthr, s.ctypes.data)
    return s


CASES = {c[0]: c for c in PR.range_cases()}


@pytest.mark.parametrize("nthr", [1, 64])
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_ranges_equal_the_mirror(rph, name, nthr):
    _, occ, enc_len, txt_len, S = CASES[name]
    want, _ = PR.ranges(occ.astype(np.float64), enc_len, txt_len, S)
    assert np.array_equal(PR.ranges(occ, enc_len, txt_len, S)[0], want)       # the sums are exact in both precisions
    got = _host_ranges(rph, occ, enc_len, txt_len, S, nthr)
    assert got.dtype == want.dtype and np.array_equal(got, want), (got, want)
    for b in range(occ.shape[0]):
        PR.check_invariants(got[b], enc_len[b], txt_len[b], S)
        assert bool(rph.rnntph_feasible(enc_len[b], txt_len[b], S)) == PR.feasible(enc_len[b], txt_len[b], S)


def test_the_cases_exercise_every_clause():
    """each named case does what its name says, on the mirror alone"""
    diag = {n: PR.range_diagnostics(c[1][0].astype(np.float64), c[2][0], c[3][0], c[4]) for n, c in CASES.items()}
    s = {n: PR.ranges(c[1], c[2], c[3], c[4])[0] for n, c in CASES.items()}
    assert not s["short_transcript"].any() and CASES["short_transcript"][3][0] + 1 <= CASES["short_transcript"][4]
    assert s["one_frame"].tolist() == [[0]] and s["one_frame_infeasible"].tolist() == [[6]]
    assert diag["monotone"]["monotone"] >= 2 and diag["step"]["step"] >= 1
    assert diag["end"]["end"] >= 3 and s["end"][0, 0] == 0 and s["end"][0, -1] == 10
    assert diag["tie"]["tie"] == 5 and s["tie"].tolist() == [[0, 0, 2, 4, 6]]          # the lowest start, then the end rule
    assert not PR.feasible(2, 10, 3) and s["infeasible"][0, 0] > 0 and s["infeasible"][0, -1] == 8
    b = s["batch"]
    assert (b[1, 4:] == b[1, 3]).all() and (b[2] == 0).all() and b[0, -1] == 10
    assert s["wide"].max() == 48 and s["many_starts"][0, -1] == 138


def test_invariants_on_random_cases(rph):
    rng = np.random.default_rng(7)
    n_infeasible = 0
    for _ in range(200):
        T, U1, S = int(rng.integers(1, 13)), int(rng.integers(1, 41)), int(rng.integers(2, 9))
        Tb, Ub = int(rng.integers(1, T + 1)), int(rng.integers(0, U1))
        occ = (rng.integers(0, 1024, size=(1, T, U1)) / 1024.0).astype(np.float32)
        got = _host_ranges(rph, occ, [Tb], [Ub], S, 64)
        assert np.array_equal(got, PR.ranges(occ.astype(np.float64), [Tb], [Ub], S)[0])
        PR.check_invariants(got[0], Tb, Ub, S)
        n_infeasible += int(not PR.feasible(Tb, Ub, S))
    assert 10 <= n_infeasible <= 190


def test_host_program_runs_clean(tmp_path):
    """the stand-alone program (its own main) under the host sanitizers"""
    exe = str(tmp_path / "rnnt_prune_host")
    subprocess.check_call(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DRNNT_PRUNE_HOST_MAIN", "-o", exe,
                           os.path.join(HERE, "native", "rnnt_prune_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- the mirror itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,U,S", [(4, 3, 2), (7, 3, 3), (3, 7, 5), (5, 2, 5)])
def test_band_mirror_is_the_dense_loss_with_minus_infinity_outside(T, U, S):
    """band_lnp on the band layout equals the dense alpha recursion on lpb / lpl with -inf outside the band; and a band
    that covers the lattice (S >= U + 1, s = 0) is the dense loss itself"""
    g = torch.Generator().manual_seed(10 * T + U)
    V = 5
    occ = torch.rand((1, T, U + 1), generator=g).numpy()
    s = PR.ranges(occ, [T], [U], S)[0][0].tolist()
    z = torch.randn((T, S, V), generator=g, dtype=torch.float64)
    y = torch.randint(1, V, (U,), generator=g)
    lp = RR.log_probs(z)
    lpb, lpl = PR.band_terms(lp, y, s, T, U, S)
    got = PR.band_lnp(lpb, lpl, s, T, U, S)
    dense_b = torch.full((T, U + 1), PR.NEG, dtype=torch.float64)
    dense_l = torch.full((T, U + 1), PR.NEG, dtype=torch.float64)
    for t in range(T):
        for k in range(S):
            if s[t] + k <= U:
                dense_b[t, s[t] + k], dense_l[t, s[t] + k] = lpb[t, k], lpl[t, k]
    want = PR.diag_lnp(dense_b, dense_l, T, U)
    assert abs(float(got) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    if S >= U + 1:
        assert s == [0] * T
        zz = z[:, :U + 1]
        assert abs(float(got) - float(RR.alpha_lnp(RR.log_probs(zz), y))) <= 1e-12


def test_simple_mirror_occupations():
    """c = eb + el sums to one on every anti-diagonal, and the gradients are those of the dense reference"""
    g = torch.Generator().manual_seed(3)
    am, lm = torch.randn((1, 4, 6), generator=g, dtype=torch.float64), torch.randn((1, 3, 6), generator=g,
                                                                                   dtype=torch.float64)
    txt = torch.tensor([[2, 2]])
    r = PR.simple_pass(am, lm, txt, [4], [2])
    for d in range(4 + 2):
        tot = sum(float(r["c"][0, d - u, u]) for u in range(3) if 0 <= d - u < 4)
        assert abs(tot - 1.0) <= 1e-12
    z = am[:, :, None] + lm[:, None]
    nll, grad = RR.batch_nll_grad(z, txt, [4], [2])
    assert float((r["nll"] - nll).abs().max()) <= 1e-12
    assert float((r["dam"] - grad.sum(2)).abs().max()) <= 1e-12 and float((r["dlm"] - grad.sum(1)).abs().max()) <= 1e-12


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_without_gpu():
    """null pointers and impossible sizes are ASRK_EINVAL (-1) / ASRK_ESHAPE (-2) before any HIP call; B == 0 is ASRK_OK"""
    _mod("build").build(verbose=False)
    L = _mod("_lib").load()
    z, f = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    # simple rows: am, lda, lm, ldl, txt, txt_stride, enc_len, txt_len, B, T, U1, V, blank, lse, lpb, lpl
    sr = [f, 5, f, 5, f, 3, f, f, 2, 3, 4, 5, 0, f, f, f, z]
    for pos, bad in ((0, z), (2, z), (4, z), (6, z), (13, z), (1, 4), (3, 4), (5, 2), (12, 5), (9, 0), (11, 0)):
        a = list(sr)
        a[pos] = bad
        assert L.asrk_rnnt_simple_rows_f32(*a) == -1, pos
    a = list(sr)
    a[8], a[9] = 2 ** 15, 2 ** 16
    assert L.asrk_rnnt_simple_rows_f32(*a) == -2
    a = list(sr)
    a[8] = 0
    assert L.asrk_rnnt_simple_rows_f32(*a) == 0
    assert L.asrk_rnnt_simple_occ_f32(f, f, f, f, f, f, f, 2, 3, 4, f, f, z, z) == -1
    assert L.asrk_rnnt_simple_occ_f32(z, z, z, z, z, z, z, 0, 3, 4, z, z, z, z) == 0
    sg = [f, 5, f, 5, f, 3, f, f, 2, 3, 4, 5, 0, f, f, f, f, f, f, 5, f, 5, z]
    for pos, bad in ((0, z), (13, z), (17, z), (18, z), (20, z), (19, 4), (21, 4)):
        a = list(sg)
        a[pos] = bad
        assert L.asrk_rnnt_simple_grad_f32(*a) == -1, pos
    # ranges: occ, enc_len, txt_len, B, T, U1, S, s
    assert L.asrk_rnnt_prune_ranges_f32(f, f, f, 2, 3, 4, 0, f, z) == -1
    assert L.asrk_rnnt_prune_ranges_f32(f, f, f, 2, 3, 4, 33, f, z) == -1
    assert L.asrk_rnnt_prune_ranges_f32(z, f, f, 2, 3, 4, 5, f, z) == -1
    assert L.asrk_rnnt_prune_ranges_f32(z, z, z, 0, 3, 4, 5, z, z) == 0
    # band joint: E, lde, P, ldp, s, B, T, S, U1, J, H, ldh
    assert L.asrk_rnnt_joint_band_f32(f, 8, f, 8, z, 2, 3, 2, 4, 8, f, 8, z) == -1
    assert L.asrk_rnnt_joint_band_f32(f, 8, f, 7, f, 2, 3, 2, 4, 8, f, 8, z) == -1
    assert L.asrk_rnnt_joint_band_f32(f, 8, f, 8, f, 2, 3, 0, 4, 8, f, 8, z) == -1
    assert L.asrk_rnnt_joint_band_f32(z, 8, z, 8, z, 0, 3, 2, 4, 8, z, 8, z) == 0
    assert L.asrk_rnnt_joint_band_bwd_f32(f, 8, f, 8, f, 2, 3, 2, 4, 8, f, 8, z, 8, z) == -1
    assert L.asrk_rnnt_joint_band_bwd_f32(z, 8, z, 8, z, 0, 3, 2, 4, 8, z, 8, z, 8, z) == 0
    # band rows: z, ldz, txt, txt_stride, enc_len, txt_len, s, B, T, S, U1, V, blank, lse, lpb, lpl
    br = [f, 5, f, 3, f, f, f, 2, 3, 2, 4, 5, 0, f, f, f, z]
    for pos, bad in ((0, z), (2, z), (6, z), (13, z), (1, 4), (3, 2), (9, 0), (9, 33), (12, 5)):
        a = list(br)
        a[pos] = bad
        assert L.asrk_rnnt_rows_band_f32(*a) == -1, pos
    a = list(br)
    a[7], a[8] = 2 ** 20, 2 ** 10
    assert L.asrk_rnnt_rows_band_f32(*a) == -2
    assert L.asrk_rnnt_band_scatter_f32(f, f, z, f, f, 2, 3, 2, 4, f, f, z) == -1
    assert L.asrk_rnnt_band_scatter_f32(z, z, z, z, z, 0, 3, 2, 4, z, z, z) == 0
    bg = [f, 5, f, 3, f, f, f, 2, 3, 2, 4, 5, 0, f, f, f, f, f, f, f, f, 5, z]
    for pos, bad in ((0, z), (6, z), (13, z), (17, z), (19, z), (20, z), (21, 4)):
        a = list(bg)
        a[pos] = bad
        assert L.asrk_rnnt_grad_band_f32(*a) == -1, pos
    a = list(bg)
    a[20], a[21] = f, 6                              # in place means the same stride
    assert L.asrk_rnnt_grad_band_f32(*a) == -1
    a = list(bg)
    a[7] = 0
    assert L.asrk_rnnt_grad_band_f32(*a) == 0


@pytest.mark.parametrize("seed", PR.LATTICE_RANGE_SEEDS)
def test_lattice_range_seeds_are_decisive_in_float64(seed):
    """the seeds of the GPU comparison of ranges from a real simple lattice: on the float64 mirror alone fewer than a
    tenth of the frames have a best and a second-best window within 1e-3 of each other"""
    am, lm, txt, enc_len, txt_len = PR.lattice_range_case(seed)
    r = PR.simple_pass(am.double(), lm.double(), txt, enc_len, txt_len)
    s, margin = PR.ranges(r["occ"], enc_len, txt_len, PR.LATTICE_RANGE_S)
    frames = sum(enc_len)
    undecided = sum(int((margin[b, :enc_len[b]] < PR.MIN_RANGE_MARGIN).sum()) for b in range(len(enc_len)))
    assert 10 * undecided <= frames
    assert len(set(s[0, :enc_len[0]].tolist())) >= 4                 # the band really moves
    for b in range(len(enc_len)):
        PR.check_invariants(s[b], enc_len[b], txt_len[b], PR.LATTICE_RANGE_S)
