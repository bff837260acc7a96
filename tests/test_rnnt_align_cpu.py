"""CPU: the transducer forced alignment without a GPU.

 * the numpy f32 reference (tests/rnnt_align_reference.py) finds the path a float64 enumeration of all paths finds;
   the all-ties lattice emits everything at frame 0; a NaN cell gives a NaN score, a -inf column a -inf score, both
   with -1 / 0 outputs;
 * csrc/rnnt_align.inc built for the host (tests/native/rnnt_align_host.cpp) equals the reference bit for bit, with
   one lane and with the kernel's 128, alone and in a ragged batch whose padding is NaN;
 * decode.transducer's `align` and `timestamps` keys: validated, returned only when named, the exclusions raise;
 * the ABI's argument checks return before any HIP call.

The host build can be run once as a stand-alone sanitizer program: g++ -fsanitize=address,undefined
-DRNNT_ALIGN_HOST_MAIN tests/native/rnnt_align_host.cpp."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import rnnt_align_reference as AR
from conftest import PKG_NAME

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = [(1, 0), (1, 1), (1, 5), (5, 0), (2, 1), (7, 3), (3, 7)]
LATTICES = SMALL + [(64, 63), (65, 64), (9, 300), (130, 100)]
LANES = 128                                        # RA_THREADS of csrc/rnnt_align.hip


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,U", SMALL)
def test_reference_equals_enumeration(T, U):
    for k in range(20):
        lpb, lpl = AR.random_lattice(T, U, 1000 * T + 10 * U + k)
        r = AR.align_f32(lpb, lpl, T, U)
        frames, best = AR.enumerate_best(lpb, lpl, T, U)
        assert list(r["frames"]) == frames
        # T + U rounded adds, every partial sum at most |best| in magnitude (all terms are <= 0)
        assert abs(float(r["score"]) - best) <= (T + U) * 2.0 ** -24 * max(1.0, abs(best))
        f64, s64, _ = AR.viterbi64(lpb, lpl, T, U)
        assert f64 == frames and abs(s64 - best) <= 1e-12 * max(1.0, abs(best))
        # labels_done is the path seen from the frames' side
        done = r["labels_done"]
        assert done[T - 1] == U and all(done[t] == sum(1 for f in frames if f <= t) for t in range(T))
        assert AR.path_score64(lpb, lpl, frames, T, U) == best


def test_all_ties_emit_at_frame_zero():
    T, U = 6, 4
    lpb = np.full((T, U + 1), -1.0, np.float32)
    lpl = np.full((T, U + 1), -1.0, np.float32)
    r = AR.align_f32(lpb, lpl, T, U)
    assert list(r["frames"]) == [0] * U and list(r["labels_done"]) == [U] * T
    assert float(r["score"]) == -float(T + U)


def test_nan_cell_and_inf_column():
    T, U = 5, 3
    lpb, lpl = AR.random_lattice(T, U, 5)
    bad = lpl.copy()
    bad[:, 1] = np.nan                              # what the row pass writes for a label outside [0, V)
    r = AR.align_f32(lpb, bad, T, U)
    assert np.isnan(r["score"]) and (r["frames"] == -1).all() and (r["labels_done"] == -1).all()
    assert (r["tok_logp"] == 0).all()
    one = lpl.copy()
    one[2, 1] = np.nan                              # one cell is enough: the NaN wins every compare behind it
    assert np.isnan(AR.align_f32(lpb, one, T, U)["score"])
    inf = lpl.copy()
    inf[:, 2] = -np.inf
    r = AR.align_f32(lpb, inf, T, U)
    assert r["score"] == -np.inf and (r["frames"] == -1).all() and (r["labels_done"] == -1).all()
    assert (r["tok_logp"] == 0).all()


# ---- host build of csrc/rnnt_align.inc -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rah(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rah") / "librah.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "native", "rnnt_align_host.cpp")])
    L = ctypes.CDLL(so)
    L.rnnth_align.restype = None
    L.rnnth_align.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 8
    return L


def _host(rah, lpb, lpl, el, tl, nthr):
    B, T, U1 = lpb.shape
    frames = np.full((B, U1 - 1), 77, np.int32)
    done = np.full((B, T), 77, np.int32)
    logp = np.full((B, U1 - 1), 7.0, np.float32)
    score = np.zeros(B, np.float32)
    el, tl = np.asarray(el, np.int64), np.asarray(tl, np.int64)
    p = lambda a: a.ctypes.data
    rah.rnnth_align(p(lpb), p(lpl), p(el), p(tl), B, T, U1, nthr, None, None, None, p(frames), p(done), p(logp), None,
                    p(score))
    return frames, done, logp, score


def _same(host, ref, b=0):
    frames, done, logp, score = host
    assert np.array_equal(frames[b], ref["frames"]) and np.array_equal(done[b], ref["labels_done"])
    assert logp[b].tobytes() == ref["tok_logp"].tobytes()
    assert score[b:b + 1].tobytes() == np.float32(ref["score"]).tobytes()


@pytest.mark.parametrize("nthr", [1, LANES])
@pytest.mark.parametrize("T,U", LATTICES)
def test_host_equals_reference_exactly(rah, T, U, nthr):
    lpb, lpl = AR.random_lattice(T, U, 31 * T + U)
    _same(_host(rah, lpb[None], lpl[None], [T], [U], nthr), AR.align_f32(lpb, lpl, T, U))


@pytest.mark.parametrize("nthr", [1, LANES])
def test_host_edge_cases(rah, nthr):
    T, U = 6, 4
    ties = np.full((1, T, U + 1), -1.0, np.float32)
    frames, done, _, score = _host(rah, ties, ties, [T], [U], nthr)
    assert list(frames[0]) == [0] * U and list(done[0]) == [U] * T and score[0] == -float(T + U)
    lpb, lpl = AR.random_lattice(T, U, 9)
    for col, val in ((1, np.nan), (2, -np.inf)):
        x = lpl.copy()
        x[:, col] = val
        h = _host(rah, lpb[None], x[None], [T], [U], nthr)
        _same(h, AR.align_f32(lpb, x, T, U))
        assert (h[0] == -1).all() and (h[1] == -1).all() and (h[2] == 0).all()


def test_host_ragged_batch_never_reads_outside(rah):
    """B = 3, padded in T and U1 beyond the longest utterance, one U_b = 0, NaN in every cell outside a lattice, and
    lengths outside [1, T] x [0, U] clamped: each utterance equals the same utterance aligned alone"""
    T, U1 = 9, 8
    sizes = [(7, 5), (4, 0), (6, 6)]
    lpb = np.full((3, T, U1), np.nan, np.float32)
    lpl = np.full((3, T, U1), np.nan, np.float32)
    for b, (Tb, Ub) in enumerate(sizes):
        a, c = AR.random_lattice(Tb, Ub, 40 + b)
        lpb[b, :Tb, :Ub + 1] = a
        lpl[b, :Tb, :Ub] = c[:, :Ub]
    h = _host(rah, lpb, lpl, [s[0] for s in sizes], [s[1] for s in sizes], LANES)
    for b, (Tb, Ub) in enumerate(sizes):
        ref = AR.align_f32(lpb[b], lpl[b], Tb, Ub)
        assert np.isfinite(ref["score"]) and (ref["frames"][:Ub] >= 0).all()
        _same(h, ref, b)
    full = np.ascontiguousarray(lpb[2:3, :6, :7]), np.ascontiguousarray(lpl[2:3, :6, :7])
    h2 = _host(rah, full[0], full[1], [99], [77], 1)                   # clamped to T = 6, U = 6
    assert np.array_equal(h2[0][0], h[0][2][:6]) and h2[3][0] == h[3][2]


# ---- config handling ------------------------------------------------------------------------------------------------------
def test_decode_block_keys():
    tr = _mod("src.transducer")
    base = {'max_symbols': 3, 'max_len_ratio': 0.5}
    # a block without the keys returns exactly what it returned before they existed
    d = {'beam_size': 4, 'transducer': {'enable': True}}
    assert tr.take_decode_block(d) == base and d == {'beam_size': 4}
    assert tr.take_decode_block({'transducer': {'enable': True, 'beam_size': 2, 'nbest': 2}}) == \
        dict(base, beam_size=2, nbest=2)
    # named: returned as booleans, false included
    assert tr.take_decode_block({'transducer': {'enable': True, 'align': True}}) == dict(base, align=True)
    assert tr.take_decode_block({'transducer': {'enable': True, 'align': False}}) == dict(base, align=False)
    assert tr.take_decode_block({'transducer': {'enable': True, 'timestamps': True, 'beam_size': 2}}) == \
        dict(base, timestamps=True, beam_size=2)
    assert tr.take_decode_block({'transducer': {'enable': True, 'align': False, 'timestamps': True}}) == \
        dict(base, align=False, timestamps=True)
    assert tr.take_decode_block({'transducer': {'enable': True, 'align': True, 'beam_size': 1, 'lm_weight': 0}}) == \
        dict(base, align=True, beam_size=1, lm_weight=0.0)
    assert tr.take_decode_block({'transducer': {'enable': False, 'align': True}}) is None
    for key in ('align', 'timestamps'):
        for v in (1, 0, 'yes', None, 1.0):
            with pytest.raises(ValueError, match=key):
                tr.take_decode_block({'transducer': {'enable': True, key: v}})
    for extra in ({'beam_size': 2}, {'timestamps': True},
                  {'lm_weight': 0.3}):
        with pytest.raises(ValueError, match="align"):
            tr.take_decode_block({'lm_path': 'x.arpa', 'transducer': dict({'enable': True, 'align': True}, **extra)})
    # the CTC aligner and the transducer block still exclude each other, with the message they had
    with pytest.raises(ValueError, match="decode.transducer excludes decode.align and decode.rescore"):
        tr.take_decode_block({'align': True, 'transducer': {'enable': True, 'align': True}})
    with pytest.raises(ValueError, match="unknown"):
        tr.take_decode_block({'transducer': {'enable': True, 'aligned': True}})


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_without_gpu():
    """ASRK_EINVAL (-1) / ASRK_ESHAPE (-2) before any HIP call; B == 0 is ASRK_OK; the workspace size of every route"""
    _mod("build").build(verbose=False)
    L = _mod("_lib").load()
    z, f, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4104)
    AUTO, LDS, GLOBAL = 0, 1, 2
    # lpb, lpl, enc_len, txt_len, B, T, U1, flags, alpha, beta, nll, frames, labels_done, tok_logp, tok_post, score,
    # stamps, ws, ws_bytes, stream
    ok = [f, f, f, f, 2, 30, 9, LDS, z, z, z, f, f, f, z, f, z, z, 0, z]
    for pos in (0, 1, 2, 3, 11, 12, 13, 15):
        a = list(ok)
        a[pos] = z
        assert L.asrk_rnnt_align_f32(*a) == -1, pos
    for pos, bad in ((4, -1), (5, 0), (6, 0), (5, -3), (7, 3), (7, -1), (7, 4)):
        a = list(ok)
        a[pos] = bad
        assert L.asrk_rnnt_align_f32(*a) == -1, (pos, bad)
    for some in ((f, z, z), (z, f, z), (z, z, f), (f, f, z), (f, z, f), (z, f, f)):
        a = list(ok)
        a[8:11] = some
        a[14] = f
        assert L.asrk_rnnt_align_f32(*a) == -1, some
    a = list(ok)
    a[8:11] = (f, f, f)                             # the lattice without a place for tok_post
    assert L.asrk_rnnt_align_f32(*a) == -1
    a = list(ok)
    a[6] = 2049
    assert L.asrk_rnnt_align_f32(*a) == -2
    a = list(ok)
    a[4], a[5] = 2 ** 20, 2 ** 10                   # B*T*U1 > INT32_MAX
    assert L.asrk_rnnt_align_f32(*a) == -2
    a = list(ok)
    a[4] = 0
    a[:4] = (z, z, z, z)
    assert L.asrk_rnnt_align_f32(*a) == 0
    # routes: (T + U1 - 1) * ceil(U1 / 64) words of 8 bytes per utterance; LDS holds 128 KiB of them
    assert L.asrk_rnnt_align_ws_bytes(2, 30, 9, AUTO) == 0 and L.asrk_rnnt_align_ws_bytes(2, 30, 9, LDS) == 0
    assert L.asrk_rnnt_align_ws_bytes(2, 30, 9, GLOBAL) == 2 * 38 * 1 * 8
    assert L.asrk_rnnt_align_ws_bytes(3, 200, 65, GLOBAL) == 3 * 264 * 2 * 8
    T_fit, T_over = 8192 - 64, 8192 - 63            # U1 = 65: 2 words per diagonal, 8192 diagonals fit
    assert L.asrk_rnnt_align_ws_bytes(1, T_fit, 65, AUTO) == 0
    assert L.asrk_rnnt_align_ws_bytes(1, T_over, 65, AUTO) == (T_over + 64) * 2 * 8
    assert L.asrk_rnnt_align_ws_bytes(1, T_over, 65, LDS) == 0       # rejected
    assert L.asrk_rnnt_align_ws_bytes(1, 30, 9, 3) == 0 and L.asrk_rnnt_align_ws_bytes(0, 30, 9, GLOBAL) == 0
    a = list(ok)
    a[4], a[5], a[6] = 1, T_over, 65                # a forced LDS route that does not fit
    assert L.asrk_rnnt_align_f32(*a) == -2
    # the global route needs its workspace: NULL, misaligned or short are refused
    need = 2 * 38 * 8
    for ws, n in ((z, need), (odd, need), (f, need - 1), (f, 0)):
        a = list(ok)
        a[7], a[17], a[18] = GLOBAL, ws, n
        assert L.asrk_rnnt_align_f32(*a) == -1, (ws, n)
