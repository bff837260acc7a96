"""CPU: the reference and the case table of tests/audio_reference.py.

The float64 reference is pinned to oracle/fbank_oracle.py and to the independent scipy implementation at 1e-10; no mel
energy of the table comes near the clamp; every row selects the route it names and the table names every instantiation
the dispatch of csrc/audio.hip knows; three seeded faults exceed the derived bound."""
import importlib
import os
import re

import numpy as np
import pytest

import audio_reference as R
import fbank_independent as FI
from conftest import PKG_NAME, ROOT
from oracle import fbank_oracle as FO

AUDIO_HIP = os.path.join(ROOT, PKG_NAME, "csrc", "audio.hip")


@pytest.fixture(scope="module")
def audio():
    return importlib.import_module(PKG_NAME + ".src.audio")


@pytest.mark.parametrize("sr,frame_ms,nmel", R.GEOMETRIES)
def test_reference_equals_oracle_and_scipy_at_default_options(sr, frame_ms, nmel):
    win, shift, N = R.geometry(sr, frame_ms)
    assert (win, shift, N) == FO.frame_geometry(0, sr, frame_ms)[:3]
    x = R.signal(win + shift * 11 + 3, sr, seed=5)
    a = R.logmel(x, sr, nmel, frame_ms)
    assert a.shape == (12, nmel) and a.dtype == np.float64
    assert np.max(np.abs(a - FO.kaldi_fbank(x, sr, nmel, frame_ms))) < 1e-10
    assert np.max(np.abs(a - FI.scipy_fbank(x, sr, nmel, frame_ms))) < 1e-10
    for order, window, cm in [(0, 2, True), (1, 2, False), (2, 2, True), (1, 3, True), (2, 4, True), (1, 7, False)]:
        want = FO.audio_transform(x, sr, nmel, order, window, cm, frame_length=frame_ms)
        got = R.features(a, FO.delta_filters(order, window), cm)
        assert got.shape == want.shape == (12, (order + 1) * nmel)
        assert np.max(np.abs(got - want)) < 1e-10, (order, window, cm)
    if nmel >= R.NUM_CEPS:
        assert np.max(np.abs(R.mfcc(a, R.NUM_CEPS) -
                             FO.kaldi_mfcc(x, sr, nmel, R.NUM_CEPS, frame_length=frame_ms))) < 1e-10


def test_float32_run_stays_in_float32():
    c = R.LOGMEL_CASES[2]
    rows = R.case_rows(c, "int16", np.float32)
    assert all(r.dtype == np.float32 for r in rows)
    y = R.features(rows[1], FO.delta_filters(2, 2), True, np.float32)
    assert y.dtype == np.float32
    for kind in ("int16", "float32"):
        assert 0.0 < R.logmel_expected(c, kind)[1] < 1e-3


def test_batches_have_the_edges_the_table_promises():
    per_route = {}
    for c in R.LOGMEL_CASES:
        f = c.frames
        assert 3 <= len(f) <= 5 and 1 in f and max(f) <= 10 and f.index(max(f)) != 0, c.name
        assert f[len(f) // 2] == 0 or f[(len(f) - 1) // 2] == 0, c.name              # the 0-frame one in the middle
        assert c.win == R.geometry(c.sr, c.frame_ms)[0]
        lens = [len(w) for w in R.case_waves(c, "int16")]
        assert lens == [c.win - 1 if m == 0 else c.win + R.geometry(c.sr, 1)[1] * (m - 1) + 3 for m in f]
        per_route.setdefault(c.route, set()).add(max(f))
    for route, tmaxes in per_route.items():
        assert tmaxes & {5, 6, 7}, route                                              # a ragged last 4-frame workgroup
    assert {c.nmel for c in R.LOGMEL_CASES} == {13, 23, 40, 80}
    for tmax, frames in R.DELTA_FRAMES.items():
        assert max(frames) == tmax and frames[0] == 0 and frames[-1] == 0 and 0 in frames[1:-1]
    assert set(sum(R.DELTA_FRAMES.values(), ())) == {0, 1, 2, 127, 128, 129, 130, 257}
    assert {(c.C, c.L) for c in R.DELTA_CASES} == {(1, 1), (2, 5), (3, 9), (2, 7), (2, 11), (3, 13), (2, 15), (2, 3)}
    assert {c.D for c in R.DELTA_CASES} == {1, 63, 64, 65, 130} and {c.cmvn for c in R.DELTA_CASES} == {0, 1}


def test_no_mel_energy_is_clamped():
    """condition of the table: no element is ever excluded from a comparison, so none may sit on the log floor"""
    smallest = np.inf
    for c in R.LOGMEL_CASES:
        for kind in ("int16", "float32"):
            for w in R.case_waves(c, kind):
                e = R.mel_energy(R.as_float(w), c.sr, c.nmel, c.frame_ms, **R.fbank_kwargs(c))
                if e.size:
                    smallest = min(smallest, float(e.min()))
                    assert e.min() >= 1e3 * R.FLT_EPS, (c.name, kind, float(np.log(e.min())))
    print("smallest log-mel of the table: %.2f (floor %.2f)" % (np.log(smallest), R.LOG_FLOOR))


def test_constant_input_gives_the_floor_in_the_reference():
    for c in R.LOGMEL_CASES:
        if c.feat_type == "fbank" and dict(c.opts).get("remove_dc_offset", True):
            for dt in (np.float64, np.float32):
                y = R.logmel(np.full(c.win + 50, 0.37), c.sr, c.nmel, c.frame_ms, dtype=dt, **R.fbank_kwargs(c))
                assert y.size and np.allclose(y, FI.LOG_FLOOR, atol=1e-5), c.name


# ------------------------------------------------------------------------------------------------ routes
def _dispatch_in_source():
    """the instantiations csrc/audio.hip can launch, read off its dispatch code"""
    src = open(AUDIO_HIP).read()
    switch = re.search(r"switch \(log2n\) \{(.*?)\}", src, re.S).group(1)
    l2s = sorted(int(v) for v in re.findall(r"ASRK_FBANK_CASE\((\d+)\)", switch))
    chain = re.search(r"if \(L == 1\) ASRK_DC_CASE\(1\);(.*?)#undef ASRK_DC_CASE", src, re.S).group(1)
    steps = [(int(a), int(b)) for a, b in re.findall(r"else if \(L <= (\d+)\) ASRK_DC_CASE\((\d+)\);", chain)]
    last = int(re.search(r"else ASRK_DC_CASE\((\d+)\);", chain).group(1))
    n_dc = len(re.findall(r"ASRK_DC_CASE\(\d+\);", src))
    assert n_dc == 2 + len(steps), "the delta/CMVN dispatch has a form this test does not read"
    sample_types = set(re.findall(r"fbank_logmel_batch_kernel<(\w+), L2_>", src))
    frame_types = set(re.findall(r"fbank_frames_batch_kernel<(\w+)>", src))
    return l2s, steps, last, sample_types, frame_types


def test_every_row_selects_the_route_it_names(audio):
    l2s, steps, last, _, _ = _dispatch_in_source()
    for c in R.LOGMEL_CASES:
        o = dict(c.opts)
        tb = audio._FbankTables.get(c.sr, c.frame_ms, R.SHIFT_MS, c.nmel, o.get("low_freq", 20.0),
                                    o.get("high_freq", 0.0), "cpu")
        assert (tb.win, tb.padded, tb.shift) == (c.win, c.N, R.geometry(c.sr, c.frame_ms)[1]), c.name
        if c.route[0] == "fused":
            assert tb.fused and tb.log2n == c.route[1] and tb.log2n in l2s, c.name
        else:
            assert not tb.fused and tb.log2n not in l2s, c.name
            assert (tb.log2n < min(l2s)) == (c.route[1] == "below") and (tb.log2n > max(l2s)) == (c.route[1] == "above")
        # the mel ranges the fused kernel walks hold every non-zero weight of the reference's triangles
        w = FO.mel_banks(c.nmel, c.N, c.sr, o.get("low_freq", 20.0), o.get("high_freq", 0.0))
        for m in range(c.nmel):
            k0, k1 = (int(v) for v in tb.mel_range[m])
            nz = np.flatnonzero(w[m] > 0)
            assert len(nz) and k0 <= nz[0] and nz[-1] < k1, (c.name, m)
    c44 = [c for c in R.LOGMEL_CASES if c.sr == 44100][0]
    tb = audio._FbankTables.get(44100, c44.frame_ms, R.SHIFT_MS, c44.nmel, 20.0, 0.0, "cpu")
    assert (tb.ldf, tb.nb) == (1104, 1028)
    for c in R.DELTA_CASES:
        picked = 1 if c.L == 1 else next((lt for lim, lt in steps if c.L <= lim), last)
        assert c.lt == picked == R.lt_class(c.L) and c.L <= last, c.name
    for order, window in R.MODULE_PAIRS:
        assert FO.delta_filters(order, window).shape == (order + 1, 2 * order * window + 1)


def test_the_table_names_every_instantiation_of_the_dispatch():
    l2s, steps, last, sample_types, frame_types = _dispatch_in_source()
    assert l2s == [8, 9, 10] and sample_types == frame_types == {"int16_t", "float"}
    names = {"int16_t": "int16", "float": "float"}
    want = {("logmel", names[t], l2) for t in sample_types for l2 in l2s}
    want |= {("unfused", side, form) for side in ("below", "above")
             for form in ["per_file"] + ["batch_" + names[t] for t in frame_types]}
    want |= {("delta_cmvn", lt) for lt in [1] + [lt for _, lt in steps] + [last]}
    assert {t[1] for t in want if t[0] == "delta_cmvn"} == {1, 5, 9, 16}
    assert R.all_instantiations() == want, sorted(R.all_instantiations() ^ want, key=str)


# ------------------------------------------------------------------------------------------------ seeded faults
def _worst_ratio(pairs):
    """pairs of (error of the faulty float64 run against the reference, derived bound) -> largest error / bound"""
    return max(e / b for e, b in pairs)


def _report(what, pairs, old, old_name):
    """information only: on how many rows the bound in force before this table would have noticed the fault"""
    errs = [e for e, _ in pairs]
    print("%s: error of the faulty run %.3e .. %.3e over %d rows; beyond the derived bound on %d, beyond the old bound "
          "(%s) on %d" % (what, min(errs), max(errs), len(errs), sum(e > b for e, b in pairs), old_name,
                          sum(e >= o for e, o in zip(errs, old))))


def test_bounds_would_catch_a_mel_triangle_without_its_last_bin():
    pairs = []
    for c in R.LOGMEL_CASES:
        if c.feat_type != "fbank":
            continue
        o = R.fbank_kwargs(c)
        w = FO.mel_banks(c.nmel, c.N, c.sr, o["low_freq"], o["high_freq"]).copy()
        m = c.nmel // 2
        w[m, np.flatnonzero(w[m] > 0)[-1]] = 0.0
        ref, e32 = R.logmel_expected(c, "float32")
        bad = R.pad_batch(R.case_rows(c, "float32", np.float64, mel_w=w), c.nmel)
        pairs.append((R.max_err(bad, ref), R.bound("logmel", e32)))
    assert all(e > b for e, b in pairs), pairs            # on EVERY row, not just some
    _report("mel triangle without its last FFT bin", pairs, [2e-3] * len(pairs), "max |d log-mel| < 2e-3")


def test_bounds_would_catch_a_dropped_delta_tap():
    pairs, old = [], []
    for c in R.DELTA_CASES:
        if c.L == 1:
            continue
        ref, e32 = R.delta_expected(c)
        bad, _ = R.delta_expected(c, dropped_tap=(c.C - 1, 0))      # the outermost tap of the highest order
        pairs.append((R.max_err(bad, ref), R.bound(R.delta_kind(c.cmvn), e32)))
        old.append(1e-3 * float(np.nanmax(np.abs(ref))))
    assert all(e > b for e, b in pairs), min(e / b for e, b in pairs)
    _report("outermost delta tap dropped", pairs, old, "rel_err < 1e-3")


def _preemph_fault_pairs(**fault):
    pairs = []
    for c in R.LOGMEL_CASES:
        if c.feat_type != "fbank" or R.fbank_kwargs(c)["preemph"] == 0.0:
            continue
        ref, e32 = R.logmel_expected(c, "int16")
        bad = R.pad_batch(R.case_rows(c, "int16", np.float64, **fault), c.nmel)
        pairs.append((R.max_err(bad, ref), R.bound("logmel", e32)))
    return pairs


def test_first_sample_preemphasised_from_zero_is_not_observable():
    """The fault `the first sample's predecessor is 0 instead of the replicated sample` changes v[0] alone, and the povey
    window is hann(N, symmetric)^0.85 with w[0] = 0: the windowed frame is the same, bit for bit.  No bound of any test
    can see it - measured: error exactly 0 on every row - so the third seeded fault below sits one step further in the
    same expression of the kernel."""
    for win in sorted({c.win for c in R.LOGMEL_CASES}):
        assert FO.povey_window(win)[0] == 0.0
    pairs = _preemph_fault_pairs(replicate_first=False)
    assert len(pairs) >= 10 and all(e == 0.0 for e, _ in pairs), pairs


def test_bounds_would_catch_a_preemphasis_predecessor_with_its_dc_left_in():
    """prev = x[j-1] instead of x[j-1] - mean in `(cur - preemph * prev) * window[j]`: the frame gains
    -preemph * mean * w[j], a window-shaped bump at the lowest FFT bins"""
    pairs = _preemph_fault_pairs(predecessor_keeps_dc=True)
    assert _worst_ratio(pairs) > 1.0, pairs
    _report("pre-emphasis predecessor with its DC left in", pairs, [2e-3] * len(pairs), "max |d log-mel| < 2e-3")


def test_cmvn_bounds_stay_tight():
    """a CMVN row whose derived bound passed 1e-3 would have to be lengthened, not accepted"""
    f = R.floors()
    print("floors:", {k: "%.2e" % v for k, v in f.items()})
    for c in R.DELTA_CASES:
        assert R.bound(R.delta_kind(c.cmvn), R.delta_expected(c)[1]) < 1e-3, c.name
    for c in R.LOGMEL_CASES:
        for kind in ("int16", "float32"):
            assert R.bound(R.case_kind(c), R.logmel_expected(c, kind)[1]) < 1e-3, c.name
