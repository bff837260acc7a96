"""Reference and case table for every kernel variant of the audio front end (csrc/audio.hip, src/audio.py).

A plain numpy restatement of the chain with a `dtype` argument (float64: the reference; float32: the same operations
rounded to the device's number format, whose distance from the float64 run, e32, sets the tolerance):

    framing (snip_edges) -> per-frame DC removal (optional) -> pre-emphasis, first sample replicated -> povey window
    -> zero-padded real FFT (scipy.fft.rfft keeps float32) -> |X|^2 -> triangular mel weights between low_freq and
    high_freq -> log(max(., FLT_EPSILON)) [-> DCT-II + lifter for mfcc]
    -> delta with any filter bank (cross-correlation, zero padded in time) -> CMVN over time (unbiased std, eps added to
    the std) -> [T, C*D] layout, zero padded to the longest utterance of a batch.

It shares no code with src/audio.py; mel_banks, povey_window and delta_filters come from oracle/fbank_oracle.py.

CASES holds one row per kernel instantiation and edge; every row names the instantiation it is expected to select
(tests/test_audio_reference_cpu.py holds the rows to the dispatch, tests/test_audio_variants_gpu.py runs them).

Tolerance: per row, input kind and output kind e32 = max |float32 run - float64 run|; the device has to
be within max(8 * e32, floor) of the float64 run, element by element, floor = the largest e32 of that output kind over
the table.  Nothing here is a fixed number: bound() computes it from the reference.
"""
import functools
import warnings
from collections import namedtuple

import numpy as np
import scipy.fft

from oracle import fbank_oracle as FO

FLT_EPS = float(np.finfo(np.float32).eps)
LOG_FLOOR = float(np.log(FLT_EPS))
SHIFT_MS = 10.0
CMVN_EPS = 1e-10
FACTOR = 8.0


# ------------------------------------------------------------------------------------------------ the chain
def geometry(sr, frame_ms, shift_ms=SHIFT_MS):
    """-> (win, shift, N): samples per frame, hop, FFT size (next power of two)"""
    win, shift = int(sr * frame_ms * 0.001), int(sr * shift_ms * 0.001)
    n = 1
    while n < win:
        n *= 2
    return win, shift, n


def frame_count(n_samples, win, shift):
    return 0 if n_samples < win else 1 + (n_samples - win) // shift


def logmel(x, sr, nmel, frame_ms, preemph=0.97, remove_dc=True, low_freq=20.0, high_freq=0.0, dtype=np.float64,
           mel_w=None, replicate_first=True, predecessor_keeps_dc=False):
    """x: 1-D samples in [-1, 1) -> log-mel energies [m, nmel] computed in `dtype`.  The seeded faults of the CPU test:
    mel_w ([nmel, N/2 + 1]) replaces the mel weights, replicate_first=False takes the sample in front of a frame as 0,
    predecessor_keeps_dc=True pre-emphasises with a predecessor from which the frame's mean was not removed."""
    dt = np.dtype(dtype)
    x = np.asarray(x).astype(dt)
    win, shift, N = geometry(sr, frame_ms)
    m = frame_count(len(x), win, shift)
    if m == 0:
        return np.zeros((0, nmel), dt)
    fr = np.stack([x[i * shift:i * shift + win] for i in range(m)])
    mean = fr.mean(axis=1, keepdims=True, dtype=dt) if remove_dc else np.zeros((m, 1), dt)
    pred = fr - (np.zeros((m, 1), dt) if predecessor_keeps_dc else mean)
    fr = fr - mean
    first = pred[:, :1] if replicate_first else np.zeros_like(pred[:, :1])
    fr = fr - dt.type(preemph) * np.concatenate([first, pred[:, :-1]], axis=1)
    fr = fr * FO.povey_window(win).astype(dt)[None, :]
    spec = scipy.fft.rfft(fr, n=N, axis=1)
    assert spec.real.dtype == dt, spec.dtype
    power = spec.real ** 2 + spec.imag ** 2
    w = FO.mel_banks(nmel, N, sr, low_freq, high_freq) if mel_w is None else mel_w
    energy = power @ np.ascontiguousarray(w.T).astype(dt)
    out = np.log(np.maximum(energy, dt.type(FLT_EPS)))
    assert out.dtype == dt
    return out


def mel_energy(x, sr, nmel, frame_ms, **kw):
    """float64 mel energies in front of the clamp and the log (for the no-clamp condition)"""
    return np.exp(logmel(x, sr, nmel, frame_ms, dtype=np.float64, **kw))


def mfcc(mel, num_ceps=13, lifter=22.0, dtype=np.float64):
    """log-mel [m, nmel] -> cepstra [m, num_ceps]: orthonormal DCT-II (column 0 = sqrt(1/N)), lifter 1 + Q/2 sin(pi i/Q)"""
    dt = np.dtype(dtype)
    n = mel.shape[1]
    j, k = np.arange(n, dtype=np.float64)[:, None], np.arange(num_ceps, dtype=np.float64)[None, :]
    dct = np.sqrt(2.0 / n) * np.cos(np.pi * k * (2.0 * j + 1.0) / (2.0 * n))
    dct[:, 0] = np.sqrt(1.0 / n)
    if lifter:
        dct = dct * (1.0 + 0.5 * lifter * np.sin(np.pi * k / lifter))
    return np.asarray(mel).astype(dt) @ dct.astype(dt)


def delta(feat_td, filt, dtype=np.float64):
    """feat [T, D], filt [C, L] (L odd) -> [C, D, T]: y[c, d, t] = sum_j filt[c, j] feat[t + j - (L-1)/2, d], zero
    outside the utterance"""
    dt = np.dtype(dtype)
    x, f = np.asarray(feat_td).astype(dt), np.asarray(filt).astype(dt)
    (T, D), (C, L) = x.shape, f.shape
    half = (L - 1) // 2
    xp = np.concatenate([np.zeros((half, D), dt), x, np.zeros((half, D), dt)], axis=0)
    out = np.zeros((C, D, T), dt)
    for c in range(C):
        for j in range(L):
            out[c] += f[c, j] * xp[j:j + T].T
    return out


def cmvn(y_cdt, eps=CMVN_EPS, dtype=np.float64):
    """over time per (channel, feature): unbiased std, eps added to the std; T == 1 gives NaN as torch.std does"""
    dt = np.dtype(dtype)
    y = np.asarray(y_cdt).astype(dt)
    with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)            # T == 1: "degrees of freedom <= 0"
        mean = y.mean(axis=2, keepdims=True, dtype=dt)
        std = y.std(axis=2, ddof=1, keepdims=True, dtype=dt)
        return ((y - mean) / (dt.type(eps) + std)).astype(dt)


def features(feat_td, filt, apply_cmvn, dtype=np.float64):
    """[T, D] -> delta -> (CMVN) -> [T, C*D], feature index c * D + d"""
    y = delta(feat_td, filt, dtype)
    if apply_cmvn and y.shape[2] > 0:
        y = cmvn(y, dtype=dtype)
    C, D, T = y.shape
    return np.transpose(y, (2, 0, 1)).reshape(T, C * D)


def pad_batch(rows, width):
    """list of [m_b, width] -> [B, max m, width], zeros beyond each utterance (an utterance without a frame: a zero row)"""
    tmax = max(r.shape[0] for r in rows)
    out = np.zeros((len(rows), tmax, width), rows[0].dtype)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out


def max_err(a, ref):
    """max |a - ref| over EVERY element; NaN must sit exactly where the reference has it"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(a), nan), "NaN pattern differs from the reference's"
    assert np.all(np.isfinite(a[~nan])) and np.all(np.isfinite(ref[~nan]))
    return float(np.max(np.abs(a[~nan] - ref[~nan]))) if (~nan).any() else 0.0


# ------------------------------------------------------------------------------------------------ signals
def signal(n, sr, seed):
    """two tones at 0.0275 sr and 0.17 sr, noise, DC: every mel bin of every geometry below stays far above the clamp"""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(sr)
    return (0.3 * np.sin(2 * np.pi * 0.0275 * sr * t) + 0.2 * np.sin(2 * np.pi * 0.17 * sr * t + 1.0) +
            0.05 * rng.randn(n) + 0.02)


def to_pcm(x):
    return np.clip(np.round(np.asarray(x) * 32768.0), -32768, 32767).astype(np.int16)


# ------------------------------------------------------------------------------------------------ log-mel rows
# route: ('fused', log2n) | ('unfused', 'below' | 'above').  frames: frame count per utterance of the ragged batch
# (0 = an utterance of win - 1 samples); every batch has a 1-frame utterance, a 0-frame one in the middle and the
# longest not first.  opts: non-default fbank options.  seeds: one per utterance - the lowest mel bins hold only
# pre-emphasised noise (chi-square distributed per frame), so each seed was searched upwards from 0 until the utterance kept every
# mel energy above 2e3 * FLT_EPSILON (the table's condition asks for 1e3: no bin near the clamp, no element left out).
LogmelCase = namedtuple("LogmelCase", "name sr frame_ms nmel win N route frames opts feat_type seeds")

_OPTS = [dict(preemphasis_coefficient=0.0), dict(remove_dc_offset=False), dict(low_freq=100.0, high_freq=-400.0)]
_ALL_OPTS = dict(preemphasis_coefficient=0.0, remove_dc_offset=False, low_freq=100.0, high_freq=-400.0)


def _lm(sr, ms, nmel, win, N, route, frames, opts=None, feat_type="fbank", seeds=None):
    o = dict(opts or {})
    tag = "".join("-%s=%g" % (k.split("_")[0], v) for k, v in sorted(o.items()))
    name = "%s-%d-%gms-mel%d%s" % (feat_type, sr, ms, nmel, tag)
    seeds = tuple(seeds or range(len(frames)))
    assert len(seeds) == len(frames)
    return LogmelCase(name, sr, ms, nmel, win, N, route, tuple(frames), tuple(sorted(o.items())), feat_type, seeds)


LOGMEL_CASES = [
    _lm(16000, 16, 23, 256, 256, ("fused", 8), [1, 0, 6]),                 # win == N; ragged last workgroup
    _lm(8000, 25, 23, 200, 256, ("fused", 8), [3, 1, 0, 10, 2]),
    _lm(16000, 25, 40, 400, 512, ("fused", 9), [1, 9, 0, 10, 4], seeds=(0, 1, 2, 12, 3)),
    _lm(16000, 32, 80, 512, 512, ("fused", 9), [2, 0, 7, 1], seeds=(14, 0, 155, 2)),     # win == N; 7 frames
    _lm(16000, 40, 40, 640, 1024, ("fused", 10), [1, 0, 5]),               # 5 frames
    _lm(32000, 25, 80, 800, 1024, ("fused", 10), [4, 1, 0, 9, 8], seeds=(12, 2, 0, 155, 203)),
    _lm(16000, 64, 40, 1024, 1024, ("fused", 10), [1, 3, 0, 10]),          # win == N
    _lm(16000, 8, 13, 128, 128, ("unfused", "below"), [1, 0, 6]),          # win == N below the fused range
    _lm(4000, 25, 13, 100, 128, ("unfused", "below"), [2, 1, 0, 10, 3]),
    _lm(44100, 25, 40, 1102, 2048, ("unfused", "above"), [1, 0, 7, 4]),    # ldf 1104, nb 1028
] + [_lm(16000, 25, 40, 400, 512, ("fused", 9), [1, 0, 9, 5], o, seeds=(0, 1, 4, 6)) for o in _OPTS] \
  + [_lm(16000, 40, 40, 640, 1024, ("fused", 10), [2, 1, 0, 6], o) for o in _OPTS] \
  + [_lm(4000, 25, 13, 100, 128, ("unfused", "below"), [1, 0, 5], _ALL_OPTS),
     _lm(16000, 25, 23, 400, 512, ("fused", 9), [1, 0, 10, 3], None, "mfcc"),
     _lm(4000, 25, 13, 100, 128, ("unfused", "below"), [3, 0, 6, 1], None, "mfcc")]

GEOMETRIES = sorted({(c.sr, c.frame_ms, c.nmel) for c in LOGMEL_CASES})
NUM_CEPS = 13


def fbank_kwargs(case):
    """the case's options under the reference's own argument names"""
    o = dict(case.opts)
    return dict(preemph=o.get("preemphasis_coefficient", 0.97), remove_dc=o.get("remove_dc_offset", True),
                low_freq=o.get("low_freq", 20.0), high_freq=o.get("high_freq", 0.0))


def case_samples(case, m):
    shift = int(case.sr * SHIFT_MS * 0.001)
    return case.win - 1 if m == 0 else case.win + shift * (m - 1) + 3


@functools.lru_cache(maxsize=None)
def case_waves(case, kind):
    """kind 'int16': the quantised signals (the reference reads pcm / 32768 exactly); 'float32': the signals rounded to
    float32.  -> tuple of 1-D arrays, one per utterance (shared, never modified)"""
    out = []
    for b, m in enumerate(case.frames):
        x = signal(case_samples(case, m), case.sr, case.seeds[b])
        a = to_pcm(x) if kind == "int16" else x.astype(np.float32)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def as_float(w):
    """what the device is defined to read: int16 -> pcm / 32768 (exact in float32 and float64), float32 as it is"""
    return w.astype(np.float64) / 32768.0 if w.dtype == np.int16 else w.astype(np.float64)


def case_rows(case, kind, dtype, **fault):
    """per utterance [m, nmel or NUM_CEPS]: the row's output in `dtype`"""
    rows = []
    for w in case_waves(case, kind):
        y = logmel(as_float(w), case.sr, case.nmel, case.frame_ms, dtype=dtype, **dict(fbank_kwargs(case), **fault))
        if case.feat_type == "mfcc":
            y = mfcc(y, NUM_CEPS, 22.0, dtype)
        rows.append(y)
    return rows


def case_width(case):
    return case.nmel if case.feat_type == "fbank" else NUM_CEPS


def case_kind(case):
    return "logmel" if case.feat_type == "fbank" else "mfcc"


@functools.lru_cache(maxsize=None)
def logmel_expected(case, kind):
    """-> (float64 reference padded to [B, Tmax, width], e32)"""
    r64 = pad_batch(case_rows(case, kind, np.float64), case_width(case))
    r32 = pad_batch(case_rows(case, kind, np.float32), case_width(case))
    r64.setflags(write=False)
    return r64, max_err(r32, r64)


def logmel_instantiations(case):
    """what running the row per file, as an int16 batch and as a float32 batch reaches"""
    if case.route[0] == "fused":
        return {("logmel", "int16", case.route[1]), ("logmel", "float", case.route[1])}
    return {("unfused", case.route[1], form) for form in ("per_file", "batch_int16", "batch_float")}


# ------------------------------------------------------------------------------------------------ delta / CMVN rows
# driven through asrk_delta_cmvn_batch_f32 on random `mel`.  taps: (order, window) of the regression filters, or the
# hand-made 3-tap bank (asymmetric: a flipped or shifted tap index shows).  lt: the template instantiation the launch
# is expected to pick.  frames: per utterance; Tmax straddles the 128-frame stride of the kernel's time loop.
DeltaCase = namedtuple("DeltaCase", "name C L lt taps D cmvn frames")

HAND_TAPS = ((0.25, 1.0, -0.5), (-0.5, 0.125, 0.75))
_BANKS = [(1, 1, 1, (0, 2)), (2, 5, 5, (1, 2)), (3, 9, 9, (2, 2)), (2, 7, 9, (1, 3)), (2, 11, 16, (1, 5)),
          (3, 13, 16, (2, 3)), (2, 15, 16, (1, 7)), (2, 3, 5, "hand")]
DELTA_DS = [1, 63, 64, 65, 130]
DELTA_FRAMES = {129: (0, 1, 129, 0, 127, 2, 128, 0), 257: (0, 130, 1, 0, 257, 128, 0)}

DELTA_CASES = [DeltaCase("C%dL%d-D%d-cmvn%d-T%d" % (C, L, D, cm, tmax), C, L, lt, taps, D, cm, DELTA_FRAMES[tmax])
               for (C, L, lt, taps) in _BANKS for D in DELTA_DS for cm in (0, 1) for tmax in (129, 257)]

# the per-file modules Delta -> CMVN -> Postprocess at (order, window): L = 7, 11, 13, 15 and 17 (which the batch form refuses)
MODULE_PAIRS = [(1, 3), (1, 5), (2, 3), (1, 7), (2, 4)]
MODULE_T, MODULE_D = 130, 65

CASES = LOGMEL_CASES + DELTA_CASES


def lt_class(L):
    return 1 if L == 1 else 5 if L <= 5 else 9 if L <= 9 else 16


def filter_bank(taps, dtype=np.float64):
    f = np.asarray(HAND_TAPS, np.float64) if taps == "hand" else FO.delta_filters(taps[0], taps[1])
    return f.astype(dtype)


@functools.lru_cache(maxsize=None)
def delta_inputs(case):
    """-> (mel float32 [sum m, D], filters float32 [C, L]): the launch's inputs, which the reference reads as data"""
    rng = np.random.RandomState(7 + DELTA_CASES.index(case))
    mel = rng.randn(sum(case.frames), case.D).astype(np.float32)
    filt = filter_bank(case.taps, np.float32)
    assert filt.shape == (case.C, case.L)
    mel.setflags(write=False)
    filt.setflags(write=False)
    return mel, filt


def delta_batch(mel, filt, frames, apply_cmvn, dtype):
    offs = np.concatenate([[0], np.cumsum(frames)])
    rows = [features(mel[offs[b]:offs[b + 1]], filt, apply_cmvn, dtype) for b in range(len(frames))]
    return pad_batch(rows, filt.shape[0] * mel.shape[1])


def delta_kind(apply_cmvn):
    return "normalised" if apply_cmvn else "delta"


@functools.lru_cache(maxsize=None)
def delta_expected(case, dropped_tap=None):
    """-> (float64 reference [B, Tmax, C*D], e32).  dropped_tap=(c, j) zeroes one tap: a seeded fault"""
    mel, filt = delta_inputs(case)
    if dropped_tap is not None:
        filt = filt.copy()
        filt[dropped_tap] = 0.0
    r64 = delta_batch(mel, filt, case.frames, case.cmvn, np.float64)
    r32 = delta_batch(mel, filt, case.frames, case.cmvn, np.float32)
    r64.setflags(write=False)
    return r64, max_err(r32, r64)


def module_input():
    x = np.random.RandomState(99).randn(MODULE_T, MODULE_D).astype(np.float32)       # [T, D]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def module_expected(order, window, apply_cmvn):
    """the per-file chain on module_input(): float64 reference [T, C*D] with the regression filters in float64, e32"""
    x, filt = module_input(), FO.delta_filters(order, window)
    r64 = features(x, filt, apply_cmvn, np.float64)
    return r64, max_err(features(x, filt, apply_cmvn, np.float32), r64)


# ------------------------------------------------------------------------------------------------ the bound
@functools.lru_cache(maxsize=None)
def floors():
    """output kind -> the largest e32 of that kind over the table"""
    f = dict(logmel=0.0, mfcc=0.0, delta=0.0, normalised=0.0)
    for c in LOGMEL_CASES:
        for kind in ("int16", "float32"):
            f[case_kind(c)] = max(f[case_kind(c)], logmel_expected(c, kind)[1])
    for c in DELTA_CASES:
        f[delta_kind(c.cmvn)] = max(f[delta_kind(c.cmvn)], delta_expected(c)[1])
    for order, window in MODULE_PAIRS:
        for cm in (0, 1):
            f[delta_kind(cm)] = max(f[delta_kind(cm)], module_expected(order, window, cm)[1])
    return f


def bound(kind, e32):
    return max(FACTOR * e32, floors()[kind])


def all_instantiations():
    s = set()
    for c in LOGMEL_CASES:
        s |= logmel_instantiations(c)
    return s | {("delta_cmvn", c.lt) for c in DELTA_CASES}
