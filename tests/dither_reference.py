"""Reference of the dithered filterbank front end (include/asrk.h "Dither"; csrc/audio.hip DITHER instantiations).

A numpy restatement with a `dtype` argument, in the style of tests/audio_reference.py (float64: the reference; float32:
the same operations rounded to the device's number format, whose distance from the float64 run, e32, sets the
tolerance):

    noise      z(key, f, j) = Box-Muller of the words of Philox4x32-10(counter (j >> 2, f, 0, 0), key); the Philox rounds
               are oracle/regularizer_oracle.philox4x32_10 (checked there against the paper's vectors)
    framing    v[f][j] = x[f * shift + j] + dither * z(key, f, j)            (snip_edges; per frame AND position)
    then       audio_reference.logmel's steps on v: per-frame DC removal -> pre-emphasis with the replicated v[f][0] ->
               povey window -> zero-padded real FFT -> |X|^2 -> mel weights -> log(max(., FLT_EPSILON)) [-> mfcc]

With dither 0 logmel() below is audio_reference.logmel bit for bit (tests/test_dither_cpu.py holds them together).  It
shares no code with src/audio.py.  The seeded faults of the CPU test: fault='none' (no noise), 'key' (another key),
'per_sample' (one noise value per waveform sample, what dithering the waveform instead of the frames would give).

Tolerance: bound(kind, e32) = max(8 * e32, audio_reference.floors()[kind]); nothing is a fixed number.
"""
import functools
from collections import namedtuple

import numpy as np
import scipy.fft

import audio_reference as R
from oracle import fbank_oracle as FO
from oracle import regularizer_oracle as RO

Z_MAX = float(np.sqrt(48.0 * np.log(2.0)))           # u1 >= 2^-24


def noise(key, m, win, dtype=np.float64):
    """-> z [m, win] in `dtype`: the noise of frames 0..m-1, positions 0..win-1 under the 64-bit `key`"""
    dt = np.dtype(dtype)
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    ng = (win + 3) // 4
    if m == 0:
        return np.zeros((0, win), dt)
    f = np.repeat(np.arange(m, dtype=np.uint32), ng)
    g = np.tile(np.arange(ng, dtype=np.uint32), m)
    ctr = np.stack([g, f, np.zeros_like(g), np.zeros_like(g)], axis=1)
    r = RO.philox4x32_10(ctr, (key & 0xFFFFFFFF, key >> 32))                  # [m * ng, 4] uint32
    z = np.empty((m * ng, 4), dt)
    two_pi = dt.type(2.0 * np.pi)
    for p in range(2):
        u1 = ((r[:, 2 * p] >> np.uint32(8)).astype(np.int64) + 1).astype(dt) * dt.type(2.0 ** -24)
        u2 = (r[:, 2 * p + 1] >> np.uint32(8)).astype(dt) * dt.type(2.0 ** -24)
        rad = np.sqrt(dt.type(-2.0) * np.log(u1))
        ang = two_pi * u2
        z[:, 2 * p], z[:, 2 * p + 1] = rad * np.cos(ang), rad * np.sin(ang)
    assert z.dtype == dt
    return z.reshape(m, 4 * ng)[:, :win]


def logmel(x, sr, nmel, frame_ms, dither=0.0, key=0, preemph=0.97, remove_dc=True, low_freq=20.0, high_freq=0.0,
           dtype=np.float64, fault=None):
    """x: 1-D samples in [-1, 1) -> log-mel energies [m, nmel] of the dithered frames, computed in `dtype`"""
    dt = np.dtype(dtype)
    x = np.asarray(x).astype(dt)
    win, shift, N = R.geometry(sr, frame_ms)
    m = R.frame_count(len(x), win, shift)
    if m == 0:
        return np.zeros((0, nmel), dt)
    fr = np.stack([x[i * shift:i * shift + win] for i in range(m)])
    if dither and fault != "none":
        if fault == "per_sample":
            zs = noise(key, 1, len(x), dt)[0]
            z = np.stack([zs[i * shift:i * shift + win] for i in range(m)])
        else:
            z = noise(key ^ 1 if fault == "key" else key, m, win, dt)
        fr = fr + dt.type(dither) * z
    mean = fr.mean(axis=1, keepdims=True, dtype=dt) if remove_dc else np.zeros((m, 1), dt)
    fr = fr - mean
    fr = fr - dt.type(preemph) * np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = fr * FO.povey_window(win).astype(dt)[None, :]
    spec = scipy.fft.rfft(fr, n=N, axis=1)
    assert spec.real.dtype == dt, spec.dtype
    power = spec.real ** 2 + spec.imag ** 2
    w = FO.mel_banks(nmel, N, sr, low_freq, high_freq)
    energy = power @ np.ascontiguousarray(w.T).astype(dt)
    out = np.log(np.maximum(energy, dt.type(R.FLT_EPS)))
    assert out.dtype == dt
    return out


def mel_energy(x, sr, nmel, frame_ms, **kw):
    """float64 mel energies in front of the clamp and the log (for the no-clamp condition)"""
    return np.exp(logmel(x, sr, nmel, frame_ms, dtype=np.float64, **kw))


# ------------------------------------------------------------------------------------------------ rows
# One geometry per framing instantiation (route as in audio_reference); every batch is ragged with an utterance without a
# frame and idle waves in the last workgroup of each utterance (a workgroup holds 4 frames).
Case = namedtuple("Case", "name sr frame_ms nmel win N route frames opts feat_type")
FRAMES = (3, 0, 7, 1)
KEYS = (0x9E3779B97F4A7C15, 5, (1 << 40) + 7, 0xFFFFFFFF00000001)      # distinct; three of them above 2^32
DITHERS = (2.0 ** -9, 2.0 ** -6)


def _case(sr, ms, nmel, route, opts=None, feat_type="fbank", frames=FRAMES):
    win, _, N = R.geometry(sr, ms)
    o = dict(opts or {})
    tag = "".join("-%s=%g" % (k.split("_")[0], v) for k, v in sorted(o.items()))
    return Case("%s-%d-%gms-mel%d%s" % (feat_type, sr, ms, nmel, tag), sr, ms, nmel, win, N, route, tuple(frames),
                tuple(sorted(o.items())), feat_type)


GEOMETRIES = [
    _case(8000, 25, 23, ("fused", 8)),
    _case(16000, 25, 40, ("fused", 9)),
    _case(16000, 32, 80, ("fused", 9)),                   # win == N
    _case(16000, 40, 40, ("fused", 10)),
    _case(4000, 25, 13, ("unfused", "below")),
    _case(44100, 25, 40, ("unfused", "above")),
]
EXTRA = [
    _case(16000, 25, 23, ("fused", 9), None, "mfcc"),
    _case(4000, 25, 13, ("unfused", "below"), None, "mfcc"),
    _case(16000, 25, 40, ("fused", 9), dict(remove_dc_offset=False, preemphasis_coefficient=0.0)),
    _case(4000, 25, 13, ("unfused", "below"), dict(remove_dc_offset=False, preemphasis_coefficient=0.0)),
]
CASES = GEOMETRIES + EXTRA


def case_kwargs(case):
    o = dict(case.opts)
    return dict(preemph=o.get("preemphasis_coefficient", 0.97), remove_dc=o.get("remove_dc_offset", True))


@functools.lru_cache(maxsize=None)
def case_waves(case, kind):
    """kind 'int16' | 'float32' -> one 1-D array per utterance (shared, never modified): audio_reference.signal"""
    out = []
    for b, m in enumerate(case.frames):
        x = R.signal(R.case_samples(case, m), case.sr, 20 + b)
        a = R.to_pcm(x) if kind == "int16" else x.astype(np.float32)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def rows(waves, case, dither, keys, dtype, fault=None):
    """per utterance [m, width]: the case's output in `dtype` for these waveforms (as the device reads them) and keys"""
    out = []
    for w, k in zip(waves, keys):
        y = logmel(R.as_float(w), case.sr, case.nmel, case.frame_ms, dither=dither, key=k, dtype=dtype, fault=fault,
                   **case_kwargs(case))
        if case.feat_type == "mfcc":
            y = R.mfcc(y, R.NUM_CEPS, 22.0, dtype)
        out.append(y)
    return out


@functools.lru_cache(maxsize=None)
def expected(case, kind, dither, fault=None):
    """-> (float64 reference padded to [B, Tmax, width], e32) under KEYS"""
    waves, width = case_waves(case, kind), R.case_width(case)
    r64 = R.pad_batch(rows(waves, case, dither, KEYS, np.float64, fault), width)
    r32 = R.pad_batch(rows(waves, case, dither, KEYS, np.float32, fault), width)
    r64.setflags(write=False)
    return r64, R.max_err(r32, r64)


def bound(kind, e32):
    return R.bound(kind, e32)


@functools.lru_cache(maxsize=None)
def noise_e32(key, m, win):
    """max |float32 noise - float64 noise| of these frames"""
    return R.max_err(noise(key, m, win, np.float32), noise(key, m, win, np.float64))
