"""Reference and case table of the reverberation / noise entry (include/asrk.h: asrk_reverb_mix_f32).

reverb_mix() restates the header's formulas with a `dtype` argument and shares no code with the kernel or with ops:

    s[i] = x[i] * scale (0 outside 0..n-1);  y[i] = sum_{k<K} h[k] s[i + p - k]  (y = s without a response)
    Ps = sum s^2, Py = sum y^2, Pv = sum v_i^2 over i < n, v_i = v[i mod m] * scale
    a = sqrt(Ps / Py) (response and Py > 0, else 1);  g = sqrt(Ps / (Pv snr_lin)) (m > 0, Pv > 0, Ps > 0, else 0)
    out[i] = a y[i] + g v_i

float64: the reference, one dot product per output sample.  float32: the same operations rounded to the device's
number format - products and sums of the filter in f32, tap after tap in ascending k; the three powers in float64 of
the f32 values; a and g rounded to f32; two f32 products and one f32 sum per output.  Its distance from the float64 run,
e32, sets the tolerance as in tests/audio_reference.py: the device has to be within max(FACTOR * e32, floor) of the
float64 run, element by element, floor = the largest e32 of the table.  Nothing here is a fixed number.

The seeded faults of the CPU test (`fault=`): 'tap' drops one tap, 'peak' shifts the output by one sample, 'wrap' tiles
the noise with a period one short, 'snr' takes snr_lin for the amplitude ratio.
"""
import functools
from collections import namedtuple

import numpy as np

from audio_reference import FACTOR

TILE = 2048          # RM_TILE of csrc/reverb_mix.hip: outputs per workgroup, one partial sum each
CHUNK = 384          # RM_KC: taps per staged chunk
MAX_TAPS = 8192


def reverb_mix(x, scale, h, p, v, snr_lin, dtype=np.float64, fault=None, parts=False):
    """x [n] int16 or float32; h [K] float32 or None; p: the peak; v [m] of x's type or None; -> out [n] in `dtype`
    (parts: -> (out, a * y, g * v_i), the two terms apart)"""
    dt = np.dtype(dtype)
    n = len(x)
    s = np.asarray(x).astype(dt) * dt.type(np.float32(scale))
    if h is None:
        y = s.copy()
    else:
        hh = np.asarray(h, dtype=np.float32).astype(dt)
        K = len(hh)
        if fault == 'tap':
            hh = hh.copy()
            hh[K // 2] = 0
        if fault == 'peak':
            p = p + 1
        pad = np.concatenate([np.zeros(K + 1, dt), s, np.zeros(K + 1, dt)])     # pad[K + 1 + j] = s[j]
        if dt == np.float64:
            y = np.zeros(n, dt)
            for i in range(n):
                lo = K + 1 + i + p - (K - 1)                                    # s[i + p - k], k = K-1 .. 0
                y[i] = np.dot(hh[::-1], pad[lo:lo + K])
        else:
            y = np.zeros(n, dt)
            for k in range(K):
                lo = K + 1 + p - k
                y = y + hh[k] * pad[lo:lo + n]
            assert y.dtype == dt
    m = 0 if v is None else len(v)
    if m > 0:
        period = m - 1 if (fault == 'wrap' and m > 1) else m
        vi = np.asarray(v).astype(dt)[np.arange(n) % period] * dt.type(np.float32(scale))
    else:
        vi = np.zeros(n, dt)
    Ps = float(np.sum(s.astype(np.float64) ** 2))
    Py = float(np.sum(y.astype(np.float64) ** 2))
    Pv = float(np.sum(vi.astype(np.float64) ** 2))
    a = np.sqrt(Ps / Py) if (h is not None and Py > 0.0) else 1.0
    snr = float(np.float32(snr_lin))
    if fault == 'snr':
        snr = snr * snr
    g = np.sqrt(Ps / (Pv * snr)) if (m > 0 and Pv > 0.0 and Ps > 0.0) else 0.0
    a, g = dt.type(a), dt.type(g)
    out = a * y + g * vi if g != 0 else a * y
    assert out.dtype == dt
    return (out, a * y, g * vi) if parts else out


def wrap_indices(n, m):
    """the noise sample every output reads"""
    return np.arange(n) % m


# ------------------------------------------------------------------------------------------------ the table
Row = namedtuple("Row", "n K peak m kind")       # K = 0: no response; peak: 'first' | 'mid' | 'last'; m = 0: no noise
Case = namedtuple("Case", "name dtype pad rows")  # pad: ld_out = roundup4(max n) + pad


def _r(n, K, peak='mid', m=0, kind=''):
    return Row(n, K, peak, m, kind)


CASES = [
    Case("short-i16", "int16", 0, [_r(0, 1, 'first', 0), _r(1, 1, 'first', 1), _r(2, 2, 'last', 7),
                                   _r(255, 63, 'mid', 254), _r(256, 64, 'first', 256), _r(257, 65, 'last', 258)]),
    Case("mid-f32-odd", "float32", 1, [_r(1023, 255, 'mid', 7), _r(1025, 257, 'first', 0), _r(2049, 1025, 'last', 2048),
                                       _r(4099, 1025, 'mid', 1), _r(300, 8192, 'mid', 299)]),
    Case("tile-i16-odd", "int16", 3, [_r(TILE - 1, CHUNK - 1, 'mid', TILE - 1), _r(TILE, CHUNK, 'first', TILE + 1),
                                      _r(TILE + 1, CHUNK + 1, 'last', 7), _r(4099, 64, 'mid', 0), _r(1023, 0, 'mid', 0)]),
    Case("special-f32", "float32", 0, [_r(257, 65, 'mid', 100, 'zero-x'), _r(1025, 255, 'mid', 1025, 'zero-v'),
                                       _r(2049, 0, 'mid', 0), _r(2049, 257, 'mid', 1000), _r(300, 8192, 'last', 0)]),
    Case("long-i16", "int16", 0, [_r(300, 8192, 'first', 300), _r(4099, 2, 'first', 4098), _r(1023, 0, 'mid', 1024),
                                  _r(255, 1, 'first', 0), _r(TILE + 2, CHUNK + 11, 'mid', 4100),
                                  _r(2 * TILE + 1, 2 * CHUNK + 1, 'mid', 2 * TILE)]),
    Case("lone-f32-odd", "float32", 2, [_r(2, 63, 'last', 2), _r(0, 0, 'mid', 0), _r(1, 0, 'mid', 7)]),
]
SNR_DB = (0.0, 5.0, 10.0, 20.0, -3.0, 15.0)


def peak_index(K, peak):
    return {'first': 0, 'mid': K // 2, 'last': K - 1}[peak]


@functools.lru_cache(maxsize=None)
def case_data(ci):
    """-> list of per-row dicts (x, scale, h, p, v, snr_lin) of CASES[ci]; shared, never modified"""
    case = CASES[ci]
    rng = np.random.default_rng(1000 + ci)
    rows = []
    for b, r in enumerate(case.rows):
        t = np.arange(r.n) / 16000.0
        x = 0.3 * np.sin(2 * np.pi * (200.0 + 37.0 * b) * t) + 0.2 * rng.standard_normal(r.n)
        nz = 0.25 * rng.standard_normal(r.m)
        if r.kind == 'zero-x':
            x[:] = 0.0
        if r.kind == 'zero-v':
            nz[:] = 0.0
        if case.dtype == "int16":
            x = np.clip(np.round(x * 16384.0), -32768, 32767).astype(np.int16)
            nz = np.clip(np.round(nz * 16384.0), -32768, 32767).astype(np.int16)
            scale = 1.0 / 32768.0
        else:
            x, nz, scale = x.astype(np.float32), nz.astype(np.float32), 1.0
        h, p = None, 0
        if r.K > 0:
            p = peak_index(r.K, r.peak)
            h = rng.standard_normal(r.K) * np.exp(-np.abs(np.arange(r.K) - p) / max(r.K / 6.0, 1.0)) * 0.3
            h[p] = 1.0 if b % 2 == 0 else -1.0
            h = h.astype(np.float32)
            assert int(np.argmax(np.abs(h))) == p
        snr_db = SNR_DB[(b + ci) % len(SNR_DB)]
        rows.append(dict(x=x, scale=scale, h=h, p=p, v=nz if r.m > 0 else None,
                         snr_lin=float(np.float32(10.0 ** (snr_db / 10.0))), snr_db=snr_db))
    return rows


@functools.lru_cache(maxsize=None)
def expected(ci, b, dtype="float64", fault=None):
    d = case_data(ci)[b]
    return reverb_mix(d['x'], d['scale'], d['h'], d['p'], d['v'], d['snr_lin'], dtype=np.dtype(dtype), fault=fault)


def all_rows():
    return [(ci, b) for ci, c in enumerate(CASES) for b in range(len(c.rows))]


def max_err(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape
    return float(np.abs(a - ref).max()) if a.size else 0.0


@functools.lru_cache(maxsize=None)
def e32(ci, b):
    return max_err(expected(ci, b, "float32"), expected(ci, b, "float64"))


@functools.lru_cache(maxsize=None)
def floor():
    return max(e32(ci, b) for ci, b in all_rows())


def bound(ci, b):
    return max(FACTOR * e32(ci, b), floor())
