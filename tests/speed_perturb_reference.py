"""Float64 reference of the speed-perturbation resampler (asrk_resample_rows_f32), written from the formulas of the
specification - torchaudio's sinc_interp_hann resampler with lowpass_filter_width 6 and rolloff 0.99 - with a direct
convolution loop per output sample.  Independent of csrc/resample.hip and of ops.resample_taps."""
import math

import numpy as np

W = 6
ROLLOFF = 0.99


def geometry(orig, new):
    """-> (base, width, taps)"""
    base = min(orig, new) * ROLLOFF
    width = int(math.ceil(W * orig / base))
    return base, width, 2 * width + orig


def taps_table(orig, new):
    """h [new, 2*width + orig] in float64"""
    base, width, taps = geometry(orig, new)
    h = np.zeros((new, taps), dtype=np.float64)
    for j in range(new):
        for k in range(taps):
            t = (-j / new + (k - width) / orig) * base
            t = min(max(t, -W), W)
            s = 1.0 if t == 0.0 else math.sin(math.pi * t) / (math.pi * t)
            h[j, k] = s * math.cos(math.pi * t / (2 * W)) ** 2 * base / orig
    return h


def out_samples(n, orig, new):
    return (new * n + orig - 1) // orig


def resample(x, orig, new, scale=1.0):
    """x: 1-D array of n samples -> float64 [n_out]; ratio (1, 1) is x * scale"""
    x = np.asarray(x, dtype=np.float64) * scale
    n = x.shape[0]
    if (orig, new) == (1, 1):
        return x.copy()
    _, width, taps = geometry(orig, new)
    h = taps_table(orig, new)
    pad = np.concatenate([np.zeros(width), x, np.zeros(taps + orig)])       # pad[width + m] = x[m]
    n_out = out_samples(n, orig, new)
    y = np.zeros(n_out, dtype=np.float64)
    for o in range(n_out):
        i, j = divmod(o, new)
        y[o] = np.dot(h[j], pad[i * orig:i * orig + taps])                  # x[i*orig + k - width], k = 0..taps-1
    return y


def error_bound(orig, new, max_abs_x):
    """|kernel - resample| allowed per sample: 2 * taps * 2^-24 * max_j sum_k |h[j][k]| * max |x * scale| - the f32
    accumulation bound (taps roundings of relative size 2^-24 on partial sums no larger than sum |h| max |x|) plus the
    rounding of the table to f32 (one more 2^-24 per tap)"""
    h = np.abs(taps_table(orig, new))
    return 2.0 * h.shape[1] * 2.0 ** -24 * h.sum(axis=1).max() * max_abs_x
