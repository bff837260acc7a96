"""Float64 reference of SpecAugment (shared by tests/test_specaug_cpu.py, tests/test_specaug_gpu.py and
tests/specaug_worker.py), written from the formulas of the specification (include/asrk.h, asrk_spec_augment_f32), with
plain Python integers wherever an index is computed - never from the code under test.

reference(x, lens, params, D, C, n_fmask, n_tmask, fill) walks every (utterance, frame) and returns, per cell of the
first C*D columns: the expected value in float64, its class (FILL / COPY / BLEND), the frame it must be a bit-copy of
(COPY) and the magnitude max(|x_i|, |x_j|) the tolerance of a BLEND cell scales with."""
import numpy as np

FILL, COPY, BLEND = 0, 1, 2
# one rounding each for a, 1 - a, two products and a sum (contracted to an FMA or not), doubled
BLEND_TOL = 8.0 * 2.0 ** -24


def warp_source(t, n, c, w):
    """-> (i, j, r, den) of output frame t < n; den = 1, r = 0, i = j = t when the warp is not active"""
    t, n, c, w = int(t), int(n), int(c), int(w)
    d = c + w
    if not (w != 0 and 0 < c < n - 1 and 0 < d < n - 1):
        return t, t, 0, 1
    if t <= d:
        num, den = t * c, d
    else:
        num, den = c * (n - 1 - d) + (t - d) * (n - 1 - c), n - 1 - d
    i, r = num // den, num % den
    return i, min(i + 1, n - 1), r, den


def reference(x, lens, params, D, C, n_fmask, n_tmask, fill):
    x = np.asarray(x)
    B, T, _ = x.shape
    CD = C * D
    params = np.asarray(params).reshape(B, 2 + 2 * n_fmask + 2 * n_tmask)
    val = np.zeros((B, T, CD), dtype=np.float64)
    kind = np.full((B, T, CD), COPY, dtype=np.int8)
    src = np.zeros((B, T), dtype=np.int64)
    mag = np.zeros((B, T, CD), dtype=np.float64)
    mel = np.arange(CD) % D
    for b in range(B):
        n = min(max(int(lens[b]), 0), T)
        row = [int(v) for v in params[b]]
        fm = np.zeros(CD, dtype=bool)
        for k in range(n_fmask):
            f0, fw = row[2 + 2 * k], row[3 + 2 * k]
            if fw > 0:
                fm |= (mel >= f0) & (mel < f0 + fw)
        for t in range(T):
            if t >= n:                                    # padding: copied, no mask
                val[b, t], src[b, t] = x[b, t, :CD], t
                continue
            tm = False
            for k in range(n_tmask):
                t0, tw = row[2 + 2 * n_fmask + 2 * k], row[3 + 2 * n_fmask + 2 * k]
                tm = tm or (tw > 0 and t0 <= t < t0 + tw)
            i, j, r, den = warp_source(t, n, row[0], row[1])
            assert 0 <= i <= j <= n - 1, (t, n, row[:2], i, j)
            xi, xj = x[b, i, :CD].astype(np.float64), x[b, j, :CD].astype(np.float64)
            src[b, t] = i
            if r == 0:
                val[b, t] = xi
            else:
                a = r / den
                val[b, t] = (1.0 - a) * xi + a * xj
                kind[b, t] = BLEND
                mag[b, t] = np.maximum(np.abs(xi), np.abs(xj))
            if tm:
                kind[b, t], val[b, t] = FILL, fill
            else:
                kind[b, t, fm], val[b, t, fm] = FILL, fill
    return val, kind, src, mag


def check(y, x, lens, params, D, C, n_fmask, n_tmask, fill, sentinel=None):
    """the criterion: FILL cells equal `fill` exactly, COPY cells (r == 0, and every frame t >= n) are bit-equal to
    their source frame, BLEND cells are within BLEND_TOL * max(|x_i|, |x_j|) of float64; columns >= C*D keep `sentinel`.
    Returns the largest BLEND error in units of its bound (for printing)."""
    y, x = np.asarray(y, dtype=np.float32), np.asarray(x, dtype=np.float32)
    B, T, ld = x.shape
    CD = C * D
    val, kind, src, mag = reference(x, lens, params, D, C, n_fmask, n_tmask, fill)
    yc = y[:, :, :CD]
    m = kind == FILL
    assert np.array_equal(yc[m], np.full(int(m.sum()), np.float32(fill))), "masked cells differ from fill"
    gathered = np.take_along_axis(x[:, :, :CD], src[:, :, None].repeat(CD, axis=2), axis=1)
    m = kind == COPY
    assert np.array_equal(yc[m].view(np.uint32), gathered[m].view(np.uint32)), "copied cells are not bit-equal"
    m = kind == BLEND
    worst = 0.0
    if m.any():
        err = np.abs(yc[m].astype(np.float64) - val[m])
        bound = BLEND_TOL * mag[m]
        over = err > bound
        assert not over.any(), "blend error %g above bound %g" % (err[over].max(), bound[over].min())
        nz = bound > 0
        worst = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    if sentinel is not None and ld > CD:
        assert np.array_equal(y[:, :, CD:], np.full((B, T, ld - CD), np.float32(sentinel))), "stray columns written"
    return worst
