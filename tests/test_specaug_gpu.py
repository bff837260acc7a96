"""GPU: asrk_spec_augment_f32 / ops.spec_augment / SpecAugment against the float64 reference of
tests/specaug_reference.py (a numpy loop written from the specification), on the element path (ld = 15), the 16-byte
vector path (ld = 120) and with stray columns behind the features (ld = 128); then the solver with and without a
`specaug:` block on the miniature wav corpus of tests/test_e2e_gpu.py.

Criterion (specaug_reference.check): masked cells equal `fill` exactly; cells with r == 0 and every frame t >= n are
bit-equal to the input; every other cell is within 8 * 2^-24 * max(|x_i|, |x_j|) of float64."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from specaug_reference import BLEND_TOL, check, warp_source

pytestmark = pytest.mark.gpu
PKG = "end-to-end-asr-pytorch_amd"
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 777.0
W = 5           # time_warp of the hand-written and the sampled tables: admissible from n = 12

# name -> (B, T, D, C, ld, lens)
SHAPES = {
    "element": (3, 37, 5, 3, 15, [37, 20, 2]),
    "vector": (2, 70, 40, 3, 120, [70, 51]),
    "padcols": (2, 37, 40, 3, 128, [37, 25]),
    "wide": (1, 33, 301, 1, 301, [29]),          # more columns than threads in a workgroup
}


def _input(name):
    B, T, D, C, ld, lens = SHAPES[name]
    rng = np.random.default_rng(B * 1000 + T + ld)
    x = rng.standard_normal((B, T, ld)).astype(np.float32) * 3.0
    for b, n in enumerate(lens):                  # zero padding behind each utterance, as the collate function leaves it
        x[b, n:] = 0.0
    return x


def _run_abi(ops, x, lens, params, D, C, nf, nt, fill, misalign=False):
    """the C entry point itself, so that ld > C*D and a pre-filled y can be given; -> y as numpy"""
    L = importlib.import_module(PKG + "._lib")
    B, T, ld = x.shape
    if misalign:                                  # 4 bytes off a 16-byte boundary: the element path on vector-shaped rows
        xs = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")[1:].view(B, T, ld)
        ys = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")[1:].view(B, T, ld)
        assert xs.data_ptr() % 16 == 4 and ys.data_ptr() % 16 == 4
    else:
        xs = torch.empty((B, T, ld), dtype=torch.float32, device="cuda")
        ys = torch.empty((B, T, ld), dtype=torch.float32, device="cuda")
    xs.copy_(torch.from_numpy(x))
    ys.fill_(SENTINEL)
    lg = torch.tensor(lens, dtype=torch.int64, device="cuda")
    pg = torch.tensor(params, dtype=torch.int32, device="cuda").reshape(B, 2 + 2 * nf + 2 * nt).contiguous()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.load().asrk_spec_augment_f32(p(xs), p(ys), B, T, ld, D, C, p(lg), p(pg), nf, nt, float(fill), ops._stream())
    L.check(rc, "spec_augment")
    torch.cuda.synchronize()
    return ys.cpu().numpy()


def _warp_rows(lens, low_c, sign):
    """(c, w) per utterance: c at the low or the high end of U{W..n-1-W}, w = +-(W-1); zeros where n < 2W + 2"""
    return [[(W if low_c else n - 1 - W), sign * (W - 1)] if n >= 2 * W + 2 else [0, 0] for n in lens]


def _mask_rows(lens, D):
    """4 frequency + 4 time masks per utterance: two that overlap, one of zero width, one that runs over the end"""
    rows = []
    for n in lens:
        f = [1, 2, 2, 2, 3, 0, D - 1, 4]                                   # [1,3) u [2,4), nothing, [D-1, D+3) clipped
        t = [3, 5, 6, 4, 5, 0, n - 2, 7]                                   # [3,8) u [6,10), nothing, [n-2, n+5) clipped
        rows.append(f + t)
    return rows


def _tables(lens, D):
    zero2 = [[0, 0] for _ in lens]
    masks = _mask_rows(lens, D)
    cases = {
        "zero": (zero2, 0, 0, 0.0),
        "warp_low_c_forward": (_warp_rows(lens, True, +1), 0, 0, 0.0),
        "warp_low_c_backward": (_warp_rows(lens, True, -1), 0, 0, 0.0),
        "warp_high_c_forward": (_warp_rows(lens, False, +1), 0, 0, 0.0),
        "warp_high_c_backward": (_warp_rows(lens, False, -1), 0, 0, 0.0),
        "masks": ([z + m for z, m in zip(zero2, masks)], 4, 4, -1.5),
        "all": ([w + m for w, m in zip(_warp_rows(lens, True, -1), masks)], 4, 4, 0.25),
        # entries no sampler would produce: the kernel ignores or clips them, whatever they are
        "untrusted": ([[2 ** 31 - 1, -2 ** 31, -7, 9, 2 ** 31 - 1, 2 ** 31 - 1, -5, 2 ** 31 - 1, 2, -3]
                       for _ in lens], 2, 2, 2.0),
    }
    return cases


CASES = ["zero", "warp_low_c_forward", "warp_low_c_backward", "warp_high_c_forward", "warp_high_c_backward", "masks",
         "all", "untrusted"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_hand_written_tables(ops, shape, case):
    B, T, D, C, ld, lens = SHAPES[shape]
    x = _input(shape)
    params, nf, nt, fill = _tables(lens, D)[case]
    y = _run_abi(ops, x, lens, params, D, C, nf, nt, fill)
    worst = check(y, x, lens, params, D, C, nf, nt, fill, sentinel=SENTINEL)
    print("%s/%s: worst blend error = %.3f of the bound" % (shape, case, worst))
    if case == "zero":
        assert np.array_equal(y[:, :, :C * D].view(np.uint32), x[:, :, :C * D].view(np.uint32))
    if case == "untrusted":                      # the mask over every frame and the one over bins [-7, 2) are applied
        for b, n in enumerate(lens):
            assert np.all(y[b, :n, :C * D] == np.float32(2.0)) and np.array_equal(y[b, n:, :C * D], x[b, n:, :C * D])


def test_short_utterances(ops):
    """n = 1 and n = 2: nothing to warp (table entries are ignored), masks still apply"""
    B, T, D, C, ld, _ = SHAPES["element"]
    lens = [1, 2, 37]
    x = _input("element")
    params = [[1, 1, 1, 2, 0, 1], [1, -1, 0, 1, 1, 1], [5, 4, 4, 1, 36, 1]]
    y = _run_abi(ops, x, lens, params, D, C, 1, 1, 9.0)
    check(y, x, lens, params, D, C, 1, 1, 9.0, sentinel=SENTINEL)
    assert np.all(y[0, 0] == 9.0) and np.all(y[1, 1] == 9.0)
    assert np.array_equal(y[1, 0, [1, 2, 3, 4]], x[1, 0, [1, 2, 3, 4]]) and y[1, 0, 0] == 9.0


def test_misaligned_pointers_take_the_element_path(ops):
    B, T, D, C, ld, lens = SHAPES["vector"]
    x = _input("vector")
    params, nf, nt, fill = _tables(lens, D)["all"]
    y = _run_abi(ops, x, lens, params, D, C, nf, nt, fill, misalign=True)
    check(y, x, lens, params, D, C, nf, nt, fill)
    assert np.array_equal(y, _run_abi(ops, x, lens, params, D, C, nf, nt, fill))      # both paths: the same bits


@pytest.mark.parametrize("shape", ["element", "vector", "wide"])
def test_sampled_tables_through_the_policy(ops, shape):
    SpecAugment = importlib.import_module(PKG + ".src.audio").SpecAugment
    B, T, D, C, ld, lens = SHAPES[shape]
    x = _input(shape)
    sa = SpecAugment(D, C, freq_mask_width=max(2, D // 4), n_freq_mask=2, time_mask_width=6, n_time_mask=2,
                     time_mask_ratio=0.5, time_warp=W, mask_value=-0.5)
    xg = torch.from_numpy(x).cuda()
    for step in (0, 1, 2, 3):
        tab = sa.sample(lens, seed=11, step=step)
        y = sa(xg, torch.tensor(lens), seed=11, step=step)
        assert y.shape == xg.shape and y.data_ptr() != xg.data_ptr()
        check(y.cpu().numpy(), x, lens, tab.numpy(), D, C, 2, 2, -0.5)
        again = sa(xg, lens, seed=11, step=step, feat_len_dev=torch.tensor(lens, device="cuda"))
        assert torch.equal(y, again)
    assert torch.equal(xg.cpu(), torch.from_numpy(x))                                  # the input is left alone


def _check_warped_frames(xg, yg, b, n, c, w, frames):
    """the criterion on chosen output frames of a warp-only launch (tensors stay on the device: only the frames that are
    looked at, and their sources, come back)"""
    src = [warp_source(t, n, c, w) for t in frames]
    dev = xg.device
    xi = xg[b, torch.tensor([s[0] for s in src], device=dev)].cpu().numpy()
    xj = xg[b, torch.tensor([s[1] for s in src], device=dev)].cpu().numpy()
    yy = yg[b, torch.tensor(frames, device=dev)].cpu().numpy()
    blended = 0
    for k, (i, j, r, den) in enumerate(src):
        if r == 0:
            assert np.array_equal(yy[k].view(np.uint32), xi[k].view(np.uint32)), frames[k]
            continue
        a = r / den
        want = (1.0 - a) * xi[k].astype(np.float64) + a * xj[k].astype(np.float64)
        bound = BLEND_TOL * np.maximum(np.abs(xi[k]), np.abs(xj[k])).astype(np.float64)
        assert np.all(np.abs(yy[k].astype(np.float64) - want) <= bound), (frames[k], i, j, r, den)
        blended += 1
    return blended


def test_long_utterance_takes_the_64_bit_division(ops):
    """t * c passes 2^32 from n = 2^16 on: the quotient and the remainder then come from the 64-bit division"""
    B, T, CD = 1, 70001, 4
    n, c, w = 70001, 69995, 4                              # c = n - 1 - W, w = W - 1: d = n - 2, almost every t <= d
    xg = torch.randn(B, T, CD, generator=torch.Generator().manual_seed(7)).cuda()
    lens = torch.tensor([n], device="cuda")
    par = torch.tensor([[c, w]], dtype=torch.int32, device="cuda")
    yg = ops.spec_augment(xg, lens, par, 0, 0)
    frames = list(range(0, 40)) + list(range(61350, 61390)) + list(range(65530, 65545)) + list(range(n - 40, n))
    assert 61360 * c < 2 ** 32 < 61370 * c
    assert _check_warped_frames(xg, yg, 0, n, c, w, frames) > 100
    assert torch.equal(yg[0, 0], xg[0, 0]) and torch.equal(yg[0, n - 1], xg[0, n - 1]) and \
        torch.equal(yg[0, c + w], xg[0, c])


def test_offsets_past_2_31_elements(ops):
    """B * T * ld = 2^31 + 2^17 elements (8.6 GB each way): the second utterance's last frames lie behind what a 32-bit
    element offset reaches"""
    B, T, CD = 2, 2 ** 20 + 64, 1024
    n, c, w = T, T - 1 - W, W - 1
    xg = torch.empty((B, T, CD), dtype=torch.float32, device="cuda").normal_()
    lens = torch.tensor([n, n], device="cuda")
    par = torch.tensor([[0, 0], [c, w]], dtype=torch.int32, device="cuda")
    yg = ops.spec_augment(xg, lens, par, 0, 0)
    frames = list(range(0, 8)) + list(range(2 ** 19, 2 ** 19 + 8)) + list(range(n - 24, n))
    assert (B * T - 24) * CD > 2 ** 31
    assert _check_warped_frames(xg, yg, 1, n, c, w, frames) >= 24
    assert torch.equal(yg[0, :64], xg[0, :64]) and torch.equal(yg[0, -64:], xg[0, -64:])     # utterance 0: no warp
    assert torch.equal(yg[1, n - 1], xg[1, n - 1])
    del xg, yg
    torch.cuda.empty_cache()


def test_operator_checks_its_arguments(ops):
    x = torch.zeros(2, 8, 12, device="cuda")
    lens = torch.tensor([8, 4], device="cuda")
    par = torch.zeros(2, 2, dtype=torch.int32, device="cuda")
    assert torch.equal(ops.spec_augment(x, lens, par, 0, 0, channels=3), x)
    for bad in (lambda: ops.spec_augment(x, lens.cpu(), par, 0, 0), lambda: ops.spec_augment(x, lens, par.cpu(), 0, 0),
                lambda: ops.spec_augment(x, lens.int(), par, 0, 0), lambda: ops.spec_augment(x, lens, par, 1, 0),
                lambda: ops.spec_augment(x, lens, par, 0, 0, channels=5), lambda: ops.spec_augment(x[0], lens, par, 0, 0)):
        with pytest.raises(ValueError):
            bad()
    assert ops.spec_augment(x[:0], lens[:0], par[:0], 0, 0).shape == (0, 8, 12)


def test_solver_applies_it_to_training_batches_only(tmp_path):
    """three short runs of the product solver (2 steps, one validation pass) in a fresh process with
    ASRK_DETERMINISTIC=1: no `specaug:` block, an enabled block, `enable: false`"""
    out = str(tmp_path)
    env = dict(os.environ, ASRK_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "specaug_worker.py"), out], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    runs = {k: np.load(os.path.join(out, k + ".npz")) for k in ("plain", "aug", "off")}
    plain, aug, off = runs["plain"], runs["aug"], runs["off"]
    D, C, nf, nt = 40, 3, int(aug["n_fmask"]), int(aug["n_tmask"])
    # step 0: the augmented run's features = the reference applied to the plain run's, with the table of (seed, step 0)
    SpecAugment = importlib.import_module(PKG + ".src.audio").SpecAugment
    lens = plain["train_len_0"]
    assert np.array_equal(lens, aug["train_len_0"]) and plain["train_feat_0"].shape == aug["train_feat_0"].shape
    sa = SpecAugment.from_config({"specaug": {k[4:]: aug[k].item() for k in aug.files if k.startswith("cfg_")}}, D, C)
    tab = sa.sample(lens, int(aug["seed"]), 0).numpy()
    assert (tab[:, 3:2 + 2 * nf:2] > 0).any() or (tab[:, 3 + 2 * nf::2] > 0).any()      # something is masked
    assert not np.array_equal(plain["train_feat_0"], aug["train_feat_0"])
    check(aug["train_feat_0"], plain["train_feat_0"], lens, tab, D, C, nf, nt, float(aug["cfg_mask_value"]))
    # step 1 too: the key follows the step
    tab1 = sa.sample(plain["train_len_1"], int(aug["seed"]), 1).numpy()
    check(aug["train_feat_1"], plain["train_feat_1"], plain["train_len_1"], tab1, D, C, nf, nt,
          float(aug["cfg_mask_value"]))
    # validation batches are never augmented
    assert int(plain["n_valid"]) == int(aug["n_valid"]) >= 1
    for k in range(int(plain["n_valid"])):
        a, b = plain["valid_feat_%d" % k], aug["valid_feat_%d" % k]
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # a disabled block is the parent's step, bit for bit
    assert len(plain["loss"]) >= 2 and np.array_equal(plain["loss"].view(np.uint32), off["loss"].view(np.uint32))
    assert np.array_equal(plain["train_feat_0"].view(np.uint32), off["train_feat_0"].view(np.uint32))
    assert not np.array_equal(plain["loss"], aug["loss"])
