"""GPU: the two MFMA shapes of the split GEMM (csrc/gemm_split.hip, ASRK_SPLIT_MFMA = 16: v_mfma_f32_16x16x32_bf16,
32: v_mfma_f32_32x32x16_bf16) under every kernel routing (ASRK_SPLIT_W256 = 0 / 2, = 1 with ASRK_SPLIT_TAIL = 0).

Knobs are read once per process, so each of the six knob sets runs in ONE child pytest process (cached for the module):
the float64 selections of test_kernels_gpu.py and all of test_gemm_panels_splitk_gpu.py, plus the `inner` tests of this
file, which also run here under the default knobs.  The inner shapes are the smallest at which the k loop can go wrong:
K = 8 (one ragged k-tile), 40 (two tiles, no steady state), 96 and 160 (the ring wraps: three 32-k stages in the
128 x 128 kernel, two 32-k stage pairs in the 128 x 256 kernel), 264 (ragged tail after a full ring) crossed with
M = 64 / 130 (a single mostly empty row tile, two row tiles) and N = 128 / 520 / 1030 (one tile, the clamped last B row
block of the wide kernel, ragged N), with alpha, beta, both biases and three guard columns behind N; and the split-K
launch 256 x 80 x 4096 with 2 and 8 slices.  Bound: the existing float64 test's, 1e-7 * max(4, sqrt(K)) of the product
scale max(|A| |B|).  The children store their results, and the two shapes must agree within the sum of their bounds."""
import itertools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS, MS, NS = (8, 40, 96, 160, 264), (64, 130), (128, 520, 1030)
SK_SHAPE, SK_SLICES = (256, 80, 4096), (2, 8)
ROUTES = ({"ASRK_SPLIT_W256": "0"}, {"ASRK_SPLIT_W256": "2"}, {"ASRK_SPLIT_W256": "1", "ASRK_SPLIT_TAIL": "0"})
KNOB_SETS = [dict(r, ASRK_SPLIT_MFMA=m) for m in ("16", "32") for r in ROUTES]
DUMP_ENV = "ASRK_TEST_MFMA_SHAPE_DUMP"
SELECTION = ("test_gemm_split_matches_float64 or test_gemm_panels_ranges or test_gemm_split_propagates_nan or "
             "test_gemm_split_exact_on_bf16_representable_inputs or test_splitk or inner")


def t(x):
    return torch.as_tensor(x).to(DEV)


def bound(K):
    return 1e-7 * max(4.0, K ** 0.5)


def small_case(M, N, K):
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    A = torch.randn(M, K, generator=g) * torch.exp(torch.randn(K, generator=g) * 2.0)     # wide dynamic range along K
    B = torch.randn(N, K, generator=g)
    C0 = torch.randn(M, N + 3, generator=g)
    b1, b2 = torch.randn(N, generator=g), torch.randn(N, generator=g)
    ref = 0.75 * (A.double() @ B.double().t()) + 0.5 * C0[:, :N].double() + b1.double() + b2.double()
    mag = (A.double().abs() @ B.double().abs().t()).max().item()
    return A, B, C0, b1, b2, ref, mag


def splitk_case():
    M, N, K = SK_SHAPE
    g = torch.Generator().manual_seed(17)
    A, B = torch.randn(K, M, generator=g), torch.randn(N, K, generator=g)       # A stored [K][rows]
    ref = A.double().t() @ B.double().t()
    mag = (A.double().abs().t() @ B.double().abs().t()).max().item()
    return A, B, ref, mag


def dump(name, C):
    d = os.environ.get(DUMP_ENV)
    if d:
        torch.save(C, os.path.join(d, name + ".pt"))


@pytest.fixture()
def always_split(ops):
    prev = ops.get_gemm_split()
    ops.set_gemm_split(2)
    yield ops
    ops.set_gemm_split(prev)


@pytest.mark.parametrize("M,N,K", list(itertools.product(MS, NS, KS)))
def test_inner_small_shapes_match_float64(always_split, M, N, K):
    ops = always_split
    A, B, C0, b1, b2, ref, mag = small_case(M, N, K)
    C = t(C0.clone())
    ops.gemm(0, 1, M, N, K, t(A), K, t(B), K, C, N + 3, alpha=0.75, beta=0.5, bias=t(b1), bias2=t(b2))
    C = C.cpu()
    assert torch.equal(C[:, N:], C0[:, N:])                        # guard columns beyond N unchanged
    err = (C[:, :N].double() - ref).abs().max().item() / mag
    print("M %d N %d K %d: err %.3g of the product scale, bound %.3g" % (M, N, K, err, bound(K)))
    dump("small_%d_%d_%d" % (M, N, K), C[:, :N])
    assert err < bound(K), (M, N, K, err)


@pytest.mark.parametrize("slices", SK_SLICES)
def test_inner_splitk_matches_float64_and_repeats_bit_identical(ops, slices):
    M, N, K = SK_SHAPE
    A, B, ref, mag = splitk_case()
    pa, pb = ops.SplitPanel(t(A), M, M, K, True), ops.SplitPanel(t(B), K, N, K, False)
    out = []
    for _ in range(2):
        C = t(torch.zeros(M, N))
        ops.gemm_panels(M, N, K, pa, 0, 0, pb, 0, 0, C, N, splitk=slices)
        out.append(C.cpu())
    assert torch.equal(out[0], out[1])
    err = (out[0].double() - ref).abs().max().item() / mag
    print("split-K %d slices: err %.3g of the product scale, bound %.3g" % (slices, err, bound(K)))
    dump("splitk_%d" % slices, out[0])
    assert err < bound(K), (slices, err)


# ---------------------------------------------------------------------------------------- one child per knob set
_children = {}


def child(env, tmp_path_factory):
    key = tuple(sorted(env.items()))
    if key not in _children:
        here = os.path.dirname(os.path.abspath(__file__))
        d = str(tmp_path_factory.mktemp("mfma_shape"))
        files = [os.path.join(here, f) for f in ("test_kernels_gpu.py", "test_gemm_panels_splitk_gpu.py",
                                                 os.path.basename(__file__))]
        r = subprocess.run([sys.executable, "-m", "pytest"] + files + ["-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                                                                     "-k", SELECTION],
                           capture_output=True, text=True, env=dict(os.environ, **env, **{DUMP_ENV: d}), timeout=900,
                           cwd=os.path.dirname(here))
        _children[key] = (r, d)
    return _children[key]


@pytest.mark.parametrize("env", KNOB_SETS, ids=lambda e: "-".join("%s%s" % (k[11:], v) for k, v in sorted(e.items())))
def test_float64_parity_under_each_shape_and_routing(env, tmp_path_factory):
    r, _ = child(env, tmp_path_factory)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-500:])
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("route", ROUTES, ids=lambda e: "-".join("%s%s" % (k[11:], v) for k, v in sorted(e.items())))
def test_the_two_shapes_agree_within_the_sum_of_their_bounds(route, tmp_path_factory):
    d16 = child(dict(route, ASRK_SPLIT_MFMA="16"), tmp_path_factory)[1]
    d32 = child(dict(route, ASRK_SPLIT_MFMA="32"), tmp_path_factory)[1]
    load = lambda d, n: torch.load(os.path.join(d, n + ".pt")).double()
    for M, N, K in itertools.product(MS, NS, KS):
        mag = small_case(M, N, K)[-1]
        n = "small_%d_%d_%d" % (M, N, K)
        diff = (load(d16, n) - load(d32, n)).abs().max().item() / mag
        assert diff < 2 * bound(K), (M, N, K, diff)
    mag = splitk_case()[-1]
    for s in SK_SLICES:
        diff = (load(d16, "splitk_%d" % s) - load(d32, "splitk_%d" % s)).abs().max().item() / mag
        assert diff < 2 * bound(SK_SHAPE[2]), (s, diff)
