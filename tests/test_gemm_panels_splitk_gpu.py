"""GPU: fixed-order split-K over split panels (csrc/gemm_split.hip: gemm_bf16x6_kernel<.., SK> + splitk_reduce_kernel,
ops.gemm_panels(splitk=...)) against float64.

Shapes: the smallest at which the path can go wrong.  A is stored [K][R] (transposed) with R = 256 rows (two row tiles),
K = 1000: 32 k-tiles of 32, the last one ragged (it runs into the panels' zero padding).  B has N = 80 rows - fewer than
one 128-wide tile, so three quarters of the B rows a workgroup multiplies are padding and the workspace rows are 80 floats
long.  Slice counts 1 (the plain launch), 2, 3 and 5 (uneven cuts: 10 / 11 and 6 / 7 k-tiles), 32 (one k-tile per slice:
prologue only, no main loop) and 40 (more slices than k-tiles: clamped to 32)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
R, K, N = 256, 1000, 80
SLICES = (1, 2, 3, 5, 32, 40)
# (M, K range, a_row0, a_k0 = b_k0)
CASES = {"full": (256, 1000, 0, 0), "k_offset": (256, 960, 0, 40), "row_offset": (128, 1000, 128, 0)}


def t(x):
    return torch.as_tensor(x).to(DEV)


@pytest.fixture(scope="module")
def data(ops):
    """panels seeded like test_gemm_panels_ranges_match_float64, the epilogue operands of test_gemm_split_matches_float64
    (alpha 0.75, beta 0.5, two biases, ldc = N + 3 with three guard columns) and the float64 reference of every case"""
    g = torch.Generator().manual_seed(11)
    A = torch.randn(K, R, generator=g)            # stored [K][rows] -> trans
    Bm = torch.randn(N, K, generator=g)           # stored [rows][K]
    C0 = torch.randn(R, N + 3, generator=g)
    b1, b2 = torch.randn(N, generator=g), torch.randn(N, generator=g)
    a64, b64 = A.double().t(), Bm.double()
    refs = {}
    for name, (M, Kk, ar, ak) in CASES.items():
        refs[name] = (0.75 * (a64[ar:ar + M, ak:ak + Kk] @ b64[:, ak:ak + Kk].t()) + 0.5 * C0[:M, :N].double()
                      + b1.double() + b2.double())
    return dict(pa=ops.SplitPanel(t(A), R, R, K, True), pb=ops.SplitPanel(t(Bm), K, N, K, False), C0=C0, b1=t(b1),
                b2=t(b2), refs=refs)


def run(ops, d, case, splitk):
    M, Kk, ar, ak = CASES[case]
    C = t(d["C0"][:M].clone())
    ops.gemm_panels(M, N, Kk, d["pa"], ar, ak, d["pb"], 0, ak, C, N + 3, alpha=0.75, beta=0.5, bias=d["b1"],
                    bias2=d["b2"], splitk=splitk)
    return C.cpu()


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("splitk", SLICES + (0,))
def test_splitk_matches_float64(ops, data, case, splitk):
    """every slice count (0: the library's choice), full range / k offset 40 with K = 960 / row offset 128 with M = 128:
    relative max error < 5e-6 of the reference's max (the bound of test_gemm_panels_ranges_match_float64), nothing
    written to the three guard columns"""
    M = CASES[case][0]
    C = run(ops, data, case, splitk)
    ref = data["refs"][case]
    assert torch.equal(C[:, N:], data["C0"][:M, N:])              # nothing written beyond N
    err = (C[:, :N].double() - ref).abs().max().item() / ref.abs().max().item()
    print("case %s splitk %d: rel max err %.3g" % (case, splitk, err))
    assert err < 5e-6, (case, splitk, err)


@pytest.mark.parametrize("case", list(CASES))
def test_splitk_is_reproducible_and_one_slice_is_the_plain_launch(ops, data, case):
    """no atomics: two calls with the same slice count agree bit for bit; one slice IS ops.gemm_panels without splitk;
    40 slices over 32 (30 with the k offset) k-tiles are clamped to one k-tile per slice"""
    for n in SLICES:
        assert torch.equal(run(ops, data, case, n), run(ops, data, case, n)), n
    assert torch.equal(run(ops, data, case, 1), run(ops, data, case, None))
    nk = (CASES[case][1] + 31) // 32
    assert torch.equal(run(ops, data, case, 40), run(ops, data, case, nk))


def test_splitk_short_workspace_and_bad_counts_raise(ops, data):
    lib = ops._L()
    d = data
    C = t(d["C0"].clone())
    need = lib.asrk_gemm_panels_splitk_ws_bytes(R, N, 5)
    assert need == 5 * R * N * 4
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call(splitk, nbytes):
        return lib.asrk_gemm_panels_splitk_f32(R, N, K, 1.0, d["pa"].buf.data_ptr(), R, K, 0, 0, d["pb"].buf.data_ptr(),
                                               N, K, 0, 0, 0.0, C.data_ptr(), N + 3, None, None, splitk, ws.data_ptr(),
                                               nbytes, 0, None)

    assert call(5, need - 1) == -3                                # ASRK_EWORKSPACE
    assert call(5, need) == 0
    with pytest.raises(Exception):
        ops.gemm_panels(R, N, K, d["pa"], 0, 0, d["pb"], 0, 0, C, N + 3, splitk=-1)
    torch.cuda.synchronize()
    ops.check_errors()
