"""CPU: host side of the fixed-order split-K panel GEMM (include/asrk.h: asrk_gemm_panels_splitk_*): the workspace
size and every argument check happen before any device call, so they need no GPU."""
import ctypes
import importlib

import pytest

from conftest import PKG_NAME


@pytest.fixture(scope="module")
def lib():
    importlib.import_module(PKG_NAME + ".build").build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib").load()


def test_workspace_bytes_is_slices_times_padded_output(lib):
    for M, N, n in ((8192, 80, 4), (256, 80, 32), (128, 1, 1), (130, 83, 5), (4096, 36, 8)):
        assert lib.asrk_gemm_panels_splitk_ws_bytes(M, N, n) == n * M * ((N + 3) // 4 * 4) * 4
    assert lib.asrk_gemm_panels_splitk_ws_bytes(256, 80, -1) == 0
    assert lib.asrk_gemm_panels_splitk_ws_bytes(0, 80, 2) == 0
    # splitk = 0 (the library chooses): a whole number of slices, enough for whatever it chooses at any K
    auto = lib.asrk_gemm_panels_splitk_ws_bytes(8192, 80, 0)
    assert auto > 0 and auto % (8192 * 80 * 4) == 0
    # N >= 512 fills the chip with tiles: one slice
    assert lib.asrk_gemm_panels_splitk_ws_bytes(4096, 1024, 0) == 4096 * 1024 * 4


def test_multiply_rejects_bad_workspace_and_slice_count_before_the_device(lib):
    EINVAL, EWORKSPACE = -1, -3
    fake = ctypes.c_void_p(4096)
    M, N, K = 256, 80, 1000

    def call(splitk, ws, ws_bytes, **kw):
        a = dict(M=M, N=N, K=K, a_row0=0, a_k0=0)
        a.update(kw)
        return lib.asrk_gemm_panels_splitk_f32(a["M"], a["N"], a["K"], 1.0, fake, 256, 1000, a["a_row0"], a["a_k0"],
                                               fake, 80, 1000, 0, 0, 0.0, fake, N, None, None, splitk, ws, ws_bytes, 0,
                                               None)

    need = lib.asrk_gemm_panels_splitk_ws_bytes(M, N, 4)
    assert call(4, None, need) == EINVAL                                  # no workspace: the library allocates nothing
    assert call(4, ctypes.c_void_p(4096 + 8), need) == EINVAL             # not 16-byte aligned
    assert call(-1, fake, need) == EINVAL                                 # negative slice count
    assert call(4, fake, need - 1) == EWORKSPACE
    assert call(4, fake, 0) == EWORKSPACE
    assert call(1, fake, lib.asrk_gemm_panels_splitk_ws_bytes(M, N, 1) - 1) == EWORKSPACE
    # the library's own choice needs at least one slice's worth
    assert call(0, fake, M * N * 4 - 1) == EWORKSPACE
    # the panel-range checks of asrk_gemm_panels_f32 hold here too
    assert call(4, fake, need, a_row0=64) == EINVAL                       # row offset not a multiple of 128
    assert call(4, fake, need, a_k0=4) == EINVAL                          # k offset not a multiple of 8
    assert call(4, fake, need, K=900) != 0                                # ragged K ending inside both panels
