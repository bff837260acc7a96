"""CPU: the lock-step (multi-utterance, LM fusion) prefix-beam entry point of libasrk.so - bound, exported, its
workspace query, and the argument validation that happens on the host before any HIP call."""
import ctypes
import importlib

import pytest

from conftest import PKG_NAME

EINVAL, ESHAPE, EWORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    build = importlib.import_module(PKG_NAME + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib")


def test_entry_points_are_bound_and_exported(lib):
    L = lib.load()
    for name in ("asrk_ctc_prefix_beam_multi_f32", "asrk_ctc_prefix_beam_multi_ws_bytes"):
        assert name in lib.SIGNATURES
        assert hasattr(L, name)


@pytest.mark.parametrize("U,beam,T", [(1, 20, 200), (4, 4, 14), (16, 20, 200), (3, 32, 1)])
def test_workspace_is_one_single_utterance_slab_per_utterance(lib, U, beam, T):
    L = lib.load()
    single = int(L.asrk_ctc_prefix_beam_ws_bytes(beam, T))
    assert single > 0
    aligned = (single + 15) & ~15
    slab = ctypes.c_size_t(0)
    total = int(L.asrk_ctc_prefix_beam_multi_ws_bytes(U, beam, T, ctypes.byref(slab)))
    assert int(slab.value) == aligned
    assert total == U * aligned
    assert int(L.asrk_ctc_prefix_beam_multi_ws_bytes(U, beam, T, None)) == total      # the stride is optional


def test_workspace_query_rejects_what_the_entry_point_rejects(lib):
    L = lib.load()
    assert L.asrk_ctc_prefix_beam_multi_ws_bytes(0, 4, 14, None) == 0
    assert L.asrk_ctc_prefix_beam_multi_ws_bytes(2, 33, 14, None) == 0
    assert L.asrk_ctc_prefix_beam_multi_ws_bytes(2, 4, -1, None) == 0


def test_argument_errors_without_gpu(lib):
    """every rejection below happens before the first HIP call: this test runs without a GPU (the fake pointers
    are never dereferenced)"""
    L = lib.load()
    z = ctypes.c_void_p(0)
    f = ctypes.c_void_p(4096)                                   # non-null, 16-byte aligned, never touched
    U, T, V, beam, cand = 4, 14, 40, 4, 5
    need = int(L.asrk_ctc_prefix_beam_multi_ws_bytes(U, beam, T, None))

    def call(ctc=f, stride=V, U=U, T=T, V=V, allowed=f, beam=beam, cand=cand, lm=f, frames=f, t_start=f, j=0,
             parent=f, last=f, gidx=f, ws=f, ws_bytes=need):
        return L.asrk_ctc_prefix_beam_multi_f32(ctc, stride, U, T, V, allowed, beam, cand, lm, 0.5, frames, t_start, j,
                                                parent, last, gidx, ws, ws_bytes, z)

    for name in ("ctc", "allowed", "lm", "frames", "t_start", "parent", "last", "gidx", "ws"):
        assert call(**{name: z}) == EINVAL, name                # lm is required: the entry point exists for LM fusion
    assert call(U=0) == EINVAL
    assert call(U=-3) == EINVAL
    assert call(U=(1 << 20) + 1, ws_bytes=1 << 62) == EINVAL    # documented bound: global row indices are int32
    assert call(beam=33) == EINVAL
    assert call(beam=0) == EINVAL
    assert call(cand=0) == EINVAL
    assert call(cand=V + 1) == EINVAL
    # the limits of the single-utterance entry point, with its error code for them
    assert call(V=5000, stride=5000, beam=32, cand=32) == ESHAPE            # 32 * 33 = 1056 entries > 1024
    assert L.asrk_ctc_prefix_beam_f32(f, T, 5000, f, 32, 32, z, 0.0, 0, 1, 0, 1, 0, f, 1 << 30, z) == ESHAPE
    assert call(V=16385, stride=16385) == ESHAPE
    assert call(stride=V - 1) == EINVAL                         # rows would overlap
    assert call(j=-1) == EINVAL
    assert call(j=T) == EINVAL                                  # no utterance has a frame t_start + j >= Tmax
    assert call(ws_bytes=need - 1) == EWORKSPACE
    assert call(ws_bytes=0) == EWORKSPACE
    assert call(ws=ctypes.c_void_p(4096 + 8)) == EINVAL         # misaligned workspace
