"""CPU: argument checks of the length-aware convolution entries (before any HIP call) and the predicate that lets
prenet models take the batched decode path."""
import ctypes
import importlib

import pytest

from conftest import PKG_NAME

EINVAL, ESHAPE = -1, -2


@pytest.fixture(scope="module")
def lib():
    build = importlib.import_module(PKG_NAME + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib")


def test_length_aware_conv_argument_errors_without_gpu(lib):
    L = lib.load()
    z, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    B, H, W = 2, 8, 20
    # implicit-GEMM layers: a null hlen (or any other null pointer) is ASRK_EINVAL, shapes are checked as in asrk_conv3x3_f32
    assert L.asrk_conv3x3_len_f32(p, p, p, p, z, B, H, W, 64, 64, 1, z) == EINVAL
    assert L.asrk_conv3x3_len_f32(z, p, p, p, p, B, H, W, 64, 64, 1, z) == EINVAL
    assert L.asrk_conv3x3_len_f32(p, z, p, p, p, B, H, W, 64, 64, 1, z) == EINVAL
    assert L.asrk_conv3x3_len_f32(p, p, p, z, p, B, H, W, 64, 64, 1, z) == EINVAL
    assert L.asrk_conv3x3_len_f32(p, p, p, p, p, B, 0, W, 64, 64, 1, z) == EINVAL
    assert L.asrk_conv3x3_len_f32(p, p, p, p, p, B, H, W, 48, 64, 1, z) == ESHAPE
    assert L.asrk_conv3x3_len_f32(p, p, p, p, p, B, H, 200, 64, 64, 1, z) == ESHAPE
    assert L.asrk_conv3x3_len_f32(p, p, p, ctypes.c_void_p(4100), p, B, H, W, 64, 64, 1, z) == ESHAPE   # y alignment
    assert L.asrk_conv3x3_len_f32(z, z, z, z, z, 0, H, W, 64, 64, 1, z) == 0                            # empty batch
    # first layer
    st = (H * W, W, 1, W)
    assert L.asrk_conv3x3_first_len_f32(p, p, p, p, z, B, H, W, 1, 64, *st, 1, z) == EINVAL
    assert L.asrk_conv3x3_first_len_f32(z, p, p, p, p, B, H, W, 1, 64, *st, 1, z) == EINVAL
    assert L.asrk_conv3x3_first_len_f32(p, p, p, z, p, B, H, W, 1, 64, *st, 1, z) == EINVAL
    assert L.asrk_conv3x3_first_len_f32(p, p, p, p, p, B, H, W, 4, 64, *st, 1, z) == ESHAPE
    assert L.asrk_conv3x3_first_len_f32(p, p, p, p, p, B, H, W, 1, 48, *st, 1, z) == ESHAPE
    # gathers: geometry as asrk_im2col_ld_f32 / asrk_im2col_cl_f32
    geo = (B, H, 1, 40, 4, 1, 2, 1, 1, 0, H * 40, 40, 0, 1)
    assert L.asrk_im2col_ld_len_f32(p, p, z, 160, *geo, z) == EINVAL
    assert L.asrk_im2col_ld_len_f32(z, p, p, 160, *geo, z) == EINVAL
    assert L.asrk_im2col_ld_len_f32(p, p, p, 100, *geo, z) == EINVAL                                    # ldcol < K
    assert L.asrk_im2col_cl_len_f32(p, p, z, *geo, z) == EINVAL
    assert L.asrk_im2col_cl_len_f32(p, z, p, *geo, z) == EINVAL
    bad = (B, H, 1, 39, 4, 1, 2, 1, 1, 0, H * 39, 39, 0, 1)                                             # C % 4 != 0
    assert L.asrk_im2col_cl_len_f32(p, p, p, *bad, z) == ESHAPE
    assert L.asrk_conv_zero_tail_f32(p, z, B, H, 16, z) == EINVAL
    assert L.asrk_conv_zero_tail_f32(z, p, B, H, 16, z) == EINVAL
    assert L.asrk_conv_zero_tail_f32(p, p, B, 0, 16, z) == EINVAL


@pytest.mark.parametrize("prenet", ["vgg", "cnn", ""])
def test_supports_packed_follows_the_recurrent_layers_not_the_prenet(pkg, prenet):
    """construction only - no kernel runs"""
    asr = importlib.import_module(PKG_NAME + ".src.asr")
    cfg = dict(prenet=prenet, bidirection=True, dim=[16, 16], dropout=[0, 0], layer_norm=[False, False],
               proj=[True, True], sample_rate=[1, 1], sample_style='drop')
    assert asr.Encoder(40, module='LSTM', **cfg).supports_packed()
    assert not asr.Encoder(40, module='GRU', **cfg).supports_packed()
    assert not asr.Encoder(40, module='LSTM', **dict(cfg, dim=[16, 18])).supports_packed()   # H % 4 != 0
