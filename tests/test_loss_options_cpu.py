"""CPU: the `loss:` config block (src/loss.py), the constructors of the two loss modules with their new options, and the
host-side argument checks of the new C entry points (all made before any device call)."""
import ctypes
import importlib

import pytest

from conftest import PKG_NAME


@pytest.fixture(scope="module")
def LossOptions(pkg):
    return importlib.import_module(PKG_NAME + ".src.loss").LossOptions


@pytest.fixture(scope="module")
def L():
    importlib.import_module(PKG_NAME + ".build").build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib").load()


def test_absent_block_is_the_defaults(LossOptions):
    for cfg in ({}, {'loss': None}, {'model': {}}, None):
        o = LossOptions.from_config(cfg)
        assert o.label_smoothing == 0.0 and o.ctc_zero_infinity is False and not o.active
    o = LossOptions.from_config({'loss': {}}, ctc=False)
    assert o.label_smoothing == 0.0 and not o.active


def test_full_block(LossOptions):
    o = LossOptions.from_config({'loss': {'label_smoothing': 0.1, 'ctc_zero_infinity': True}})
    assert o.label_smoothing == 0.1 and o.ctc_zero_infinity is True and o.active
    assert '0.1' in o.create_msg() and 'on' in o.create_msg()
    o = LossOptions.from_config({'loss': {'label_smoothing': 0}})          # an integer 0 is a number
    assert o.label_smoothing == 0.0 and isinstance(o.label_smoothing, float)
    assert LossOptions.from_config({'loss': {'ctc_zero_infinity': True}}).active
    assert LossOptions.from_config({'loss': {'label_smoothing': 0.25}}, ctc=False).label_smoothing == 0.25


@pytest.mark.parametrize("block, key", [
    ([0.1], 'loss'),                                        # not a mapping
    ('label_smoothing', 'loss'),
    ({'label_smooth': 0.1}, 'label_smooth'),                # unknown key
    ({'label_smoothing': True}, 'label_smoothing'),         # a bool where a number is wanted
    ({'label_smoothing': '0.1'}, 'label_smoothing'),
    ({'label_smoothing': 1.0}, 'label_smoothing'),          # out of range
    ({'label_smoothing': -0.1}, 'label_smoothing'),
    ({'label_smoothing': float('nan')}, 'label_smoothing'),
    ({'ctc_zero_infinity': 1}, 'ctc_zero_infinity'),        # a number where a bool is wanted
    ({'ctc_zero_infinity': 'yes'}, 'ctc_zero_infinity'),
])
def test_rejections_name_the_key(LossOptions, block, key):
    with pytest.raises(ValueError, match=key):
        LossOptions.from_config({'loss': block})


def test_lm_block_has_no_ctc_key(LossOptions):
    with pytest.raises(ValueError, match='ctc_zero_infinity'):
        LossOptions.from_config({'loss': {'label_smoothing': 0.1, 'ctc_zero_infinity': False}}, ctc=False)


def test_loss_modules_take_the_options(pkg):
    ops = importlib.import_module(PKG_NAME + ".ops")
    ce = ops.CrossEntropyLoss(ignore_index=0, label_smoothing=0.1)
    assert ce.label_smoothing == 0.1 and ce.ignore_index == 0
    assert ops.CrossEntropyLoss(ignore_index=0).label_smoothing == 0.0
    for bad in (1.0, -0.1, True, '0.1'):
        with pytest.raises(ValueError, match='label_smoothing'):
            ops.CrossEntropyLoss(label_smoothing=bad)
    ctc = ops.CTCLoss(blank=0, zero_infinity=True)
    assert ctc.zero_infinity is True and ctc.n_infeasible is None        # nothing ran yet
    assert ops.CTCLoss(blank=0).zero_infinity is False


def test_smoothed_cross_entropy_argument_checks_need_no_gpu(L):
    z, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    bwd = L.asrk_cross_entropy_ls_bwd_f32
    for eps in (1.0, -0.1, 1.5, float('nan')):
        assert bwd(p, 4, 8, 8, p, 0, eps, p, p, p, z) == -1
        assert bwd(p, 0, 8, 8, p, 0, eps, p, p, p, z) == -1              # also with nothing to do
    for hole in range(5):                                                # each pointer in turn
        a = [p, 4, 8, 8, p, 0, 0.1, p, p, p, z]
        a[(0, 4, 7, 8, 9)[hole]] = z
        assert bwd(*a) == -1
    assert bwd(p, -1, 8, 8, p, 0, 0.1, p, p, p, z) == -1
    assert bwd(p, 4, 8, 7, p, 0, 0.1, p, p, p, z) == -1                  # ld < V
    assert bwd(z, 0, 8, 8, z, 0, 0.1, z, z, z, z) == 0                   # rows == 0, as asrk_cross_entropy_bwd_f32
    assert L.asrk_cross_entropy_bwd_f32(z, 0, 8, 8, z, 0, z, z, z, z) == 0
    fwd = L.asrk_cross_entropy_ls_fwd_f32
    for hole in range(5):
        a = [p, 4, 8, 8, p, 0, p, p, p, z]
        a[(0, 4, 6, 7, 8)[hole]] = z
        assert fwd(*a) == -1
    assert fwd(p, 4, 0, 0, p, 0, p, p, p, z) == -1
    assert fwd(z, 0, 8, 8, z, 0, z, z, z, z) == -1                       # sums is always needed, as the plain forward
    assert L.asrk_cross_entropy_fwd_f32(z, 0, 8, 8, z, 0, z, z, z) == -1


def test_ctc_flag_entry_points_argument_checks_need_no_gpu(L):
    z, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    ZI = 1                                                               # ASRK_CTC_ZERO_INFINITY
    fwd, bwd = L.asrk_ctc_loss_fwd_ex_f32, L.asrk_ctc_loss_bwd_ex_f32
    fargs = lambda B, flags, loss, ptr=p: [ptr, 8, 8, 4, B, 8, ptr, 2, 2, ptr, ptr, 0, ptr, ptr, ptr, ptr, flags, loss,
                                           ptr, z]
    bargs = lambda B, flags, ptr=p: [ptr, 8, 8, 4, B, 8, ptr, 2, 2, ptr, ptr, 0, ptr, ptr, ptr, ptr, ptr, ptr, 8, 8,
                                     flags, z]
    assert fwd(*fargs(0, 0, z, z)) == 0 and fwd(*fargs(0, ZI, p, z)) == 0    # B == 0, as asrk_ctc_loss_fwd_f32
    assert L.asrk_ctc_loss_fwd_f32(z, 8, 8, 4, 0, 8, z, 2, 2, z, z, 0, z, z, z, z, z) == 0
    assert bwd(*bargs(0, ZI, z)) == 0 and bwd(*bargs(0, 0, z)) == 0
    assert L.asrk_ctc_loss_bwd_f32(z, 8, 8, 4, 0, 8, z, 2, 2, z, z, 0, z, z, z, z, z, z, 8, 8, z) == 0
    assert fwd(*fargs(2, ZI, p, z)) == -1 and fwd(*fargs(2, 0, z, z)) == -1  # null pointers
    assert bwd(*bargs(2, ZI, z)) == -1 and bwd(*bargs(2, 0, z)) == -1
    assert fwd(*fargs(2, ZI, z)) == -1                                   # the flag without a place for the loss
    assert fwd(*fargs(0, ZI, z)) == -1
    assert fwd(*fargs(2, 2, p)) == -1 and bwd(*bargs(2, 2)) == -1        # unknown flag bits
    assert fwd(*fargs(0, -1, p)) == -1 and bwd(*bargs(0, 4)) == -1
    a = fargs(2, ZI, p)
    a[11] = 8                                                            # blank outside [0, V)
    assert fwd(*a) == -1
