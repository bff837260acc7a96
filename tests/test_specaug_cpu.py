"""CPU: the host side of SpecAugment (src/audio.py:SpecAugment - sampler bounds, keying by (seed, step, rank), config
parsing), the properties of the integer warp map the device kernel evaluates, and the argument checks of
asrk_spec_augment_f32, all of which happen before any device call."""
import ctypes
import importlib
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import PKG_NAME
from specaug_reference import warp_source


@pytest.fixture(scope="module")
def SpecAugment():
    return importlib.import_module(PKG_NAME + ".src.audio").SpecAugment


@pytest.fixture(scope="module")
def lib():
    build = importlib.import_module(PKG_NAME + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib")


def _admissible(n, c, w):
    return w != 0 and 0 < c < n - 1 and 0 < c + w < n - 1


@pytest.mark.parametrize("W", [0, 1, 2, 5])
def test_sampler_bounds(SpecAugment, W):
    D, F, Tw, ratio, nf, nt = 11, 4, 9, 0.25, 2, 3
    sa = SpecAugment(D, 3, freq_mask_width=F, n_freq_mask=nf, time_mask_width=Tw, n_time_mask=nt,
                     time_mask_ratio=ratio, time_warp=W)
    lens = [1, 2, 3, 2 * W + 1, 2 * W + 2, 200]
    P = 2 + 2 * nf + 2 * nt
    seen_c, seen_w, seen_fw, seen_tw = set(), set(), set(), set()
    for step in range(500):                                    # 3000 rows
        tab = sa.sample(lens, seed=1, step=step)
        assert tab.dtype == torch.int32 and tuple(tab.shape) == (len(lens), P) and not tab.is_cuda
        for n, row in zip(lens, tab.tolist()):
            c, w = row[0], row[1]
            if W >= 2 and n >= 2 * W + 2:
                assert W <= c <= n - 1 - W and -(W - 1) <= w <= W - 1
                assert w == 0 or _admissible(n, c, w)          # the kernel's own condition holds for every draw
                if n == 200:
                    seen_c.add(c)
                    seen_w.add(w)
            else:
                assert c == 0 and w == 0                       # warp off below 2W + 2 (and for W < 2)
            for k in range(nf):
                f0, fw = row[2 + 2 * k], row[3 + 2 * k]
                assert 0 <= fw <= min(F, D) and 0 <= f0 <= D - fw
                seen_fw.add(fw)
            for k in range(nt):
                t0, tw = row[2 + 2 * nf + 2 * k], row[3 + 2 * nf + 2 * k]
                assert 0 <= tw <= min(Tw, int(np.floor(ratio * n))) and 0 <= t0 <= n - tw
                if n == 200:
                    seen_tw.add(tw)
    assert seen_fw == set(range(F + 1)) and seen_tw == set(range(Tw + 1))      # both ends of each range are drawn
    if W >= 2:
        assert seen_w == set(range(-(W - 1), W)) and min(seen_c) < W + 10 and max(seen_c) > 189 - W


def test_sampler_caps_and_layout(SpecAugment):
    # freq_mask_width above the bin count is capped by D; the ratio caps short utterances, the width long ones
    sa = SpecAugment(5, 1, freq_mask_width=27, n_freq_mask=1, time_mask_width=100, n_time_mask=1, time_mask_ratio=0.1,
                     time_warp=0)
    fws, tws = set(), {}
    for step in range(400):
        for n, row in zip([9, 10, 57, 5000], sa.sample([9, 10, 57, 5000], 0, step).tolist()):
            assert len(row) == 6 and row[0] == 0 and row[1] == 0
            fws.add(row[3])
            assert 0 <= row[2] <= 5 - row[3]
            tws.setdefault(n, set()).add(row[5])
    assert fws == set(range(6))
    assert tws[9] == {0} and tws[10] == {0, 1} and tws[57] == set(range(6)) and max(tws[5000]) == 100
    # no masks at all: the row is just (c, w); lengths may come as a tensor or an array
    sa = SpecAugment(40, 3, n_freq_mask=0, n_time_mask=0, time_warp=5)
    for lens in (torch.tensor([30, 12]), np.array([30, 12]), [30, 12]):
        assert tuple(sa.sample(lens, 0, 0).shape) == (2, 2)
    assert tuple(SpecAugment(40, 3).sample([300], 0, 0).shape) == (1, 10)      # defaults: 2 + 2*2 + 2*2
    assert tuple(sa.sample([], 0, 0).shape) == (0, 2)


def test_sampler_is_keyed_by_seed_step_rank(SpecAugment):
    sa = SpecAugment(40, 3, time_warp=5)
    lens = [400, 380, 200, 13]
    base = sa.sample(lens, seed=3, step=10, rank=1)
    torch.manual_seed(123)                                      # the global generator plays no part
    again = sa.sample(lens, seed=3, step=10, rank=1)
    assert torch.equal(base, again)
    assert torch.equal(base, SpecAugment(40, 3, time_warp=5).sample(torch.tensor(lens), 3, 10, 1))
    for other in (dict(seed=4, step=10, rank=1), dict(seed=3, step=11, rank=1), dict(seed=3, step=10, rank=0),
                  dict(seed=10, step=3, rank=1), dict(seed=3, step=1, rank=10)):
        assert not torch.equal(base, sa.sample(lens, **other)), other
    assert torch.equal(sa.sample(lens, 3, 10), sa.sample(lens, 3, 10, rank=0))


def test_from_config(SpecAugment):
    assert SpecAugment.from_config({}, 40, 3) is None
    assert SpecAugment.from_config({'data': {}, 'hparas': {}}, 40, 3) is None
    assert SpecAugment.from_config({'specaug': {'enable': False}}, 40, 3) is None
    assert SpecAugment.from_config({'specaug': {'enable': False, 'time_warp': 5}}, 40, 3) is None
    sa = SpecAugment.from_config({'specaug': {'enable': True}}, 40, 3)
    assert (sa.feat_dim, sa.channels, sa.freq_mask_width, sa.n_freq_mask, sa.time_mask_width, sa.n_time_mask,
            sa.time_mask_ratio, sa.time_warp, sa.mask_value) == (40, 3, 27, 2, 100, 2, 1.0, 80, 0.0)
    sa = SpecAugment.from_config({'specaug': {'enable': True, 'freq_mask_width': 8, 'n_freq_mask': 1,
                                              'time_mask_width': 10, 'n_time_mask': 8, 'time_mask_ratio': 0.2,
                                              'time_warp': 5, 'mask_value': -1.5}}, 80, 1)
    assert (sa.freq_mask_width, sa.n_freq_mask, sa.time_mask_width, sa.n_time_mask, sa.time_mask_ratio, sa.time_warp,
            sa.mask_value, sa.P) == (8, 1, 10, 8, 0.2, 5, -1.5, 20)
    for bad in ({'enable': True, 'time_wrap': 5},              # unknown key
                {'enable': True, 'freq_mask_width': -1}, {'enable': True, 'time_mask_width': -3},
                {'enable': True, 'time_warp': -80}, {'enable': True, 'n_freq_mask': -1},
                {'enable': True, 'time_mask_ratio': -0.5},
                {'enable': True, 'n_freq_mask': 9}, {'enable': True, 'n_time_mask': 9},
                {'enable': False, 'n_time_mask': 9}):           # a disabled block is still checked
        with pytest.raises(ValueError):
            SpecAugment.from_config({'specaug': bad}, 40, 3)


def test_warp_map_properties():
    """the integer map the kernel evaluates: strictly increasing, fixes frames 0 and n - 1, sends d = c + w to c, and
    every source index stays inside the utterance - for all n < 40 and every admissible (c, w)"""
    for n in range(3, 40):
        for c in range(1, n - 1):
            for w in range(-(n - 1), n):
                if not _admissible(n, c, w):
                    continue
                pos = []
                for t in range(n):
                    i, j, r, den = warp_source(t, n, c, w)
                    assert 0 <= i <= j <= n - 1 and 0 <= r < den
                    pos.append(i + Fraction(r, den))
                assert pos[0] == 0 and pos[-1] == n - 1 and pos[c + w] == c
                assert all(q > p for p, q in zip(pos, pos[1:])), (n, c, w)


def test_argument_errors_without_gpu(lib):
    L = lib.load()
    z, a, b = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    lens, par = ctypes.c_void_p(12288), ctypes.c_void_p(16384)
    ESHAPE = -2
    f = L.asrk_spec_augment_f32
    ok = dict(x=a, y=b, B=2, T=8, ld=120, D=40, C=3, lens=lens, params=par, nf=2, nt=2, fill=0.0, s=z)

    def call(**kw):
        v = dict(ok, **kw)
        return f(v['x'], v['y'], v['B'], v['T'], v['ld'], v['D'], v['C'], v['lens'], v['params'], v['nf'], v['nt'],
                 v['fill'], v['s'])
    for bad in (dict(B=-1), dict(T=-1), dict(ld=-1), dict(D=-1), dict(C=-1), dict(ld=119), dict(nf=-1), dict(nf=9),
                dict(nt=-1), dict(nt=9), dict(y=a), dict(x=z), dict(y=z), dict(lens=z), dict(params=z)):
        assert call(**bad) == ESHAPE, bad
    # empty batches return 0 without a launch (null pointers allowed)
    assert call(B=0, x=z, y=z, lens=z, params=z) == 0
    assert call(T=0, x=z, y=z, lens=z, params=z) == 0
    assert "shape" in lib.strerror(ESHAPE)


def test_operator_refuses_host_tensors(pkg):
    """no CPU fallback: a feature batch that is not on the GPU is an error, with or without a GPU in the machine"""
    ops = importlib.import_module(PKG_NAME + ".ops")
    with pytest.raises(RuntimeError):
        ops.spec_augment(torch.zeros(1, 4, 6), torch.tensor([4]), torch.zeros(1, 2, dtype=torch.int32), 0, 0)
