"""CPU: the host side of speed perturbation - the tap tables and the float64 reference resampler, SpeedPerturb (ratios,
sample counts, config parsing, the stateless per-utterance draw), the argument checks of asrk_resample_rows_f32 (all
before any device call) and the collate function's use of perturbed lengths, with a stub in place of the device front
end."""
import ctypes
import importlib
import math
import os
import wave

import numpy as np
import pytest
import torch

from conftest import PKG_NAME
import speed_perturb_reference as ref


@pytest.fixture(scope="module")
def audio():
    return importlib.import_module(PKG_NAME + ".src.audio")


@pytest.fixture(scope="module")
def lib():
    build = importlib.import_module(PKG_NAME + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib")


@pytest.mark.parametrize("orig,new", [(9, 10), (11, 10), (19, 20), (2, 1)])
def test_tables(orig, new):
    """every phase is a unit-gain low-pass; the package's table is the reference's"""
    h = ref.taps_table(orig, new)
    base, width, taps = ref.geometry(orig, new)
    assert h.shape == (new, 2 * width + orig) and taps == h.shape[1]
    assert np.abs(h.sum(axis=1) - 1.0).max() < 1e-3
    ops = importlib.import_module(PKG_NAME + ".ops")
    assert ops.resample_width(orig, new) == width
    mine = ops.resample_taps(orig, new)
    assert mine.shape == h.shape and np.abs(mine - h).max() < 1e-14
    assert np.abs(mine.astype(np.float32).astype(np.float64).sum(axis=1) - 1.0).max() < 1e-3


def test_width_is_taken_exactly():
    """the library and the package derive the filter half-width in integers; wherever the float formula of the
    specification is not within an ulp of an integer the two agree (all admissible ratios)"""
    ops = importlib.import_module(PKG_NAME + ".ops")
    for orig in range(1, 101):
        for new in range(1, 101):
            if math.gcd(orig, new) != 1 or orig > 2 * new or new > 2 * orig:
                continue
            q = 6 * orig / (min(orig, new) * 0.99)
            if abs(q - round(q)) > 1e-9:
                assert ops.resample_width(orig, new) == math.ceil(q), (orig, new)
            else:
                assert ops.resample_width(orig, new) == round(q), (orig, new)


def test_sine_at_9_to_10():
    """a 1 kHz tone slowed down by 0.9 is a 900 Hz tone, in phase: catches a swapped ratio or a phase slip"""
    n, sr = 4000, 16000
    x = np.sin(2 * np.pi * 1000.0 * np.arange(n) / sr)
    y = ref.resample(x, 9, 10)
    assert y.shape[0] == ref.out_samples(n, 9, 10) == 4445
    o = np.arange(y.shape[0])
    want = np.sin(2 * np.pi * 900.0 * o / sr)
    err = np.abs(y - want)[200:-200].max()
    print("interior error of the 9:10 sine: %.3e" % err)
    assert err < 2e-3
    swapped = ref.resample(x, 10, 9)                              # the swapped ratio is a 1111 Hz tone of 3600 samples
    assert swapped.shape[0] == 3600 and np.abs(swapped - want[:3600])[200:-200].max() > 0.5


def test_out_samples(audio):
    SP = audio.SpeedPerturb
    assert SP.ratio(0.9) == (9, 10) and SP.ratio(1.1) == (11, 10) and SP.ratio(1.0) == (1, 1) and SP.ratio(1) == (1, 1)
    assert SP.ratio(0.95) == (19, 20) and SP.ratio(2.0) == (2, 1) and SP.ratio(0.5) == (1, 2)
    assert SP.ratio(1.05) == (21, 20) and SP.ratio(0.99) == (99, 100) and SP.ratio(1.98) == (99, 50)
    for f in (1.01, 1.99, 1.37):                                  # orig > 100: beyond the kernel's table limit
        with pytest.raises(ValueError):
            SP.ratio(f)
    big = 2 ** 31 // 100
    for f in (0.9, 1.0, 1.1, 0.95, 2.0, 0.5, 0.87):
        orig, new = SP.ratio(f)
        assert math.gcd(orig, new) == 1 and abs(orig / new - f) < 1e-12
        for n in list(range(51)) + list(range(big - 3, big + 4)):
            want = -(-new * n // orig)                                       # ceil(new * n / orig)
            assert SP.out_samples(n, f) == want == ref.out_samples(n, orig, new)


def test_from_config(audio):
    SP = audio.SpeedPerturb
    assert SP.from_config({}) is None
    assert SP.from_config({'data': {}, 'hparas': {}}) is None
    assert SP.from_config({'speed_perturb': {'enable': False}}) is None
    assert SP.from_config({'speed_perturb': {'enable': False, 'factors': [0.9, 1.0]}}) is None
    sp = SP.from_config({'speed_perturb': {'enable': True}}, seed=7)
    assert sp.factors == [0.9, 1.0, 1.1] and sp.ratios == [(9, 10), (1, 1), (11, 10)] and sp.seed == 7
    sp = SP.from_config({'speed_perturb': {'enable': True, 'factors': [0.95, 1, 1.05, 2.0]}})
    assert sp.factors == [0.95, 1.0, 1.05, 2.0] and sp.ratios == [(19, 20), (1, 1), (21, 20), (2, 1)]
    assert '19:20' in sp.create_msg() and '0.95' in sp.create_msg()
    for bad in ({'enable': True, 'factor': [0.9]},                     # unknown key
                {'enable': True, 'factors': [0.9, 'fast']}, {'enable': True, 'factors': [True]},
                {'enable': True, 'factors': [None]}, {'enable': True, 'factors': 0.9},
                {'enable': True, 'factors': [0.905]},                  # more than two decimals
                {'enable': True, 'factors': [0.49]}, {'enable': True, 'factors': [2.01]},
                {'enable': True, 'factors': [1.01]},                   # 101:100 is beyond the kernel's limits
                {'enable': True, 'factors': [float('nan')]}, {'enable': True, 'factors': [-1.0]},
                {'enable': True, 'factors': []},
                {'enable': True, 'factors': [0.9, 0.91, 0.92, 0.93, 0.94, 0.95, 0.96, 0.97, 0.98]},
                {'enable': 'yes'},
                {'enable': False, 'factors': []}):                     # a disabled block is still checked
        with pytest.raises(ValueError):
            SP.from_config({'speed_perturb': bad})
    with pytest.raises(ValueError):
        SP.from_config({'speed_perturb': [0.9, 1.0]})


def test_sampling_is_stateless_and_rank_independent(audio):
    SP = audio.SpeedPerturb
    names = ['%d-%d-%04d' % (100 + i % 7, 2000 + i % 13, i) for i in range(3000)]
    a = SP([0.9, 1.0, 1.1], seed=3)
    a.begin_epoch(120)
    draws = [a.factor(nm) for nm in names]
    torch.manual_seed(99)                                         # no generator, global or otherwise, plays a part
    # "another rank": a fresh object in a different order of calls gives every utterance the same factor
    b = SP([0.9, 1.0, 1.1], seed=3)
    b.begin_epoch(120)
    assert [b.factor(nm) for nm in reversed(names)] == draws[::-1]
    assert [a.factor(nm) for nm in names] == draws
    # the documented formula
    z = audio._splitmix64(3 ^ audio._splitmix64(120) ^ __import__('zlib').crc32(names[5].encode()))
    assert draws[5] == [0.9, 1.0, 1.1][z % 3]
    for f in (0.9, 1.0, 1.1):
        share = draws.count(f) / len(draws)
        assert 0.28 <= share <= 0.39, (f, share)
    # another epoch key or another seed is another draw
    b.begin_epoch(121)
    assert [b.factor(nm) for nm in names] != draws
    c = SP([0.9, 1.0, 1.1], seed=4)
    c.begin_epoch(120)
    assert [c.factor(nm) for nm in names] != draws
    assert SP([1.1]).factor('x') == 1.1


def test_argument_errors_without_gpu(lib):
    L = lib.load()
    f = L.asrk_resample_rows_f32
    z, a, b, c = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288)
    ESHAPE = -2
    vp = lambda arr: ctypes.c_void_p(arr.ctypes.data)

    def call(**kw):
        v = dict(x=a, sb=2, ld_in=100, n=[100, 50, 0], idx=[0, 1, 2], B=3, ratios=[(9, 10), (1, 1), (11, 10)],
                 taps=[16384, 0, 20480], nr=None, y=b, ld_out=112, n_dev=c, idx_dev=c, scale=1.0)
        v.update(kw)
        n, idx = np.asarray(v['n'] or [], dtype=np.int64), np.asarray(v['idx'] or [], dtype=np.int32)
        rat = np.asarray(v['ratios'] or [], dtype=np.int32).reshape(-1, 2)
        taps = (ctypes.c_void_p * max(1, len(v['taps'] or [])))(*(v['taps'] or []))
        nr = len(v['ratios']) if v['nr'] is None else v['nr']
        return f(v['x'], v['sb'], v['ld_in'], z if v['n'] is None else vp(n), v['n_dev'],
                 z if v['idx'] is None else vp(idx), v['idx_dev'], v['B'], z if v['ratios'] is None else vp(rat),
                 z if v['taps'] is None else taps, nr, v['y'], v['ld_out'], v['scale'], z)

    nine = [(9, 10)] * 9
    for bad in (dict(B=-1), dict(ld_in=-1), dict(ld_out=-1), dict(nr=-1), dict(sb=1), dict(sb=3), dict(sb=8),
                dict(y=a),                                                     # x == y
                dict(ld_out=111),                                              # row 0 needs ceil(1000 / 9) = 112
                dict(n=[101, 50, 0]), dict(n=[100, -1, 0]),                    # a length outside 0..ld_in
                dict(idx=[0, 1, 3]), dict(idx=[0, -1, 2]),                     # a ratio index out of range
                dict(ratios=nine, taps=[16384] * 9, idx=[0, 0, 0]),            # more than 8 ratios
                dict(ratios=[(101, 100), (1, 1), (11, 10)]), dict(ratios=[(9, 10), (1, 1), (100, 101)]),
                dict(ratios=[(0, 10), (1, 1), (11, 10)]), dict(ratios=[(9, -10), (1, 1), (11, 10)]),
                dict(ratios=[(18, 20), (1, 1), (11, 10)]),                     # not coprime
                dict(ratios=[(21, 10), (1, 1), (11, 10)], ld_out=200), dict(ratios=[(10, 21), (1, 1), (11, 10)], ld_out=400),
                dict(x=z), dict(y=z), dict(n=None), dict(idx=None), dict(ratios=None, nr=3), dict(taps=None),
                dict(n_dev=z), dict(idx_dev=z),
                dict(taps=[0, 0, 20480])):                                     # the table of a ratio that has work
        assert call(**bad) == ESHAPE, bad
    # nothing to do: 0 without a launch, null pointers allowed
    assert call(B=0, x=z, y=z, n=None, idx=None, ratios=None, taps=None, nr=0, n_dev=z, idx_dev=z) == 0
    assert call(n=[0, 0, 0], x=z, y=z, n_dev=z, idx_dev=z, ld_out=0) == 0
    # the table of a ratio that no row with samples uses is not needed (here both filtered ratios), but 50 samples of a
    # 1:1 row are work: x, y and the device copies must be there
    assert call(n=[0, 50, 0], taps=[0, 0, 0], x=z, y=z, n_dev=z, idx_dev=z) == ESHAPE
    assert "shape" in lib.strerror(ESHAPE)


def test_operator_refuses_host_tensors(pkg):
    """no CPU fallback: a waveform batch that is not on the GPU is an error, with or without a GPU in the machine"""
    ops = importlib.import_module(PKG_NAME + ".ops")
    with pytest.raises(RuntimeError):
        ops.resample_rows(torch.zeros(1, 40), [40], [0], [(9, 10)], 1.0)


# ---- the collate function under a policy, with a stub in place of the device front end ---------------------------

class _StubBatch:
    """BatchFeatureTransform's interface: one frame per sample, records what it is called with"""

    def __init__(self, SP):
        self.SP, self.calls = SP, []

    def frame_count(self, n_samples, sample_rate):
        return n_samples

    def __call__(self, waves, sample_rate, speeds=None):
        self.calls.append(dict(lens=[len(w) for w in waves], speeds=None if speeds is None else list(speeds)))
        fs = [1.0] * len(waves) if speeds is None else speeds
        lens = [self.SP.out_samples(len(w), f) for w, f in zip(waves, fs)]
        return torch.zeros(len(waves), max(lens), 1), torch.LongTensor(lens)


class _StubTransform:
    def __init__(self, batch):
        self.batch = batch


def _write_wav(path, n):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.arange(n) % 100).astype('<i2').tobytes())


def _named(sp, want, taken):
    """an utterance name the policy gives factor `want` in the current epoch"""
    for i in range(10000):
        nm = 'utt%05d' % i
        if nm not in taken and sp.factor(nm) == want:
            taken.add(nm)
            return nm
    raise AssertionError


def test_collate_uses_perturbed_lengths(audio, tmp_path):
    data = importlib.import_module(PKG_NAME + ".src.data")
    SP = audio.SpeedPerturb
    sp = SP([0.9, 1.0, 1.1], seed=5)
    sp.begin_epoch(40)
    taken = set()
    # (samples, factor): the first utterance decides halving - 750 samples are 834 frames at 0.9 (> 800), 682 at 1.1
    plan = [(750, 0.9), (700, 1.1), (690, 0.9), (720, 1.0), (300, 1.1), (310, 0.9), (305, 1.0), (10, 0.9)]
    batch = []
    for k, (n, f) in enumerate(plan):
        p = os.path.join(str(tmp_path), _named(sp, f, taken) + '.wav')
        _write_wav(p, n)
        batch.append((p, [k + 1, 3]))
    pert = [SP.out_samples(n, f) for n, f in plan]
    assert pert[0] == 834 and pert[1] == 637

    def run(batch, mode, shard=None, policy=sp):
        stub = _StubBatch(SP)
        out = data.collect_audio_batch(list(batch), _StubTransform(stub), mode, shard=shard, speed_perturb=policy)
        assert len(stub.calls) == 1
        return out, stub.calls[0]

    # halving by the PERTURBED frame count of the first utterance (plain: 750 <= 800, no halving)
    (names, feat, flen, txt), call = run(batch, 'train')
    assert len(names) == 4 and sorted(call['lens']) == sorted(n for n, _ in plan[:4])
    (names_plain, _, flen_plain, _), call_plain = run(batch, 'train', policy=None)
    assert len(names_plain) == 8 and call_plain['speeds'] is None
    assert flen_plain.tolist() == sorted((n for n, _ in plan), reverse=True)
    # order within the batch: descending PERTURBED length (690 at 0.9 = 767 comes before 720 at 1.0); feat_len likewise
    assert flen.tolist() == sorted(pert[:4], reverse=True) == [834, 767, 720, 637]
    assert call['lens'] == [750, 690, 720, 700] and call['speeds'] == [0.9, 0.9, 1.0, 1.1]
    assert txt[:, 0].tolist() == [1, 3, 4, 2]                     # transcripts follow their utterances, untouched
    assert [os.path.basename(b[0])[:-4] for b in (batch[0], batch[2], batch[3], batch[1])] == list(names)
    # 'test' mode never halves
    assert len(run(batch, 'test')[0][0]) == 8
    # a first utterance at 1.1 does not halve
    swapped = [batch[1]] + [batch[0]] + batch[2:]
    assert len(run(swapped, 'train')[0][0]) == 8
    # world 2: the halved global batch is dealt by perturbed length; the shards are disjoint and cover it
    shards = [run(batch, 'train', shard=(r, 2)) for r in range(2)]
    got = [list(s[0][0]) for s in shards]
    assert not set(got[0]) & set(got[1]) and sorted(got[0] + got[1]) == sorted(names)
    assert [s[0][2].tolist() for s in shards] == [[834, 720], [767, 637]]      # deal_global_batch on [834, 637, 767, 720]
    assert shards[0][1]['speeds'] == [0.9, 1.0] and shards[1][1]['speeds'] == [0.9, 1.1]
