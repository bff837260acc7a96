"""CPU: the float64 reference of the reverberation / noise entry checks itself, its bound has teeth (four seeded faults),
the NoiseReverb policy draws what it says, refuses what it should, loads responses and fills noise rows as specified,
and asrk_reverb_mix_f32 validates its arguments before any device call."""
import ctypes
import importlib
import math
import os
import wave

import numpy as np
import pytest

import noise_reverb_reference as ref
from conftest import PKG_NAME


# ------------------------------------------------------------------------------------------------ the reference
def test_table_covers_what_the_kernel_can_get_wrong():
    rows = [r for c in ref.CASES for r in c.rows]
    ns, Ks = {r.n for r in rows}, {r.K for r in rows}
    assert {0, 1, 2, 255, 256, 257, 1023, 1025, 2049, 4099} <= ns
    assert {1, 2, 63, 64, 65, 255, 257, 1025, 8192} <= Ks
    assert all(r.n == 300 for r in rows if r.K == 8192)
    assert {ref.TILE - 1, ref.TILE, ref.TILE + 1} <= ns and {ref.CHUNK - 1, ref.CHUNK, ref.CHUNK + 1} <= Ks
    assert {r.peak for r in rows if r.K > 2} == {'first', 'mid', 'last'}
    assert all(3 <= len(c.rows) <= 6 for c in ref.CASES)
    assert {c.dtype for c in ref.CASES} == {"int16", "float32"}
    assert {c.pad % 4 == 0 for c in ref.CASES} == {True, False}
    noisy = [r for r in rows if r.m > 0 and r.n > 0]
    assert any(r.m == 1 for r in noisy) and any(r.m == 7 and r.n > 100 for r in noisy)
    assert any(r.m == r.n - 1 for r in noisy) and any(r.m == r.n for r in noisy) and any(r.m == r.n + 1 for r in noisy)
    assert any(r.kind == 'zero-x' for r in rows) and any(r.kind == 'zero-v' for r in rows)
    assert any(any(r.K == 0 and r.m == 0 for r in c.rows) and any(r.K > 0 and r.m > 0 for r in c.rows) for c in ref.CASES)


def test_unit_response_is_the_identity():
    d = ref.case_data(2)[0]
    s = d['x'].astype(np.float64) * d['scale']
    out = ref.reverb_mix(d['x'], d['scale'], np.ones(1, np.float32), 0, None, 1.0)
    assert np.array_equal(out, s)
    assert np.array_equal(ref.reverb_mix(d['x'], d['scale'], None, 0, None, 1.0), s)


def test_power_after_reverberation_and_achieved_snr():
    for ci, b in ref.all_rows():
        d, row = ref.case_data(ci)[b], ref.CASES[ci].rows[b]
        out, rev, noise = ref.reverb_mix(d['x'], d['scale'], d['h'], d['p'], d['v'], d['snr_lin'], parts=True)
        assert np.all(np.isfinite(out))
        s = d['x'].astype(np.float64) * float(np.float32(d['scale']))
        Ps = float(np.sum(s ** 2))
        if row.kind == 'zero-x':
            assert not out.any()
            continue
        if row.n == 0:
            continue
        assert abs(float(np.sum(rev ** 2)) - Ps) <= 1e-9 * Ps, (ci, b)
        if row.m > 0 and row.kind != 'zero-v':
            got_db = 10.0 * math.log10(Ps / float(np.sum(noise ** 2)))
            want_db = 10.0 * math.log10(d['snr_lin'])
            assert abs(got_db - want_db) <= 1e-9, (ci, b, got_db, want_db)
        else:
            assert not noise.any()


def test_wrap_indices():
    assert ref.wrap_indices(7, 3).tolist() == [0, 1, 2, 0, 1, 2, 0]
    assert ref.wrap_indices(3, 7).tolist() == [0, 1, 2]
    assert ref.wrap_indices(4, 1).tolist() == [0, 0, 0, 0]
    x, v = np.zeros(5, np.float32), np.asarray([1.0, 2.0], np.float32)
    x[0] = 1.0
    _, _, noise = ref.reverb_mix(x, 1.0, None, 0, v, 1.0, parts=True)
    assert np.allclose(noise / noise[0], [1, 2, 1, 2, 1])


def test_bound_is_derived_and_small():
    fl = ref.floor()
    assert 0.0 < fl < 1e-4                       # f32 accumulation of signals of order one: far below any audible level
    for ci, b in ref.all_rows():
        assert ref.bound(ci, b) >= fl
        assert ref.bound(ci, b) <= max(8.0 * ref.e32(ci, b), fl)


@pytest.mark.parametrize("fault", ["tap", "peak", "wrap", "snr"])
def test_seeded_faults_exceed_the_bound(fault):
    worst = 0.0
    for ci, b in ref.all_rows():
        err = ref.max_err(ref.expected(ci, b, "float64", fault), ref.expected(ci, b, "float64"))
        worst = max(worst, err / ref.bound(ci, b))
    print("fault %s: worst error / bound = %.3g" % (fault, worst))
    assert worst > 1.0


# ------------------------------------------------------------------------------------------------ the policy
@pytest.fixture(scope="module")
def audio():
    return importlib.import_module(PKG_NAME + ".src.audio")


def _write(path, samples, sr=16000, channels=1):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    q = np.asarray(samples, dtype='<i2')
    if channels > 1:
        q = np.stack([q] + [np.full_like(q, 77)] * (channels - 1), axis=1)
    with wave.open(path, 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(q.tobytes())


@pytest.fixture()
def dirs(tmp_path):
    rng = np.random.default_rng(0)
    rir, noise = str(tmp_path / "rir"), str(tmp_path / "noise")
    for i in range(5):
        h = (rng.standard_normal(200) * np.exp(-np.arange(200) / 40.0) * 3000).astype(np.int16)
        h[3 + i] = 20000
        _write(os.path.join(rir, "room%d" % (i % 2), "r%d.wav" % i), h)
    for i in range(3):
        _write(os.path.join(noise, "n%d.wav" % i), (rng.standard_normal(500 + 100 * i) * 2000).astype(np.int16))
    return rir, noise


def test_draw_is_deterministic_and_stateless(audio, dirs):
    rir, noise = dirs
    mk = lambda seed: audio.NoiseReverb(rir={'path': rir, 'prob': 0.5}, noise={'path': noise, 'prob': 0.5,
                                                                               'snr_db': [5, 20]}, seed=seed)
    a, b = mk(3), mk(3)
    names = ["utt-%04d" % i for i in range(200)]
    assert [a.draw(n) for n in names] == [b.draw(n) for n in names]
    # independent of the batch an utterance sits in (and of the rank: nothing but seed, epoch, name enters)
    batch = a.draws(names[10:20])
    assert len(batch) == 10 and batch.draws[4] == a.draw(names[14])
    assert a.draws(list(reversed(names[10:20]))).draws[5] == a.draw(names[14])
    # changes across epochs, comes back with the key; another seed is another stream
    e0 = [a.draw(n) for n in names]
    a.begin_epoch(17)
    e1 = [a.draw(n) for n in names]
    assert e0 != e1
    a.begin_epoch(0)
    assert [a.draw(n) for n in names] == e0
    assert [mk(4).draw(n) for n in names] != e0
    for d in e0 + e1:
        assert -1 <= d.rir < 5 and -1 <= d.noise < 3 and 0.0 <= d.offset < 1.0 and 5.0 <= d.snr_db <= 20.0
    assert len({d.rir for d in e0}) == 6 and len({d.noise for d in e0}) == 4
    assert batch.any()


def test_prob_zero_and_one_and_frequency(audio, dirs):
    rir, noise = dirs
    names = ["spk-%05d" % i for i in range(10000)]
    never = audio.NoiseReverb(rir={'path': rir, 'prob': 0.0}, noise={'path': noise, 'prob': 0}, seed=1)
    assert all(never.draw(n).rir == -1 and never.draw(n).noise == -1 for n in names[:500])
    assert not never.draws(names[:50]).any()
    always = audio.NoiseReverb(rir={'path': rir, 'prob': 1.0}, noise={'path': noise, 'prob': 1, 'snr_db': [7, 7]}, seed=1)
    assert all(always.draw(n).rir >= 0 and always.draw(n).noise >= 0 and always.draw(n).snr_db == 7.0
               for n in names[:500])
    only_rir = audio.NoiseReverb(rir={'path': rir, 'prob': 1.0}, seed=1)
    assert all(only_rir.draw(n).rir >= 0 and only_rir.draw(n).noise == -1 for n in names[:100])
    only_noise = audio.NoiseReverb(noise={'path': noise, 'prob': 1.0}, seed=1)
    assert all(only_noise.draw(n).rir == -1 and only_noise.draw(n).noise >= 0 for n in names[:100])
    p = 0.3
    pol = audio.NoiseReverb(rir={'path': rir, 'prob': p}, noise={'path': noise, 'prob': 0.5}, seed=9)
    hits = sum(pol.draw(n).rir >= 0 for n in names)
    assert abs(hits / len(names) - p) <= 3.0 * math.sqrt(p * (1 - p) / len(names)), hits
    assert 'NoiseReverb' in pol.create_msg() and '\n' not in pol.create_msg()


def test_configuration_errors(audio, dirs, tmp_path):
    rir, noise = dirs
    NR = audio.NoiseReverb
    ok = {'enable': True, 'rir': {'path': rir, 'prob': 0.5, 'max_taps': 100},
          'noise': {'path': noise, 'prob': 0.5, 'snr_db': [0, 10]}}
    pol = NR.from_config({'noise_reverb': ok}, seed=2)
    assert pol is not None and pol.max_taps == 100 and len(pol.rirs) == 5 and all(len(h) == 100 for h in pol.rirs)
    assert NR.from_config({}, seed=2) is None and NR.from_config(None) is None
    assert NR.from_config({'noise_reverb': dict(ok, enable=False)}) is None
    assert NR.from_config({'noise_reverb': {'rir': ok['rir']}}).noise_files == []
    assert NR.from_config({'noise_reverb': {'noise': ok['noise']}}).rirs == []
    empty = str(tmp_path / "empty")
    os.makedirs(empty)

    def sub(block, key, value):
        out = {k: dict(v) if isinstance(v, dict) else v for k, v in ok.items()}
        out[block][key] = value
        return out
    bad = [
        [1, 2],
        dict(ok, enable='yes'),
        dict(ok, reverb={}),
        dict(ok, rir=[rir]),
        dict(ok, noise='x'),
        sub('rir', 'taps', 5),
        sub('noise', 'snr', [0, 1]),
        sub('rir', 'prob', -0.1),
        sub('rir', 'prob', 1.5),
        sub('rir', 'prob', 'half'),
        sub('noise', 'prob', 2),
        sub('noise', 'prob', True),
        sub('noise', 'snr_db', [10, 0]),
        sub('noise', 'snr_db', [0, 1, 2]),
        sub('noise', 'snr_db', 5),
        sub('noise', 'snr_db', [0, float('inf')]),
        sub('rir', 'path', empty),
        sub('rir', 'path', str(tmp_path / "missing")),
        sub('noise', 'path', empty),
        sub('noise', 'path', None),
        sub('rir', 'max_taps', 0),
        sub('rir', 'max_taps', 8193),
        sub('rir', 'max_taps', 64.0),
    ]
    for block in bad:
        with pytest.raises(ValueError, match='noise_reverb'):
            NR.from_config({'noise_reverb': block})
        if isinstance(block, dict) and isinstance(block.get('enable'), bool):      # a disabled block is still checked
            with pytest.raises(ValueError, match='noise_reverb'):
                NR.from_config({'noise_reverb': dict(block, enable=False)})


def test_rir_loader(audio, tmp_path):
    d = str(tmp_path / "r")
    h = np.zeros(100, np.int16)
    h[10], h[30] = -9000, 9000                   # two equal maxima: the first one is the peak
    h[50] = 100
    _write(os.path.join(d, "b", "late.wav"), h, channels=2)
    taps, sr = audio.load_rir(os.path.join(d, "b", "late.wav"), 40)
    assert sr == 16000 and taps.dtype == np.float32 and taps.shape == (40,)     # truncated, first channel
    assert int(np.argmax(np.abs(taps))) == 10 and taps[10] == np.float32(-9000 / 32768.0) and taps[30] == -taps[10]
    assert audio.load_rir(os.path.join(d, "b", "late.wav"), 8192)[0].shape == (100,)
    with pytest.raises(ValueError, match='late.wav'):
        audio.load_rir(os.path.join(d, "b", "late.wav"), 10)                    # the peak lies beyond max_taps
    _write(os.path.join(d, "a", "zero.wav"), np.zeros(20, np.int16))
    with pytest.raises(ValueError, match='zero.wav'):
        audio.load_rir(os.path.join(d, "a", "zero.wav"), 100)
    os.remove(os.path.join(d, "a", "zero.wav"))
    _write(os.path.join(d, "a", "Early.WAV"), h)
    with open(os.path.join(d, "a", "notes.txt"), 'w') as f:
        f.write("not audio")
    files = audio.scan_audio_dir(d)
    assert [os.path.relpath(f, d) for f in files] == [os.path.join("a", "Early.WAV"), os.path.join("b", "late.wav")]
    pol = audio.NoiseReverb(rir={'path': d, 'prob': 1.0, 'max_taps': 64})
    assert [len(x) for x in pol.rirs] == [64, 64] and pol.rir_rate == 16000
    with pytest.raises(ValueError, match='Early.WAV'):
        pol.bank('cpu', 8000)                                                   # the corpus' rate differs: refused
    _write(os.path.join(d, "c", "slow.wav"), h, sr=8000)
    with pytest.raises(ValueError, match='slow.wav'):
        audio.NoiseReverb(rir={'path': d})


def test_noise_rows(audio, tmp_path):
    d = str(tmp_path / "n")
    _write(os.path.join(d, "ten.wav"), np.arange(10))
    _write(os.path.join(d, "x8k.wav"), np.arange(10), sr=8000)
    NR = audio.NoiseReverb
    pcm = np.arange(10, dtype=np.int16)
    row = np.full(32, -1, np.int16)
    assert NR.fill_row(row, pcm, 25, 0.35) == 10                 # shorter than the utterance: rotated to the offset
    assert row[:10].tolist() == [3, 4, 5, 6, 7, 8, 9, 0, 1, 2] and np.all(row[10:] == -1)
    row[:] = -1
    assert NR.fill_row(row, pcm, 4, 0.85) == 4                   # longer: n samples from the offset, wrapping at the end
    assert row[:4].tolist() == [8, 9, 0, 1] and np.all(row[4:] == -1)
    row[:] = -1
    assert NR.fill_row(row, pcm, 10, 0.0) == 10 and row[:10].tolist() == list(range(10))
    assert NR.fill_row(row, pcm, 3, 0.9999999) == 3 and row[:3].tolist() == [9, 0, 1]
    assert NR.fill_row(row, pcm[:0], 5, 0.5) == 0 and NR.fill_row(row, pcm, 0, 0.5) == 0
    pol = NR(noise={'path': d, 'prob': 1.0})
    assert [os.path.basename(f) for f in pol.noise_files] == ["ten.wav", "x8k.wav"]
    q = pol.noise_pcm(0, 16000)
    assert q.dtype == np.int16 and q.tolist() == list(range(10)) and pol.noise_pcm(0, 16000) is q     # cached
    with pytest.raises(ValueError, match='x8k.wav'):
        pol.noise_pcm(1, 16000)
    pol.CACHE_BYTES = 30                                         # bounded: the least recently used file leaves
    pol.noise_pcm(1, 8000)
    assert list(pol._cache) == [1] and pol._cache_bytes == 20


class _StubBatch:
    """BatchFeatureTransform's interface: one frame per sample, records the keywords it is called with"""

    def __init__(self):
        self.calls = []

    def frame_count(self, n_samples, sample_rate):
        return n_samples

    def __call__(self, waves, sample_rate, **kw):
        import torch
        self.calls.append(kw)
        lens = [len(w) for w in waves]
        return torch.zeros(len(waves), max(lens), 1), torch.LongTensor(lens)


class _StubTransform:
    def __init__(self, batch):
        self.batch = batch


def test_collate_hands_the_draws_to_the_front_end(audio, dirs, tmp_path):
    """the collate function draws per utterance NAME, in the batch's final order, keeps every length, and without the
    policy it calls the front end exactly as before"""
    data = importlib.import_module(PKG_NAME + ".src.data")
    rir, noise = dirs
    pol = audio.NoiseReverb(rir={'path': rir, 'prob': 0.5}, noise={'path': noise, 'prob': 0.5}, seed=11)
    pol.begin_epoch(3)
    batch = []
    for k, n in enumerate((300, 500, 400, 100)):
        p = os.path.join(str(tmp_path), 'spk-%d.wav' % k)
        _write(p, np.arange(n) % 50)
        batch.append((p, [k + 1, 2]))
    stub = _StubBatch()
    names, feat, flen, txt = data.collect_audio_batch(list(batch), _StubTransform(stub), 'train', noise_reverb=pol,
                                                      train=True)
    assert names == ('spk-1', 'spk-2', 'spk-0', 'spk-3')
    assert flen.tolist() == [500, 400, 300, 100] and txt[:, 0].tolist() == [2, 3, 1, 4]
    assert len(stub.calls) == 1 and set(stub.calls[0]) == {'speeds', 'dither_keys', 'corrupt'}
    call = stub.calls[0]
    assert call['speeds'] is None and call['dither_keys'] is None
    assert call['corrupt'].policy is pol and call['corrupt'].draws == [pol.draw(n) for n in names]
    stub.calls.clear()
    data.collect_audio_batch(list(batch), _StubTransform(stub), 'test')
    assert stub.calls == [{}]                                       # no policy: the call it always was


# ------------------------------------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    build = importlib.import_module(PKG_NAME + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib")


class _Args:
    """a valid call on two rows (fake device pointers: nothing valid is ever sent); fields are overridden per check"""

    def __init__(self, L):
        self.L = L
        self.x, self.v, self.out, self.rir, self.ws = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20
        self.dev = 6 << 20
        self.sample_bytes, self.ld_in, self.ld_v, self.ld_out, self.ld_r = 2, 16, 16, 16, 8
        self.n, self.m, self.idx = [8, 16], [0, 4], [0, -1]
        self.len, self.peak = [4], [1]
        self.B, self.R = 2, 1
        self.ws_bytes = None
        self.null = ()

    def call(self, **over):
        for k, v in over.items():
            assert hasattr(self, k), k
            setattr(self, k, v)
        i64 = lambda a: (ctypes.c_int64 * max(len(a), 1))(*a)
        i32 = lambda a: (ctypes.c_int32 * max(len(a), 1))(*a)
        n, m, idx, ln, pk = i64(self.n), i64(self.m), i32(self.idx), i32(self.len), i32(self.peak)
        P = lambda name, v: None if name in self.null else v
        addr = ctypes.addressof
        ws_bytes = self.L.asrk_reverb_mix_ws_bytes(self.B, max(self.n + [0])) if self.ws_bytes is None else self.ws_bytes
        return self.L.asrk_reverb_mix_f32(
            P('x', self.x), self.sample_bytes, self.ld_in, P('n_host', addr(n)), P('n_dev', self.dev),
            P('rir', self.rir), self.ld_r, P('len_host', addr(ln)), P('len_dev', self.dev + 256),
            P('peak_host', addr(pk)), P('peak_dev', self.dev + 512), self.R, P('idx_host', addr(idx)),
            P('idx_dev', self.dev + 768), P('v', self.v), self.ld_v, P('m_host', addr(m)), P('m_dev', self.dev + 1024),
            P('snr', self.dev + 1280), self.B, P('out', self.out), self.ld_out, 1.0 / 32768.0, P('ws', self.ws),
            ws_bytes, None)


ESHAPE, EWORKSPACE = -2, -3
SHAPE_ERRORS = [
    dict(B=-1), dict(R=-1), dict(ld_in=-1), dict(ld_out=-1), dict(ld_v=-1), dict(ld_r=-1), dict(sample_bytes=3),
    dict(len=[0]), dict(len=[8193], ld_r=8200), dict(len=[9]),                 # K outside 1..8192, K beyond the bank's rows
    dict(peak=[-1]), dict(peak=[4]),                                            # the peak outside 0..K-1
    dict(idx=[1, -1]), dict(idx=[0, -2]),                                       # an index outside -1..R-1
    dict(n=[17, 16]), dict(n=[8, 16], ld_out=15), dict(n=[-1, 16]),             # n beyond ld_in / ld_out, negative
    dict(m=[0, 17]), dict(m=[-1, 4]),                                           # m beyond ld_v, negative
    dict(out=1 << 20), dict(out=2 << 20), dict(out=(1 << 20) + 8),              # out aliases x, v, overlaps x
    dict(null=('x',)), dict(null=('out',)), dict(null=('n_dev',)), dict(null=('idx_dev',)), dict(null=('m_dev',)),
    dict(null=('n_host',)), dict(null=('idx_host',)), dict(null=('m_host',)), dict(null=('len_host',)),
    dict(null=('peak_host',)),
    dict(null=('rir',)), dict(null=('len_dev',)), dict(null=('peak_dev',)),     # a response is in use
    dict(null=('v',)), dict(null=('snr',)),                                     # noise is in use
    dict(ws=(5 << 20) + 4),                                                     # misaligned workspace
]


@pytest.mark.parametrize("over", SHAPE_ERRORS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_abi_shape_errors_without_gpu(lib, over):
    assert _Args(lib.load()).call(**over) == ESHAPE


def test_abi_workspace_and_empty_calls_without_gpu(lib):
    L = lib.load()
    need = L.asrk_reverb_mix_ws_bytes(2, 16)
    assert need > 0
    assert _Args(L).call(ws_bytes=need - 1) == EWORKSPACE
    assert _Args(L).call(ws_bytes=0) == EWORKSPACE
    assert _Args(L).call(null=('ws',)) == EWORKSPACE
    # nothing to do: 0 before any device call, whatever the device pointers are
    everything = ('x', 'out', 'n_dev', 'idx_dev', 'm_dev', 'rir', 'len_dev', 'peak_dev', 'v', 'snr', 'ws')
    assert _Args(L).call(B=0, n=[], m=[], idx=[], null=everything + ('n_host', 'idx_host', 'm_host')) == 0
    assert _Args(L).call(n=[0, 0], null=everything) == 0
    # the workspace grows with B * max n, in whole tiles
    w = L.asrk_reverb_mix_ws_bytes
    assert w(0, 100) == 0 and w(3, 0) == 0
    assert w(1, 1) == w(1, ref.TILE) == 24 and w(1, ref.TILE + 1) == 48
    assert w(7, 5 * ref.TILE) == 7 * 5 * 24
    assert w(32, 256000) == 32 * 125 * 24
