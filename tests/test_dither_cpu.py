"""CPU: the dither's noise function and reference (tests/dither_reference.py), the key policy (src/audio.py Dither) and
the host-side refusals of the three dithered ABI entries.  No GPU is needed."""
import ctypes
import importlib
import zlib

import numpy as np
import pytest

import audio_reference as R
import dither_reference as DR
from conftest import PKG_NAME

EINVAL, ESHAPE = -1, -2


@pytest.fixture(scope="module")
def audio(pkg):
    return importlib.import_module(PKG_NAME + ".src.audio")


@pytest.fixture(scope="module")
def lib():
    importlib.import_module(PKG_NAME + ".build").build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib").load()


# ------------------------------------------------------------------------------------------------ the noise function
def test_noise_moments_and_range():
    z = DR.noise(DR.KEYS[0], 200, 400, np.float64)
    n = z.size
    assert z.shape == (200, 400)
    mean, var, zmax = float(z.mean()), float(z.var()), float(np.abs(z).max())
    print("DITHER noise | n %d | mean %.4f (5/sqrt n %.4f) | std %.4f | max |z| %.3f" % (n, mean, 5 / np.sqrt(n),
                                                                                       np.sqrt(var), zmax))
    assert abs(mean) <= 5.0 / np.sqrt(n)
    assert abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert zmax <= 5.78 and DR.Z_MAX <= 5.78


def test_noise_is_a_pure_function_of_key_frame_and_position():
    a = DR.noise(DR.KEYS[2], 6, 100)
    assert np.array_equal(a[:4, :37], DR.noise(DR.KEYS[2], 4, 37))            # no dependence on m or win
    assert not np.array_equal(a, DR.noise(DR.KEYS[2] ^ 1, 6, 100))
    assert not np.array_equal(a, DR.noise(DR.KEYS[2] ^ (1 << 40), 6, 100))     # the key's high word matters
    assert len(np.unique(a)) == a.size                                         # frames and positions all differ
    # the layout of the contract: position j takes word pair (j & 3) >> 1 of counter (j >> 2, f, 0, 0)
    key, f, j = DR.KEYS[3], 5, 42
    r = DR.RO.philox4x32_10(np.array([[j >> 2, f, 0, 0]], np.uint32), (key & 0xFFFFFFFF, key >> 32))[0]
    u1 = (float(r[2] >> 8) + 1.0) * 2.0 ** -24
    u2 = float(r[3] >> 8) * 2.0 ** -24
    assert j & 3 == 2
    assert DR.noise(key, 6, 100)[f, j] == pytest.approx(np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2), abs=1e-15)


def test_float32_noise_error():
    e = DR.noise_e32(DR.KEYS[0], 200, 400)
    print("DITHER noise | e32 %.3e" % e)
    assert 0.0 < e < 1e-5                 # a handful of float32 roundings of values below 5.78


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_without_dither_is_audio_reference():
    for case in DR.GEOMETRIES:
        x = R.as_float(DR.case_waves(case, "int16")[2])
        for dt in (np.float64, np.float32):
            a = DR.logmel(x, case.sr, case.nmel, case.frame_ms, dither=0.0, dtype=dt)
            assert np.array_equal(a, R.logmel(x, case.sr, case.nmel, case.frame_ms, dtype=dt)), case.name
        b = DR.logmel(x, case.sr, case.nmel, case.frame_ms, dither=2.0 ** -9, key=7, fault="none")
        assert np.array_equal(b, R.logmel(x, case.sr, case.nmel, case.frame_ms))


@pytest.mark.parametrize("case", DR.GEOMETRIES, ids=[c.name for c in DR.GEOMETRIES])
def test_seeded_faults_are_told_apart(case):
    """no dither, another key, one noise value per waveform sample: each at least 100 bounds from the true output, on
    the 7-frame utterance of every geometry at dither 2^-9; and nothing of it sits near the clamp"""
    dither, b = 2.0 ** -9, DR.FRAMES.index(7)
    x, key = R.as_float(DR.case_waves(case, "int16")[b]), DR.KEYS[b]
    run = lambda dt, fault=None: DR.logmel(x, case.sr, case.nmel, case.frame_ms, dither=dither, key=key, dtype=dt,
                                           fault=fault)
    ref = run(np.float64)
    assert ref.shape == (7, case.nmel)
    e32 = R.max_err(run(np.float32), ref)
    bound = DR.bound("logmel", e32)
    emin = float(DR.mel_energy(x, case.sr, case.nmel, case.frame_ms, dither=dither, key=key).min())
    ratios = {f: R.max_err(run(np.float64, f), ref) / bound for f in ("none", "key", "per_sample")}
    print("DITHER faults %s | e32 %.3e | bound %.3e | min energy %.0f eps | fault/bound %s"
          % (case.name, e32, bound, emin / R.FLT_EPS, {k: round(v) for k, v in ratios.items()}))
    assert emin >= 100.0 * R.FLT_EPS
    for f, ratio in ratios.items():
        assert ratio >= 100.0, (case.name, f, ratio)


def test_every_row_stays_clear_of_the_clamp():
    for case in DR.CASES:
        for d in DR.DITHERS:
            for w, k in zip(DR.case_waves(case, "int16"), DR.KEYS):
                if len(w) >= case.win:
                    e = DR.mel_energy(R.as_float(w), case.sr, case.nmel, case.frame_ms, dither=d, key=k,
                                      **DR.case_kwargs(case))
                    assert e.min() >= 100.0 * R.FLT_EPS, (case.name, d, e.min() / R.FLT_EPS)


def test_dither_lifts_digital_silence_off_the_clamp():
    x = np.zeros(16000 // 4)
    plain = DR.logmel(x, 16000, 40, 25.0)
    assert np.all(plain == R.LOG_FLOOR)
    e = DR.mel_energy(x, 16000, 40, 25.0, dither=2.0 ** -6, key=DR.KEYS[1])
    print("DITHER silence | min energy %.0f eps" % (e.min() / R.FLT_EPS))
    assert e.min() >= 100.0 * R.FLT_EPS


# ------------------------------------------------------------------------------------------------ the key policy
def test_dither_key(audio):
    D = audio.Dither
    a, b = D(3.05e-5, seed=5), D(3.05e-5, seed=5)
    k = a.key("7-9-0001", True)
    assert isinstance(k, int) and 0 <= k < 1 << 64
    assert k == b.key("7-9-0001", True) == a.key("7-9-0001", True)            # deterministic; no rank enters
    assert k != a.key("7-9-0002", True) and k != D(3.05e-5, seed=6).key("7-9-0001", True)
    assert k == a.key("7-9-0001", False)                                       # epoch key 0 is the evaluation key's
    a.begin_epoch(120)
    k1 = a.key("7-9-0001", True)
    assert k1 != k and a.key("7-9-0001", False) == k                           # training redraws, evaluation does not
    a.begin_epoch(240)
    assert a.key("7-9-0001", True) not in (k, k1) and a.key("7-9-0001", False) == k
    # not the number SpeedPerturb.factor hashes for the same (seed, epoch key, name)
    sm = audio._splitmix64
    for ek in (0, 120):
        a.begin_epoch(ek)
        speed_hash = sm((5 & audio._M64) ^ sm(ek) ^ zlib.crc32(b"7-9-0001"))
        assert a.key("7-9-0001", True) != speed_hash
        assert a.key("7-9-0001", True) == sm((5 & audio._M64) ^ sm(ek) ^ zlib.crc32(b"7-9-0001") ^ D.TAG)
    assert D.TAG >> 32 and D.TAG < 1 << 64
    assert "3.05e-05" in a.create_msg()


def test_from_config(audio):
    D = audio.Dither
    cfg = lambda **kw: {"data": {"audio": dict(feat_type="fbank", feat_dim=40, **kw)}}
    assert D.from_config(cfg()) is None and D.from_config(cfg(dither=0)) is None
    assert D.from_config(cfg(dither=0.0), seed=3) is None and D.from_config({}) is None and D.from_config(None) is None
    p = D.from_config(cfg(dither=3.05e-5), seed=3)
    assert p.amplitude == 3.05e-5 and p.seed == 3 and p.epoch_key == 0
    assert D.from_config(cfg(dither=1), seed=3).amplitude == 1.0
    for bad in (-1e-5, float("nan"), float("inf"), "0.1", True, None, [1e-5]):
        with pytest.raises(ValueError):
            D.from_config(cfg(dither=bad))
        with pytest.raises(ValueError):
            D(bad, 0)
    base = dict(feat_type="fbank", feat_dim=40, apply_cmvn=True)
    with pytest.raises(ValueError):
        audio.BatchFeatureTransform(dict(base, dither=-1.0), device="cpu")
    assert audio.BatchFeatureTransform(dict(base, dither=2.0 ** -9), device="cpu").dither == 2.0 ** -9
    assert audio.BatchFeatureTransform(dict(base), device="cpu").dither == 0.0


# ------------------------------------------------------------------------------------------------ ABI host logic
def test_dithered_entries_refuse_before_any_launch(lib):
    z, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    nan, inf = float("nan"), float("inf")

    def per_file(wave=fake, n=1000, window=fake, frames=fake, m=4, win=400, shift=160, ldf=400, dither=1e-3):
        return lib.asrk_fbank_frames_dither_f32(wave, n, window, frames, m, win, shift, ldf, 0.97, 1, dither, 7, z)

    for d in (-1e-3, nan, inf, -inf):
        assert per_file(dither=d) == EINVAL
    assert per_file(m=-1) == EINVAL and per_file(win=0) == EINVAL and per_file(shift=0) == EINVAL
    assert per_file(ldf=399) == EINVAL and per_file(n=879) == EINVAL          # frame 3 ends at sample 880
    assert per_file(wave=z) == EINVAL and per_file(window=z) == EINVAL and per_file(frames=z) == EINVAL
    assert per_file(m=0, wave=z) == 0 and per_file(m=0, dither=nan) == EINVAL

    def frames_batch(wave=fake, sb=4, ld=1000, off=fake, B=1, max_m=4, window=fake, frames=fake, win=400, ldf=400,
                     dither=1e-3, keys=fake, n_host=None):
        return lib.asrk_fbank_frames_batch_dither_f32(wave, sb, ld, n_host, off, B, max_m, window, frames, win, 160, ldf,
                                                      1.0, 0.97, 1, dither, keys, z)

    assert frames_batch(keys=z) == EINVAL
    for d in (-1e-3, nan, inf):
        assert frames_batch(dither=d) == EINVAL
    assert frames_batch(sb=3) == EINVAL and frames_batch(max_m=5) == EINVAL and frames_batch(ld=879) == EINVAL
    assert frames_batch(ldf=399) == EINVAL and frames_batch(B=-1) == EINVAL
    assert frames_batch(wave=z) == EINVAL and frames_batch(off=z) == EINVAL and frames_batch(frames=z) == EINVAL
    too_long = (ctypes.c_int64 * 1)(1001)
    assert frames_batch(n_host=ctypes.cast(too_long, ctypes.c_void_p)) == EINVAL
    assert frames_batch(B=0, keys=z) == 0 and frames_batch(max_m=0, keys=z) == 0      # nothing to do: nothing is read
    assert frames_batch(B=0, dither=-1.0) == EINVAL

    def logmel(wave=fake, sb=4, ld=1000, off=fake, B=1, max_m=4, tab=fake, mel=fake, nmel=40, ld_mel=40, win=400,
               log2n=9, dither=1e-3, keys=fake):
        return lib.asrk_fbank_logmel_batch_dither_f32(wave, sb, ld, None, off, B, max_m, tab, tab, tab, tab, tab, nmel,
                                                      ld_mel, mel, win, 160, log2n, 1.0, 0.97, 1, R.FLT_EPS, dither,
                                                      keys, z)

    assert logmel(keys=z) == EINVAL
    for d in (-1e-3, nan, inf):
        assert logmel(dither=d) == EINVAL
    assert logmel(log2n=7) == ESHAPE and logmel(log2n=11) == ESHAPE and logmel(win=513) == ESHAPE
    assert logmel(sb=3) == EINVAL and logmel(max_m=5) == EINVAL and logmel(ld=879) == EINVAL
    assert logmel(nmel=0) == EINVAL and logmel(ld_mel=39) == EINVAL
    assert logmel(wave=z) == EINVAL and logmel(tab=z) == EINVAL and logmel(mel=z) == EINVAL
    assert logmel(B=0, keys=z) == 0 and logmel(max_m=0, keys=z) == 0
