"""GPU: the dithered filterbank front end (csrc/audio.hip DITHER instantiations, src/audio.py, src/data.py, the solver)
against the float64 reference of tests/dither_reference.py.

Criterion as in tests/test_audio_variants_gpu.py: every element within max(8 * e32, floor) of the float64 reference (e32
is the float32 run of the same reference on the same input and keys; nothing is a fixed number), exact zeros in the
padding.  Each row prints e32, the bound and the measured error (pytest -s).  Every test here needs dither > 0 to be
taken, which the code before this feature refused."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import audio_reference as R
import dither_reference as DR
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def audio(ops):
    return importlib.import_module(PKG_NAME + ".src.audio")


@pytest.fixture(scope="module")
def lib(ops):
    return importlib.import_module(PKG_NAME + "._lib").load()


def _config(case, dither, **over):
    cfg = dict(feat_type=case.feat_type, feat_dim=case.nmel, frame_length=case.frame_ms, frame_shift=R.SHIFT_MS,
               dither=dither, apply_cmvn=False, delta_order=0)
    cfg.update(dict(case.opts))
    if case.feat_type == "mfcc":
        cfg["num_ceps"] = R.NUM_CEPS
    cfg.update(over)
    return cfg


def _report(name, kind, dither, e32, bound, err):
    print("DITHERVAR %s | %s | dither 2^%d | e32 %.3e | bound %.3e | device %.3e | device/e32 %.2f"
          % (name, kind, int(round(np.log2(dither))), e32, bound, err, err / e32 if e32 else 0.0))


def _check_padding(got, frames):
    for b, m in enumerate(frames):
        assert np.all(got[b, m:] == 0.0), (b, "padding beyond the utterance is not exactly zero")


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the noise itself
def _noise_setup(dtype):
    win, shift, ldf, frames = 100, 40, 104, (2, 0, 5)
    keys = [DR.KEYS[0], DR.KEYS[1], DR.KEYS[2]]
    ld = win + shift * (max(frames) - 1)
    wave = torch.zeros((3, ld), dtype=dtype, device=DEV)
    window = torch.ones(win, dtype=torch.float32, device=DEV)
    return win, shift, ldf, frames, keys, ld, wave, window


@pytest.mark.parametrize("sample", ["float", "int16"])
def test_noise_through_the_batch_framing_entry(audio, ops, lib, sample):
    """a zero waveform, a window of ones, no pre-emphasis, no DC removal, dither 1: the frame rows ARE the noise"""
    win, shift, ldf, frames, keys, ld, wave, window = _noise_setup(torch.float32 if sample == "float" else torch.int16)
    offs = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    off_g, keys_g = torch.from_numpy(offs).to(DEV), audio._keys_to_device(keys, DEV)
    total = int(offs[-1])
    base = torch.full((total * ldf + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    rc = lib.asrk_fbank_frames_batch_dither_f32(ops._p(wave), 4 if sample == "float" else 2, ld, None, ops._p(off_g), 3,
                                                max(frames), ops._p(window), ops._p(base), win, shift, ldf,
                                                1.0 if sample == "float" else 1.0 / 32768.0, 0.0, 0, 1.0,
                                                ops._p(keys_g), ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    host = base.cpu().numpy()
    assert np.all(host[total * ldf:] == SENTINEL), "wrote beyond the frame rows"
    got = host[:total * ldf].reshape(total, ldf)
    assert np.all(got[:, win:] == 0.0)                                       # pad columns: exact zeros
    for b, m in enumerate(frames):
        ref = DR.noise(keys[b], m, win)
        if m == 0:
            continue
        bound = 8.0 * DR.noise_e32(keys[b], m, win)
        err = R.max_err(got[offs[b]:offs[b + 1], :win], ref)
        print("DITHERVAR noise %s key %#x | e32 %.3e | bound %.3e | device %.3e" % (sample, keys[b], bound / 8, bound, err))
        assert err <= bound, (b, err, bound)
    assert np.abs(got[:, :win]).max() <= DR.Z_MAX
    ops.check_errors()


def test_noise_through_the_per_file_entry(audio, ops, lib):
    win, shift, ldf, frames, keys, ld, wave, window = _noise_setup(torch.float32)
    m, key = 5, keys[2]                                                      # a key above 2^32, by value
    base = torch.full((m * ldf + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    rc = lib.asrk_fbank_frames_dither_f32(ops._p(wave[0]), ld, ops._p(window), ops._p(base), m, win, shift, ldf, 0.0, 0,
                                          1.0, key, ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    host = base.cpu().numpy()
    assert np.all(host[m * ldf:] == SENTINEL)
    got = host[:m * ldf].reshape(m, ldf)
    assert np.all(got[:, win:] == 0.0)
    bound = 8.0 * DR.noise_e32(key, m, win)
    err = R.max_err(got[:, :win], DR.noise(key, m, win))
    print("DITHERVAR noise per file key %#x | e32 %.3e | bound %.3e | device %.3e" % (key, bound / 8, bound, err))
    assert err <= bound
    ops.check_errors()


# ------------------------------------------------------------------------------------------------ 2. every route
@pytest.mark.parametrize("dither", DR.DITHERS, ids=["2^-9", "2^-6"])
@pytest.mark.parametrize("case", DR.CASES, ids=[c.name for c in DR.CASES])
def test_dithered_row(audio, ops, case, dither):
    width, out_kind = R.case_width(case), R.case_kind(case)
    for kind in ("int16", "float32"):
        ref, e32 = DR.expected(case, kind, dither)
        bound = DR.bound(out_kind, e32)
        bt = audio.BatchFeatureTransform(_config(case, dither))
        feat, flen = bt([w.copy() for w in DR.case_waves(case, kind)], case.sr, dither_keys=list(DR.KEYS))
        assert flen.tolist() == list(case.frames)
        assert tuple(feat.shape) == ref.shape == (len(case.frames), max(case.frames), width)
        got = feat.cpu().numpy()
        _check_padding(got, case.frames)
        err = R.max_err(got, ref)
        _report(case.name, "batch " + kind, dither, e32, bound, err)
        assert err <= bound, (case.name, kind, err, bound, e32)
    ref, e32 = DR.expected(case, "float32", dither)
    bound, worst = DR.bound(out_kind, e32), 0.0
    extract = audio.kaldi_fbank if case.feat_type == "fbank" else audio.kaldi_mfcc
    kw = dict(num_ceps=R.NUM_CEPS) if case.feat_type == "mfcc" else {}
    for b, w in enumerate(DR.case_waves(case, "float32")):
        y = extract(torch.from_numpy(w.copy()).unsqueeze(0).to(DEV), case.sr, num_mel_bins=case.nmel,
                    frame_length=case.frame_ms, frame_shift=R.SHIFT_MS, dither=dither, dither_key=DR.KEYS[b],
                    **dict(case.opts), **kw)
        m = case.frames[b]
        assert tuple(y.shape) == (m, width) and y.dtype == torch.float32
        if m:
            worst = max(worst, R.max_err(y.cpu().numpy(), ref[b, :m]))
    _report(case.name, "per file", dither, e32, bound, worst)
    assert worst <= bound, (case.name, worst, bound, e32)
    ops.check_errors()


# ------------------------------------------------------------------------------------------------ 3. silence
def test_silence(audio, ops):
    case, dither, frames = DR.GEOMETRIES[1], 2.0 ** -6, (4, 0, 9)
    waves = [np.zeros(R.case_samples(case, m), np.int16) for m in frames]
    # the lowest mel bins of pure noise are chi-square distributed with few degrees of freedom: as for the seeds of
    # audio_reference.LOGMEL_CASES, the keys were searched upwards from 0 until the reference kept every mel energy
    # above 200 * FLT_EPSILON (the condition below asks for 100: no element near the clamp, none left out)
    keys = [5, 6, 7]
    run = lambda dt: R.pad_batch(DR.rows(waves, case, dither, keys, dt), case.nmel)
    ref = run(np.float64)
    e32 = R.max_err(run(np.float32), ref)
    bound = DR.bound("logmel", e32)
    emin = min(float(DR.mel_energy(R.as_float(w), case.sr, case.nmel, case.frame_ms, dither=dither, key=k).min())
               for w, k, m in zip(waves, keys, frames) if m)
    assert emin >= 100.0 * R.FLT_EPS                                         # nothing near the clamp
    feat, flen = audio.BatchFeatureTransform(_config(case, dither))(waves, case.sr, dither_keys=keys)
    got = feat.cpu().numpy()
    _check_padding(got, frames)
    err = R.max_err(got, ref)
    _report("silence-" + case.name, "batch int16 (min energy %.0f eps)" % (emin / R.FLT_EPS), dither, e32, bound, err)
    assert err <= bound
    plain, _ = audio.BatchFeatureTransform(_config(case, 0))(waves, case.sr)
    plain = plain.cpu().numpy()
    for b, m in enumerate(frames):
        assert np.all(plain[b, :m] == np.float32(R.LOG_FLOOR)), "digital silence without dither is the clamp"
    ops.check_errors()


# ------------------------------------------------------------------------------------------------ 4. batch independence
@pytest.mark.parametrize("chain", [dict(), dict(delta_order=2, delta_window_size=2, apply_cmvn=True)],
                         ids=["logmel", "delta-cmvn"])
@pytest.mark.parametrize("case", [DR.GEOMETRIES[1], DR.GEOMETRIES[4]], ids=["fused", "unfused"])
def test_an_utterance_does_not_depend_on_its_batch(audio, ops, case, chain):
    dither = 2.0 ** -9
    frames = (12, 5, 9)
    pcm = [R.to_pcm(R.signal(R.case_samples(case, m), case.sr, 30 + b)) for b, m in enumerate(frames)]
    flt = [(w.astype(np.float32) / np.float32(32768.0)) for w in pcm]        # the equal float32 samples
    ka, kb, kc = DR.KEYS[:3]
    bt = audio.BatchFeatureTransform(_config(case, dither, **chain))
    abc, _ = bt(pcm, case.sr, dither_keys=[ka, kb, kc])
    ca, _ = bt([pcm[2], pcm[0]], case.sr, dither_keys=[kc, ka])
    abc_f, _ = bt(flt, case.sr, dither_keys=[ka, kb, kc])
    assert torch.equal(_bits(abc[0, :12]), _bits(ca[1, :12]))                # a: first of three, second of two
    assert torch.equal(_bits(abc[2, :9]), _bits(ca[0, :9]))                  # c
    assert torch.equal(_bits(abc), _bits(abc_f))                             # int16 and the equal float32 samples
    other, _ = bt(pcm, case.sr, dither_keys=[ka ^ 1, kb, kc])
    assert not torch.equal(_bits(abc[0]), _bits(other[0])) and torch.equal(_bits(abc[1:]), _bits(other[1:]))
    ops.check_errors()


# ------------------------------------------------------------------------------------------------ 5. after speed perturbation
def test_dither_acts_on_the_perturbed_waveform(audio, ops):
    case, dither = DR.GEOMETRIES[1], 2.0 ** -9
    lengths, speeds, keys = [4000, 3001], [0.9, 1.1], list(DR.KEYS[:2])
    pcm = [R.to_pcm(R.signal(n, case.sr, 40 + b)) for b, n in enumerate(lengths)]
    bt = audio.BatchFeatureTransform(_config(case, dither))
    feat, flen = bt(pcm, case.sr, speeds=speeds, dither_keys=keys)
    host = np.zeros((2, max(lengths)), dtype=np.int16)
    for b, w in enumerate(pcm):
        host[b, :len(w)] = w
    y, n_out = ops.resample_rows(torch.from_numpy(host).to(DEV), lengths, [0, 1], [(9, 10), (11, 10)], 1.0 / 32768.0)
    rows = [y[b, :int(n_out[b])].cpu().numpy() for b in range(2)]
    frames = [R.frame_count(len(r), case.win, int(case.sr * R.SHIFT_MS * 0.001)) for r in rows]
    assert flen.tolist() == frames and frames != [bt.frame_count(n, case.sr) for n in lengths]
    run = lambda dt: R.pad_batch(DR.rows(rows, case, dither, keys, dt), case.nmel)
    ref = run(np.float64)
    e32 = R.max_err(run(np.float32), ref)
    bound = DR.bound("logmel", e32)
    got = feat.cpu().numpy()
    _check_padding(got, frames)
    err = R.max_err(got, ref)
    _report("speeds-" + case.name, "batch int16", dither, e32, bound, err)
    assert err <= bound
    ops.check_errors()


# ------------------------------------------------------------------------------------------------ 6. switch-off
def test_switch_off(audio, ops):
    case = DR.GEOMETRIES[1]
    waves = [w.copy() for w in DR.case_waves(case, "int16")]
    zero, _ = audio.BatchFeatureTransform(_config(case, 0))(waves, case.sr, dither_keys=list(DR.KEYS))
    cfg = _config(case, 0)
    del cfg["dither"]
    absent, _ = audio.BatchFeatureTransform(cfg)(waves, case.sr)
    assert torch.equal(_bits(zero), _bits(absent))
    on = audio.BatchFeatureTransform(_config(case, 2.0 ** -9))
    with pytest.raises(ValueError):
        on(waves, case.sr)
    with pytest.raises(ValueError):
        on(waves, case.sr, dither_keys=list(DR.KEYS[:2]))
    dithered, _ = on(waves, case.sr, dither_keys=list(DR.KEYS))
    assert not torch.equal(_bits(dithered), _bits(zero))
    ops.check_errors()


def test_per_file_module_takes_a_key_and_defaults_to_the_evaluation_key(audio, ops):
    tr, dim = audio.create_transform(dict(feat_type="fbank", feat_dim=40, frame_length=25, frame_shift=10,
                                          dither=2.0 ** -9, apply_cmvn=False, delta_order=0))
    assert tr.batch is not None and tr.batch.dither == 2.0 ** -9
    x = torch.from_numpy(R.signal(3000, 16000, 3).astype(np.float32)).unsqueeze(0)
    a, b = tr((x, 16000, None, 11)), tr((x, 16000, None, 12))
    assert a.shape == (17, dim) and not torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(tr((x, 16000))), _bits(tr((x, 16000, None, 0))))      # a tensor without a name: key 0
    batch, _ = tr.batch([x[0].numpy()], 16000, dither_keys=[11])
    assert torch.equal(_bits(a), _bits(batch[0]))                                  # the same kernel, B = 1
    ops.check_errors()


# ------------------------------------------------------------------------------------------------ 7. solver
def test_solver_trains_with_dither(ops, tmp_path, audio):
    """the product solver on a miniature wav corpus, in a fresh process with ASRK_DETERMINISTIC=1: two runs with
    dither 3.05e-5, one with dither 0, one on a data path that was never given the keyword"""
    out = str(tmp_path)
    env = dict(os.environ, ASRK_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "dither_worker.py"), out], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    runs = {k: np.load(os.path.join(out, k + ".npz")) for k in ("dither_a", "dither_b", "plain", "never")}
    a, b, plain, never = runs["dither_a"], runs["dither_b"], runs["plain"], runs["never"]
    bits = lambda v: v.view(np.uint32)
    # three steps train with a finite loss, and the two runs are bit-identical
    assert len(a["loss"]) >= 3 and np.all(np.isfinite(a["loss"])) and int(a["n_train"]) >= 3
    assert np.array_equal(bits(a["loss"]), bits(b["loss"]))
    for k in range(int(a["n_train"])):
        assert np.array_equal(bits(a["train_feat_%d" % k]), bits(b["train_feat_%d" % k]))
    # they are not the undithered run, whose lengths they share
    assert np.array_equal(a["train_len_0"], plain["train_len_0"])
    assert not np.array_equal(bits(a["train_feat_0"]), bits(plain["train_feat_0"]))
    assert not np.array_equal(bits(a["loss"][:1]), bits(plain["loss"][:1]))
    # dither 0 is the step of a solver that never heard of the feature
    assert np.array_equal(bits(plain["loss"][:1]), bits(never["loss"][:1]))
    assert np.array_equal(bits(plain["train_feat_0"]), bits(never["train_feat_0"]))
    # dev features: the same on two validation passes, and not the undithered ones
    nv = int(a["n_dev_batches"])
    assert nv >= 1 and nv == int(plain["n_dev_batches"]) and int(a["n_valid"]) >= 2 * nv and int(plain["n_valid"]) >= nv
    for k in range(nv, int(a["n_valid"])):
        assert np.array_equal(bits(a["valid_feat_%d" % k]), bits(a["valid_feat_%d" % (k % nv)]))
    for k in range(nv):
        assert np.array_equal(a["valid_len_%d" % k], plain["valid_len_%d" % k])
        assert not np.array_equal(bits(a["valid_feat_%d" % k]), bits(plain["valid_feat_%d" % k]))
    # the first training batch is BatchFeatureTransform under Dither(amplitude, seed).key(name, True) at epoch key 0
    policy = audio.Dither(float(a["dither"]), int(a["seed"]))
    policy.begin_epoch(0)
    names = [str(n) for n in a["train_names_0"]]
    cfg = dict(feat_type="fbank", feat_dim=40, frame_length=25, frame_shift=10, dither=float(a["dither"]),
               apply_cmvn=True, delta_order=2, delta_window_size=2)
    pcm = [audio.load_pcm(os.path.join(out, "work", "corpus", "train-x", "7", "9", n + ".wav"))[0] for n in names]
    feat, flen = audio.BatchFeatureTransform(cfg)(pcm, 16000, dither_keys=[policy.key(n, True) for n in names])
    assert flen.tolist() == a["train_len_0"].tolist()
    assert np.array_equal(bits(feat.cpu().numpy()), bits(a["train_feat_0"]))


def test_a_dithered_config_trains_and_decodes_through_main(ops, tmp_path):
    """`dither: 3.05e-5` in the yaml: main.py trains, checkpoints, and `--test` decodes greedily (batch-wise) and with
    the beam search (instance-wise); two greedy decodes of the same checkpoint write the same hypotheses, because the
    evaluation keys do not depend on the pass"""
    import yaml
    import test_e2e_gpu as E2E
    main = importlib.import_module(PKG_NAME + ".main")
    tmp = str(tmp_path)
    root = os.path.join(tmp, "corpus")
    vocab = E2E._make_corpus(root)
    train, tr_path = E2E._configs(root, vocab, tmp)
    train["data"]["audio"]["dither"] = 3.05e-5
    train["hparas"].update(valid_step=2, max_step=2)
    yaml.safe_dump(train, open(tr_path, "w"))
    common = ["--logdir", os.path.join(tmp, "log"), "--ckpdir", os.path.join(tmp, "ckpt"),
              "--outdir", os.path.join(tmp, "result"), "--njobs", "2", "--no-msg"]
    solver = main.main(["--config", tr_path] + common)
    assert solver.dither is not None and solver.dither.amplitude == 3.05e-5 and solver.step >= 2
    latest = os.path.join(tmp, "ckpt", "asr_tiny_sd0", "latest.pth")
    assert os.path.exists(latest)
    outs = []
    for name in ("dec_a", "dec_b"):
        cfg = E2E._decode_cfg(tmp, tr_path, latest, name, beam_size=1, min_len_ratio=0.01, max_len_ratio=0.3)
        main.main(["--config", cfg, "--test"] + common)
        outs.append([open(os.path.join(tmp, "result", "%s_%s_output.csv" % (name, s))).read() for s in ("dev", "test")])
        assert len(outs[-1][0].splitlines()) == 4 and len(outs[-1][1].splitlines()) == 3
    assert outs[0] == outs[1]
    bcfg = E2E._decode_cfg(tmp, tr_path, latest, "dec_beam", beam_size=2, min_len_ratio=0.01, max_len_ratio=0.1,
                           lm_path="", lm_config="", lm_weight=0.0, ctc_weight=0.3)
    main.main(["--config", bcfg, "--test"] + common)
    assert len(open(os.path.join(tmp, "result", "dec_beam_test_output.csv")).read().splitlines()) == 3
    ops.check_errors()
