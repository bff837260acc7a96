"""GPU: every kernel instantiation of the audio front end (csrc/audio.hip) on the table of tests/audio_reference.py.

Log-mel / mfcc rows run per file (float) and as a ragged batch in int16 and in float32; delta / CMVN rows drive
asrk_delta_cmvn_batch_f32 directly, its output inside a sentinel-filled allocation.  Criterion: every element within
max(8 * e32, floor) of the float64 reference (audio_reference.bound: e32 is the float32 run of the same reference on the
same input, nothing is a fixed number), exact zeros in the padding, NaN exactly where the reference has it.  Each test
prints e32, the bound and the measured error (pytest -s)."""
import importlib

import numpy as np
import pytest
import torch

import audio_reference as R
import fbank_independent as FI
from conftest import PKG_NAME
from oracle import fbank_oracle as FO

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -12345.5
FRONT, BACK = 37, 41            # guard floats around the delta / CMVN output (an odd offset: the stores are scalar)
EINVAL, ESHAPE = -1, -2


@pytest.fixture(scope="module")
def audio(ops):
    return importlib.import_module(PKG_NAME + ".src.audio")


@pytest.fixture(scope="module")
def lib(ops):
    return importlib.import_module(PKG_NAME + "._lib").load()


def _config(case, **over):
    cfg = dict(feat_type=case.feat_type, feat_dim=case.nmel, frame_length=case.frame_ms, frame_shift=R.SHIFT_MS,
               dither=0, apply_cmvn=False, delta_order=0)
    cfg.update(dict(case.opts))
    if case.feat_type == "mfcc":
        cfg["num_ceps"] = R.NUM_CEPS
    cfg.update(over)
    return cfg


def _per_file(audio, case, w):
    extract = audio.kaldi_fbank if case.feat_type == "fbank" else audio.kaldi_mfcc
    kw = dict(num_ceps=R.NUM_CEPS) if case.feat_type == "mfcc" else {}
    return extract(torch.from_numpy(w.copy()).unsqueeze(0).to(DEV), case.sr, num_mel_bins=case.nmel,
                   frame_length=case.frame_ms, frame_shift=R.SHIFT_MS, dither=0, **dict(case.opts), **kw)


def _report(name, kind, e32, bound, err):
    print("AUDIOVAR %s | %s | e32 %.3e | bound %.3e | device %.3e | device/e32 %.2f"
          % (name, kind, e32, bound, err, err / e32 if e32 else 0.0))


def _check_padding(got, frames):
    for b, m in enumerate(frames):
        assert np.all(got[b, m:] == 0.0), (b, "padding beyond the utterance is not exactly zero")


@pytest.mark.parametrize("case", R.LOGMEL_CASES, ids=[c.name for c in R.LOGMEL_CASES])
def test_logmel_row(audio, ops, case):
    width, out_kind = R.case_width(case), R.case_kind(case)
    for kind in ("int16", "float32"):
        ref, e32 = R.logmel_expected(case, kind)
        bound = R.bound(out_kind, e32)
        bt = audio.BatchFeatureTransform(_config(case))
        feat, flen = bt([w.copy() for w in R.case_waves(case, kind)], case.sr)
        assert flen.dtype == torch.int64 and flen.tolist() == list(case.frames)
        assert tuple(feat.shape) == ref.shape == (len(case.frames), max(case.frames), width)
        got = feat.cpu().numpy()
        _check_padding(got, case.frames)
        err = R.max_err(got, ref)
        _report(case.name, "batch " + kind, e32, bound, err)
        assert err <= bound, (case.name, kind, err, bound, e32)
    ref, e32 = R.logmel_expected(case, "float32")
    bound, worst = R.bound(out_kind, e32), 0.0
    for b, w in enumerate(R.case_waves(case, "float32")):
        y = _per_file(audio, case, w)
        m = case.frames[b]
        assert tuple(y.shape) == (m, width) and y.dtype == torch.float32
        if m:
            worst = max(worst, R.max_err(y.cpu().numpy(), ref[b, :m]))
    _report(case.name, "per file", e32, bound, worst)
    assert worst <= bound, (case.name, worst, bound, e32)
    ops.check_errors()


_ROUTES = [c for c in R.LOGMEL_CASES if c.feat_type == "fbank" and not c.opts]


@pytest.mark.parametrize("case", _ROUTES, ids=[c.name for c in _ROUTES])
def test_clamp_on_every_route(audio, ops, case):
    """constant input with DC removal: every mel energy is below FLT_EPSILON, every log-mel is ln(FLT_EPSILON)"""
    frames = (2, 0, 5)
    lens = [R.case_samples(case, m) for m in frames]
    for waves in ([np.full(n, 12124, np.int16) for n in lens], [np.full(n, 0.37, np.float32) for n in lens]):
        feat, flen = audio.BatchFeatureTransform(_config(case))(waves, case.sr)
        assert flen.tolist() == list(frames) and tuple(feat.shape) == (3, 5, case.nmel)
        got = feat.cpu().numpy()
        _check_padding(got, frames)
        for b, m in enumerate(frames):
            assert np.allclose(got[b, :m], FI.LOG_FLOOR, atol=1e-5), (case.name, b)
    y = _per_file(audio, case, np.full(lens[2], 0.37, np.float32)).cpu().numpy()
    assert y.shape == (5, case.nmel) and np.allclose(y, FI.LOG_FLOOR, atol=1e-5)
    ops.check_errors()


def test_batch_chain_with_a_16_tap_filter_bank_vs_float64(audio, ops):
    """PCM -> log-mel -> delta (order 2, window 3: L = 13, the 16-tap instantiation) -> CMVN -> layout in the two launches
    of BatchFeatureTransform, against the float64 chain; utterances long enough for CMVN to be well conditioned"""
    case = R.LOGMEL_CASES[1]                                         # 8 kHz, 23 mel bins
    frames, filt = (40, 0, 130, 25), FO.delta_filters(2, 3)
    waves = [R.to_pcm(R.signal(R.case_samples(case, m), case.sr, 50 + b)) for b, m in enumerate(frames)]
    run = lambda dt: R.pad_batch([R.features(R.logmel(R.as_float(w), case.sr, case.nmel, case.frame_ms, dtype=dt), filt,
                                             True, dt) for w in waves], 3 * case.nmel)
    ref = run(np.float64)
    e32 = R.max_err(run(np.float32), ref)
    bound = R.bound("normalised", e32)
    assert bound < 1e-3, bound
    feat, flen = audio.BatchFeatureTransform(_config(case, delta_order=2, delta_window_size=3, apply_cmvn=True))(
        waves, case.sr)
    assert flen.tolist() == list(frames) and tuple(feat.shape) == ref.shape
    got = feat.cpu().numpy()
    _check_padding(got, frames)
    err = R.max_err(got, ref)
    _report("chain-8000-25ms-mel23-order2-window3", "normalised", e32, bound, err)
    assert err <= bound, (err, bound, e32)
    ops.check_errors()


# ------------------------------------------------------------------------------------------------ delta / CMVN through the ABI
def _delta_abi(ops, lib, mel, filt, frames, apply_cmvn):
    """-> out [B, Tmax, C*D] (numpy) as the launch left it; the guard floats around it must be untouched"""
    B, D, (C, L), tmax = len(frames), mel.shape[1], filt.shape, max(frames)
    offs = np.zeros(B + 1, dtype=np.int64)
    offs[1:] = np.cumsum(frames)
    assert offs[-1] == mel.shape[0]
    mel_g, filt_g = torch.from_numpy(mel.copy()).to(DEV), torch.from_numpy(filt.copy()).to(DEV)
    off_g = torch.from_numpy(offs).to(DEV)
    n = B * tmax * C * D
    base = torch.full((FRONT + n + BACK,), SENTINEL, dtype=torch.float32, device=DEV)
    out = base[FRONT:FRONT + n]
    rc = lib.asrk_delta_cmvn_batch_f32(ops._p(mel_g), ops._p(off_g), B, D, ops._p(filt_g), C, L, int(apply_cmvn),
                                       R.CMVN_EPS, ops._p(out), tmax, ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    host = base.cpu().numpy()
    assert np.all(host[:FRONT] == SENTINEL) and np.all(host[FRONT + n:] == SENTINEL), "wrote outside the output"
    return host[FRONT:FRONT + n].reshape(B, tmax, C * D)


@pytest.mark.parametrize("case", R.DELTA_CASES, ids=[c.name for c in R.DELTA_CASES])
def test_delta_cmvn_row(ops, lib, case):
    mel, filt = R.delta_inputs(case)
    ref, e32 = R.delta_expected(case)
    kind = R.delta_kind(case.cmvn)
    bound = R.bound(kind, e32)
    got = _delta_abi(ops, lib, mel, filt, case.frames, case.cmvn)
    _check_padding(got, case.frames)
    for b, m in enumerate(case.frames):
        if m == 0:
            assert np.all(got[b] == 0.0), b                                   # an utterance without a frame: a zero row
        if m == 1 and case.cmvn:
            assert np.all(np.isnan(got[b, 0])), b                             # torch.std of one frame
    err = R.max_err(got, ref)                                                 # NaN exactly where the reference has it
    _report(case.name, kind, e32, bound, err)
    assert err <= bound, (case.name, err, bound, e32)
    ops.check_errors()


@pytest.mark.parametrize("cmvn", [0, 1])
@pytest.mark.parametrize("order,window", R.MODULE_PAIRS)
def test_per_file_modules_at_other_windows(audio, ops, order, window, cmvn):
    """Delta -> CMVN -> Postprocess (delta_kernel, cmvn_kernel, transpose_kernel) at filter lengths 7, 11, 13, 15, 17"""
    ref, e32 = R.module_expected(order, window, cmvn)
    kind = R.delta_kind(cmvn)
    bound = R.bound(kind, e32)
    y = torch.from_numpy(R.module_input().T.copy()).unsqueeze(0).to(DEV)       # [1, D, T]
    y = audio.Delta(order, window)(y)
    assert tuple(y.shape) == (order + 1, R.MODULE_D, R.MODULE_T)
    if cmvn:
        y = audio.CMVN()(y)
    y = audio.Postprocess()(y)
    err = R.max_err(y.cpu().numpy(), ref)
    _report("modules-order%d-window%d" % (order, window), kind, e32, bound, err)
    assert err <= bound, (order, window, cmvn, err, bound, e32)
    ops.check_errors()


def test_batch_form_refuses_17_taps_and_takes_15(audio):
    cfg = dict(feat_type="fbank", feat_dim=40, frame_length=25, frame_shift=10, dither=0, apply_cmvn=True)
    with pytest.raises(NotImplementedError):
        audio.BatchFeatureTransform(dict(cfg, delta_order=2, delta_window_size=4))
    tr, dim = audio.create_transform(dict(cfg, delta_order=2, delta_window_size=4))
    assert tr.batch is None and dim == 120                                     # the per-file chain still serves it
    for order, window in R.MODULE_PAIRS[:-1]:
        bt = audio.BatchFeatureTransform(dict(cfg, delta_order=order, delta_window_size=window))
        assert bt.filters.shape[-1] == 2 * order * window + 1 <= 15


# ------------------------------------------------------------------------------------------------ ABI refusals
def _fbank_args(audio):
    tb = audio._FbankTables.get(16000, 25, 10.0, 40, 20.0, 0.0, torch.device(DEV))
    wave = torch.zeros((1, 1000), dtype=torch.float32, device=DEV)
    off = torch.tensor([0, 4], dtype=torch.int64, device=DEV)
    return tb, wave, off


def test_fused_logmel_entry_refusals(audio, ops, lib):
    tb, wave, off = _fbank_args(audio)
    mel = torch.full((4, 40), SENTINEL, dtype=torch.float32, device=DEV)

    def call(sample_bytes=4, ld_wave=1000, max_m=4, win=tb.win, log2n=tb.log2n):
        return lib.asrk_fbank_logmel_batch_f32(ops._p(wave), sample_bytes, ld_wave, None, ops._p(off), 1, max_m,
                                               ops._p(tb.window), ops._p(tb.tw_fft), ops._p(tb.tw_unpack),
                                               ops._p(tb.melT), ops._p(tb.mel_range), 40, 40, ops._p(mel), win, tb.shift,
                                               log2n, 1.0, 0.97, 1, R.FLT_EPS, ops._stream())

    assert call(log2n=7) == ESHAPE and call(log2n=11) == ESHAPE
    assert call(win=513) == ESHAPE and call(win=257, log2n=8) == ESHAPE      # win > 1 << log2n
    assert call(max_m=5) == EINVAL                                           # frame 4 would end at sample 1040 > ld_wave
    assert call(ld_wave=879) == EINVAL                                       # frame 3 ends at sample 880
    assert call(sample_bytes=3) == EINVAL
    torch.cuda.synchronize()
    assert torch.all(mel == SENTINEL).item()                                 # a refused call launches nothing
    assert call(ld_wave=880) == 0                                            # the same arguments at the limit are taken
    torch.cuda.synchronize()
    assert torch.all(mel != SENTINEL).item()
    ops.check_errors()


def test_frames_batch_entry_refusals(audio, ops, lib):
    tb, wave, off = _fbank_args(audio)
    frames = torch.full((4, tb.ldf), SENTINEL, dtype=torch.float32, device=DEV)

    def call(sample_bytes=4, ld_wave=1000, max_m=4, ldf=tb.ldf):
        return lib.asrk_fbank_frames_batch_f32(ops._p(wave), sample_bytes, ld_wave, None, ops._p(off), 1, max_m,
                                               ops._p(tb.window), ops._p(frames), tb.win, tb.shift, ldf, 1.0, 0.97, 1,
                                               ops._stream())

    assert call(max_m=5) == EINVAL and call(ld_wave=879) == EINVAL
    assert call(sample_bytes=3) == EINVAL
    assert call(ldf=tb.win - 1) == EINVAL                                    # a frame row narrower than the frame
    torch.cuda.synchronize()
    assert torch.all(frames == SENTINEL).item()
    assert call(ld_wave=880) == 0
    torch.cuda.synchronize()
    assert torch.all(frames == 0.0).item()                                   # silence: every windowed sample is +-0
    ops.check_errors()
