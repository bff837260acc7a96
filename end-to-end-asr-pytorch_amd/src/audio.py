"""On-the-fly audio feature pipeline — MI355X mirror of the reference's src/audio.py
(ExtractAudioFeature -> Delta -> CMVN -> Postprocess, built by create_transform).

Same module names, constructor arguments, tensor shapes between stages ([C, D, T]) and final
[T, C*D] output; the arithmetic runs in the gfx950 kernels of csrc/audio.hip (+ two MFMA GEMMs).
`torchaudio` is not required: 16-bit PCM wav is read with the stdlib `wave` module
(torchaudio.load semantics: float32 in [-1, 1), [channel, samples]).
"""
import collections
import inspect
import math
import os
import wave as _wave
import zlib
from fractions import Fraction

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .. import ops
from ..ops import _L, _p, _stream, _f32c

FLT_EPS = 1.1920928955078125e-07


def load_flac(filepath, verify_md5=True):
    """FLAC (what LibriSpeech ships) -> (FloatTensor [C, N] in [-1,1), sample_rate) through the native
    decoder in libasrk (csrc/flac.cpp: frame CRCs are checked there; the STREAMINFO MD5 of the decoded
    audio is checked here when the encoder stored one)."""
    import ctypes
    import hashlib
    lib = _lib.load()
    path = str(filepath).encode()
    sr, nch, bps, total = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    md5 = (ctypes.c_uint8 * 16)()
    _lib.check(lib.asrk_flac_info(path, ctypes.byref(sr), ctypes.byref(nch), ctypes.byref(bps),
                                  ctypes.byref(total), md5), "flac_info(%s)" % filepath)
    import os
    cap = total.value if total.value > 0 else os.path.getsize(filepath) * 8 // max(1, nch.value)
    buf = np.empty((cap, nch.value), dtype=np.int32)
    got = ctypes.c_int64(0)
    rc = lib.asrk_flac_decode_i32(path, buf.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(got))
    if rc == -3:        # ASRK_EWORKSPACE: a stream without a sample count that outgrew the guess; got = size needed
        cap = got.value
        buf = np.empty((cap, nch.value), dtype=np.int32)
        rc = lib.asrk_flac_decode_i32(path, buf.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(got))
    _lib.check(rc, "flac_decode(%s)" % filepath)
    buf = buf[:got.value]
    if total.value > 0 and got.value != total.value:
        raise ValueError('%s: decoded %d of %d samples' % (filepath, got.value, total.value))
    if verify_md5 and any(md5):
        nbytes = (bps.value + 7) // 8
        raw = buf.astype('<i%d' % nbytes).tobytes() if nbytes in (1, 2, 4) else \
            b''.join(int(v).to_bytes(3, 'little', signed=True) for v in buf.reshape(-1))
        if hashlib.md5(raw).digest() != bytes(md5):
            raise ValueError('%s: MD5 of the decoded audio does not match the FLAC STREAMINFO' % filepath)
    x = buf.astype(np.float32).T / float(1 << (bps.value - 1))
    return torch.from_numpy(np.ascontiguousarray(x)), sr.value


def load_wav(filepath):
    """-> (FloatTensor [C, N] in [-1,1), sample_rate)   (what torchaudio.load returns, audio.py:102);
    16-bit PCM .wav through the standard library, .flac through the native decoder"""
    if str(filepath).lower().endswith('.flac'):
        return load_flac(filepath)
    with _wave.open(filepath, 'rb') as w:
        sr, nch, sw, n = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
        raw = w.readframes(n)
    if sw != 2:
        raise ValueError('only 16-bit PCM .wav and .flac files are supported')
    x = np.frombuffer(raw, dtype='<i2').astype(np.float32).reshape(-1, nch).T / 32768.0
    return torch.from_numpy(np.ascontiguousarray(x)), sr


class _FbankTables:
    """Immutable per-(geometry, device) tables: povey window, DFT cos|sin basis, mel weights."""
    _cache = {}

    @classmethod
    def get(cls, sample_rate, frame_length, frame_shift, num_mel_bins, low_freq, high_freq, device):
        key = (sample_rate, frame_length, frame_shift, num_mel_bins, low_freq, high_freq, str(device))
        t = cls._cache.get(key)
        if t is None:
            t = cls(sample_rate, frame_length, frame_shift, num_mel_bins, low_freq, high_freq, device)
            cls._cache[key] = t
        return t

    def __init__(self, sr, frame_length, frame_shift, nmel, low_freq, high_freq, device):
        self.win = int(sr * frame_length * 0.001)
        self.shift = int(sr * frame_shift * 0.001)
        self.padded = 1 << (self.win - 1).bit_length()           # round_to_power_of_two
        self.ldf = (self.win + 3) // 4 * 4
        nb = self.padded // 2 + 1
        self.nb = (nb + 3) // 4 * 4                               # padded bin count (GEMM alignment)
        n = np.arange(self.win, dtype=np.float64)
        window = np.hanning(self.win) ** 0.85 if self.win > 1 else np.ones(1)   # povey
        # real DFT of the zero-padded frame: X[k] = sum_n x[n] e^{-2 pi i k n / padded}
        k = np.arange(nb, dtype=np.float64)
        ang = 2.0 * math.pi * np.outer(n, k) / self.padded
        basis = np.zeros((self.ldf, 2 * self.nb))
        basis[:self.win, :nb] = np.cos(ang)
        basis[:self.win, self.nb:self.nb + nb] = -np.sin(ang)
        # mel banks (Kaldi / torchaudio get_mel_banks, vtln_warp = 1)
        nyq = 0.5 * sr
        hi = high_freq + nyq if high_freq <= 0 else high_freq
        mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)
        ml, mh = mel(low_freq), mel(hi)
        delta = (mh - ml) / (nmel + 1)
        b = np.arange(nmel, dtype=np.float64)[:, None]
        left, center, right = ml + b * delta, ml + (b + 1) * delta, ml + (b + 2) * delta
        mf = mel(sr / self.padded * np.arange(self.padded // 2, dtype=np.float64))[None, :]
        w = np.maximum(0.0, np.minimum((mf - left) / (center - left), (right - mf) / (right - center)))
        melT = np.zeros((self.nb, nmel))
        melT[:self.padded // 2, :] = w.T                          # bin padded/2 has zero weight
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
        self.window, self.basis, self.melT = f32(window), f32(basis), f32(melT)
        self.nmel = nmel
        # tables of the fused kernel (asrk_fbank_logmel_batch_f32): the zero-padded real DFT of `padded` points runs as a
        # complex FFT of padded / 2 points; twiddles in float64, rounded once
        self.log2n = self.padded.bit_length() - 1
        M = self.padded // 2
        km = np.arange(M, dtype=np.float64)
        ku = np.arange(M + 1, dtype=np.float64)
        pair = lambda ang: np.stack([np.cos(ang), -np.sin(ang)], axis=1)
        self.tw_fft = f32(pair(2.0 * math.pi * km / M))
        self.tw_unpack = f32(pair(2.0 * math.pi * ku / self.padded))
        rng = np.zeros((nmel, 2), dtype=np.int32)
        for m_ in range(nmel):
            nz = np.flatnonzero(melT[:, m_] != 0.0)
            rng[m_] = (nz[0], nz[-1] + 1) if len(nz) else (0, 0)
        self.mel_range = torch.from_numpy(rng).to(device)
        self.fused = 8 <= self.log2n <= 10


def _dither_amplitude(value):
    """the `dither` key as a float; ValueError unless it is a finite, non-negative number"""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or value < 0:
        raise ValueError('dither must be a finite, non-negative number (in units of the [-1, 1) waveform), got %r'
                         % (value,))
    return float(value)


def _keys_to_device(keys, device):
    """64-bit dither keys -> the device array the batch entries read (uint64 bits carried in an int64 tensor)"""
    k = np.asarray([int(v) & _M64 for v in keys], dtype=np.uint64)
    return torch.from_numpy(k.view(np.int64)).to(device)


def kaldi_fbank(waveform, sample_frequency, num_mel_bins=23, frame_length=25.0, frame_shift=10.0,
                dither=0.0, channel=-1, preemphasis_coefficient=0.97, remove_dc_offset=True,
                low_freq=20.0, high_freq=0.0, dither_key=0, **unused):
    """torchaudio.compliance.kaldi.fbank restated for the device (subset used at audio.py:104-108):
    waveform [C, N] on the GPU -> log-mel energies [m, num_mel_bins].  dither > 0 adds dither * z(dither_key, frame,
    position) to every frame element (the noise function of include/asrk.h: a pure function of the 64-bit key, where
    torchaudio draws from the global generator); dither == 0 makes the plain calls and ignores the key."""
    dither = _dither_amplitude(dither)
    if unused:
        raise NotImplementedError('unsupported fbank options: %s' % sorted(unused))
    ops._require_gpu(waveform)
    L = _L()
    x = _f32c(waveform[max(channel, 0)])
    tb = _FbankTables.get(int(sample_frequency), frame_length, frame_shift, num_mel_bins, low_freq,
                          high_freq, x.device)
    n = x.numel()
    m = 0 if n < tb.win else 1 + (n - tb.win) // tb.shift
    dev = x.device
    if m == 0:
        return torch.empty((0, num_mel_bins), dtype=torch.float32, device=dev)
    if tb.fused:
        keys = _keys_to_device([dither_key], dev) if dither > 0.0 else None
        return _pcm_to_logmel(x, 4, n, None, torch.tensor([0, m], dtype=torch.int64, device=dev), 1, m, m, tb,
                              num_mel_bins, 1.0, preemphasis_coefficient, remove_dc_offset, dither, keys)
    frames = torch.empty((m, tb.ldf), dtype=torch.float32, device=dev)
    if dither > 0.0:
        _lib.check(L.asrk_fbank_frames_dither_f32(_p(x), n, _p(tb.window), _p(frames), m, tb.win, tb.shift, tb.ldf,
                                                  preemphasis_coefficient, int(remove_dc_offset), dither,
                                                  int(dither_key) & _M64, _stream()), 'fbank_frames_dither')
    else:
        _lib.check(L.asrk_fbank_frames_f32(_p(x), n, _p(tb.window), _p(frames), m, tb.win, tb.shift, tb.ldf,
                                           preemphasis_coefficient, int(remove_dc_offset), _stream()),
                   'fbank_frames')
    return _frames_to_logmel(frames, tb, num_mel_bins)


def _pcm_to_logmel(wave, sample_bytes, ld_wave, n_host, frame_off, B, max_m, rows, tb, num_mel_bins, scale, preemph,
                   remove_dc, dither=0.0, keys=None):
    """padded PCM batch [B, ld_wave] -> log-mel energies [sum m, num_mel_bins] in ONE launch (csrc/audio.hip
    fbank_logmel_batch_kernel: framing, FFT in LDS, power, mel weights, log) - no frames / spectrum / power tensors.
    dither > 0: the dithered entry with keys [B] (device); dither == 0: the plain entry, keys are not looked at"""
    mel = torch.empty((rows, num_mel_bins), dtype=torch.float32, device=wave.device)
    args = (_p(wave), sample_bytes, ld_wave, n_host.ctypes.data if n_host is not None else None, _p(frame_off), B,
            max_m, _p(tb.window), _p(tb.tw_fft), _p(tb.tw_unpack), _p(tb.melT), _p(tb.mel_range), num_mel_bins,
            num_mel_bins, _p(mel), tb.win, tb.shift, tb.log2n, float(scale), float(preemph), int(remove_dc), FLT_EPS)
    if dither > 0.0:
        _lib.check(_L().asrk_fbank_logmel_batch_dither_f32(*args, float(dither), _p(keys), _stream()),
                   'fbank_logmel_batch_dither')
    else:
        _lib.check(_L().asrk_fbank_logmel_batch_f32(*args, _stream()), 'fbank_logmel_batch')
    return mel


def _frames_to_logmel(frames, tb, num_mel_bins):
    """windowed frames [rows, ldf] (any number of utterances stacked) -> log-mel energies [rows, num_mel_bins]:
    DFT as a GEMM against the cos|sin basis, |X|^2, mel weights as a second GEMM, log(max(., FLT_EPSILON))"""
    L = _L()
    m, dev = frames.shape[0], frames.device
    spec = torch.empty((m, 2 * tb.nb), dtype=torch.float32, device=dev)
    ops.gemm(0, 0, m, 2 * tb.nb, tb.ldf, frames, tb.ldf, tb.basis, 2 * tb.nb, spec, 2 * tb.nb)
    power = torch.empty((m, tb.nb), dtype=torch.float32, device=dev)
    _lib.check(L.asrk_power_spectrum_f32(_p(spec), _p(power), m, tb.nb, _stream()), 'power_spectrum')
    mel = torch.empty((m, num_mel_bins), dtype=torch.float32, device=dev)
    ops.gemm(0, 0, m, num_mel_bins, tb.nb, power, tb.nb, tb.melT, num_mel_bins, mel, num_mel_bins)
    _lib.check(L.asrk_log_floor_f32(_p(mel), mel.numel(), FLT_EPS, _stream()), 'log_floor')
    return mel


_MFCC_TABLES = {}


def _mfcc_table(num_mel_bins, num_ceps, cepstral_lifter, device):
    key = (num_mel_bins, num_ceps, float(cepstral_lifter), str(device))
    tab = _MFCC_TABLES.get(key)
    if tab is None:
        n = np.arange(num_mel_bins, dtype=np.float64)
        k = np.arange(num_mel_bins, dtype=np.float64)[:, None]
        dct = np.cos(np.pi / num_mel_bins * (n + 0.5) * k) * math.sqrt(2.0 / num_mel_bins)   # [k, n]
        dct[0, :] = math.sqrt(1.0 / num_mel_bins)
        mat = dct.T[:, :num_ceps].copy()                                                     # [n_mel, ceps]
        if cepstral_lifter != 0.0:
            i = np.arange(num_ceps, dtype=np.float64)
            mat *= (1.0 + 0.5 * cepstral_lifter * np.sin(np.pi * i / cepstral_lifter))[None, :]
        tab = torch.from_numpy(np.ascontiguousarray(mat, dtype=np.float32)).to(device)
        _MFCC_TABLES[key] = tab
    return tab


def kaldi_mfcc(waveform, sample_frequency, num_mel_bins=23, num_ceps=13, cepstral_lifter=22.0, **fbank_kwargs):
    """torchaudio.compliance.kaldi.mfcc restated for the device (feat_type: 'mfcc', audio.py:96): log-mel
    energies (the fbank chain above) x Kaldi's DCT-II matrix (orthonormal, first column sqrt(1/N),
    first num_ceps columns) as one more GEMM, then cepstral liftering 1 + Q/2 sin(pi i / Q) folded into
    the DCT table.  use_energy=False, subtract_mean=False (the defaults the reference relies on)."""
    if num_ceps > num_mel_bins:
        raise ValueError('num_ceps cannot be larger than num_mel_bins: %d vs %d' % (num_ceps, num_mel_bins))
    mel = kaldi_fbank(waveform, sample_frequency, num_mel_bins=num_mel_bins, **fbank_kwargs)
    m = mel.shape[0]
    tab = _mfcc_table(num_mel_bins, num_ceps, cepstral_lifter, mel.device)
    out = torch.empty((m, num_ceps), dtype=torch.float32, device=mel.device)
    if m > 0:
        ops.gemm(0, 0, m, num_ceps, num_mel_bins, mel, num_mel_bins, tab, num_ceps, out, num_ceps)
    return out


def _transpose2d(x):
    xc = _f32c(x)
    R, C = xc.shape
    y = torch.empty((C, R), dtype=torch.float32, device=x.device)
    _lib.check(_L().asrk_transpose_f32(_p(xc), _p(y), R, C, _stream()), 'transpose')
    return y


class CMVN(nn.Module):
    ''' per (channel, feature) mean/variance normalisation over time (reference: audio.py:7-30) '''

    def __init__(self, mode="global", dim=2, eps=1e-10):
        super(CMVN, self).__init__()
        if mode != "global":
            raise NotImplementedError("Only support global mean variance normalization.")
        if dim != 2:
            raise NotImplementedError("CMVN over the time axis (dim=2) only")
        self.mode, self.dim, self.eps = mode, dim, eps

    def forward(self, x):
        ops._require_gpu(x)
        xc = _f32c(x)
        C, D, T = xc.shape
        y = torch.empty_like(xc)
        _lib.check(_L().asrk_cmvn_f32(_p(xc), _p(y), C * D, T, self.eps, _stream()), 'cmvn')
        return y

    def extra_repr(self):
        return "mode={}, dim={}, eps={}".format(self.mode, self.dim, self.eps)


class Delta(nn.Module):
    ''' delta / delta-delta features (reference: audio.py:33-80) '''

    def __init__(self, order=1, window_size=2):
        super(Delta, self).__init__()
        self.order = order
        self.window_size = window_size
        filters = self._create_filters(order, window_size)
        self.register_buffer("filters", filters)        # [order+1, 1, 1, L] like the reference
        self.padding = (0, (filters.shape[-1] - 1) // 2)

    def forward(self, x):
        ops._require_gpu(x)
        xc = _f32c(x)
        assert xc.shape[0] == 1, 'Delta expects [1, D, T] (audio.py:50-54)'
        _, D, T = xc.shape
        C, Lf = self.order + 1, self.filters.shape[-1]
        filt = _f32c(self.filters.reshape(C, Lf).to(x.device))
        y = torch.empty((C, D, T), dtype=torch.float32, device=x.device)
        _lib.check(_L().asrk_delta_f32(_p(xc), _p(filt), _p(y), C, D, T, Lf, _stream()), 'delta')
        return y

    def _create_filters(self, order, window_size):
        ''' regression filters, order i built by convolving order i-1 (audio.py:57-77) '''
        scales = [[1.0]]
        for i in range(1, order + 1):
            prev_offset = (len(scales[i - 1]) - 1) // 2
            curr_offset = prev_offset + window_size
            curr = [0.0] * (len(scales[i - 1]) + 2 * window_size)
            normalizer = 0.0
            for j in range(-window_size, window_size + 1):
                normalizer += j * j
                for k in range(-prev_offset, prev_offset + 1):
                    curr[j + k + curr_offset] += (j * scales[i - 1][k + prev_offset])
            scales.append([v / normalizer for v in curr])
        max_len = len(scales[-1])
        for i, scale in enumerate(scales[:-1]):
            padding = (max_len - len(scale)) // 2
            scales[i] = [0.0] * padding + scale + [0.0] * padding
        return torch.tensor(scales, dtype=torch.float32).unsqueeze(1).unsqueeze(1)

    def extra_repr(self):
        return "order={}, window_size={}".format(self.order, self.window_size)


class Postprocess(nn.Module):
    ''' [channel, feature_dim, time] -> [time, channel * feature_dim] (reference: audio.py:83-89) '''

    def forward(self, x):
        C, D, T = x.shape
        return _transpose2d(_f32c(x).view(C * D, T)).detach()


class ExtractAudioFeature(nn.Module):
    ''' file (or waveform tensor) -> [1, feat_dim, T] (reference: audio.py:93-112) '''

    def __init__(self, mode="fbank", num_mel_bins=40, device='cuda', **kwargs):
        super(ExtractAudioFeature, self).__init__()
        if mode not in ("fbank", "mfcc"):
            raise ValueError("feat_type must be 'fbank' or 'mfcc', got {!r}".format(mode))
        self.mode = mode
        self.num_mel_bins = num_mel_bins
        self.kwargs = kwargs
        self.device = device

    def forward(self, filepath):
        ''' filepath: a path, (waveform, sample_rate), (waveform, sample_rate, speed), (waveform, sample_rate, speed,
            dither_key) or (waveform, sample_rate, speed, dither_key, corrupt).  With a speed (None: none) channel 0 of the
            waveform is speed-perturbed on the device first (the kernel of the whole-batch form, B = 1).  The key matters
            only under dither > 0; without one a path gets the evaluation key of seed 0 for its file name
            (Dither(.., 0).key(name, False)) and a tensor key 0.  corrupt (None: none): the one-utterance Corruption of
            NoiseReverb.draws - reverberation and noise on channel 0, behind the speed perturbation (ops.reverb_mix,
            B = 1). '''
        speed, key, corrupt = None, None, None
        if isinstance(filepath, (tuple, list)):
            if len(filepath) == 5:      # .., corrupt: a one-utterance Corruption (NoiseReverb.draws) or None
                waveform, sample_rate, speed, key, corrupt = filepath
            elif len(filepath) == 4:
                waveform, sample_rate, speed, key = filepath
            elif len(filepath) == 3:
                waveform, sample_rate, speed = filepath
            else:
                waveform, sample_rate = filepath
        else:
            waveform, sample_rate = load_wav(filepath)
            if self.kwargs.get('dither', 0.0) != 0.0:
                key = Dither(self.kwargs['dither'], 0).key(utt_name(filepath), False)
        waveform = waveform.to(self.device)
        if speed is not None and float(speed) != 1.0:
            x = _f32c(waveform[0]).reshape(1, -1)
            y, n_out = ops.resample_rows(x, [x.shape[1]], [0], [SpeedPerturb.ratio(speed)], 1.0)
            waveform = y[:, :int(n_out[0])]
        if corrupt is not None and corrupt.any():
            # the whole-batch form's entry with B = 1, behind the speed perturbation: both routes see one waveform
            x = _f32c(waveform[0]).reshape(1, -1)
            waveform = corrupt.apply(x, [x.shape[1]], 1.0, int(sample_rate))[:, :x.shape[1]]
        extract = kaldi_fbank if self.mode == "fbank" else kaldi_mfcc
        y = extract(waveform, num_mel_bins=self.num_mel_bins, channel=-1,
                    sample_frequency=sample_rate, dither_key=0 if key is None else key, **self.kwargs)
        return _transpose2d(y).unsqueeze(0).detach()

    def frame_shift_ms(self):
        ''' milliseconds between two feature frames: the configured value, else the extractor's own default '''
        extract = kaldi_fbank if self.mode == "fbank" else kaldi_mfcc
        return float(self.kwargs.get('frame_shift', inspect.signature(extract).parameters['frame_shift'].default))

    def extra_repr(self):
        return "mode={}, num_mel_bins={}".format(self.mode, self.num_mel_bins)


def audio_num_samples(filepath):
    """-> (samples per channel, sample_rate) from the file header only (wav: RIFF chunk sizes; flac: STREAMINFO) -
    what the collate function needs to order / halve / shard a batch before anything is decoded.  A FLAC stream
    without a stored sample count is decoded to find out."""
    if str(filepath).lower().endswith('.flac'):
        import ctypes
        lib = _lib.load()
        sr, nch, bps, total = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
        md5 = (ctypes.c_uint8 * 16)()
        _lib.check(lib.asrk_flac_info(str(filepath).encode(), ctypes.byref(sr), ctypes.byref(nch), ctypes.byref(bps),
                                      ctypes.byref(total), md5), "flac_info(%s)" % filepath)
        if total.value > 0:
            return int(total.value), int(sr.value)
        x, rate = load_flac(filepath, verify_md5=False)
        return int(x.shape[1]), rate
    with _wave.open(str(filepath), 'rb') as w:
        return w.getnframes(), w.getframerate()


def load_pcm(filepath):
    """-> (int16 numpy [N] of channel 0, sample_rate): the raw 16-bit PCM the batched front end uploads (2 B per
    sample over PCIe; the device applies torchaudio.load's x / 32768).  .wav through the standard library,
    .flac through the native decoder."""
    if str(filepath).lower().endswith('.flac'):
        x, sr = load_flac(filepath)
        q = torch.round(x[0] * 32768.0).clamp_(-32768, 32767).to(torch.int16).numpy()
        if not np.array_equal(q.astype(np.float32) / 32768.0, x[0].numpy()):
            raise ValueError('%s: not 16-bit audio' % filepath)
        return q, sr
    with _wave.open(filepath, 'rb') as w:
        sr, nch, sw, n = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
        raw = w.readframes(n)
    if sw != 2:
        raise ValueError('only 16-bit PCM .wav and .flac files are supported')
    return np.ascontiguousarray(np.frombuffer(raw, dtype='<i2').reshape(-1, nch)[:, 0]), sr


class BatchFeatureTransform:
    """The reference's per-file transform (create_transform: ExtractAudioFeature -> Delta -> CMVN -> Postprocess,
    src/audio.py:115-133) followed by pad_sequence (src/data.py:39) for a WHOLE BATCH in two launches: padded
    PCM [B, Nmax] (int16 or float32) -> log-mel energies of all utterances stacked [sum m, D] in the fused kernel
    (framing, FFT in LDS, power, mel weights, log; FFT sizes 256, 512, 1024) -> delta + CMVN + layout + zero padding in
    one kernel -> (feat [B, Tmax, (order+1)*D], feat_len [B]).  FFT sizes outside 256..1024 take the unfused route
    instead of the first launch: batched framing kernel -> DFT GEMM -> power -> mel GEMM -> log; mfcc adds one DCT
    GEMM; speed factors one resampling launch in front; `dither` > 0 takes the dithered entry of the first launch (one
    64-bit key per utterance, no further launch).  Same arithmetic per frame as the per-file modules (the
    framing is the same code; CMVN sums in a different order: agreement ~1e-6).  Delta filters of up to 15 taps
    (17 and more raise NotImplementedError; create_transform then serves the per-file chain alone)."""

    def __init__(self, audio_config, device='cuda'):
        cfg = dict(audio_config)
        self.feat_type = cfg.pop("feat_type")
        if self.feat_type not in ("fbank", "mfcc"):
            raise ValueError("feat_type must be 'fbank' or 'mfcc', got {!r}".format(self.feat_type))
        self.feat_dim = cfg.pop("feat_dim")
        self.delta_order = cfg.pop("delta_order", 0)
        self.delta_window_size = cfg.pop("delta_window_size", 2)
        self.apply_cmvn = cfg.pop("apply_cmvn")
        self.frame_length = cfg.pop("frame_length", 25.0)
        self.frame_shift = cfg.pop("frame_shift", 10.0)
        self.preemph = cfg.pop("preemphasis_coefficient", 0.97)
        self.remove_dc = cfg.pop("remove_dc_offset", True)
        self.low_freq, self.high_freq = cfg.pop("low_freq", 20.0), cfg.pop("high_freq", 0.0)
        self.num_ceps, self.lifter = cfg.pop("num_ceps", 13), cfg.pop("cepstral_lifter", 22.0)
        self.dither = _dither_amplitude(cfg.pop("dither", 0.0))
        cfg.pop("channel", None)
        if cfg:
            raise NotImplementedError('unsupported fbank options: %s' % sorted(cfg))
        self.device = torch.device(device)
        self.filters = Delta(self.delta_order, self.delta_window_size).filters if self.delta_order >= 1 else \
            torch.ones(1, 1, 1, 1)
        self.out_dim = (self.feat_dim if self.feat_type == "fbank" else self.num_ceps) * (self.delta_order + 1)
        if self.filters.shape[-1] > 16:
            raise NotImplementedError('delta filters longer than 16 taps')
        self._staging, self._staging_ev = {}, {}

    def frame_count(self, n_samples, sample_rate):
        win, shift = int(sample_rate * self.frame_length * 0.001), int(sample_rate * self.frame_shift * 0.001)
        return 0 if n_samples < win else 1 + (n_samples - win) // shift

    def __call__(self, waves, sample_rate, speeds=None, dither_keys=None, corrupt=None):
        """waves: list of 1-D int16 numpy arrays (raw PCM; uploaded as 2-byte samples) or float32 arrays /
        tensors in [-1, 1) -> (feat [B, Tmax, out_dim] on the device, zero padded, feat_len LongTensor [B]).
        speeds: one speed-perturbation factor per utterance (SpeedPerturb), or None.  Utterance b is resampled on the
        device by speeds[b] before the filterbank (one more launch: ops.resample_rows) and feat_len counts the frames
        of the PERTURBED waveform; None, or all factors 1.0, is the plain path: no extra launch, the same bits.
        dither_keys: one 64-bit key per utterance (Dither.key), required when the config's dither is > 0: the noise
        of utterance b is a pure function of dither_keys[b] and acts on the perturbed waveform; with dither 0 they are
        ignored and the launches are the plain ones.
        corrupt: the batch's reverberation / noise draws (NoiseReverb.draws), or None.  Applied behind the speed
        perturbation and in front of the filterbank, whose dither then acts on the corrupted waveform; the lengths do
        not change.  None, or draws that all say "nothing", is the plain path: no extra launch, the same bits."""
        L = _L()
        dev, B = self.device, len(waves)
        if corrupt is not None and len(corrupt) != B:
            raise ValueError('%d reverberation / noise draws for %d utterances' % (len(corrupt), B))
        if self.dither > 0.0 and (dither_keys is None or len(dither_keys) != B):
            raise ValueError('dither = %g needs one key per utterance: got %s for %d utterances'
                             % (self.dither, 'none' if dither_keys is None else len(dither_keys), B))
        is_i16 = all(isinstance(w, np.ndarray) and w.dtype == np.int16 for w in waves)
        arrs = [w if is_i16 else torch.as_tensor(w, dtype=torch.float32).reshape(-1).numpy() for w in waves]
        ns_src = [int(a.shape[0]) for a in arrs]
        perturb = speeds is not None and any(float(f) != 1.0 for f in speeds)
        if perturb:
            if len(speeds) != B:
                raise ValueError('%d speed factors for %d utterances' % (len(speeds), B))
            ratios, ridx = [], []
            for f in speeds:
                r = SpeedPerturb.ratio(f)
                if r not in ratios:
                    ratios.append(r)
                ridx.append(ratios.index(r))
            ns = [SpeedPerturb.out_samples(n, f) for n, f in zip(ns_src, speeds)]
        else:
            ns = ns_src
        tb = _FbankTables.get(int(sample_rate), self.frame_length, self.frame_shift, self.feat_dim, self.low_freq,
                              self.high_freq, dev)
        ms = [self.frame_count(n, sample_rate) for n in ns]
        Tmax, total = max(ms), sum(ms)
        D = self.feat_dim if self.feat_type == "fbank" else self.num_ceps
        C, Lf = self.delta_order + 1, self.filters.shape[-1]
        feat_len = torch.LongTensor(ms)
        out = torch.empty((B, Tmax, C * D), dtype=torch.float32, device=dev)
        if total == 0:
            return out, feat_len
        nmax = max(ns_src)
        # persistent pinned staging buffer (pinning per batch costs more than the whole front end); rows are
        # NOT cleared: the framing kernel never reads beyond an utterance's own last frame
        tdt = torch.int16 if is_i16 else torch.float32
        need = B * nmax
        st = self._staging.get(tdt)
        if st is None or st.numel() < need:
            if st is not None and self._staging_ev.get(tdt) is not None:
                self._staging_ev[tdt].synchronize()
            st = torch.empty((need + need // 4,), dtype=tdt).pin_memory()
            self._staging[tdt] = st
        elif self._staging_ev.get(tdt) is not None:
            self._staging_ev[tdt].synchronize()      # the previous batch's upload has left the buffer
        host_t = st[:need].view(B, nmax)
        host = host_t.numpy()
        for b, a in enumerate(arrs):
            host[b, :ns_src[b]] = a
        wave = host_t.to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._staging_ev[tdt] = ev
        sbytes, scale = (2, 1.0 / 32768.0) if is_i16 else (4, 1.0)
        if perturb:
            # [B, nmax] PCM -> [B, ld] float32 waveforms at the perturbed speeds, already scaled
            wave, _ = ops.resample_rows(wave, ns_src, ridx, ratios, scale)
            nmax, sbytes, scale = wave.shape[1], 4, 1.0
        if corrupt is not None and corrupt.any():
            # reverberation and noise on the (perturbed) waveforms: [B, nmax] -> [B, ld] float32, already scaled
            wave = corrupt.apply(wave, ns, scale, int(sample_rate))
            nmax, sbytes, scale = wave.shape[1], 4, 1.0
        offs = np.zeros(B + 1, dtype=np.int64)
        offs[1:] = np.cumsum(ms)
        frame_off = torch.from_numpy(offs).to(dev)
        n_host = np.asarray(ns, dtype=np.int64)
        keys = _keys_to_device(dither_keys, dev) if self.dither > 0.0 else None
        if tb.fused:
            mel = _pcm_to_logmel(wave, sbytes, nmax, n_host, frame_off, B, Tmax, total, tb, self.feat_dim, scale,
                                 self.preemph, self.remove_dc, self.dither, keys)
        else:
            frames = torch.empty((total, tb.ldf), dtype=torch.float32, device=dev)
            args = (_p(wave), sbytes, nmax, n_host.ctypes.data, _p(frame_off), B, Tmax, _p(tb.window), _p(frames),
                    tb.win, tb.shift, tb.ldf, scale, self.preemph, int(self.remove_dc))
            if self.dither > 0.0:
                _lib.check(L.asrk_fbank_frames_batch_dither_f32(*args, self.dither, _p(keys), _stream()),
                           'fbank_frames_batch_dither')
            else:
                _lib.check(L.asrk_fbank_frames_batch_f32(*args, _stream()), 'fbank_frames_batch')
            mel = _frames_to_logmel(frames, tb, self.feat_dim)
        if self.feat_type == "mfcc":
            tab = _mfcc_table(self.feat_dim, self.num_ceps, self.lifter, dev)
            cep = torch.empty((total, self.num_ceps), dtype=torch.float32, device=dev)
            ops.gemm(0, 0, total, self.num_ceps, self.feat_dim, mel, self.feat_dim, tab, self.num_ceps, cep,
                     self.num_ceps)
            mel = cep
        filt = _f32c(self.filters.reshape(C, Lf).to(dev))
        _lib.check(L.asrk_delta_cmvn_batch_f32(_p(mel), _p(frame_off), B, D, _p(filt), C, Lf, int(self.apply_cmvn),
                                               1e-10, _p(out), Tmax, _stream()), 'delta_cmvn_batch')
        return out, feat_len


_M64 = (1 << 64) - 1


def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


class SpecAugment:
    """SpecAugment (Park et al. 2019: time warp, frequency masks, time masks) for a padded training batch that is
    already in HBM.  The policy is sampled on the HOST into one int32 row per utterance, as a pure function of
    (lens, seed, step, rank); the device side is one launch (ops.spec_augment -> csrc/spec_augment.hip, semantics in
    include/asrk.h).  Resuming from a checkpoint at step s therefore continues the same stream of masks: nothing of it
    is state.

    Row layout, P = 2 + 2*n_freq_mask + 2*n_time_mask: c, w, f0_0, fw_0, .., t0_0, tw_0, ..  For an utterance of n
    frames, D = feat_dim mel bins, W = time_warp:
      * n >= 2W + 2 and W >= 2: c ~ U{W..n-1-W} (the frame that moves), w ~ U{-(W-1)..W-1} (by how much); else c = w = 0;
      * fw ~ U{0..min(freq_mask_width, D)}, f0 ~ U{0..D-fw};
      * tw ~ U{0..min(time_mask_width, floor(time_mask_ratio * n))}, t0 ~ U{0..n-tw}."""

    KEYS = ('freq_mask_width', 'n_freq_mask', 'time_mask_width', 'n_time_mask', 'time_mask_ratio', 'time_warp',
            'mask_value')
    MAX_MASKS = 8           # SA_MAX_MASKS of csrc/spec_augment.hip

    def __init__(self, feat_dim, channels, freq_mask_width=27, n_freq_mask=2, time_mask_width=100, n_time_mask=2,
                 time_mask_ratio=1.0, time_warp=80, mask_value=0.0):
        ints = dict(feat_dim=feat_dim, channels=channels, freq_mask_width=freq_mask_width, n_freq_mask=n_freq_mask,
                    time_mask_width=time_mask_width, n_time_mask=n_time_mask, time_warp=time_warp)
        for k, v in ints.items():
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError('specaug: %s must be a non-negative integer, got %r' % (k, v))
        if feat_dim < 1 or channels < 1:
            raise ValueError('specaug: feat_dim and channels must be positive')
        if n_freq_mask > self.MAX_MASKS or n_time_mask > self.MAX_MASKS:
            raise ValueError('specaug: at most %d masks of each kind' % self.MAX_MASKS)
        if isinstance(time_mask_ratio, bool) or not isinstance(time_mask_ratio, (int, float)) or \
                not 0.0 <= time_mask_ratio < float('inf'):
            raise ValueError('specaug: time_mask_ratio must be a non-negative number, got %r' % (time_mask_ratio,))
        if isinstance(mask_value, bool) or not isinstance(mask_value, (int, float)) or not math.isfinite(mask_value):
            raise ValueError('specaug: mask_value must be a finite number, got %r' % (mask_value,))
        self.feat_dim, self.channels = feat_dim, channels
        self.freq_mask_width, self.n_freq_mask = freq_mask_width, n_freq_mask
        self.time_mask_width, self.n_time_mask = time_mask_width, n_time_mask
        self.time_mask_ratio, self.time_warp, self.mask_value = float(time_mask_ratio), time_warp, float(mask_value)
        self.P = 2 + 2 * n_freq_mask + 2 * n_time_mask

    @classmethod
    def from_config(cls, cfg, feat_dim, channels):
        """cfg: the whole yaml config (a mapping); its top-level `specaug:` block holds `enable` and the constructor's
        keys.  -> None when the block is absent or `enable: false`."""
        block = cfg.get('specaug') if cfg is not None else None
        if block is None:
            return None
        if not isinstance(block, dict):
            raise ValueError('specaug: expected a mapping, got %r' % (block,))
        block = dict(block)
        enable = block.pop('enable', True)
        if not isinstance(enable, bool):
            raise ValueError('specaug: enable must be true or false, got %r' % (enable,))
        unknown = sorted(set(block) - set(cls.KEYS))
        if unknown:
            raise ValueError('specaug: unknown key(s) %s (known: enable, %s)' % (unknown, ', '.join(cls.KEYS)))
        policy = cls(feat_dim, channels, **block)        # a disabled block is still checked
        return policy if enable else None

    @staticmethod
    def stream_seed(seed, step, rank=0):
        """the generator seed of one (run seed, data-parallel rank, training step)"""
        z = 0
        for v in (seed, rank, step):
            z = _splitmix64(z ^ (int(v) & _M64))
        return z & 0x7fffffffffffffff

    def sample(self, lens, seed, step, rank=0):
        """lens: the utterances' frame counts ON THE HOST (list / numpy / CPU tensor) -> int32 [B, P] (CPU)"""
        if torch.is_tensor(lens):
            if lens.is_cuda:
                raise ValueError('SpecAugment.sample takes the lengths on the host (reading them back would stall the '
                                 'step)')
            lens = lens.numpy()
        n = np.maximum(np.asarray(lens, dtype=np.int64).reshape(-1), 0)
        B, D, W, nf = n.shape[0], self.feat_dim, self.time_warp, self.n_freq_mask
        g = torch.Generator()
        g.manual_seed(self.stream_seed(seed, step, rank))
        # one uniform per table entry, drawn whether the entry is used or not: an entry's value never depends on
        # which of the other entries were active.  U{0..count-1} = min(floor(u * count), count - 1) in float64.
        # (numpy from here on: the table is a few dozen numbers and this runs on the host inside the training step)
        u = torch.rand((B, self.P), generator=g, dtype=torch.float64).numpy()
        fw_cols, tw_cols = np.arange(3, 2 + 2 * nf, 2), np.arange(3 + 2 * nf, self.P, 2)
        count = np.ones((B, self.P), dtype=np.int64)
        count[:, 0], count[:, 1] = np.maximum(n - 2 * W, 1), max(2 * W - 1, 1)
        count[:, fw_cols] = min(self.freq_mask_width, D) + 1
        cap = np.minimum(np.floor(n * self.time_mask_ratio).astype(np.int64), np.minimum(n, self.time_mask_width))
        count[:, tw_cols] = cap[:, None] + 1
        tab = np.minimum((u * count).astype(np.int64), count - 1)               # c - W, w + W - 1, every fw and tw
        # the offsets depend on the widths drawn above: f0 ~ U{0..D-fw}, t0 ~ U{0..n-tw}
        count[:, fw_cols - 1] = D - tab[:, fw_cols] + 1
        count[:, tw_cols - 1] = n[:, None] - tab[:, tw_cols] + 1
        off_cols = np.concatenate([fw_cols, tw_cols]) - 1
        tab[:, off_cols] = np.minimum((u[:, off_cols] * count[:, off_cols]).astype(np.int64), count[:, off_cols] - 1)
        on = (n >= 2 * W + 2) & (W >= 2)
        tab[:, 0] = np.where(on, tab[:, 0] + W, 0)
        tab[:, 1] = np.where(on, tab[:, 1] - (W - 1), 0)
        return torch.from_numpy(tab.astype(np.int32))

    def __call__(self, feat, feat_len_host, seed, step, rank=0, feat_len_dev=None):
        """feat [B, T, channels * feat_dim] on the GPU -> its augmented copy.  feat_len_host: the lengths as the collate
        function returned them (host); feat_len_dev: the same lengths already on the device (int64) when the caller
        has them, else they are uploaded here.  Nothing in here waits for the device."""
        if feat.shape[-1] != self.channels * self.feat_dim:
            raise ValueError('specaug: features are %d wide, policy was built for %d x %d' % (
                feat.shape[-1], self.channels, self.feat_dim))
        tab = self.sample(feat_len_host, seed, step, rank)
        params = tab.pin_memory().to(feat.device, non_blocking=True)
        if feat_len_dev is None:
            feat_len_dev = torch.as_tensor(feat_len_host, dtype=torch.int64).reshape(-1).pin_memory().to(
                feat.device, non_blocking=True)
        with torch.no_grad():
            return ops.spec_augment(feat, feat_len_dev, params, self.n_freq_mask, self.n_time_mask, self.mask_value,
                                    channels=self.channels)

    def create_msg(self):
        return 'SpecAugment| time warp W = {} | {} freq. mask(s) <= {} of {} bins | {} time mask(s) <= min({}, {} * len) ' \
               '| fill = {}'.format(self.time_warp, self.n_freq_mask, self.freq_mask_width, self.feat_dim,
                                    self.n_time_mask, self.time_mask_width, self.time_mask_ratio, self.mask_value)


class SpeedPerturb:
    """Speed perturbation (the Kaldi / LibriSpeech recipe: every training utterance resampled by a factor drawn from
    {0.9, 1.0, 1.1}; pitch and duration change together) for a padded PCM batch that is already in HBM.  A factor f is
    the rational speed orig / new with two decimals in [0.5, 2.0] (both terms at most 100 once reduced: 1.01 = 101:100
    is refused); the utterance is read as sampled at f * sr and converted to sr by
    the polyphase kernel behind ops.resample_rows (csrc/resample.hip, semantics in include/asrk.h), so n samples become
    ceil(n * new / orig).

    The draw is stateless and the same on every data-parallel rank: a pure function of (seed, epoch_key, utterance
    name), so all ranks deal a global batch by the same perturbed lengths.  `begin_epoch(key)` sets epoch_key (the
    solver passes the step at which the epoch starts: a run resumed in mid-epoch draws the rest of that epoch from the
    step it resumed at - a known limit)."""

    KEYS = ('factors',)
    MAX_FACTORS = 8             # RS_MAX_RATIOS of csrc/resample.hip
    DEFAULT_FACTORS = (0.9, 1.0, 1.1)

    def __init__(self, factors=DEFAULT_FACTORS, seed=0):
        if isinstance(factors, (str, bytes)) or not isinstance(factors, (list, tuple)):
            raise ValueError('speed_perturb: factors must be a list of numbers, got %r' % (factors,))
        if not 1 <= len(factors) <= self.MAX_FACTORS:
            raise ValueError('speed_perturb: between 1 and %d factors, got %d' % (self.MAX_FACTORS, len(factors)))
        self.ratios = [self.ratio(f) for f in factors]          # validates every factor
        self.factors = [float(f) for f in factors]
        self.seed, self.epoch_key = int(seed), 0

    @staticmethod
    def ratio(f):
        """factor -> the coprime (orig, new) of speed = orig / new"""
        if isinstance(f, bool) or not isinstance(f, (int, float)) or not math.isfinite(f):
            raise ValueError('speed_perturb: a factor must be a number, got %r' % (f,))
        c = round(f * 100.0)
        if abs(f * 100.0 - c) > 1e-6:
            raise ValueError('speed_perturb: factors have at most two decimals, got %r' % (f,))
        if not 50 <= c <= 200:
            raise ValueError('speed_perturb: factors lie in [0.5, 2.0], got %r' % (f,))
        q = Fraction(int(c), 100)
        if q.numerator > 100:
            raise ValueError('speed_perturb: %r is %d:%d in lowest terms; the resampler takes terms up to 100'
                             % (f, q.numerator, q.denominator))
        return q.numerator, q.denominator

    @classmethod
    def out_samples(cls, n, f):
        """sample count of an n-sample utterance after perturbation by factor f: ceil(n * new / orig)"""
        orig, new = cls.ratio(f)
        return (new * int(n) + orig - 1) // orig

    @classmethod
    def from_config(cls, cfg, seed=0):
        """cfg: the whole yaml config (a mapping); its top-level `speed_perturb:` block holds `enable` and `factors`.
        -> None when the block is absent or `enable: false`."""
        block = cfg.get('speed_perturb') if cfg is not None else None
        if block is None:
            return None
        if not isinstance(block, dict):
            raise ValueError('speed_perturb: expected a mapping, got %r' % (block,))
        block = dict(block)
        enable = block.pop('enable', True)
        if not isinstance(enable, bool):
            raise ValueError('speed_perturb: enable must be true or false, got %r' % (enable,))
        unknown = sorted(set(block) - set(cls.KEYS))
        if unknown:
            raise ValueError('speed_perturb: unknown key(s) %s (known: enable, %s)' % (unknown, ', '.join(cls.KEYS)))
        policy = cls(seed=seed, **block)                        # a disabled block is still checked
        return policy if enable else None

    def begin_epoch(self, epoch_key):
        self.epoch_key = int(epoch_key)

    def factor(self, name):
        """the factor of utterance `name` in the current epoch"""
        z = (self.seed & _M64) ^ _splitmix64(self.epoch_key & _M64) ^ zlib.crc32(name.encode())
        return self.factors[_splitmix64(z) % len(self.factors)]

    def create_msg(self):
        return 'SpeedPerturb| factors = {} (orig:new = {}) | drawn per utterance and epoch, the same on every rank' \
            .format(self.factors, ', '.join('%d:%d' % r for r in self.ratios))


def utt_name(path):
    """file name without directories and extensions: the name the stateless draws hash"""
    return str(path).split('/')[-1].split('.')[0]


class Dither:
    """Key policy of the dithered filterbank (the reference's `data.audio.dither`, forwarded to torchaudio's kaldi
    fbank / mfcc, which add randn * dither to every frame).  The amplitude is in the units of the [-1, 1) waveform:
    Kaldi's default of 1.0 belongs to the int16 scale and is 1 / 32768 = 3.05e-5 here.

    The device draws the noise of an utterance as a pure function of one 64-bit key (include/asrk.h); this class deals
    the keys, stateless and the same on every data-parallel rank: a function of (seed, epoch_key, utterance name) for
    training - `begin_epoch(key)` as for SpeedPerturb - and of (seed, utterance name) alone for evaluation, so dev and
    test features are the same on every pass, rank and run (the reference redraws them: DESIGN.md section 1,
    deviation viii)."""

    TAG = 0x6474685F6B657931         # keeps the stream apart from SpeedPerturb.factor's hash of the same triple

    def __init__(self, amplitude, seed=0):
        self.amplitude = _dither_amplitude(amplitude)
        self.seed, self.epoch_key = int(seed), 0

    @classmethod
    def from_config(cls, cfg, seed=0):
        """cfg: the whole yaml config (a mapping) -> a policy for cfg['data']['audio']['dither'], None when the key is
        absent or 0; ValueError for a negative, non-finite or non-numeric value"""
        block = cfg.get('data') if cfg is not None else None
        block = block.get('audio') if isinstance(block, dict) else None
        if not isinstance(block, dict) or 'dither' not in block:
            return None
        policy = cls(block['dither'], seed)
        return policy if policy.amplitude > 0.0 else None

    def begin_epoch(self, epoch_key):
        self.epoch_key = int(epoch_key)

    def key(self, name, train):
        """the 64-bit key of utterance `name`: of the current epoch when train, of epoch key 0 otherwise"""
        ek = self.epoch_key if train else 0
        return _splitmix64((self.seed & _M64) ^ _splitmix64(ek & _M64) ^ zlib.crc32(name.encode()) ^ self.TAG)

    def create_msg(self):
        return 'Dither     | amplitude = {:g} of the [-1, 1) waveform ({:g} on the int16 scale) | per (frame, position), ' \
               'keyed by utterance and epoch; fixed for dev / test'.format(self.amplitude, self.amplitude * 32768.0)


def scan_audio_dir(path):
    """every .wav / .flac file under `path` (recursively), sorted by its path relative to `path`"""
    found = []
    for root, _, files in os.walk(str(path)):
        for f in files:
            if f.lower().endswith(('.wav', '.flac')):
                found.append(os.path.relpath(os.path.join(root, f), str(path)))
    return [os.path.join(str(path), r) for r in sorted(found)]


def load_rir(filepath, max_taps):
    """-> (float32 [K] of channel 0, K = min(samples, max_taps); sample_rate).  ValueError, with the file named, for an
    empty or all-zero response and for one whose peak - the first index of the largest |h| of the WHOLE file - lies at
    or beyond max_taps (truncation would cut the direct sound off)."""
    q, sr = load_pcm(filepath)
    h = q.astype(np.float32) / np.float32(32768.0)
    if h.shape[0] == 0 or not np.any(h):
        raise ValueError('noise_reverb: %s holds no impulse response (empty or all zero)' % filepath)
    peak = int(np.argmax(np.abs(h)))
    if peak >= max_taps:
        raise ValueError('noise_reverb: the peak of %s lies at sample %d, beyond max_taps = %d'
                         % (filepath, peak, max_taps))
    return np.ascontiguousarray(h[:max_taps]), sr


Draw = collections.namedtuple('Draw', 'rir noise offset snr_db')     # rir / noise: file index or -1; offset in [0, 1)


class Corruption:
    """the draws of one batch with the policy that made them: what BatchFeatureTransform's `corrupt=` takes"""

    def __init__(self, policy, draws):
        self.policy, self.draws = policy, list(draws)

    def __len__(self):
        return len(self.draws)

    def any(self):
        return any(d.rir >= 0 or d.noise >= 0 for d in self.draws)

    def apply(self, wave, ns, scale, sample_rate):
        """wave [B, ld] int16 or float32 on the GPU (row b holds ns[b] samples) -> the corrupted float32 batch, already
        multiplied by `scale` (one ops.reverb_mix call; the noise rows are of wave's type and go up in one upload)"""
        pol, B = self.policy, len(self.draws)
        if wave.shape[0] != B:
            raise ValueError('%d draws for %d utterances' % (B, wave.shape[0]))
        bank = pol.bank(wave.device, sample_rate) if any(d.rir >= 0 for d in self.draws) else None
        noise, ms = None, [0] * B
        if any(d.noise >= 0 for d in self.draws):
            host, ms = pol.noise_rows(self.draws, ns, wave.dtype == torch.int16, sample_rate)
            noise = host.to(wave.device, non_blocking=True)
            pol.mark_upload()
        snr = [10.0 ** (d.snr_db / 10.0) for d in self.draws]
        return ops.reverb_mix(wave, ns, bank, [d.rir for d in self.draws], noise, ms, snr, scale)


class NoiseReverb:
    """Multi-condition training (the Kaldi / LibriSpeech recipe): an utterance is convolved with a room impulse response
    and a noise recording is added at a drawn signal-to-noise ratio, on the batch while it sits in HBM
    (ops.reverb_mix -> csrc/reverb_mix.hip, semantics in include/asrk.h).  The utterance keeps its length.

    rir:   {path, prob, max_taps}: every .wav / .flac under `path` (recursively, sorted, first channel), truncated to
           max_taps <= 8192 samples; loaded and checked when the policy is built, uploaded once.
    noise: {path, prob, snr_db: [lo, hi]}: files are decoded when first drawn and kept in a bounded host cache; the row
           that goes up starts at a drawn offset and holds min(utterance, file) samples - a shorter file is rotated to
           the offset and tiled circularly by the kernel.
    Either block may be absent.  All files must have the corpus' sample rate (checked against the first batch's rate for
    the responses, per file for the noise; nothing is resampled).

    The draw - response or none, which, noise or none, which, offset, SNR uniform in dB - is stateless and the same on
    every data-parallel rank: a pure function of (seed, epoch_key, utterance name); `begin_epoch(key)` as for
    SpeedPerturb."""

    KEYS = ('rir', 'noise')
    RIR_KEYS = ('path', 'prob', 'max_taps')
    NOISE_KEYS = ('path', 'prob', 'snr_db')
    TAG = 0x6E7276625F647277        # keeps the stream apart from SpeedPerturb.factor's and Dither.key's
    MAX_TAPS = ops.REVERB_MAX_TAPS
    CACHE_BYTES = 256 << 20         # decoded noise kept on the host

    def __init__(self, rir=None, noise=None, seed=0):
        self.seed, self.epoch_key = int(seed), 0
        self.rir_prob, self.rir_files, self.rirs, self.rir_rate, self.max_taps = 0.0, [], [], None, self.MAX_TAPS
        self.noise_prob, self.noise_files, self.snr_db = 0.0, [], (0.0, 0.0)
        if rir is not None:
            rir = self._block('rir', rir, self.RIR_KEYS)
            self.rir_prob = self._prob('rir', rir.get('prob', 0.5))
            mt = rir.get('max_taps', self.MAX_TAPS)
            if isinstance(mt, bool) or not isinstance(mt, int) or not 1 <= mt <= self.MAX_TAPS:
                raise ValueError('noise_reverb: rir.max_taps must be an integer in 1..%d, got %r' % (self.MAX_TAPS, mt))
            self.max_taps = mt
            self.rir_files = self._files('rir', rir)
            for f in self.rir_files:
                h, sr = load_rir(f, mt)
                if self.rir_rate is None:
                    self.rir_rate = sr
                elif sr != self.rir_rate:
                    raise ValueError('noise_reverb: %s is sampled at %d Hz, %s at %d Hz'
                                     % (f, sr, self.rir_files[0], self.rir_rate))
                self.rirs.append(h)
        if noise is not None:
            noise = self._block('noise', noise, self.NOISE_KEYS)
            self.noise_prob = self._prob('noise', noise.get('prob', 0.5))
            snr = noise.get('snr_db', [5.0, 20.0])
            if (not isinstance(snr, (list, tuple)) or len(snr) != 2
                    or any(isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) for v in snr)):
                raise ValueError('noise_reverb: noise.snr_db must be [lo, hi], two finite numbers, got %r' % (snr,))
            if snr[0] > snr[1]:
                raise ValueError('noise_reverb: noise.snr_db has lo > hi: %r' % (snr,))
            self.snr_db = (float(snr[0]), float(snr[1]))
            self.noise_files = self._files('noise', noise)
        self._bank, self._cache, self._cache_bytes = None, collections.OrderedDict(), 0
        self._staging, self._staging_ev = {}, None

    @staticmethod
    def _block(name, block, keys):
        if not isinstance(block, dict):
            raise ValueError('noise_reverb: %s must be a mapping, got %r' % (name, block))
        unknown = sorted(set(block) - set(keys))
        if unknown:
            raise ValueError('noise_reverb: unknown key(s) %s in %s (known: %s)' % (unknown, name, ', '.join(keys)))
        return block

    @staticmethod
    def _prob(name, p):
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
            raise ValueError('noise_reverb: %s.prob must be a number in [0, 1], got %r' % (name, p))
        return float(p)

    @staticmethod
    def _files(name, block):
        path = block.get('path')
        if not isinstance(path, str) or not os.path.isdir(path):
            raise ValueError('noise_reverb: %s.path must be an existing directory, got %r' % (name, path))
        files = scan_audio_dir(path)
        if not files:
            raise ValueError('noise_reverb: no .wav or .flac file under %s.path = %r' % (name, path))
        return files

    @classmethod
    def from_config(cls, cfg, seed=0):
        """cfg: the whole yaml config (a mapping); its top-level `noise_reverb:` block holds `enable`, `rir` and `noise`.
        -> None when the block is absent or `enable: false`."""
        block = cfg.get('noise_reverb') if cfg is not None else None
        if block is None:
            return None
        if not isinstance(block, dict):
            raise ValueError('noise_reverb: expected a mapping, got %r' % (block,))
        block = dict(block)
        enable = block.pop('enable', True)
        if not isinstance(enable, bool):
            raise ValueError('noise_reverb: enable must be true or false, got %r' % (enable,))
        unknown = sorted(set(block) - set(cls.KEYS))
        if unknown:
            raise ValueError('noise_reverb: unknown key(s) %s (known: enable, %s)' % (unknown, ', '.join(cls.KEYS)))
        policy = cls(seed=seed, **block)                        # a disabled block is still checked
        return policy if enable else None

    def begin_epoch(self, epoch_key):
        self.epoch_key = int(epoch_key)

    def draw(self, name):
        """the Draw of utterance `name` in the current epoch.  Six uniforms are taken whether they are used or not, so
        no decision depends on which of the others were active."""
        z = _splitmix64((self.seed & _M64) ^ _splitmix64(self.epoch_key & _M64) ^ zlib.crc32(name.encode()) ^ self.TAG)
        u = [(_splitmix64((z + i) & _M64) >> 11) / float(1 << 53) for i in range(6)]
        rir = min(int(u[1] * len(self.rirs)), len(self.rirs) - 1) if self.rirs and u[0] < self.rir_prob else -1
        nf = len(self.noise_files)
        noise = min(int(u[3] * nf), nf - 1) if nf and u[2] < self.noise_prob else -1
        lo, hi = self.snr_db
        return Draw(rir, noise, u[4], min(max(lo + u[5] * (hi - lo), lo), hi))

    def draws(self, names):
        """-> the Corruption of a batch of utterance names (BatchFeatureTransform's `corrupt=`)"""
        return Corruption(self, [self.draw(n) for n in names])

    def bank(self, device, sample_rate):
        """the responses on the device (uploaded on first use); ValueError when their rate is not the corpus'"""
        if self.rir_rate != sample_rate:
            raise ValueError('noise_reverb: %s is sampled at %d Hz, the corpus at %d Hz (nothing is resampled)'
                             % (self.rir_files[0], self.rir_rate, sample_rate))
        if self._bank is None or self._bank.taps.device != torch.device(device):
            self._bank = ops.RirBank(self.rirs, device)
        return self._bank

    def noise_pcm(self, index, sample_rate):
        """int16 samples of noise file `index` through the bounded host cache (least recently used files leave)"""
        hit = self._cache.get(index)
        if hit is not None:
            self._cache.move_to_end(index)
            return hit
        path = self.noise_files[index]
        q, sr = load_pcm(path)
        if sr != sample_rate:
            raise ValueError('noise_reverb: %s is sampled at %d Hz, the corpus at %d Hz (nothing is resampled)'
                             % (path, sr, sample_rate))
        self._cache[index] = q
        self._cache_bytes += q.nbytes
        while self._cache_bytes > self.CACHE_BYTES and len(self._cache) > 1:
            _, old = self._cache.popitem(last=False)
            self._cache_bytes -= old.nbytes
        return q

    @staticmethod
    def fill_row(row, pcm, n, offset):
        """row[:m] = the m = min(n, len(pcm)) samples of `pcm` from int(offset * len(pcm)) on, wrapping at its end
        (a file shorter than the utterance: the whole file rotated to the offset) -> m"""
        Lf = int(pcm.shape[0])
        m = min(int(n), Lf)
        if m > 0:
            start = min(int(offset * Lf), Lf - 1)
            first = min(m, Lf - start)
            row[:first] = pcm[start:start + first]
            row[first:m] = pcm[:m - first]
        return m

    def noise_rows(self, draws, ns, as_int16, sample_rate):
        """-> (pinned host tensor [B, max m] of int16, or of float32 = int16 / 32768; m per row).  The buffer is
        persistent: the previous batch's upload is waited for before it is refilled."""
        pcm = [None if d.noise < 0 else self.noise_pcm(d.noise, sample_rate) for d in draws]
        ms = [0 if q is None else min(int(n), int(q.shape[0])) for q, n in zip(pcm, ns)]
        B, ld = len(draws), max(max(ms), 1)
        tdt = torch.int16 if as_int16 else torch.float32
        st = self._staging.get(tdt)
        if self._staging_ev is not None:
            self._staging_ev.synchronize()
            self._staging_ev = None
        if st is None or st.numel() < B * ld:
            st = torch.empty((B * ld + B * ld // 4,), dtype=tdt).pin_memory()
            self._staging[tdt] = st
        host_t = st[:B * ld].view(B, ld)
        host = host_t.numpy()
        for b, (q, d) in enumerate(zip(pcm, draws)):
            if q is None:
                continue
            if as_int16:
                self.fill_row(host[b], q, ns[b], d.offset)
            else:
                tmp = np.empty(ms[b], dtype=np.int16)
                self.fill_row(tmp, q, ns[b], d.offset)
                host[b, :ms[b]] = tmp.astype(np.float32) / np.float32(32768.0)
        return host_t, ms

    def mark_upload(self):
        ev = torch.cuda.Event()
        ev.record()
        self._staging_ev = ev

    def create_msg(self):
        return 'NoiseReverb| {} RIR(s) <= {} taps, prob = {:g} | {} noise file(s), prob = {:g}, SNR in [{:g}, {:g}] dB ' \
               '| drawn per utterance and epoch, the same on every rank' \
            .format(len(self.rirs), self.max_taps, self.rir_prob, len(self.noise_files), self.noise_prob,
                    self.snr_db[0], self.snr_db[1])


def create_transform(audio_config, device='cuda'):
    ''' same contract as the reference (audio.py:115-133): pops feat_type / feat_dim / delta_order /
    delta_window_size / apply_cmvn, the rest are fbank kwargs; returns (Sequential, output dim) '''
    try:                                    # the whole-batch form of the same chain (collate uses it when present)
        batch_form = BatchFeatureTransform(audio_config, device=device)
    except NotImplementedError:
        batch_form = None
    feat_type = audio_config.pop("feat_type")
    feat_dim = audio_config.pop("feat_dim")

    delta_order = audio_config.pop("delta_order", 0)
    delta_window_size = audio_config.pop("delta_window_size", 2)
    apply_cmvn = audio_config.pop("apply_cmvn")

    transforms = [ExtractAudioFeature(feat_type, feat_dim, device=device, **audio_config)]
    if delta_order >= 1:
        transforms.append(Delta(delta_order, delta_window_size))
    if apply_cmvn:
        transforms.append(CMVN())
    transforms.append(Postprocess())

    seq = nn.Sequential(*transforms)
    seq.batch = batch_form                  # plain attribute: not a submodule, not part of any state_dict
    return seq, feat_dim * (delta_order + 1)
