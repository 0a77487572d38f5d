"""Vocoder registry + the HiFi-GAN and Parallel WaveGAN wrappers — vocoders/base_vocoder.py:6-40, vocoders/hifigan.py:17-69 and
vocoders/pwg.py:18-105.

``register_vocoder`` / ``get_vocoder_cls(hparams)`` (short name, or the reference's dotted path
``vocoders.hifigan.HifiGAN``), ``BaseVocoder.spec2wav(mel[T,80]) -> wav[T*hop]``.  ``HifiGAN`` loads
``<vocoder_ckpt>/config.yaml`` + the newest ``model_ckpt_steps_*.ckpt`` (``['state_dict']['model_gen']``, weight-norm
layout, strict) — or, when there is no config.yaml, the original release's ``config.json`` + ``generator_v1``
(``['generator']``) — folds the weight norm and runs the generator on the HIP kernels.

``PWG`` (``vocoder: pwg``, the default of configs/tts/base.yaml) loads ``<vocoder_ckpt>/config.yaml`` + the newest
``model_ckpt_steps_*.ckpt`` (``['state_dict']`` keys ``model_gen.*``, not strict) or, with ``vocoder_ckpt == ''``, the official release's
files under ``wavegan_pretrained/`` (``['model']['generator']`` + mean / scale statistics), and runs ``ParallelWaveGANGenerator`` on the
kernels of csrc/pwg.hip.  Its ``wav2spec`` / ``wav2mfcc`` are data preparation and stay ``NotImplementedError``.

``denoise(wav, v)`` is the spectral post-filter behind ``hparams['vocoder_denoise_c']`` (vocoders/vocoder_utils.py:7-15: STFT, ``|S| - v``
clipped at 0 with the phase kept, inverse STFT).  The reference runs it through librosa on the host; here it is one fused HIP launch
(csrc/wavden.hip, ``bsg_wavden_*``) on the waveform where the vocoder left it, for one waveform or a padded batch with per-row lengths.
"""
import ctypes
import importlib
import os

import numpy as np
import torch

from . import _lib
from .ckpt import latest_ckpt
from .hparams import hparams, set_hparams

VOCODERS = {}


def register_vocoder(cls):
    VOCODERS[cls.__name__.lower()] = cls
    VOCODERS[cls.__name__] = cls
    return cls


def get_vocoder_cls(hp):
    name = hp['vocoder']
    if name in VOCODERS:
        return VOCODERS[name]
    if name.split('.')[-1] in VOCODERS and name.startswith('vocoders.'):
        return VOCODERS[name.split('.')[-1]]          # the reference's module path maps onto this registry
    pkg, cls_name = '.'.join(name.split('.')[:-1]), name.split('.')[-1]
    return getattr(importlib.import_module(pkg), cls_name)


class BaseVocoder:
    def spec2wav(self, mel):
        """mel [T,80] -> wav [T*hop]"""
        raise NotImplementedError

    @staticmethod
    def wav2spec(wav_fn):
        raise NotImplementedError('analysis (wav -> mel) is data preparation, outside the hot path')


def load_model(config_path, checkpoint_path, device=None):
    """vocoders/hifigan.py:17-33: `config.yaml` + a trainer checkpoint (['state_dict']['model_gen']), or the layout of the original HiFi-GAN
    release: `config.json` + `generator_v1` (['generator']).  Strict load in the weight-norm layout, then the fold."""
    from .hifigan import HifiGanGenerator
    device = device or torch.device('cuda')
    ckpt = torch.load(checkpoint_path, map_location='cpu')
    if '.yaml' in config_path:
        config = set_hparams(config_path, global_hparams=False, print_hparams=False)
        state = ckpt['state_dict']['model_gen']
    elif '.json' in config_path:
        import json
        config = json.load(open(config_path, 'r'))
        state = ckpt['generator']
        if 'audio_sample_rate' not in config and 'sampling_rate' in config:      # the release's key; only the NSF source reads it
            config['audio_sample_rate'] = config['sampling_rate']
    else:
        raise ValueError(f'{config_path}: expected config.yaml or config.json')
    config.setdefault('use_pitch_embed', False)       # absent from both config chains; the reference reads it unconditionally (hifigan.py:111)
    model = HifiGanGenerator(config)
    model.load_state_dict(state, strict=True)
    model = model.eval().to(device)
    model.remove_weight_norm()
    print(f'| Loaded model parameters from {checkpoint_path}.')
    return model, config, device


class _WavdenHandle:
    """One bsg_wavden handle: the transform bases of one (fft_size, hop_size, win_size) on one device."""

    def __init__(self, key, device):
        self.h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.load().bsg_wavden_create(ctypes.byref(self.h), key[0], key[1], key[2], _lib.stream_ptr()), 'bsg_wavden_create')

    def __del__(self):
        if getattr(self, 'h', None) is not None and self.h.value:
            try:
                _lib.load().bsg_wavden_destroy(self.h)
            except Exception:      # interpreter shutdown: the library or the runtime may be gone already
                pass
            self.h = None


_wavden_handles = {}      # (fft_size, hop_size, win_size, device index) -> _WavdenHandle; created on first use, never without a call to denoise()


def denoise(wav, v=0, lengths=None):
    """vocoders/vocoder_utils.py:7-15 with the reference's signature: numpy [L] in -> numpy [hop * (L // hop)] out, reading
    hparams['fft_size'], ['hop_size'], ['win_size'] as the reference does.  Extension: a device tensor [L] or [B, L] (``lengths``: samples per
    row, default L; a row is filtered as if it were alone at its length) returns a device tensor of the same shape, zero beyond
    hop * (lengths[b] // hop).  One launch of csrc/wavden.hip either way."""
    missing = [k for k in ('fft_size', 'hop_size', 'win_size') if hparams.get(k) is None]
    if missing:
        raise KeyError(f'denoise (vocoder_denoise_c) needs hparams {missing}: the config chain does not set them '
                       f'(the BiSinger chains use fft_size 512, hop_size 128, win_size 512)')
    key = (int(hparams['fft_size']), int(hparams['hop_size']), int(hparams['win_size']))
    as_numpy = not isinstance(wav, torch.Tensor)
    if as_numpy:
        assert lengths is None and np.ndim(wav) == 1, 'denoise: a numpy waveform is one row [L]'
        x = torch.as_tensor(np.ascontiguousarray(wav, dtype=np.float32)).cuda()
    else:
        assert wav.is_cuda and wav.dim() in (1, 2), 'denoise: expected a device tensor [L] or [B, L]'
        x = wav.detach().to(torch.float32).contiguous()
    x2 = x.view(1, -1) if x.dim() == 1 else x
    B, stride = x2.shape
    n = None
    if lengths is not None:
        lens = [int(l) for l in (lengths.tolist() if hasattr(lengths, 'tolist') else lengths)]
        assert len(lens) == B, f'denoise: {len(lens)} lengths for {B} rows'
        n = (ctypes.c_int32 * B)(*lens)
    hk = key + (x2.device.index,)
    if hk not in _wavden_handles:
        _wavden_handles[hk] = _WavdenHandle(key, x2.device)
    out = torch.empty_like(x2)
    with torch.cuda.device(x2.device):
        _lib.check(_lib.load().bsg_wavden_forward(_wavden_handles[hk].h, _lib.ptr(x2), _lib.ptr(out), n, B, stride, float(v), _lib.stream_ptr()),
                   'bsg_wavden_forward')
    if as_numpy:
        return out[0, :key[1] * (stride // key[1])].cpu().numpy()
    return out.view(x.shape)


@register_vocoder
class HifiGAN(BaseVocoder):
    def __init__(self, device=None):
        base_dir = hparams['vocoder_ckpt']
        config_path = f'{base_dir}/config.yaml'
        if os.path.exists(config_path):                                   # vocoders/hifigan.py:41-47
            ckpt = latest_ckpt(base_dir)
            assert ckpt, f'no model_ckpt_steps_*.ckpt under {base_dir}'
            print('| load HifiGAN: ', ckpt)
        else:                                                             # :48-52: the original release's files
            config_path, ckpt = f'{base_dir}/config.json', f'{base_dir}/generator_v1'
            assert os.path.exists(config_path) and os.path.exists(ckpt), f'no HiFi-GAN checkpoint under {base_dir}'
            print('| load HifiGAN: ', ckpt)
        self.model, self.config, self.device = load_model(config_path, ckpt, device)

    def spec2wav(self, mel, **kwargs):
        with torch.no_grad():
            c = torch.as_tensor(np.asarray(mel), dtype=torch.float32).unsqueeze(0).transpose(2, 1).to(self.device)
            f0 = kwargs.get('f0')
            if f0 is not None and hparams.get('use_nsf'):          # vocoders/hifigan.py:60-63
                f0 = torch.as_tensor(np.asarray(f0), dtype=torch.float32)[None, :].to(self.device)
                y = self.model(c, f0, seed=int(kwargs.get('seed', hparams.get('seed', 1234)))).view(-1)
            else:
                y = self.model(c).view(-1)
        if hparams.get('vocoder_denoise_c', 0.0) > 0:                  # vocoders/hifigan.py:66-69, on the device tensor
            y = denoise(y, v=hparams['vocoder_denoise_c'])
        return y.cpu().numpy()


def f0_to_coarse(f0):
    """utils/pitch_utils.py:15-31 on the host (numpy): f0 in Hz -> one of 255 mel-spaced bins 1 .. 255 (1: unvoiced or below 50 Hz)."""
    f0_bin, f0_min, f0_max = 256, 50.0, 1100.0
    mel_min, mel_max = 1127 * np.log(1 + f0_min / 700), 1127 * np.log(1 + f0_max / 700)
    f0_mel = 1127 * np.log(1 + np.asarray(f0, np.float64) / 700)
    f0_mel = np.where(f0_mel > 0, (f0_mel - mel_min) * (f0_bin - 2) / (mel_max - mel_min) + 1, f0_mel)
    return np.rint(np.clip(f0_mel, 1, f0_bin - 1)).astype(np.int64)


class _Scaler:
    """sklearn's StandardScaler.transform for given statistics, in numpy: (x - mean) / scale."""

    def __init__(self, mean, scale):
        self.mean_, self.scale_ = np.asarray(mean, np.float64), np.asarray(scale, np.float64)

    def transform(self, x):
        return ((np.asarray(x, np.float64) - self.mean_) / self.scale_).astype(np.float32)


def _read_hdf5(path, name):
    try:
        import h5py
    except ImportError as e:
        raise RuntimeError(f'{path}: hdf5 statistics (config format "hdf5") need h5py, which is not installed; convert them to npy '
                           f'([mean, scale]) and set format: "npy"') from e
    with h5py.File(path, 'r') as f:
        return f[name][()]


def load_pwg_model(config_path, checkpoint_path, stats_path, device=None):
    """vocoders/pwg.py:18-52: config.yaml['generator_params'] + either the official release's checkpoint (['model']['generator'], strict,
    with mean / scale statistics in hdf5 or npy) or a trainer checkpoint (['state_dict'] keys model_gen.*, not strict, no scaler);
    then the fold.  -> (model, scaler or None, config, device)."""
    import yaml
    from .pwg import ParallelWaveGANGenerator
    with open(config_path) as f:
        config = yaml.safe_load(f)
    device = device or torch.device('cuda')
    model = ParallelWaveGANGenerator(**config['generator_params'])
    ckpt_dict = torch.load(checkpoint_path, map_location='cpu')
    if 'state_dict' not in ckpt_dict:      # official vocoder
        model.load_state_dict(ckpt_dict['model']['generator'])
        fmt = 'npy' if str(stats_path).endswith('.npy') else config['format']      # the reader follows the file that is there
        if fmt == 'hdf5':
            scaler = _Scaler(_read_hdf5(stats_path, 'mean'), _read_hdf5(stats_path, 'scale'))
        elif fmt == 'npy':
            st = np.load(stats_path)
            scaler = _Scaler(st[0], st[1])
        else:
            raise ValueError('support only hdf5 or npy format.')
    else:                                  # custom PWG vocoder: the trainer's state dict holds the generator under model_gen.
        sd = {k[len('model_gen.'):]: v for k, v in ckpt_dict['state_dict'].items() if k.startswith('model_gen.')}
        model.load_state_dict(sd, strict=False)
        scaler = None
    model = model.eval().to(device)
    model.remove_weight_norm()
    print(f'| Loaded model parameters from {checkpoint_path}.')
    print(f'| PWG device: {device}.')
    return model, scaler, config, device


@register_vocoder
class PWG(BaseVocoder):
    def __init__(self, device=None):
        import glob
        import re
        if hparams['vocoder_ckpt'] == '':      # vocoders/pwg.py:58-69: the pretrained LJSpeech release
            base_dir = 'wavegan_pretrained'
            ckpts = glob.glob(f'{base_dir}/checkpoint-*steps.pkl')
            assert ckpts, f'no checkpoint-*steps.pkl under {base_dir}'
            ckpt = sorted(ckpts, key=lambda x: int(re.findall(r'checkpoint-(\d+)steps\.pkl$', x)[0]))[-1]
            print('| load PWG: ', ckpt)
            stats = f'{base_dir}/stats.h5'
            if not os.path.exists(stats) and os.path.exists(f'{base_dir}/stats.npy'):      # the npy form of the same statistics
                stats = f'{base_dir}/stats.npy'
            self.model, self.scaler, self.config, self.device = load_pwg_model(f'{base_dir}/config.yaml', ckpt, stats, device)
        else:                                  # :70-82: a trained checkpoint directory; its scaler is not used
            base_dir = hparams['vocoder_ckpt']
            print(base_dir)
            ckpt = latest_ckpt(base_dir)
            assert ckpt, f'no model_ckpt_steps_*.ckpt under {base_dir}'
            print('| load PWG: ', ckpt)
            self.scaler = None
            self.model, _, self.config, self.device = load_pwg_model(f'{base_dir}/config.yaml', ckpt, f'{base_dir}/stats.h5', device)

    def spec2wav(self, mel, **kwargs):
        """vocoders/pwg.py:84-105: mel [T,80] (, f0 [T]) -> wav [T*hop].  ``z`` [T*hop]: the noise, supplied; otherwise it is drawn on the
        device from the Philox stream of ``seed`` (default hparams['seed'])."""
        config = self.config
        w = config['generator_params']['aux_context_window']
        c = np.asarray(mel)
        if self.scaler is not None:
            c = self.scaler.transform(c)
        with torch.no_grad():
            T = c.shape[0]
            c = np.pad(c, ((w, w), (0, 0)), 'edge')
            c = torch.as_tensor(c, dtype=torch.float32).unsqueeze(0).transpose(2, 1).contiguous().to(self.device)
            p = kwargs.get('f0')
            if p is not None:
                p = f0_to_coarse(np.asarray(p))
                p = torch.as_tensor(np.pad(np.asarray(p), ((w, w),), 'edge')[None, :], dtype=torch.int64).to(self.device)
            z = kwargs.get('z')
            if z is not None:
                z = torch.as_tensor(np.asarray(z), dtype=torch.float32).view(1, 1, T * config['hop_size']).to(self.device)
            seed = kwargs.get('seed')
            y = self.model(z, c, p, seed=int(hparams.get('seed', 1234) if seed is None else seed)).view(-1)
        return y.cpu().numpy()

    def spec2wav_batch(self, mels, f0s=None, zs=None, seed=None, seeds=None):
        """Many utterances in ONE ragged forward: mels a list of [T_i,80] (, f0s a list of [T_i], zs a list of [T_i*hop]) -> a list of
        wav [T_i*hop] in the order given.  Per item: the scaler transform and ``f0_to_coarse``, as ``spec2wav`` does them; then the items
        are padded to the longest, run through ``forward_ragged`` (which edge-pads every item at its own end) and trimmed.  With ``zs``
        item i equals ``spec2wav(mels[i], f0=f0s[i], z=zs[i])`` bit for bit.  Without, the noise is drawn on the device from the Philox
        stream of ``seed`` (default hparams['seed']) at the index of the padded batch: reproducible, but item i is then NOT the waveform
        ``spec2wav(mels[i], seed=seed)`` draws.  ``seeds`` (one int per item; not with ``zs``) is the way out: item i draws the Philox
        stream of seeds[i] at its own length (``forward_ragged(row_seeds=)``) and equals ``spec2wav(mels[i], f0=f0s[i], seed=seeds[i])``
        bit for bit, whatever it is batched with."""
        if seeds is not None:
            seeds = _lib.row_seeds_list(seeds, len(mels), 'PWG.spec2wav_batch', {'zs': zs})
        hop = self.config['hop_size']
        cs = [np.asarray(m) for m in mels]
        if self.scaler is not None:
            cs = [self.scaler.transform(c) for c in cs]
        B = len(cs)
        assert B >= 1, 'spec2wav_batch: no items'
        lengths = [int(c.shape[0]) for c in cs]
        T = max(lengths)
        for name, seq in (('f0s', f0s), ('zs', zs)):
            assert seq is None or len(seq) == B, f'spec2wav_batch: {len(seq)} {name} for {B} mels'
        mel = np.zeros((B, cs[0].shape[1], T), dtype=np.float32)
        for b, c in enumerate(cs):
            mel[b, :, :lengths[b]] = np.asarray(c, dtype=np.float32).T
        pitch = z = None
        if f0s is not None:
            pitch = np.zeros((B, T), dtype=np.int64)
            for b, f0 in enumerate(f0s):
                pitch[b, :lengths[b]] = f0_to_coarse(np.asarray(f0))
            pitch = torch.from_numpy(pitch).to(self.device)
        if zs is not None:
            z = np.zeros((B, 1, T * hop), dtype=np.float32)
            for b, zi in enumerate(zs):
                z[b, 0, :lengths[b] * hop] = np.asarray(zi, dtype=np.float32).reshape(lengths[b] * hop)
            z = torch.from_numpy(z).to(self.device)
        with torch.no_grad():
            y = self.model.forward_ragged(z, torch.from_numpy(mel).to(self.device), pitch, lengths=lengths,
                                          seed=int(hparams.get('seed', 1234) if seed is None else seed), row_seeds=seeds)
        y = y.cpu().numpy()
        return [y[b, 0, :lengths[b] * hop].copy() for b in range(B)]

    @staticmethod
    def wav2mfcc(wav_fn):
        raise NotImplementedError('analysis (wav -> mfcc) is data preparation, outside the hot path')
