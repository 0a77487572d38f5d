"""CPU: the vocoder_denoise_c post-filter — its float64 restatement (tests/wavden_ref.py) against an independent implementation, and the
parts of the bsg_wavden_* surface that need no GPU."""
import ctypes
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch

from bisinger_amd import _lib
from tests import wavden_ref as ref

TRIPLES = [(512, 128, 512), (1024, 256, 1024), (1024, 256, 800)]      # (fft_size, hop_size, win_size): BiSinger chains, configs/tts, win < n_fft


def _torch_denoise(y, v, n_fft, hop, win):
    """The same filter through torch.stft / torch.istft (fp32, CPU): a second opinion on framing, padding, window and normalisation."""
    y = torch.from_numpy(np.asarray(y, dtype=np.float32))
    w = torch.hann_window(win, periodic=True)
    S = torch.stft(y, n_fft, hop_length=hop, win_length=win, window=w, center=True, pad_mode='constant', return_complex=True)
    mag = S.abs()
    S = S * torch.where(mag > 0, (mag - v).clamp(min=0) / mag.clamp(min=1e-30), torch.zeros(()))
    return torch.istft(S, n_fft, hop_length=hop, win_length=win, window=w, center=True).numpy()


@pytest.mark.parametrize('n_fft,hop,win', TRIPLES)
@pytest.mark.parametrize('T', [1, 3, 1000])
def test_restatement_against_torch_stft(n_fft, hop, win, T):
    """<= 1e-6 max-abs (1.2e-7 .. 1.4e-7 measured: fp32 rounding of the second opinion).  A sanity rail on the REFERENCE of the GPU tests,
    not on the product."""
    y = ref.make_wave(T * hop)
    for v in (0.1, 0.5):
        want = ref.denoise(y, v, n_fft, hop, win)
        got = _torch_denoise(y, v, n_fft, hop, win)
        assert want.shape == got.shape == (T * hop,)
        err = float(np.abs(want - got).max())
        moved = float(np.abs(want - y).max())
        print(f'({n_fft}, {hop}, {win}) T={T} v={v}: restatement vs torch.stft/istft {err:.2e}; the filter moves samples by up to {moved:.3f}')
        assert err <= 1e-6
        assert moved > 1e-3          # the filter does something: a pass-through would be told apart by orders of magnitude


@pytest.mark.parametrize('n_fft,hop,win', TRIPLES)
def test_output_length_when_L_is_not_a_multiple_of_hop(n_fft, hop, win):
    L = 7 * hop + hop // 3
    y = ref.make_wave(L)
    want = ref.denoise(y, 0.1, n_fft, hop, win)
    assert want.shape == (hop * (L // hop),) == _torch_denoise(y, 0.1, n_fft, hop, win).shape
    assert float(np.abs(want - _torch_denoise(y, 0.1, n_fft, hop, win)).max()) <= 1e-6
    assert ref.denoise(y[:hop - 1], 0.1, n_fft, hop, win).shape == (0,)


@pytest.mark.parametrize('n_fft,hop,win', TRIPLES)
def test_v_zero_returns_the_input(n_fft, hop, win):
    """The window satisfies NOLA at hop = n_fft / 4: with v = 0 analysis and synthesis cancel."""
    y = ref.make_wave(40 * hop + 5).astype(np.float64)
    got = ref.denoise(y, 0.0, n_fft, hop, win)
    assert float(np.abs(got - y[:40 * hop]).max()) <= 1e-12


def test_abi_carries_the_filter_and_refuses_bad_arguments():
    """Fails without the feature: no such symbol.  Every refusal is BSG_EINVAL with a message, before any device call."""
    lib = _lib.load()
    assert lib.bsg_abi_version() >= 12
    for s in ('bsg_wavden_create', 'bsg_wavden_destroy', 'bsg_wavden_forward'):
        assert s in _lib.declared_symbols() and hasattr(lib, s)
    EINVAL = -22
    h = c_void_p()
    for bad in ((2048, 512, 2048), (512, 256, 512), (512, 128, 200), (512, 128, 513), (500, 125, 500), (0, 0, 0)):
        assert lib.bsg_wavden_create(byref(h), *bad, None) == EINVAL and h.value is None
        msg = lib.bsg_last_error().decode()
        assert str(bad[0]) in msg and '512 or 1024' in msg and 'n_fft / 4' in msg, msg      # names the value and the accepted set
    one = (ctypes.c_int32 * 1)(100)
    assert lib.bsg_wavden_forward(None, c_void_p(256), c_void_p(4096), one, 1, 100, -0.5, None) == EINVAL
    assert 'v=-0.5' in lib.bsg_last_error().decode()
    assert lib.bsg_wavden_forward(None, c_void_p(256), c_void_p(4096), one, 1, 100, float('nan'), None) == EINVAL
    assert lib.bsg_wavden_forward(None, c_void_p(256), c_void_p(4096), one, 0, 100, 0.1, None) == EINVAL
    assert 'B=0' in lib.bsg_last_error().decode()
    assert lib.bsg_wavden_forward(None, c_void_p(256), c_void_p(4096), one, 1, 0, 0.1, None) == EINVAL
    assert 'stride=0' in lib.bsg_last_error().decode()
    assert lib.bsg_wavden_forward(None, c_void_p(256), c_void_p(4096), one, 1, 99, 0.1, None) == EINVAL      # n[0] = 100 > stride
    assert 'n[0]=100' in lib.bsg_last_error().decode()
    assert lib.bsg_wavden_forward(None, c_void_p(256), c_void_p(4096), one, 1, 100, 0.1, None) == EINVAL      # arguments fine: no handle
    assert 'null' in lib.bsg_last_error().decode()
    lib.bsg_wavden_destroy(None)


def test_missing_hparams_are_named(monkeypatch):
    """A config chain without fft_size / win_size: a message naming the keys (the reference raises a bare KeyError)."""
    from bisinger_amd import vocoders
    from bisinger_amd.hparams import hparams
    monkeypatch.setitem(hparams, 'hop_size', 128)
    monkeypatch.delitem(hparams, 'fft_size', raising=False)
    monkeypatch.delitem(hparams, 'win_size', raising=False)
    with pytest.raises(KeyError) as e:
        vocoders.denoise(np.zeros(256, np.float32), 0.1)
    assert "['fft_size', 'win_size']" in str(e.value)


def test_shipped_config_resolves_the_three_keys():
    from tests.util import use_config
    hp = use_config()
    assert (hp['fft_size'], hp['hop_size'], hp['win_size']) == (512, 128, 512)


def test_filter_is_off_unless_asked_for(monkeypatch):
    """vocoder_denoise_c unset / denoise_c=None: spec2wav and forward_batch take the old path — denoise() is not called, no handle is made."""
    from bisinger_amd import infer, vocoders
    from bisinger_amd.hparams import hparams
    calls = []
    monkeypatch.setattr(vocoders, 'denoise', lambda *a, **k: calls.append((a, k)))
    monkeypatch.delitem(hparams, 'vocoder_denoise_c', raising=False)
    monkeypatch.setitem(hparams, 'use_nsf', False)

    class _Voc(vocoders.HifiGAN):
        def __init__(self):
            self.device = torch.device('cpu')
            self.model = lambda c: torch.arange(c.shape[-1] * 4, dtype=torch.float32).view(1, 1, -1)

    wav = _Voc().spec2wav(np.zeros((6, 80), np.float32))
    assert wav.shape == (24,) and not calls
    monkeypatch.setitem(hparams, 'vocoder_denoise_c', 0.0)
    _Voc().spec2wav(np.zeros((6, 80), np.float32))
    assert not calls

    class _Gen:                       # vocoder stand-in: [B, 80, T] -> [B, 1, 4 T]
        h = {'upsample_rates': [2, 2]}

        def __call__(self, mel):
            return torch.ones(mel.shape[0], 1, mel.shape[2] * 4)

    class _Infer(infer.DiffSingerE2EInfer):
        def __init__(self):
            self.vocoder = _Gen()
            self.device = torch.device('cpu')

        def collate(self, items):
            return items

        def _generate(self, sample, seed=None, ragged=False):
            return {'mel_out': torch.zeros(2, 5, 80), 'mel2ph': torch.tensor([[1, 1, 2, 2, 3], [1, 1, 1, 0, 0]])}

        def estimate_frames(self, item):
            return 5

    inf = _Infer()
    wavs = inf.forward_batch([{}, {}])
    assert [w.shape for w in wavs] == [(20,), (12,)] and not calls
    inf.forward_batch([{}, {}], denoise_c=0.0)
    assert not calls and not vocoders._wavden_handles
