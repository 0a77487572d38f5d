"""The spectral post-filter hparams['vocoder_denoise_c'] restated in numpy (vocoders/vocoder_utils.py:7-15: librosa.stft -> |S| - v clipped at 0,
phase kept -> librosa.istft, with librosa's defaults: center=True, pad_mode='constant', window='hann' = periodic Hann of win points,
zero-padded symmetrically to n_fft; istft divides the overlap-added frames by the overlap-added squared window wherever that exceeds the
smallest normal number and drops n_fft / 2 samples at both ends).

`dtype` is the precision every step is evaluated in: float64 is the reference of the tests, float32 measures what fp32 arithmetic alone
costs (numpy's FFT works in the precision of its input).  librosa is not installed where these tests run, so nothing here was held
against the reference's own run; tests/test_wavden_cpu.py pins it against torch.stft / torch.istft instead."""
import numpy as np


def window(n_fft, win, dtype=np.float64):
    w = np.zeros(n_fft, dtype=np.float64)
    lp = (n_fft - win) // 2
    w[lp:lp + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    return w.astype(dtype)


def denoise(wav, v, n_fft, hop, win, dtype=np.float64):
    """wav [L] -> [hop * (L // hop)], every step in `dtype`."""
    y = np.asarray(wav).astype(dtype)
    L = len(y)
    T = L // hop
    w = window(n_fft, win, dtype)
    ypad = np.concatenate([np.zeros(n_fft // 2, dtype), y, np.zeros(n_fft // 2, dtype)])
    idx = hop * np.arange(T + 1)[:, None] + np.arange(n_fft)[None, :]
    S = np.fft.rfft(ypad[idx] * w, axis=-1)                                    # [T + 1, n_fft / 2 + 1]
    assert S.dtype == (np.complex64 if dtype == np.float32 else np.complex128)
    mag = np.abs(S)
    gain = np.where(mag > 0, np.maximum(mag - dtype(v), 0) / np.where(mag > 0, mag, 1), 0).astype(dtype)
    frames = np.fft.irfft(S * gain, n=n_fft, axis=-1).astype(dtype) * w
    acc = np.zeros(hop * T + n_fft, dtype)
    env = np.zeros(hop * T + n_fft, dtype)
    for i in range(T + 1):                                                     # overlap-add, earliest frame first
        acc[i * hop:i * hop + n_fft] += frames[i]
        env[i * hop:i * hop + n_fft] += w * w
    ok = env > np.finfo(dtype).tiny
    acc[ok] /= env[ok]
    return acc[n_fft // 2:n_fft // 2 + hop * T]


def make_wave(n, amp=1.0, seed=0):
    """Two harmonics (0.3, 0.1) and 0.01 N(0, 1) noise: max |y| ~ 0.36 amp.  v = 0.1 zeroes a third of the bins, v = 0.5 nine in ten."""
    rs = np.random.RandomState(seed)
    t = np.arange(n)
    y = 0.3 * np.sin(2 * np.pi * 220.0 / 24000.0 * t) + 0.1 * np.sin(2 * np.pi * 440.0 / 24000.0 * t + 0.5) + 0.01 * rs.randn(n)
    return (amp * y).astype(np.float32)
