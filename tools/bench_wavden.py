#!/usr/bin/env python3
"""The vocoder_denoise_c post-filter alone (csrc/wavden.hip), (fft_size, hop_size, win_size) = (512, 128, 512), at B = 1 and B = 16 rows of
1000 STFT frames (128 000 samples) and of the length the vocoder produces for 1000 mel frames; beside it, in the same process: the
HiFi-GAN forward it follows, and the reference's route restated with torch (wave to the host, torch.stft / istft at the fastest thread
count <= 16, back to the device).  HIP events on the launch's stream; 1 warm-up, then 5 windows of REPS launches: median and spread.
One JSON line.  Bytes are the algorithm's (2 x 4 B per sample) and the kernel's by construction (every sample is read 35 / 29 times — 3 halo
hops per run of 29 — and written once; the 2 MB of bases stay in L2): counters were not collected here."""
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from bisinger_amd import _lib  # noqa: E402

REPS, WINDOWS = 200, 5
N_FFT, HOP, WIN, V = 512, 128, 512, 0.1
torch.set_grad_enabled(False)
assert torch.cuda.is_available(), 'bench_wavden needs a GPU: there is no CPU path to time'
dev = torch.device('cuda', 0)
lib = _lib.load()
h = ctypes.c_void_p()
_lib.check(lib.bsg_wavden_create(ctypes.byref(h), N_FFT, HOP, WIN, _lib.stream_ptr()), 'bsg_wavden_create')


def events_ms(fn, reps=REPS, windows=WINDOWS):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return {'ms': round(statistics.median(ms), 4), 'min': round(min(ms), 4), 'max': round(max(ms), 4)}


def wave(B, L):
    t = torch.arange(L, device=dev, dtype=torch.float32)
    g = torch.Generator(device=dev).manual_seed(0)
    return (0.3 * torch.sin(2 * torch.pi * 220.0 / 24000.0 * t) + 0.1 * torch.sin(2 * torch.pi * 440.0 / 24000.0 * t + 0.5))[None, :] + \
        0.01 * torch.randn(B, L, device=dev, generator=g)


def filter_ms(B, L):
    x, out = wave(B, L).contiguous(), torch.empty(B, L, device=dev)
    r = events_ms(lambda: _lib.check(lib.bsg_wavden_forward(h, _lib.ptr(x), _lib.ptr(out), None, B, L, V, _lib.stream_ptr()), 'bsg_wavden_forward'))
    frames = B * (L // HOP + 1)
    flop = frames * 4.0 * N_FFT * N_FFT                     # two N x N real products per frame
    runs = B * -(-L // (29 * HOP))
    r.update(tflops=round(flop / (r['ms'] * 1e-3) / 1e12, 2), tflops_issued=round(runs * 32 * 4.0 * N_FFT * N_FFT / (r['ms'] * 1e-3) / 1e12, 2),
             bytes_algorithmic=8 * B * L, bytes_kernel=int(B * L * 4 * (35 / 29 + 1)),
             gbps_algorithmic=round(8 * B * L / (r['ms'] * 1e-3) / 1e9, 1), finite=bool(torch.isfinite(out).all()))
    return r


def host_route_ms(B, L):
    """vocoders/hifigan.py:66-69 as the reference runs it, with torch in librosa's place: every row to the host, filtered there, back."""
    x = wave(B, L)
    w = torch.hann_window(WIN, periodic=True)

    def once():
        rows = []
        for b in range(B):
            y = x[b].cpu()
            S = torch.stft(y, N_FFT, hop_length=HOP, win_length=WIN, window=w, center=True, pad_mode='constant', return_complex=True)
            m = S.abs()
            S = S * ((m - V).clamp(min=0) / m.clamp(min=1e-30))
            rows.append(torch.istft(S, N_FFT, hop_length=HOP, win_length=WIN, window=w, center=True))
        out = torch.stack(rows).to(dev)
        torch.cuda.synchronize()
        return out

    best = None
    for nt in (1, 2, 4, 8, 16):
        torch.set_num_threads(nt)
        once()
        t0 = time.perf_counter()
        for _ in range(5):
            once()
        ms = (time.perf_counter() - t0) / 5 * 1e3
        if best is None or ms < best[0]:
            best = (ms, nt)
    return {'ms': round(best[0], 3), 'threads': best[1]}


voc, cfg = bench.build_vocoder(dev)
voc_hop = 1
for u in cfg['upsample_rates']:
    voc_hop *= u
res = {'params': [N_FFT, HOP, WIN], 'v': V, 'reps': REPS, 'windows': WINDOWS, 'vocoder_hop': voc_hop}
for B in (1, 16):
    mel = torch.randn(B, 80, 1000, device=dev)
    res[f'B{B}'] = {'filter_1000_stft_frames': filter_ms(B, 1000 * HOP), 'filter_vocoder_length': filter_ms(B, 1000 * voc_hop),
                    'vocoder_forward_1000_mel_frames': events_ms(lambda: voc(mel), reps=20),
                    'host_route_vocoder_length': host_route_ms(B, 1000 * voc_hop)}
torch.cuda.synchronize()
lib.bsg_wavden_destroy(h)
print(json.dumps(res))
