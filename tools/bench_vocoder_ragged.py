#!/usr/bin/env python3
"""HiFi-GAN generator (plain), padded against ragged batches: ms per forward and real samples/s.

Request lists: the first 16 and all 64 of RandomState(0).randint(250, 1001, 64) (the request list of DESIGN section 4), in buckets of 16 in
the order given (a bucket is one forward at T = its longest row).  Per list and mode: 10 warm-up passes over the buckets, then 5 windows;
the figure is the median window.  `early_exit` is the share of workgroups of a ragged forward whose first output lies beyond their row's
end, counted on the host from last_path and the grids of csrc/hifigan.hip; the three GEMM-form launches (pre:h2w, up0:h2w, up1:h2w) keep
their empty tiles and are counted as never leaving.

    python tools/bench_vocoder_ragged.py [--windows 5] [--passes 10]      -> one JSON line
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HOP = 256


def cdiv(a, b):
    return -(-a // b)


def workgroups(path, cfg, B, T, lens):
    """(all workgroups, those that leave early) of one ragged forward, from its launch record."""
    rates, ks, dils = cfg['upsample_rates'], cfg['resblock_kernel_sizes'], cfg['resblock_dilation_sizes']
    C0 = cfg['upsample_initial_channel']
    total = early = 0

    def tiles(nt, first_out, bound_mul, per_row=1):
        """nt tiles per row (x per_row workgroups each); tile x leaves if first_out(x) >= lens[b] * bound_mul."""
        nonlocal total, early
        for n in lens:
            total += nt * per_row
            early += sum(1 for x in range(nt) if first_out(x) >= n * bound_mul) * per_row

    for tok in path.split():
        if tok == 'ragged':
            continue
        site, form = tok.split(':')
        var = int(form.split('/')[1][2:]) if '/' in form else 0
        form = form.split('/')[0]
        if site == 'pre':
            i, mul = -1, 1
        elif site == 'post':
            i, mul = len(rates), HOP
        else:
            i = int(site[2]) if site[:2] in ('up', 'rb') else int(site[3])
            mul = int(np.prod(rates[:i + (0 if site.startswith('up') else 1)]))      # of the tensor the launch reads (up) / works on (rb, src)
        L = T * mul
        if form == 'h2w':      # the product kernels keep their empty tiles
            rows, wn = (L, C0) if site == 'pre' else (L + 1, (C0 >> (i + 1)) * 8)
            bm = 128 if cdiv(rows, 128) * (wn // 128) * B >= 512 else 64
            total += cdiv(rows, bm) * (wn // 128) * B
        elif form in ('pair_h2', 'pair_h16', 'pair_mfma'):
            pout = 128 * var - (ks[int(site.split('.')[1])] - 1)
            tiles(cdiv(L, pout), lambda x: x * pout, mul)
        elif form == 'chain':
            j = int(site.split('.')[1])
            pout = 64 * var - 2 * sum((ks[j] - 1) // 2 * (d + 1) for d in dils[j])
            tiles(cdiv(L, pout), lambda x: x * pout, mul)
        elif form == 'up2':
            tiles(cdiv(2 * L, 1024), lambda x: 1024 * x, 2 * mul)
        elif form == 'upk':
            tiles(cdiv(L + 1, 256), lambda x: 256 * x - 1, mul, cdiv(C0 >> (i + 1), 8))      # (leaves if 256 x > bound)
        elif form == 'poly':
            co = C0 >> (i + 1)
            tiles(cdiv(L + 1, 256 * var), lambda x: 256 * var * x - 1, mul, cdiv(co, 16 if co >= 16 else 8) * rates[i])
        elif form == 'post4':
            tiles(cdiv(L, 1024), lambda x: 1024 * x, mul)      # (stores zeros and leaves)
        else:
            raise SystemExit(f'bench_vocoder_ragged: launch form {tok!r} is not counted here')
    return total, early


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--passes', type=int, default=10, help='warm-up passes, and passes per window')
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device('cuda', 0)
    voc, cfg = bench.build_vocoder(dev)
    all_lens = [int(v) for v in np.random.RandomState(0).randint(250, 1001, 64)]
    out = {}
    for name, lens in (('first16', all_lens[:16]), ('all64', all_lens)):
        buckets = [lens[i:i + 16] for i in range(0, len(lens), 16)]
        mels = [torch.randn(len(b), 80, max(b), device=dev) * 1.5 - 3.0 for b in buckets]
        real = sum(lens) * HOP
        rec = {'rows': len(lens), 'real_frames': sum(lens), 'padded_frames': sum(len(b) * max(b) for b in buckets)}
        rec['waste'] = round(1 - rec['real_frames'] / rec['padded_frames'], 4)
        for mode in ('padded', 'ragged'):
            def one_pass():
                for m, b in zip(mels, buckets):
                    voc(m, lengths=b) if mode == 'ragged' else voc(m)
            for _ in range(a.passes):
                one_pass()
            torch.cuda.synchronize()
            wins = []
            for _ in range(a.windows):
                t0 = time.perf_counter()
                for _ in range(a.passes):
                    one_pass()
                torch.cuda.synchronize()
                wins.append((time.perf_counter() - t0) / a.passes)
            dt = float(np.median(wins))
            rec[mode] = {'ms_per_forward': round(dt / len(buckets) * 1e3, 4), 'ms_per_list': round(dt * 1e3, 4),
                         'real_samples_per_s': round(real / dt), 'windows_ms': [round(w * 1e3, 4) for w in wins]}
        tot = ear = 0
        for m, b in zip(mels, buckets):
            voc(m, lengths=b)
            t, e = workgroups(voc.last_path(), cfg, len(b), max(b), b)
            tot, ear = tot + t, ear + e
        rec['workgroups'], rec['early_exit'] = tot, round(ear / tot, 4)
        rec['speedup'] = round(rec['padded']['ms_per_list'] / rec['ragged']['ms_per_list'], 4)
        out[name] = rec
    print(json.dumps(out))


if __name__ == '__main__':
    main()
