#!/usr/bin/env python3
"""Parallel WaveGAN generator (plain form, formula weights), padded against ragged batches against one lone call per item: ms and real
samples/s.

Request lists: the first 16 and all 64 of RandomState(0).randint(250, 1001, 64) (the request list of DESIGN section 4), in buckets of 16 in
the order given.  Per list three modes:
    padded  one `forward` per bucket at T = its longest row (every row edge-padded at the RECTANGLE's end: what a caller without the ragged
            entry can batch; its short rows are not the utterances alone)
    ragged  one `forward_ragged` per bucket
    lone    one `forward` per item at its own length (the only correct form before the ragged entry)
Per list and mode: 10 warm-up passes over the list, then 5 windows of 10 passes; the figure is the median window.  `tiles` is
bsg_pwg_last_tiles summed over the buckets of a ragged pass, `padded_tiles` the same of a padded pass: what a residual-layer launch walks.
`full16x1000`: the padded call at B = 16, T = 1000 and the ragged call with all lengths = T on the same inputs (they differ by the tile
lookup only).

    python tools/bench_pwg_ragged.py [--windows 5] [--passes 10] [--out FILE]      -> one JSON line
"""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bisinger_amd import synth  # noqa: E402
from bisinger_amd.pwg import ParallelWaveGANGenerator  # noqa: E402

HOP, W = 256, 2


def build_generator(dev):
    spec = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'pwg_state_dict_spec.json')))
    w = synth.synth_state_dict(OrderedDict((k, tuple(s)) for k, s in spec['plain_weight_norm']), 21)
    gen = ParallelWaveGANGenerator(**json.loads(json.dumps(spec['generator_params'])))
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    gen = gen.eval().to(dev)
    gen.remove_weight_norm()
    return gen


def edge(mel):
    return torch.nn.functional.pad(mel, (W, W), mode='replicate').contiguous()


def timed(one_pass, passes, windows):
    for _ in range(passes):
        one_pass()
    torch.cuda.synchronize()
    wins = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(passes):
            one_pass()
        torch.cuda.synchronize()
        wins.append((time.perf_counter() - t0) / passes)
    return float(np.median(wins)), wins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--passes', type=int, default=10, help='warm-up passes, and passes per window')
    ap.add_argument('--out', default=None, help='also write the line to this file')
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    assert torch.cuda.is_available(), 'bench_pwg_ragged needs a GPU: there is no CPU path to time'
    dev = torch.device('cuda', 0)
    gen = build_generator(dev)
    all_lens = [int(v) for v in np.random.RandomState(0).randint(250, 1001, 64)]
    out = {'device': torch.cuda.get_device_name(0), 'windows': a.windows, 'passes': a.passes}
    for name, lens in (('first16', all_lens[:16]), ('all64', all_lens)):
        buckets = [lens[i:i + 16] for i in range(0, len(lens), 16)]
        mels = [torch.randn(len(b), 80, max(b), device=dev) * 1.5 - 3.0 for b in buckets]
        zs = [torch.randn(len(b), 1, max(b) * HOP, device=dev) for b in buckets]
        padded_c = [edge(m) for m in mels]
        lone = [(z[i:i + 1, :, :n * HOP].contiguous(), edge(m[i:i + 1, :, :n])) for m, z, b in zip(mels, zs, buckets) for i, n in enumerate(b)]
        real = sum(lens) * HOP
        rec = {'rows': len(lens), 'real_frames': sum(lens), 'padded_frames': sum(len(b) * max(b) for b in buckets)}
        rec['waste'] = round(1 - rec['real_frames'] / rec['padded_frames'], 4)
        tiles = {'padded': 0, 'ragged': 0}

        def run(mode, count=False):
            if mode == 'lone':
                for z, c in lone:
                    gen(z, c)
                return
            for m, c, z, b in zip(mels, padded_c, zs, buckets):
                gen.forward_ragged(z, m, lengths=b) if mode == 'ragged' else gen(z, c)
                if count:
                    tiles[mode] += gen.last_tiles()

        for mode in ('padded', 'ragged', 'lone'):
            dt, wins = timed(lambda: run(mode), a.passes, a.windows)
            calls = len(lone) if mode == 'lone' else len(buckets)
            rec[mode] = {'ms_per_forward': round(dt / calls * 1e3, 4), 'ms_per_list': round(dt * 1e3, 4),
                         'real_samples_per_s': round(real / dt), 'windows_ms': [round(w * 1e3, 4) for w in wins]}
            print(f'{name} {mode}: {dt * 1e3:.2f} ms per list', file=sys.stderr, flush=True)
        run('padded', count=True)
        run('ragged', count=True)
        rec['tiles'], rec['padded_tiles'] = tiles['ragged'], tiles['padded']
        rec['tile_share'] = round(tiles['ragged'] / tiles['padded'], 4)
        rec['ragged_over_padded'] = round(rec['ragged']['ms_per_list'] / rec['padded']['ms_per_list'], 4)
        rec['ragged_over_lone'] = round(rec['ragged']['ms_per_list'] / rec['lone']['ms_per_list'], 4)
        out[name] = rec
        del mels, zs, padded_c, lone
    # the padded call at B = 16, T = 1000 against the ragged call with all lengths = T
    B, T = 16, 1000
    mel = torch.randn(B, 80, T, device=dev) * 1.5 - 3.0
    z, c = torch.randn(B, 1, T * HOP, device=dev), edge(mel)
    full = {}
    for mode, fn in (('padded', lambda: gen(z, c)), ('ragged_all_T', lambda: gen.forward_ragged(z, mel, lengths=[T] * B)),
                     ('padded_again', lambda: gen(z, c))):
        dt, wins = timed(fn, a.passes, a.windows)
        full[mode] = {'ms': round(dt * 1e3, 4), 'windows_ms': [round(w * 1e3, 4) for w in wins]}
        print(f'full16x1000 {mode}: {dt * 1e3:.2f} ms', file=sys.stderr, flush=True)
    full['ragged_over_padded'] = round(full['ragged_all_T']['ms'] / full['padded']['ms'], 4)
    out['full16x1000'] = full
    torch.cuda.synchronize()
    gen.release()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
