#!/usr/bin/env python3
"""Pitch extractor, padded against ragged: ms per forward at B = 16, T = 1000.

The model is the extractor of the parity tests (tests/pe_cases.pitch_extractor: formula weights of seed 11), the lengths are those of
tests/test_gpu_f2_fullsize.py test_pitch_extractor_fullsize_vs_fp64 (row 0 at T, the others RandomState(21).randint(120, 1000) sorted
downwards), the mel is exactly 0 beyond each row's end in both modes.  Per mode: `passes` warm-up forwards, then `windows` windows of
`passes` forwards; the figure is the median window.  `--pipe fp32` times the fp32 matrix pipe instead of the split-fp16 GEMMs.
`early_exit` is the share of GEMM workgroups (64- or 128-row tiles, by the form the dispatch takes at this size) of a ragged forward whose
first row lies beyond their row's end, counted on the host.

    python tools/bench_pe_ragged.py [--windows 5] [--passes 20] [--pipe split|fp32]      -> one JSON line
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
from bisinger_amd import _lib  # noqa: E402
from tests import pe_cases  # noqa: E402

B, T = 16, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--passes', type=int, default=20, help='warm-up forwards, and forwards per window')
    ap.add_argument('--pipe', choices=['split', 'fp32'], default='split')
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    with open(os.path.join(ROOT, 'tests', 'golden', 'state_dict_spec.json')) as f:
        pe = pe_cases.pitch_extractor(json.load(f)).cuda()
    pe.set_gemm_split(a.pipe == 'split')
    rs = np.random.RandomState(5 + B)
    lens = [T] + sorted(rs.randint(120, T, size=B - 1).tolist(), reverse=True)
    mel = torch.from_numpy(pe_cases.mel(rs, B, T, lens)).cuda()
    out = {'B': B, 'T': T, 'pipe': a.pipe, 'lengths': lens, 'real_frames': sum(lens), 'padded_frames': B * T,
           'waste': round(1 - sum(lens) / (B * T), 4)}
    for mode in ('padded', 'ragged'):
        kw = {'lengths': lens} if mode == 'ragged' else {}
        for _ in range(a.passes):
            pe(mel, **kw)
        torch.cuda.synchronize()
        wins = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            for _ in range(a.passes):
                pe(mel, **kw)
            torch.cuda.synchronize()
            wins.append((time.perf_counter() - t0) / a.passes)
        out[mode] = {'ms_per_forward': round(float(np.median(wins)) * 1e3, 4), 'windows_ms': [round(w * 1e3, 4) for w in wins]}
    # the products' tiles: 2 column tiles x ceil(T / BM) row tiles x B; BM = 128 from 3 x 256 (split-fp16) / 2 x 256 (fp32) such workgroups on
    bm = 128 if 2 * -(-T // 128) * B >= (768 if a.pipe == 'split' else 512) else 64
    tiles = -(-T // bm)
    out['gemm_tile_rows'] = bm
    out['early_exit'] = round(sum(tiles - -(-n // bm) for n in lens) / (tiles * B), 4)
    out['speedup'] = round(out['padded']['ms_per_forward'] / out['ragged']['ms_per_forward'], 4)
    out['range_retries'] = _lib.range_retries
    print(json.dumps(out))


if __name__ == '__main__':
    main()
