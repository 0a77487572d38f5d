#!/usr/bin/env python3
"""The FastSpeech2-MIDI front, padded against ragged: ms per forward (encode + decode, mel2ph given) at B = 16, T_txt = 100, T = 1000.

The model is the front of the parity tests (tests/fs2_pitch_ref.build('midi', pitch=False): formula weights of seed 0, the configuration
of every BiSinger experiment).  Two sets of lengths: `uniform` (every row T_txt tokens and T frames: what the lengths cost where they
skip nothing) and `mixed` (the frame counts of tools/bench_ragged.py, RandomState(0).randint(250, 1001), a tenth as many tokens).  The
inputs are 0 beyond each row's end in both modes.  Windows of `passes` forwards alternate between the two modes (padded, ragged, padded,
...) after `passes` warm-up forwards of each, so that a drift of the clocks meets both alike; the figure is the median window.
`skipped_rows` is the share of the padded rows that the ragged stacks do not compute (bsg_fs2midi_last_rows: 32-row granules).
`lengths_read_ms` is what the ragged forward spends before its first launch: the lengths of both axes in one host read
(fs2.prefix_lengths), timed alone the same way — the part of a ragged forward that no skipped row pays back.

    python tools/bench_fs2_ragged.py [--windows 7] [--passes 20]      -> one JSON line
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
from tests import fs2_pitch_ref as R  # noqa: E402
from tests import fs2_ragged_cases as RC  # noqa: E402

B, TT, T = 16, 100, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--passes', type=int, default=20, help='warm-up forwards of each mode, and forwards per window')
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    m, hp = R.build('midi', 2, True, None, pitch=False)
    m = m.cuda()
    mixed = [int(v) for v in np.random.RandomState(0).randint(250, 1001, size=B)]
    out = {'B': B, 'T_txt': TT, 'T': T}
    for name, frames in (('uniform', [T] * B), ('mixed', mixed)):
        c = RC.Case('midi', None, B, TT, T, [max(1, n * TT // T) for n in frames], frames)
        d = {k: torch.from_numpy(v).cuda() for k, v in RC.inputs(c).items()}
        kw = {k: d[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')}
        run = {mode: (lambda rag=(mode == 'ragged'): m(d['txt_tokens'], d['mel2ph'], d['spk_embed'], infer=True, **({'ragged': True} if rag else {}), **kw))
               for mode in ('padded', 'ragged')}
        wins = {'padded': [], 'ragged': []}
        for mode in run:
            for _ in range(a.passes):
                run[mode]()
        torch.cuda.synchronize()
        for _ in range(a.windows):
            for mode in run:
                t0 = time.perf_counter()
                for _ in range(a.passes):
                    run[mode]()
                torch.cuda.synchronize()
                wins[mode].append((time.perf_counter() - t0) / a.passes)
        rows = m.last_rows()      # of the last ragged forward: (token rows, rows of the decoder stack)
        from bisinger_amd.fs2 import prefix_lengths
        reads = []
        for _ in range(a.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.passes):
                prefix_lengths([d['txt_tokens'] > 0, d['mel2ph'] > 0], ['txt_tokens', 'mel2ph'], [1, 0])
            reads.append((time.perf_counter() - t0) / a.passes)
        rec = {'frames': frames, 'waste': round(1 - sum(frames) / (B * T), 4), 'path': m.last_path(),
               'skipped_rows': {'tokens': round(1 - rows[0] / (B * TT), 4), 'frames': round(1 - rows[1] / (B * T), 4)}}
        for mode in run:
            rec[mode] = {'ms_per_forward': round(float(np.median(wins[mode])) * 1e3, 4), 'windows_ms': [round(w * 1e3, 4) for w in wins[mode]]}
        rec['lengths_read_ms'] = round(float(np.median(reads)) * 1e3, 4)
        rec['speedup'] = round(rec['padded']['ms_per_forward'] / rec['ragged']['ms_per_forward'], 4)
        out[name] = rec
    out['range_retries'] = _lib.range_retries
    print(json.dumps(out))


if __name__ == '__main__':
    main()
