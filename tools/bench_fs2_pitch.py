#!/usr/bin/env python3
"""Time the FastSpeech2 front (encode + decode, mel2ph given) on one build in three variants:
    midi        FastSpeech2MIDI without the pitch adaptor (the path of every shipped configuration)
    midi+pitch  FastSpeech2MIDI with use_pitch_embed (5-layer predictor, predicted f0)
    plain+pitch the plain FastSpeech2 front with use_pitch_embed (2-layer predictor, predicted f0)
at B = 1 and B = 16, T_txt = 100, T = 1000, and count the launches of one call from bsg_fs2midi_last_path's forms.

    python tools/bench_fs2_pitch.py [--reps 300] [--json out.json]

Method: formula weights and inputs, one warm-up call per variant and shape, then `reps` calls between two events on the current stream
(0.3 - 0.8 s per window; every call is a guarded module call, which waits for its stream once: the figure is the time of one
such call, host path included, not the sum of its kernels), median of 5 such windows, the three variants
interleaved per shape so that clock drift hits them alike; the shader clock (rocm-smi's current sclk, read only) is printed beside them.
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bisinger_amd import synth          # noqa: E402
from tests import fs2_pitch_ref as R    # noqa: E402

torch.set_grad_enabled(False)


def launches(m):
    """The front's own launches of the last call, as the handle recorded them (bsg_fs2midi_last_path): `pit.launches:<n>` is counted by
    the library where each of the adaptor's launches is made; without the adaptor the frame gather is one launch that leaves no token;
    `tok:front` is the plain front's one embedding launch.  The stacks' launches are the same in every variant and are not counted."""
    path = m.last_path().split()
    n = [int(t.split(':')[1]) for t in path if t.startswith('pit.launches:')]
    return (n[0] if n else 1) + ('tok:front' in path), [t for t in path if t.startswith(('pit.', 'tok:'))]


def sclk():
    try:
        out = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=20).stdout
        return [l.strip() for l in out.splitlines() if 'sclk' in l][:1]
    except Exception as e:      # noqa: BLE001
        return [f'unavailable ({type(e).__name__})']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=300)
    ap.add_argument('--json')
    a = ap.parse_args()
    variants = {'midi': R.build('midi', 5, True, pitch=False), 'midi+pitch': R.build('midi', 5, True), 'plain+pitch': R.build('plain', 2, True)}
    variants = {k: (m.cuda(), hp) for k, (m, hp) in variants.items()}
    res = {'clock': sclk(), 'device': torch.cuda.get_device_name(0), 'rows': []}
    for B in (1, 16):
        inp = {k: torch.from_numpy(v).cuda() for k, v in synth.synth_inputs(B, 100, 1000, seed=5).items()}
        kw = {k: inp[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')}

        def call(name):
            m, hp = variants[name]
            if hp['use_midi']:
                return m(inp['txt_tokens'], inp['mel2ph'], inp['spk_embed'], infer=True, **kw)
            return m(inp['txt_tokens'], inp['mel2ph'], None, infer=True)
        times = {k: [] for k in variants}
        for name in variants:
            call(name)
        torch.cuda.synchronize()
        for _ in range(5):
            for name in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    call(name)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / a.reps)
        for name in variants:
            call(name)
            n, forms = launches(variants[name][0])
            t = sorted(times[name])
            row = dict(variant=name, B=B, T=1000, ms_median=round(t[2], 4), ms_min=round(t[0], 4), ms_max=round(t[-1], 4), front_launches=n, forms=forms)
            res['rows'].append(row)
            print(row, flush=True)
    print('clock', res['clock'])
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
