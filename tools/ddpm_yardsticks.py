#!/usr/bin/env python3
"""Yardsticks of the DDPM sweep (tests/test_gpu_ddpm_shapes.py): for every case of tests/ddpm_cases.all_cases() the deviation of the plain
fp32 oracle window (oracle.diffusion.p_sample over oracle.diffnet.diffnet_forward) from the same in float64 — over the whole batch, the
row ends and the tile seams — with max |want| and the largest share of clamped x_recon over the window's steps, into
tests/golden/ddpm_yardsticks.json.  CPU only, no GPU and no reference checkout needed; run before the GPU test, whose bars are 4 x the
largest whole-batch figure of each window.  Cases already in the file are kept (--redo recomputes them); the file is rewritten after
every case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ddpm_cases as dc      # noqa: E402
from tests import plms_cases as pc      # noqa: E402
from tools.plms_yardsticks import state_dict      # noqa: E402

torch.set_grad_enabled(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--redo', action='store_true')
    a = ap.parse_args()
    sd = state_dict()
    js = {'yardsticks': {}}
    if os.path.exists(dc.YARDSTICKS) and not a.redo:
        js = json.load(open(dc.YARDSTICKS))
    for window, B, T, lens in sorted(dc.all_cases(), key=lambda c: c[1] * c[2]):
        cn = dc.case_name(B, T, lens is not None)
        if cn in js['yardsticks'].get(window, {}):
            continue
        t0 = time.time()
        x, cond, noise = dc.inputs(window, B, T)
        want, shares = dc.reference(sd, window, x, cond, noise, torch.float64, lengths=lens)
        w32, _ = dc.reference(sd, window, x, cond, noise, torch.float32, lengths=lens)
        dev = pc.deviations(w32, want, lens)
        js['yardsticks'].setdefault(window, {})[cn] = {'dev': [float('%.4g' % v) for v in dev], 'max': float('%.4g' % np.abs(want).max()),
                                                       'clamp': float('%.4g' % max(shares))}
        print(f'{window} {cn}: fp32 oracle vs float64 whole {dev[0]:.3e} ends {dev[1]:.3e} seams {dev[2]:.3e}; max |want| {np.abs(want).max():.3f}; '
              f'clamp share per step {" ".join("%.3f" % s for s in shares)}; {time.time() - t0:.0f} s', flush=True)
        json.dump(js, open(dc.YARDSTICKS, 'w'), indent=1, sort_keys=True)
    for window, cases in sorted(js['yardsticks'].items()):
        worst = max(cases, key=lambda k: cases[k]['dev'][0])
        print(f"{window}: largest {cases[worst]['dev'][0]:.3e} ({worst}) -> bar {4 * cases[worst]['dev'][0]:.3e}; "
              f"largest clamp share {max(c['clamp'] for c in cases.values()):.3f}")


if __name__ == '__main__':
    main()
