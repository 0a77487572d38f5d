#!/usr/bin/env python3
"""Yardsticks of the PLMS sweep (tests/test_gpu_plms_shapes.py): for every case of tests/plms_cases.cpu_cases() the deviation of the plain
fp32 oracle trajectory (oracle.diffusion.plms_sample over oracle.diffnet.diffnet_forward) from the same in float64 — over the whole batch,
the row ends and the tile seams — into tests/golden/plms_yardsticks.json.  CPU only, no GPU and no reference checkout needed; run before
the GPU test, whose bars are 4 x the largest whole-batch figure of each sampler setting.  Cases already in the file are kept (--redo
recomputes them); the file is rewritten after every case."""
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
from bisinger_amd import synth          # noqa: E402
from tests import plms_cases as pc      # noqa: E402

torch.set_grad_enabled(False)


def state_dict():
    spec = json.load(open(os.path.join(pc.GOLD, 'state_dict_spec.json')))['GaussianDiffusion']
    spec = OrderedDict((k, tuple(s)) for k, s in spec)
    return {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(spec, 0, synth.DIFFNET_GAIN).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--redo', action='store_true')
    a = ap.parse_args()
    sd = state_dict()
    js = {'yardsticks': {}}
    if os.path.exists(pc.YARDSTICKS) and not a.redo:
        js = json.load(open(pc.YARDSTICKS))
    for setting, B, T, ragged in sorted(pc.cpu_cases(), key=lambda c: pc.cost(*c[:3])):
        lens = pc.ragged_lengths() if ragged else None
        sn, cn = pc.setting_name(setting), pc.case_name(B, T, lens)
        if cn in js['yardsticks'].get(sn, {}):
            continue
        t0 = time.time()
        x, cond = pc.inputs(B, T)
        want = pc.trajectory(sd, x, cond, setting, torch.float64, lengths=lens)
        w32 = pc.trajectory(sd, x, cond, setting, torch.float32, lengths=lens)
        dev = pc.deviations(w32, want, lens)
        js['yardsticks'].setdefault(sn, {})[cn] = [float('%.4g' % v) for v in dev]
        js['yardsticks'][sn][cn].append(float('%.4g' % np.abs(want).max()))
        print(f'{sn} {cn}: fp32 oracle vs float64 whole {dev[0]:.3e} ends {dev[1]:.3e} seams {dev[2]:.3e}; max |want| {np.abs(want).max():.3f}; '
              f'{time.time() - t0:.0f} s', flush=True)
        json.dump(js, open(pc.YARDSTICKS, 'w'), indent=1, sort_keys=True)
    for sn, cases in sorted(js['yardsticks'].items()):
        worst = max(cases, key=lambda k: cases[k][0])
        print(f'{sn}: largest {cases[worst][0]:.3e} ({worst}) -> bar {4 * cases[worst][0]:.3e}')


if __name__ == '__main__':
    main()
