#!/usr/bin/env python3
"""Yardsticks of the bf16 sweep (tests/test_gpu_bf16_shapes.py): for every case of tests/bf16_cases.all_cases() and every position class,
rms and frame_max of
  yard   the rounding-emulating oracle in float32 against the same emulation in float64 (1-ulp bf16 flips carried forward: how far two
         correct implementations of the bf16 configuration sit from each other; the GPU test's bar is 4 x this), and
  cost   the float64 emulation against the plain float64 oracle (what the roundings themselves cost; printed beside the HIP figure)
into tests/golden/bf16_yardsticks.json.  CPU only; no GPU and no reference checkout needed.  Run before the GPU test: no bar is taken
from a HIP run.  Cases already in the file are kept (--redo recomputes them)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import bf16_cases as bc      # noqa: E402

torch.set_grad_enabled(False)


def dump(js):
    """One line per class: case, class, yard [rms, frame_max], cost [rms, frame_max]."""
    lines = []
    for cn in sorted(js['yardsticks']):
        rows = ',\n'.join(f'   {json.dumps(k)}: {json.dumps(v, sort_keys=True)}' for k, v in sorted(js['yardsticks'][cn].items()))
        lines.append(f'  {json.dumps(cn)}: {{\n{rows}\n  }}')
    with open(bc.YARDSTICKS, 'w') as f:
        f.write('{\n "yardsticks": {\n' + ',\n'.join(lines) + '\n }\n}\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--redo', action='store_true')
    a = ap.parse_args()
    js = {'yardsticks': {}}
    if os.path.exists(bc.YARDSTICKS) and not a.redo:
        js = json.load(open(bc.YARDSTICKS))
    sds = {}
    for case in bc.all_cases():
        if bc.name(case) in js['yardsticks']:
            continue
        t0 = time.time()
        if case.L not in sds:
            sds[case.L] = bc.state_dict(case.L)
        rec = bc.yardstick(sds[case.L], case)
        js['yardsticks'][bc.name(case)] = {k: {s: [float('%.4g' % x) for x in v[s]] for s in v} for k, v in rec.items()}
        print(f'{bc.name(case)} ({time.time() - t0:.1f} s): ' + '  '.join(
            f"{k} {v['yard'][0]:.2e} / {v['yard'][1]:.2e} (cost {v['cost'][0]:.2e})" for k, v in rec.items()), flush=True)
        dump(js)
    keep = {bc.name(c) for c in bc.all_cases()}
    js['yardsticks'] = {k: v for k, v in js['yardsticks'].items() if k in keep}
    dump(js)


if __name__ == '__main__':
    main()
