"""GPU: the half-batch chains of channel-split launches (the `small` branch of dual_scope, csrc/diffnet.hip) against float64.

A whole batch whose per-layer form would be a pair-split or 16-wave launch is decoded by the fused PLMS loop as two half batches on two
streams, each half a chain of 4-way or pair-split launches with the un-padded LDS size, so that workgroups of both chains share CUs and
all of them are resident.  The second half runs at a row offset into every buffer of the handle: the conditioner term, the exchange tiles
and flags, the skip sum, the history ring.  The chains need a whole-batch plan without a stack form, so like the f23 child of
tests/test_gpu_plms_shapes.py the cases run in a child process under BSG_H2=0 BSG_WINO=1; its child script, sampler call, inputs
(tests/plms_cases.inputs), float64 trajectory, deviation windows and the bar of setting MAIN (4 x the fp32 oracle's own deviation from
float64, tests/golden/plms_yardsticks.json) are reused as they are.  The float64 trajectories are evaluated once, by torch on the GPU
(test_device_float64_equals_cpu of that file licenses it), and serve both children.

Shapes, the smallest that reach the two windows on 256 CUs: 8 x 270 (72 tiles of 32 frames; halves of 36) and 16 x 320 (160 tiles; halves
of 80).  Which form ran and in how many chains is read from the handle (last_path, last_launch) and printed, never restated from the
thresholds; where a device's CU count or occupancy gives something else, the assertion message says what it saw.

  child `dual`     two chains, last_path split4 / split2, no hand-off gave up (asserted inside the child's sampler call), finite, whole batch /
                   row ends / tile seams within the bar over ALL rows, those of the second half included
  child `no_dual`  BSG_DUAL=0 added: one chain, the same bar

Nothing is started after a child that failed.

Recorded on an MI355X (256 CUs) at the commit before the launch state moved from the handle into the plan (the test passed there first):
  dual     8 x 270 split4, chains / groups (2, 0)    16 x 320 split2, chains / groups (2, 0)
  no_dual  8 x 270 split2, chains / groups (1, 0)    16 x 320 wide,   chains / groups (1, 0)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import plms_cases as pc
from tests import test_gpu_plms_shapes as shapes
from tests.util import cpu_sd

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SHAPES = [(8, 270), (16, 320)]
F23 = {'BSG_H2': '0', 'BSG_WINO': '1'}
CHILDREN = [('dual', F23, 2), ('no_dual', dict(F23, BSG_DUAL='0'), 1)]      # (name, switches, chains expected)


def test_half_batch_chains_of_split_launches_vs_fp64(tmp_path):
    model = shapes._build(100)
    sd = {k: v.cuda() for k, v in cpu_sd(model).items()}
    model.denoise_fn.release()
    want = {(B, T): pc.trajectory(sd, *pc.inputs(B, T), pc.MAIN, torch.float64, 'cuda') for B, T in SHAPES}
    bar = pc.bar(pc.MAIN)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    jobs = [(f'{B}x{T}', pc.MAIN, B, T) for B, T in SHAPES]
    for name, env, chains in CHILDREN:
        d = tmp_path / name
        d.mkdir()
        res = subprocess.run([sys.executable, '-c', shapes.CHILD, str(d), json.dumps(jobs)], env=dict(os.environ, **env), capture_output=True,
                             text=True, timeout=300)
        assert res.returncode == 0, (name, res.stderr[-2000:])      # (a hand-off that gave up or a warning fails the child's _sample)
        seen = json.loads(res.stdout.strip().splitlines()[-1])
        for tag, _, B, T in jobs:
            path, launch = seen[tag][0], tuple(seen[tag][1])
            got = np.load(str(d / f'{tag}.npy'))
            dev = pc.deviations(got, want[(B, T)])
            print(f"\nplms {name} 100/100/5 {tag}: hip {' / '.join('%.2e' % v for v in dev)} | bar {bar:.2e} | {path}, chains / groups {launch} | {cus} CUs")
            saw = (name, tag, path, launch, f'{cus} CUs')
            assert launch[0] == chains, ('chains', *saw)
            if name == 'dual':
                assert path in ('split2', 'split4'), ('the half batches ran no channel-split launch', *saw)
            assert np.isfinite(got).all(), saw
            for window, v in zip(('whole batch', 'row ends', 'tile seams'), dev):
                assert v <= bar, (window, v, bar, *saw)
