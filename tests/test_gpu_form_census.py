"""GPU: the denoiser's planner is pinned.  tests/data/stack_form_census.json holds, for every case of tools/stack_form_census.py (fp32 and
bf16 handle x handle state x binding x B x T), which launch form ran, in how many chains and groups, and what the two queries said, as
the commit before the launch-form table wrote it.  The census runs again here and must be equal: a change to which form a shape takes
is an edit to that file.

The second test needs two GPUs: a model on cuda:1 in a process whose first handle lives on cuda:0 takes every launch form of a small
sampler call (quad part form with the 96 KB step tail and the split-fp16 input projection, then the forms behind set_parts / set_h2q /
set_h2 0) and returns what cuda:0 returns.  The LDS grant of a kernel is made per handle, on the handle's device."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from bisinger_amd import _lib
from tests.util import ROOT

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _tool():
    spec = importlib.util.spec_from_file_location('stack_form_census', os.path.join(ROOT, 'tools', 'stack_form_census.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_shape_takes_the_recorded_form():
    tool = _tool()
    with open(tool.DATA) as f:
        want = json.load(f)
    got = json.loads(json.dumps(tool.census()))
    n_cases = len(tool.DTYPES) * len(tool.STATES) * len(tool.BINDINGS) * len(tool.BATCHES) * len(tool.FRAMES)
    assert len(want) == n_cases and set(got) == set(want)
    diff = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    for k in sorted(diff)[:20]:
        print(k, 'recorded', diff[k][0], 'now', diff[k][1])
    assert not diff, f'{len(diff)} of {len(want)} cases take another form than recorded'


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs')
def test_second_device_takes_every_form():
    import bench
    B, T = 1, 96
    g = torch.Generator().manual_seed(3)
    cond0 = 0.5 * torch.randn(B, 256, T, generator=g)
    x0 = torch.randn(B, 1, 80, T, generator=g)
    lib = _lib.load()

    def run(index):
        dev = torch.device('cuda', index)
        with torch.cuda.device(dev):
            model = bench.build_model(dev)
            net = model.denoise_fn
            cond, outs = cond0.to(dev), []
            for setter in (None, 'bsg_diffnet_set_parts', 'bsg_diffnet_set_h2q', 'bsg_diffnet_set_h2'):
                if setter:
                    _lib.check(getattr(lib, setter)(net.handle(), 0), setter)
                x = model.sample(cond, x0.to(dev).clone(), seed=5, n_steps=3)
                outs.append((net.last_path(), x.cpu().numpy()))
            net.release()
        return outs

    first, second = run(0), run(1)
    assert first[0][0] == 'stack_h2_quad', first[0][0]
    for (p0, a0), (p1, a1) in zip(first, second):
        assert p0 == p1, (p0, p1)
        assert np.array_equal(a0, a1), p0
