#!/usr/bin/env python3
"""tests/golden/inv_freq.npz: the float32 inverse-frequency vectors of the sinusoidal tables as the host that made the goldens evaluates
them.  Run on that host only.  The exponents are the reference's expressions (net.py:37-44 SinusoidalPosEmb,
common_layers.py:124-146 get_embedding, espnet_positional_embedding.py:25-46); their float32 exp differs by an ulp here and there between
math-library code paths, and the tables multiply it by the row index, so the CPU oracle tests evaluate the oracle with these vectors
(oracle/freq.py).  Checked before writing: the oracle's step embedding with them reproduces the golden step_emb bit for bit."""
import json
import math
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bisinger_amd import synth          # noqa: E402
from oracle import diffnet as odn, freq  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
torch.set_grad_enabled(False)

half = 256 // 2
out = {'sinusoidal.exponent': (torch.arange(half, dtype=torch.float) * -(math.log(10000) / (half - 1))).numpy(),
       'rel_pos.exponent': (torch.arange(0, 256, 2, dtype=torch.float32) * -(math.log(10000.0) / 256)).numpy()}
for k in ('sinusoidal', 'rel_pos'):
    out[k + '.value'] = torch.exp(torch.from_numpy(out[k + '.exponent'])).numpy()

spec = OrderedDict((k, tuple(s)) for k, s in json.load(open(os.path.join(GOLD, 'state_dict_spec.json')))['GaussianDiffusion'])
sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(spec, 0, synth.DIFFNET_GAIN).items()}
assert np.array_equal(out['sinusoidal.exponent'], (torch.arange(half) * -(math.log(10000) / (half - 1))).numpy())
freq.inv_freq = lambda x: torch.from_numpy(out['sinusoidal.value'].copy())
d = odn.step_embedding(sd, torch.tensor([7, 93]), 256, 'denoise_fn.')
assert np.array_equal(d.numpy(), np.load(os.path.join(GOLD, 'diffnet.npz'))['step_emb']), 'not the host that made the goldens'
np.savez_compressed(os.path.join(GOLD, 'inv_freq.npz'), **out)
print({k: v.shape for k, v in out.items()})
