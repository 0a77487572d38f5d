#!/usr/bin/env python3
"""Goldens of the PLMS loop at its schedule edges, from the reference's own p_sample_plms.  Build container only (needs the reference
checkout).  The reference's GaussianDiffusion over its WaveNet denoiser gets the formula weights (synth.synth_state_dict, seed 0,
DIFFNET_GAIN: the weights of every sampler test) and runs its inference loop (shallow_diffusion_tts.py:258-264 over :168-201) from a
supplied x_T at B = 1 (it raises for B > 1), T = 32, for every (K_step, interval) of tests/plms_cases.py: the history-depth and schedule
edges and 100 / 5, all on the 100-step schedule to beta 0.06.  (5, 5) and (3, 5) have no golden: their only iteration is at i = 0, where
the reference's `max(t - interval, 0)` is an int that its denoiser cannot take; the test holds the oracle to x_T there.
tests/golden/plms_edges.npz holds the results only ('x0.<K_step>_<interval>'); x_T and the condition are regenerated from RandomState(47)
by the test (tests/test_oracle_golden.py)."""
import os
import sys
from collections import deque

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bisinger_amd import synth          # noqa: E402
from tests import plms_cases as pc      # noqa: E402
import ref_import                       # noqa: E402
from make_golden import load_synth      # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
torch.set_grad_enabled(False)


def main():
    R = ref_import.import_reference()
    hp, sdt = R['hparams'], R['sdt']
    from oracle import diffnet as odn, diffusion as odf
    hp['timesteps'], hp['K_step'], hp['max_beta'] = 100, 100, 0.06
    betas = sdt.linear_beta_schedule(100, max_beta=0.06)
    m = R['GaussianDiffusion'](R['phone_encoder'], 80, R['DiffNet'](80), timesteps=100, K_step=100, loss_type='l1', betas=betas,
                               spec_min=hp['spec_min'], spec_max=hp['spec_max']).eval()
    load_synth(m, 0, synth.DIFFNET_GAIN)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    xT, cond = pc.golden_inputs()
    sch = odf.make_schedule(100, 'linear', 0.06)
    out = {}
    for K_step, interval in pc.EDGES + [pc.MAIN[1:]]:
        x = xT.clone()
        m.noise_list = deque(maxlen=4)                                   # :259
        if K_step <= interval:
            # a first iteration at i < interval: the reference's `max(t - interval, 0)` (:189) is then the int 0, which its denoiser
            # cannot take (AttributeError), so the reference has no result to record.  a_prev = a_t there: the loop leaves x_T as it is
            try:
                m.p_sample_plms(x, torch.zeros(1, dtype=torch.long), interval, cond)
                raise SystemExit('the reference ran a first iteration at i < interval: record it')
            except AttributeError as e:
                print(f'K_step {K_step} interval {interval}: the reference raises ({e}); no golden')
            continue
        for i in reversed(range(0, K_step, interval)):                   # :261-264
            x = m.p_sample_plms(x, torch.full((1,), i, dtype=torch.long), interval, cond)
        out[f'x0.{K_step}_{interval}'] = x.numpy()
        den = lambda x_, t_: odn.diffnet_forward(sd, x_, t_, cond, 'denoise_fn.')
        mine = odf.plms_sample(sch, den, xT, K_step, interval)
        den64 = lambda x_, t_: odn.diffnet_forward(sd, x_, t_, cond, 'denoise_fn.', dtype=torch.float64)
        m64 = odf.plms_sample(sch, den64, xT.double(), K_step, interval)
        print(f'K_step {K_step} interval {interval}: oracle vs reference {float((mine - x).abs().max()):.3e}; reference vs float64 oracle '
              f'{float((x.double() - m64).abs().max()):.3e}; fp32 oracle vs float64 {float((mine.double() - m64).abs().max()):.3e}; '
              f'moved from x_T by {float((x - xT).abs().max()):.3e}')
    path = os.path.join(GOLD, 'plms_edges.npz')
    np.savez_compressed(path, **out)
    print(f'{path} {os.path.getsize(path) / 1024:.1f} KB')


if __name__ == '__main__':
    main()
