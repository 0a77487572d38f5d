"""Cases, inputs, references and windows of the DDPM sweep, shared by tests/test_gpu_ddpm_shapes.py (HIP against float64),
tools/ddpm_yardsticks.py (the fp32 oracle's own deviation from float64, computed on the CPU before any kernel runs:
tests/golden/ddpm_yardsticks.json) and tests/test_ddpm_cases_cpu.py.  No GPU is needed to import this module.

A case is a short WINDOW of ancestral steps of the 100-step schedule to beta 0.06, not the whole loop: p_sample clamps x_recon to
[-1, 1], and a clamped element's new x does not depend on eps at all.  From x_T ~ N(0, 1) 84 % of the elements are clamped at t = 99 and
81 % still at t = 90, so a wrong halo, tile seam or row offset in eps is hidden on four elements of five wherever a check starts at
t = 99.  The windows start from a scaled x at a step where most of x_recon is inside the clamp, so that eps reaches x:

  LOW   t = 5 .. 0     x = 0.5 x inputs(B, T)[0]   ends in the sigma[0] = 0 step with no head; clamp share <= 0.10 at every step
  MID   t = 40 .. 35   x = 0.4 x                   last step has noise and no head; the highest eps gain (pc1 sqrt_recipm1, about 0.04)
                                                   among the low-clamp windows; clamp share <= 0.20 at every step
  HIGH  t = 99 .. 94   x = 1.0 x                   the clamp branch itself and the largest coefficients.  EXEMPT from the cap: its clamp
                                                   share is about 0.83, which is why it cannot stand alone and runs at two shapes only
  T0    t = 0          x = 0.5 x                   one call of one step: only the sigma = 0 step, no head
  T99   t = 99         x = 1.0 x                   one call of one step from the top of the schedule

The caps are a CONDITION on the float64 reference, asserted on the CPU over the recorded file and again by the GPU test on the reference
it computes; were a case to break one, the window's x scale goes down, never the cap up.  The eps sensitivity of one DDPM update is
pc1[t] sqrt_recipm1[t]: 0.010 at t = 0, 0.04 around t = 40, 0.06 at t = 99."""
import json
import os

import numpy as np
import torch

from oracle import diffnet as odn, diffusion as odf
from tests import plms_cases as pc

YARDSTICKS = os.path.join(pc.GOLD, 'ddpm_yardsticks.json')

#          t_start, steps, x scale
WINDOWS = {'LOW': (5, 6, 0.5), 'MID': (40, 6, 0.4), 'HIGH': (99, 6, 1.0), 'T0': (0, 1, 0.5), 'T99': (99, 1, 1.0)}
SWEEP = ('LOW', 'MID')                        # the windows every shape runs
CLAMP_CAP = {'LOW': 0.10, 'MID': 0.20, 'T0': 0.10}      # (T0 is LOW's last step from LOW's entry scale)
HIGH_SHAPES = [(3, 77), (16, 1000)]
EDGE_SHAPES = [(3, 77), (9, 1000)]            # the API edges: n_steps = 0 / 1, a window in two calls, the refusals
PHILOX_SHAPES = [(3, 77), (5, 333), (32, 997), (16, 1000)]
PHILOX_SEEDS = (20240917, 20240918)
SAMPLE_LENS = [1000] * 15 + [777, 517, 300, 65, 64, 1]      # tests/test_gpu_ragged.SAMPLE_LENS (the GPU test asserts they are the same)
RAGGED = {'6x200r': (6, 200, [200, 1, 63, 64, 65, 129], ('LOW', 'MID')),
          '21x1000r': (len(SAMPLE_LENS), 1000, SAMPLE_LENS, ('LOW',))}      # two launch groups
PLANT = 3e-4             # what the planted-error check adds to eps on one edge frame: 4e-4 x max |eps| (0.7)
PLANT_SHAPE = (3, 77)
TIE_CASES = [('LOW', 2, 5), ('MID', 3, 17), ('HIGH', 3, 77), ('T0', 3, 77)]      # recomputed by the CPU test and held to the record


def case_name(B, T, ragged=False):
    return f'{B}x{T}' + ('r' if ragged else '')


def all_cases():
    """[(window, B, T, lengths or None)] of everything that is compared against float64 with supplied noise; every one is cheap enough
    for the CPU (six evaluations), so every one enters the bar of its window."""
    cases = [(w, B, T, None) for w in SWEEP for B, T in pc.SHAPES]
    cases += [('HIGH', B, T, None) for B, T in HIGH_SHAPES]
    cases += [(w, B, T, None) for w in ('T0', 'T99') for B, T in EDGE_SHAPES]
    cases += [(w, B, T, lens) for B, T, lens, ws in RAGGED.values() for w in ws]
    return cases


def inputs(window, B, T):
    """(x at entry [B, 1, 80, T], cond [B, 256, T], noise [steps, B, 80, T]) float32: plms_cases.inputs with x scaled for the window, and
    the draws of the window's steps from a seed derived from (B, T, window)."""
    _, n, scale = WINDOWS[window]
    x, cond = pc.inputs(B, T)
    rs = np.random.RandomState(7 * (1000 * B + T) + list(WINDOWS).index(window) + 1)
    noise = rs.standard_normal((n, B, 80, T)).astype(np.float32)
    return (x * np.float32(scale)).contiguous(), cond, torch.from_numpy(noise)


def steps(sd, x, cond, noise, t_start, n, dtype, device='cpu', lengths=None, plant=None):
    """n steps of oracle.diffusion.p_sample over oracle.diffnet.diffnet_forward(dtype) at i = t_start .. t_start - n + 1 with the draws
    noise[k] ([n, B, 80, T]) -> (x as float64 numpy [B, 1, 80, T], [n] shares of the elements whose x_recon is clamped at each step).
    `lengths`: every row alone at T = lengths[b] with its slice of the batch's noise; frames beyond are x's, the shares those of the
    batch's own elements (a case is the batch: the 80 elements of a 1-frame row alone scatter up to 0.23 in MID). `plant` = (k, delta): delta added to the eps of step k at every row's last frame.  `sd`: the state dict with the
    'denoise_fn.' keys, on `device`."""
    if lengths is not None:
        out, shares = x.double().numpy().copy(), [0.0] * n
        for b, nf in enumerate(lengths):
            got, sh = steps(sd, x[b:b + 1, :, :, :nf].contiguous(), cond[b:b + 1, :, :nf].contiguous(),
                            noise[:, b:b + 1, :, :nf].contiguous(), t_start, n, dtype, device, None, plant)
            out[b:b + 1, :, :, :nf] = got
            shares = [a + c * nf / sum(lengths) for a, c in zip(shares, sh)]
        return out, shares
    sch = {k: v.to(device) for k, v in pc.schedule(100).items()}
    c = cond.to(device)
    xx, nz = x.to(device=device, dtype=dtype), noise.to(device=device, dtype=dtype)
    shares = []
    for k in range(n):
        def den(x_, t_):
            eps = odn.diffnet_forward(sd, x_, t_, c, 'denoise_fn.', dtype=dtype)
            if plant is not None and plant[0] == k:
                eps = eps.clone()
                eps[..., -1] += plant[1]
            x0 = (odf.extract(sch['sqrt_recip_alphas_cumprod'].to(dtype), t_, x_.shape) * x_
                  - odf.extract(sch['sqrt_recipm1_alphas_cumprod'].to(dtype), t_, x_.shape) * eps)
            shares.append(float((x0.abs() > 1).double().mean()))
            return eps
        t = torch.full((xx.shape[0],), t_start - k, dtype=torch.long, device=device)
        xx = odf.p_sample(sch, den, xx, t, nz[k][:, None])
    return xx.double().cpu().numpy(), shares


def reference(sd, window, x, cond, noise, dtype, device='cpu', lengths=None, plant=None):
    t_start, n, _ = WINDOWS[window]
    return steps(sd, x, cond, noise, t_start, n, dtype, device, lengths, plant)


def load_yardsticks():
    """-> {window: {case name: {'dev': [whole, ends, seams] of the fp32 oracle window against the float64 one, 'max': max |want|,
    'clamp': the largest clamp share over the steps (and rows)}}} as recorded by tools/ddpm_yardsticks.py."""
    with open(YARDSTICKS) as f:
        return json.load(f)['yardsticks']


def bar(window, yard=None):
    """4 x the largest whole-batch deviation of the fp32 oracle window from the float64 one over the window's cases (normalised units)."""
    yard = load_yardsticks() if yard is None else yard
    return 4.0 * max(v['dev'][0] for v in yard[window].values())
