"""Cases, inputs, references and windows of the PLMS sweep, shared by tests/test_gpu_plms_shapes.py (HIP against float64),
tools/plms_yardsticks.py (the fp32 oracle's own deviation from float64, computed on the CPU before any kernel runs:
tests/golden/plms_yardsticks.json) and tests/test_oracle_golden.py (the recorded yardsticks and the reference's goldens of the schedule
edges).  No GPU is needed to import this module.

A sampler setting is (timesteps, K_step, interval): the 100-step schedule to beta 0.06 of configs/bisinger_diff100.yaml, or the shipped
1000-step schedule to beta 0.02.  Iterations run at i = K_step' .. 0 in steps of the interval, K_step' the largest multiple of the
interval below K_step; the first one costs two evaluations."""
import json
import os

import numpy as np
import torch

from oracle import diffnet as odn, diffusion as odf

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
YARDSTICKS = os.path.join(GOLD, 'plms_yardsticks.json')

MAIN = (100, 100, 5)                  # 20 iterations, 21 evaluations
SHIPPED = (1000, 1000, 5)             # 200 iterations, 201 evaluations
# (K_step, interval) of the history-depth and schedule edges, on the 100-step schedule.  The iteration at i = 0 has a_prev = a_t, so its
# x_delta is 0 x (...): the LAST iteration of every schedule runs its launches but leaves x as it is, and its blend cannot be told from a
# wrong one by the numbers.  What acts on x is one iteration less than what runs
EDGES = [(5, 5),       # one iteration: only the unfused predictor / corrector, ip = 0; x stays x_T
         (10, 5),      # two iterations: the fused one (n_hist = 1) is the no-op at i = 0, so only the unfused first iteration acts
         (15, 5),      # three: n_hist = 1 acts, n_hist = 2 runs as the no-op
         (20, 5),      # four: n_hist = 1, 2 act, n_hist = 3 runs as the no-op (the three-entry blend first acts in the long schedules)
         (3, 5),       # interval > K_step: a single iteration at i = 0 (a_prev = a_t: x stays what the predictor / corrector leaves)
         (100, 7),     # last = 98, not K_step - 1
         (98, 5)]      # K_step no multiple of the interval
EDGE_SETTINGS = [(100, k, iv) for k, iv in EDGES]
MAX_BETA = {100: 0.06, 1000: 0.02}

# the default path over plan_stack's map (the forms named are what it gives on 256 CUs today; the GPU test reads them from last_path)
SHAPES = [(1, 1), (2, 5), (3, 17), (2, 31),              # rows shorter than the dilation halo, T < one tile: stack_h2_quad
          (3, 65), (3, 77), (5, 333),                    # one frame into a second tile; partial tile; T % 4 != 0: quad / quad64
          (1, 1000), (2, 1000),                          # stack_h2_quad
          (4, 1000), (1, 2500),                          # stack_h2_quad64
          (5, 1000), (8, 1000), (7, 129),                # stack_h2_pair64
          (9, 1000), (16, 1000),                         # stack_h2q_tail, one launch group (16 x 1000: the bench shape)
          (20, 777), (32, 997),                          # stack_h2q_tail, several launch groups of whole rows, T % 4 != 0, partial last tile
          (10, 900)]                                     # 290 tiles > CUs: two half-batch chains
EDGE_SHAPES = [(3, 77), (9, 1000)]
SHIPPED_SHAPES = [(2, 333), (9, 1000)]
SHORT_LIST = [(2, 5), (3, 77), (5, 333), (16, 1000)]     # what every fallback / switch form runs at 100 / 5 ...
SHORT_EDGE = ((3, 77), (100, 15, 5))                      # ... and (15, 5) at 3 x 77
RAGGED_B, RAGGED_T = 12, 1000
CPU_COST = 40000             # evaluations x frames up to which a case's yardstick is computed on the CPU

WINDOW = 8


def setting_name(setting):
    return '%d/%d/%d' % setting


def case_name(B, T, lengths=None):
    return f'{B}x{T}' + ('' if lengths is None else 'r')


def cost(setting, B, T):
    return (setting[1] // setting[2] + 2) * B * T


def all_cases():
    """[(setting, B, T, ragged)] of everything that is compared against float64 on the default path."""
    cases = [(MAIN, B, T, False) for B, T in SHAPES]
    cases += [(s, B, T, False) for s in EDGE_SETTINGS for B, T in EDGE_SHAPES]
    cases += [(SHIPPED, B, T, False) for B, T in SHIPPED_SHAPES] + [(MAIN, RAGGED_B, RAGGED_T, True)]
    return cases


def on_cpu(setting, B, T, ragged=False):
    """True for the cases whose fp32 yardstick is computed on the CPU and recorded (tools/plms_yardsticks.py), and so enters the bar of
    its setting: those of at most CPU_COST evaluations x frames, the ragged batch (rows of at most 1000 frames, one by one) and the
    smaller shape of the shipped schedule.  The others have both oracle trajectories evaluated by torch on the GPU inside the GPU test;
    they add no term to the bar, which can only make it smaller than the one over all cases."""
    return ragged or cost(setting, B, T) <= CPU_COST or (setting, B, T) == (SHIPPED, *SHIPPED_SHAPES[0])


def cpu_cases():
    return [c for c in all_cases() if on_cpu(*c)]


def ragged_lengths():
    """B = 12 rows of 250 .. 1000 frames from RandomState(0), with a 1-frame row, a row of exactly 64, one of 65 and a full row planted."""
    lens = np.random.RandomState(0).randint(250, RAGGED_T + 1, size=RAGGED_B)
    lens[2], lens[5], lens[7], lens[10] = 1, 64, 65, RAGGED_T
    return [int(v) for v in lens]


def inputs(B, T):
    """(x_T [B, 1, 80, T], cond [B, 256, T]) float32 from a seed derived from (B, T)."""
    rs = np.random.RandomState(1000 * B + T)
    x = rs.standard_normal((B, 1, 80, T)).astype(np.float32)
    cond = rs.standard_normal((B, 256, T)).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(cond)


def golden_inputs():
    """(x_T [1, 1, 80, 32], cond [1, 256, 32]) of tests/golden/plms_edges.npz (tools/make_golden_plms_edges.py)."""
    rs = np.random.RandomState(47)
    x = rs.standard_normal((1, 1, 80, 32)).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(rs.standard_normal((1, 256, 32)).astype(np.float32))


def schedule(timesteps):
    return odf.make_schedule(timesteps, 'linear', MAX_BETA[timesteps])


def trajectory(sd, x_T, cond, setting, dtype, device='cpu', lengths=None):
    """oracle.diffusion.plms_sample over oracle.diffnet.diffnet_forward(dtype) -> float64 numpy [B, 1, 80, T].  `lengths`: every row
    alone at T = lengths[b]; frames beyond are x_T's.  `sd`: the state dict with the 'denoise_fn.' keys, on `device`."""
    timesteps, K_step, interval = setting
    sch = schedule(timesteps)
    if lengths is not None:
        out = x_T.double().numpy().copy()
        for b, n in enumerate(lengths):
            out[b:b + 1, :, :, :n] = trajectory(sd, x_T[b:b + 1, :, :, :n].contiguous(), cond[b:b + 1, :, :n].contiguous(), setting, dtype, device)
        return out
    c = cond.to(device)
    den = lambda x_, t_: odn.diffnet_forward(sd, x_, t_, c, 'denoise_fn.', dtype=dtype)
    return odf.plms_sample(sch, den, x_T.to(device=device, dtype=dtype), K_step, interval).double().cpu().numpy()


def window_mask(T, lengths=None, B=1):
    """(ends, seams): boolean [B, T] masks of the first and last 8 frames of every row (of its own frames, for a ragged batch), and of the
    8 frames on each side of every multiple of 64 inside it: where padding, halo exchange and partial tiles live."""
    ends, seams = np.zeros((B, T), bool), np.zeros((B, T), bool)
    for b in range(B):
        n = T if lengths is None else lengths[b]
        ends[b, :min(WINDOW, n)] = True
        ends[b, max(0, n - WINDOW):n] = True
        for m in range(64, n, 64):
            seams[b, m - WINDOW:min(n, m + WINDOW)] = True
    return ends, seams


def deviations(got, want, lengths=None):
    """(whole, ends, seams) max-abs of got - want over [B, 1, M, T] (a ragged batch: over every row's own frames); seams is 0.0 where no
    row reaches frame 64."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))[:, 0]      # [B, M, T]
    B, _, T = d.shape
    ends, seams = window_mask(T, lengths, B)
    valid = np.ones((B, T), bool) if lengths is None else np.arange(T)[None, :] < np.asarray(lengths)[:, None]
    pick = lambda m: float(d.transpose(0, 2, 1)[m].max()) if m.any() else 0.0
    return pick(valid), pick(ends), pick(seams)


def load_yardsticks():
    """-> {setting name: {case name: [whole, ends, seams] of the fp32 oracle trajectory against the float64 one}} as recorded by
    tools/plms_yardsticks.py."""
    with open(YARDSTICKS) as f:
        return json.load(f)['yardsticks']


def bar(setting, yard=None):
    """4 x the largest deviation of the fp32 oracle trajectory from the float64 one over the setting's cases (normalised units)."""
    yard = load_yardsticks() if yard is None else yard
    return 4.0 * max(v[0] for v in yard[setting_name(setting)].values())
