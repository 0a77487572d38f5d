"""Cases, inputs, position classes, statistics and the rounding-emulating reference of the bf16 sweep, shared by
tests/test_gpu_bf16_shapes.py (HIP against the float64 emulation), tools/make_golden_bf16_yardsticks.py (the emulation's own float32
against float64 deviation, computed on the CPU before any kernel runs: tests/golden/bf16_yardsticks.json) and tests/test_oracle_golden.py
(the record, the classes and the sensitivity of the bars).  No GPU is needed to import this module.

A case is (kind, L, B, T): L residual layers (hparams['residual_layers'], a run-time value of the library), B rows of T frames.
  eval          one evaluation, DiffNet.forward: stack launch (skip sum rounded once), fp32 in / skip / out projections
  eval_running  the same through the per-layer launches (BSG_STACK_BF16=0): the running skip sum rounded after every layer
  group         eval at the smallest batch that splits into two launch groups on 256 CUs
  ddpm          3 fused DDPM steps with supplied noise: bf16 step tail, the input projection in bf16 from the second evaluation on
  ddpm_f32tail  the same with BSG_TAIL_BF16=0: the skip sum still rounded once, every projection fp32
  plms          PLMS at K_step 30, interval 5 (6 iterations, 7 evaluations: the warm-up pair, the blends of 1 and 2 entries, the four-term
                formula twice, the no-op at i = 0).  bsg_plms_sample runs the first iteration unfused: evaluations 1 and 2 take fp32
                projections throughout, evaluation 3 an fp32 input projection (conv1x1 behind the first iteration) and the bf16 tail,
                evaluations 4.. the tail's bf16 input projection too
  ragged_eval, ragged_ddpm   B = 5 rows of RAGGED_LENS frames at T = 200; every row against the emulation of that row alone

Position classes of a row of n valid frames (a frame belongs to exactly one of the first four; at n <= 8 `start` takes every frame and
`end` is empty, at n <= 16 `end` takes what `start` left):
  start     frames 0 .. 7
  end       the last 8 valid frames not in start
  seam      t % 64 < 8 or t % 64 >= 56, not in start or end: the frames a neighbour tile's halo carries
  interior  the rest
  group     (the launch-group case) every frame of the last row of one group and the first row of the next
  all       every valid frame (printed and held to the same bar; the whole-tensor figure of the older tests)
Statistics per class over d = got - want [B, 80, T]: `rms` over all bins and frames of the class; `frame_max`, the largest per-frame rms
over the 80 bins.  A class without a frame is left out."""
import json
import math
import os
from collections import namedtuple

import numpy as np
import torch

from oracle import diffnet as odn, diffusion as odf

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
YARDSTICKS = os.path.join(GOLD, 'bf16_yardsticks.json')
PREFIX = 'denoise_fn.'
MARGIN = 4.0

Case = namedtuple('Case', 'kind L B T')

LAYERS = (1, 2, 5, 20)       # x and halo from HBM, no exchange | the first exchanged halo | every dilation and the wrap 8 -> 1 | shipped
SINGLE_T = (1, 8, 9,         # a row shorter than one halo; exactly one halo; one more frame
            63, 64, 65,      # one partial tile; one tile; a second tile with ONE frame
            71, 72, 73,      # a second tile of 7, 8, 9 frames: less than, exactly, more than the halo its left neighbour reads at dilation 8
            127, 128, 129,   # the same edges one tile further
            200)             # three tiles, T % 4 == 0, last tile of 8
GROUP = Case('group', 5, 26, 640)          # 10 tiles per row, 25 rows per group on 256 CUs
GROUP_ROWS = (24, 25)
SAMPLER_T = (63, 65, 129)
SWITCH_T = (65, 129, 200)
RAGGED_LENS = (200, 129, 65, 64, 1)
RAGGED_T = 200
DDPM_STEPS = 3
PLMS = (100, 30, 5)          # timesteps, K_step, interval, on tests/plms_cases.py's 100-step schedule to beta 0.06
PAD_X, PAD_COND = 3000.0, 40.0             # what a ragged row's padding holds: no real frame may see it


def batch_of(T):
    return 3 if T % 2 else 2


def eval_cases():
    return [Case('eval', L, batch_of(T), T) for L in LAYERS for T in SINGLE_T if T > 9 or L >= 5]


def sampler_cases():
    return [Case(kind, 5, 2, T) for kind in ('ddpm', 'plms') for T in SAMPLER_T]


def ragged_cases():
    return [Case('ragged_eval', 5, len(RAGGED_LENS), RAGGED_T), Case('ragged_ddpm', 5, len(RAGGED_LENS), RAGGED_T)]


def switch_cases():
    """{switch set: cases}.  BSG_COND_BF16_DIRECT=0 changes where the conditioner term is rounded, not what is computed: the eval cases."""
    return {'stack_off': [Case('eval_running', 5, batch_of(T), T) for T in SWITCH_T],
            'cond_indirect': [Case('eval', 5, batch_of(T), T) for T in SWITCH_T],
            'tail_f32': [Case('ddpm_f32tail', 5, 2, T) for T in SWITCH_T]}


def all_cases():
    out = eval_cases() + [GROUP] + sampler_cases() + ragged_cases()
    for cases in switch_cases().values():
        out += [c for c in cases if c not in out]
    return out


def name(case):
    return f'{case.kind}/L{case.L}/{case.B}x{case.T}'


def lengths_of(case):
    return list(RAGGED_LENS) if case.kind.startswith('ragged') else None


def about(case):
    """The classes a case is there for (tests/test_oracle_golden.py: each is non-empty)."""
    if case.kind == 'group':
        return ('group', 'seam')
    if case.kind.startswith('ragged'):
        return ('start', 'end', 'seam', 'interior')
    return ('start',) + (('end',) if case.T > 8 else ()) + (('seam',) if case.T >= 65 else ())


# ------------------------------------------------------------------------------------------------------------------
# inputs and the model
# ------------------------------------------------------------------------------------------------------------------
def inputs(case):
    """dict of float32 / int64 tensors from RandomState(seed of the case): x [B, 1, 80, T], cond [B, 256, T], t [B] (every row its own
    diffusion step), noise [DDPM_STEPS, B, 80, T].  A ragged case holds PAD_X / PAD_COND beyond every row's length."""
    kinds = ('eval', 'eval_running', 'group', 'ddpm', 'ddpm_f32tail', 'plms', 'ragged_eval', 'ragged_ddpm')
    shared = {'eval_running': 'eval', 'ddpm_f32tail': 'ddpm'}      # a switch set runs the inputs of the form it is compared with
    rs = np.random.RandomState(1000003 * kinds.index(shared.get(case.kind, case.kind)) + 10007 * case.L + 1009 * case.B + case.T)
    B, T = case.B, case.T
    d = dict(x=rs.standard_normal((B, 1, 80, T)).astype(np.float32), cond=rs.standard_normal((B, 256, T)).astype(np.float32),
             t=rs.randint(0, 100, size=(B,)).astype(np.int64), noise=rs.standard_normal((DDPM_STEPS, B, 80, T)).astype(np.float32))
    lens = lengths_of(case)
    if lens is not None:
        for b, n in enumerate(lens):
            d['x'][b, :, :, n:] = PAD_X
            d['cond'][b, :, n:] = PAD_COND
    return {k: torch.from_numpy(v) for k, v in d.items()}


def build_net(L):
    """DiffNet(80) of L residual layers on the formula weights of seed 0 (host tensors; the caller moves it).  The hparam is restored."""
    from bisinger_amd import synth
    from bisinger_amd.hparams import hparams
    from tests.util import load_formula_weights, use_config
    use_config()
    from bisinger_amd.diffnet import DiffNet
    keep = hparams['residual_layers']
    hparams['residual_layers'] = L
    try:
        net = DiffNet(80)
    finally:
        hparams['residual_layers'] = keep
    assert net.n_layers == L and len(net.residual_layers) == L
    return load_formula_weights(net, 0, synth.DIFFNET_GAIN, prefix=PREFIX)


def state_dict(L):
    """{'denoise_fn.' + key: host tensor} of build_net(L)."""
    from tests.util import cpu_sd
    return cpu_sd(build_net(L), PREFIX)


# ------------------------------------------------------------------------------------------------------------------
# position classes and statistics
# ------------------------------------------------------------------------------------------------------------------
def class_masks(B, T, lengths=None, group_rows=None):
    """{class: bool [B, T]}, classes without a frame left out."""
    m = {k: np.zeros((B, T), bool) for k in ('start', 'end', 'seam', 'interior', 'group', 'all')}
    t = np.arange(T)
    for b in range(B):
        n = T if lengths is None else lengths[b]
        valid = t < n
        start = valid & (t < 8)
        end = valid & (t >= n - 8) & ~start
        seam = valid & ((t % 64 < 8) | (t % 64 >= 56)) & ~start & ~end
        m['start'][b], m['end'][b], m['seam'][b], m['interior'][b], m['all'][b] = start, end, seam, valid & ~start & ~end & ~seam, valid
        if group_rows is not None and b in group_rows:
            m['group'][b] = valid
    return {k: v for k, v in m.items() if v.any()}


def masks_of(case):
    return class_masks(case.B, case.T, lengths_of(case), GROUP_ROWS if case.kind == 'group' else None)


def stats(got, want, masks):
    """{class: (rms, frame_max)} of got - want, both [B, 1, 80, T]."""
    d = np.asarray(got, np.float64) - np.asarray(want, np.float64)
    ms = (d[:, 0] ** 2).mean(axis=1)      # [B, T]: mean square over the 80 bins
    return {k: (float(math.sqrt(ms[m].mean())), float(math.sqrt(ms[m].max()))) for k, m in masks.items()}


# ------------------------------------------------------------------------------------------------------------------
# the emulation
# ------------------------------------------------------------------------------------------------------------------
def _forward(sd, L, x, t, cond, dtype, plain=False, **kw):
    if plain:
        return odn.diffnet_forward(sd, x, t, cond, PREFIX, n_layers=L, dtype=dtype)
    return odn.diffnet_forward(sd, x, t, cond, PREFIX, n_layers=L, dtype=dtype, operand_bf16=True, **kw)


def _emulate_rows(sd, case, x, cond, t, noise, dtype, plain, forward):
    B, L = x.shape[0], case.L
    kind = case.kind.replace('ragged_', '')
    if kind in ('eval', 'group'):
        return forward(sd, L, x, t, cond, dtype, plain, skip_rounding='final')
    if kind == 'eval_running':
        return forward(sd, L, x, t, cond, dtype, plain, skip_rounding='running')
    calls = []
    if kind in ('ddpm', 'ddpm_f32tail'):
        tail = kind == 'ddpm'

        def den(x_, t_):
            calls.append(1)
            return forward(sd, L, x_, t_, cond, dtype, plain, skip_rounding='final', tail_bf16=tail, in_bf16=tail and len(calls) > 1)
        sch = odf.make_schedule(100, 'linear', 0.06)
        xx = x.to(dtype)
        for k in range(DDPM_STEPS):
            xx = odf.p_sample(sch, den, xx, torch.full((B,), 99 - k, dtype=torch.long), noise[k][:, None].to(dtype))
        return xx
    assert kind == 'plms', case

    def den(x_, t_):      # evaluations 1, 2: the unfused first iteration; 3: fp32 input projection, bf16 tail; 4..: both bf16
        calls.append(1)
        return forward(sd, L, x_, t_, cond, dtype, plain, skip_rounding='final', tail_bf16=len(calls) > 2, in_bf16=len(calls) > 3)
    return odf.plms_sample(odf.make_schedule(PLMS[0], 'linear', 0.06), den, x.to(dtype), PLMS[1], PLMS[2])


def emulate(sd, case, inp, dtype, plain=False, forward=_forward):
    """The reference of a case -> float64 numpy [B, 1, 80, T]: eps of an evaluation, x after a sampler run.  dtype: the arithmetic between
    the roundings (float64: the reference; float32: what the yardstick compares with it).  plain: the oracle without any rounding.  A
    ragged case: every row alone at its own length; beyond it what the ragged contract documents: eps 0, x as given."""
    lens = lengths_of(case)
    if lens is None:
        return _emulate_rows(sd, case, inp['x'], inp['cond'], inp['t'], inp['noise'], dtype, plain, forward).double().numpy()
    out = np.zeros(tuple(inp['x'].shape)) if case.kind == 'ragged_eval' else inp['x'].double().numpy().copy()
    for b, n in enumerate(lens):
        r = _emulate_rows(sd, case, inp['x'][b:b + 1, :, :, :n].contiguous(), inp['cond'][b:b + 1, :, :n].contiguous(), inp['t'][b:b + 1],
                          inp['noise'][:, b:b + 1, :, :n].contiguous(), dtype, plain, forward)
        out[b:b + 1, :, :, :n] = r.double().numpy()
    return out


def slipped_forward(layer=3):
    """A forward for emulate() with a one-frame slip of the halo planted: before residual layer `layer` (dilation 8) column 64 k - 1 of
    the residual stream, the last frame a tile hands its right neighbour, is replaced by column 64 k - 2.  Restates diffnet_forward's bf16
    branch over oracle.diffnet.residual_block; tests/test_oracle_golden.py holds it to diffnet_forward bit for bit with the slip off."""
    import torch.nn.functional as F

    def forward(sd, L, x, t, cond, dtype, plain=False, skip_rounding='final', tail_bf16=False, in_bf16=False, slip=True):
        assert not plain and not tail_bf16 and not in_bf16 and skip_rounding == 'final'
        g = lambda k: sd[PREFIX + k].to(dtype)
        cond = cond.to(dtype)
        h = F.relu(odn._conv1d(x.to(dtype)[:, 0], g('input_projection.weight'), g('input_projection.bias')))
        d = odn.step_embedding(sd, t, h.shape[1], PREFIX, dtype)
        run = None
        for i in range(L):
            if slip and i == layer:
                h = h.clone()
                cols = slipped_columns(h.shape[-1])
                h[:, :, cols] = h[:, :, [c - 1 for c in cols]]
            h, s = odn.residual_block(sd, f'{PREFIX}residual_layers.{i}.', h, cond, d, 2 ** (i % 4), dtype, True)
            run = s if run is None else run + s
        h = odn._bf16(run / math.sqrt(L))
        h = F.relu(odn._conv1d(h, g('skip_projection.weight'), g('skip_projection.bias')))
        return odn._conv1d(h, g('output_projection.weight'), g('output_projection.bias'))[:, None]
    return forward


def slipped_columns(T):
    return [c for c in range(63, T, 64)]


# ------------------------------------------------------------------------------------------------------------------
# the record
# ------------------------------------------------------------------------------------------------------------------
def yardstick(sd, case):
    """-> {class: {'yard': [rms, frame_max] of the float32 emulation against the float64 one, 'cost': the same of the float64 emulation
    against the plain float64 oracle (what the roundings cost; printed)}}"""
    inp, masks = inputs(case), masks_of(case)
    e64 = emulate(sd, case, inp, torch.float64)
    yard = stats(emulate(sd, case, inp, torch.float32), e64, masks)
    cost = stats(e64, emulate(sd, case, inp, torch.float64, plain=True), masks)
    return {k: {'yard': list(yard[k]), 'cost': list(cost[k])} for k in masks}


def load_yardsticks():
    with open(YARDSTICKS) as f:
        return json.load(f)['yardsticks']


SPARSE_L = 2      # stacks of at most this many layers: the yardstick of a class is a sample of a few flips (bars)


def bars(case, yard=None):
    """{class: (rms bar, frame_max bar)}: MARGIN x the recorded yardstick of that case, class and statistic.
    One exception, for the single evaluations of at most SPARSE_L layers only: there a class is held to MARGIN x the largest `all`
    yardstick over the cases of the same layer count where that is larger than its own.  At L = 1 a flip of the once-rounded skip sum
    moves one frame by 1e-4 .. 4e-4 rms and the float32 emulation flips in 1 .. 10 frames of a case (eval/L1/2x72: exactly one, all-rms
    8.9e-6 = 1.07e-4 / sqrt(144); eval/L1/3x65: 4.9e-5), and the 16 .. 24 frames of `start` or `end` often hold none: their record is
    then plain float32 rounding, 6e-8.  A correct implementation whose flips fall elsewhere sits far above 4 x such a record without
    being wrong; tests/test_gpu_bf16_shapes.py lists the measured HIP figures of every class this moves.  Everywhere else (L >= 5, the
    samplers, the ragged forms, the launch groups, the switch sets) the record is dense and the bar is the class's own."""
    yard = load_yardsticks() if yard is None else yard
    rec = yard[name(case)]
    floor = [0.0, 0.0]
    if case.kind == 'eval' and case.L <= SPARSE_L:
        pool = [yard[name(c)]['all']['yard'] for c in eval_cases() if c.L == case.L]
        floor = [max(p[i] for p in pool) for i in (0, 1)]
    return {k: (MARGIN * max(v['yard'][0], floor[0]), MARGIN * max(v['yard'][1], floor[1])) for k, v in rec.items()}
