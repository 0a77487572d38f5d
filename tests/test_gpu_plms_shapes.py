"""GPU parity of the PLMS sampler (bsg_plms_sample, the loop the shipped configuration decodes with) on every denoiser launch form,
against the float64 evaluation of the CPU oracle: oracle.diffusion.plms_sample over oracle.diffnet.diffnet_forward(dtype=float64).

  * the shapes (tests/plms_cases.SHAPES) walk plan_stack's map at timesteps = K_step = 100, interval 5: rows shorter than the dilation
    halo, one frame into a second tile, partial tiles, T % 4 != 0, one and several launch groups, the bench shape.  WHICH form ran is read
    from DiffNet.last_path() behind the sampler call, never restated from the thresholds; every case asserts handoff_timeouts() == 0 and
    that no range-guard warning fired, so the path named is the path that produced the output;
  * the history-depth and schedule edges (plms_cases.EDGES: one to four iterations, interval > K_step, an interval that does not divide
    K_step, a K_step that is no multiple of it) at 3 x 77 and 9 x 1000; the shipped schedule (1000 steps to beta 0.02, 201 evaluations) at
    2 x 333 and 9 x 1000; a ragged batch of 12 rows with a 1-frame row, a row of 64, one of 65 and a full row, each row against its own
    float64 trajectory at T = lengths[b], x beyond every length bit-identical to the caller's;
  * the deviation is taken over the whole batch, over the first and last 8 frames of every row, and over the 8 frames on each side of every
    multiple of 64; all three meet the same bar;
  * the fallback and switch forms, one child process per switch set, run the short list against the same float64 references and bars;
  * state left on the handle by a long call, and three replays of a captured call, are bit-identical to a fresh / eager call.

Reference and bar.  Cases of at most plms_cases.CPU_COST evaluations x frames, the ragged batch and 2 x 333 of the shipped schedule have the
float64 and the fp32 oracle trajectory computed on the CPU by tools/plms_yardsticks.py BEFORE any kernel ran (tests/golden/
plms_yardsticks.json; tests/test_oracle_golden.py ties the file to the oracle).  The bar of a sampler setting is 4 x the largest of these
fp32-against-float64 deviations over the setting's cases, in normalised units, the project's convention (test_gpu_hifigan_shapes.py); the
fallback forms are held to the same figure.  The larger cases would take hours on the CPU: both oracle trajectories are evaluated by torch
on the GPU (oracle.diffnet._conv1d: one float64 matrix product over the stacked taps; test_device_float64_equals_cpu holds it to the CPU's
result to 1e-12 at 2 x 31).  Their fp32 figure is printed beside the HIP figure and adds no term to the bar, which can only make the bar
smaller than the one over all cases (the arrangement of tests/test_gpu_pwg.py).

Yardsticks computed on the CPU (fp32 oracle against float64: whole batch / row ends / tile seams) and the bars they give:

  100 / 5        1 x 1 1.35e-6   2 x 5 3.12e-6   3 x 17 3.74e-6   2 x 31 4.12e-6   3 x 65 4.46e-6 / 4.46e-6 / 4.46e-6
                 3 x 77 3.70e-6 / 3.00e-6 / 3.70e-6   7 x 129 4.54e-6 / 3.73e-6 / 3.94e-6   1 x 1000 4.29e-6 / 3.13e-6 / 4.11e-6
                 5 x 333 5.12e-6 / 4.57e-6 / 3.85e-6   ragged 12 x 1000 5.21e-6 / 4.32e-6 / 4.65e-6          -> bar 2.08e-5  (max |x| 10 .. 22)
  (5, 5) (3, 5)  3 x 77 0, 9 x 1000 0: the only iteration is at i = 0, a_prev = a_t, x_delta = 0 x (...)      -> bar 0: x_T bit for bit
  (10, 5)        3 x 77 1.27e-7   9 x 1000 2.35e-7                                                          -> bar 9.39e-7
  (15, 5)        3 x 77 2.46e-7                                                                             -> bar 9.86e-7
  (20, 5)        3 x 77 3.36e-7                                                                             -> bar 1.34e-6
  (100, 7)       3 x 77 3.58e-6                                                                             -> bar 1.43e-5
  (98, 5)        3 x 77 3.70e-6 (the iterations of 100 / 5)                                                 -> bar 1.48e-5
  1000 / 5       2 x 333 5.45e-4 / 3.43e-4 / 4.66e-4  (max |x| 680: the formula weights' x grows over 201 evaluations) -> bar 2.18e-3

Every test prints its figures: "plms <setting> <B>x<T>: hip whole / ends / seams | fp32 oracle on the GPU (and the CPU record) | bar |
hip / fp32 (marked where it exceeds 2) | max |want| | the form read from last_path, chains / launch groups".  The table above holds the
oracle's side only: the HIP figure per case, the worst hip / fp32 ratio and whether any exceeds 2 are still to be copied into it from
these printed lines of an MI355X run, and until then neither "nothing deviates" nor a deviation is claimed here.  No kernel and no launch
was changed for this file; bsg_diffnet_last_launch is a read of host state (two ints of the handle, written by the samplers' host code).

dual_fork (two half-batch chains) needs a whole-batch plan without a stack form, so on the default path no shape of the list takes it: 10 x 900
and the 129..256-tile window run as ONE chain of stack launches (asserted), and the chains are reached under BSG_H2=0 BSG_WINO=1 (per-layer
launches) at 16 x 1000 only.  The chain count and the launch groups of the last stack launch are host state of the handle
(bsg_diffnet_last_launch, ABI v14): the f23 child asserts 2 chains at 16 x 1000, f23_no_dual asserts 1.

What the short schedules can detect: the iteration at i = 0 always has a_prev = a_t, so x_delta = 0 x (...) and that iteration leaves x
as it is, in the oracle and in every tail alike.  The LAST iteration of every schedule is therefore numerically a no-op: (10, 5) checks the
unfused first iteration only, (15, 5) one effective fused iteration (n_hist = 1), (20, 5) two (n_hist = 1, 2).  The three-entry blend first
acts in a schedule of five iterations; only 100 / 5, 100 / 7, 98 / 5 and 1000 / 5 exercise it and the four-slot ring's rotation.  The short
schedules still run the launches of the deeper blend (do_head = false, the history stores), so a fault or a non-finite value there shows.
"""
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np
import pytest
import torch

from bisinger_amd import synth
from bisinger_amd.hparams import hparams
from oracle import diffusion as odf
from tests import plms_cases as pc
from tests.util import ROOT, cpu_sd, load_formula_weights, use_config

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

F64, F32 = torch.float64, torch.float32
_REF = {}        # (setting, B, T, ragged) -> references
_CASES = {}      # (setting, B, T, ragged) -> figures of the default path
_T0 = time.time()


class _Enc:
    def __len__(self):
        return 65

    def pad(self):
        return 0


def _build(timesteps):
    use_config()
    from bisinger_amd.diffnet import DIFF_DECODERS
    from bisinger_amd.diffusion import GaussianDiffusion
    m = GaussianDiffusion(_Enc(), 80, DIFF_DECODERS['wavenet'](hparams), timesteps=timesteps, K_step=timesteps,
                          betas=odf.linear_beta_schedule(timesteps, pc.MAX_BETA[timesteps]), spec_min=hparams['spec_min'],
                          spec_max=hparams['spec_max'])
    load_formula_weights(m, 0, synth.DIFFNET_GAIN)
    return m.cuda()


@pytest.fixture(scope='module')
def models():
    """{timesteps: GaussianDiffusion over the WaveNet denoiser on the formula weights}, as tests/test_gpu_sampler.py builds it."""
    return {100: _build(100), 1000: _build(1000)}


@pytest.fixture(scope='module')
def sds(models):
    sd = cpu_sd(models[100])
    return {'cpu': sd, 'cuda': {k: v.cuda() for k, v in sd.items()}}


def _ref(sds, setting, B, T, ragged=False):
    """float64 reference and fp32 yardstick of one case: on the CPU record where there is one (the float64 trajectory itself is then
    evaluated on the GPU too, which test_device_float64_equals_cpu licenses: the record holds figures, not arrays), else on the GPU."""
    key = (setting, B, T, ragged)
    if key not in _REF:
        lens = pc.ragged_lengths() if ragged else None
        x, cond = pc.inputs(B, T)
        want = pc.trajectory(sds['cuda'], x, cond, setting, F64, 'cuda', lens)
        dev32 = pc.deviations(pc.trajectory(sds['cuda'], x, cond, setting, F32, 'cuda', lens), want, lens)
        rec = pc.load_yardsticks().get(pc.setting_name(setting), {}).get(pc.case_name(B, T, lens))
        assert (rec is not None) == pc.on_cpu(setting, B, T, ragged), (key, 'tests/golden/plms_yardsticks.json is stale: tools/plms_yardsticks.py')
        _REF[key] = dict(x=x, cond=cond, lens=lens, want=want, dev32=dev32, cpu32=rec, bar=pc.bar(setting))
    return _REF[key]


def _sample(model, setting, x, cond, lens=None):
    """One sampler call under the setting; (x_0 as float64 numpy, last_path).  No warning may fire and no hand-off may give up."""
    timesteps, K_step, interval = setting
    assert model.num_timesteps == timesteps
    xd = x.cuda().contiguous()
    hparams['pndm_speedup'], model.K_step = interval, K_step
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            out = model.sample(cond.cuda().contiguous(), xd, lengths=lens)
            torch.cuda.synchronize()
            path = model.denoise_fn.last_path()
            model.last_plms_launch = model.denoise_fn.last_launch()      # (chains, launch groups) of this call, read from the handle
    finally:
        hparams['pndm_speedup'], model.K_step = 0, timesteps
    assert not caught, [str(w.message) for w in caught]
    assert model.denoise_fn.handoff_timeouts() == 0
    return out.double().cpu().numpy(), path


def _case(models, sds, setting, B, T, ragged=False):
    key = (setting, B, T, ragged)
    if key not in _CASES:
        ref = _ref(sds, setting, B, T, ragged)
        got, path = _sample(models[setting[0]], setting, ref['x'].clone(), ref['cond'], ref['lens'])
        rec = dict(path=path, launch=models[setting[0]].last_plms_launch, finite=bool(np.isfinite(got).all()),
                   dev=pc.deviations(got, ref['want'], ref['lens']),
                   got=got if ((B, T) in pc.SHORT_LIST or ragged or (B, T) == pc.SHORT_EDGE[0]) else None)
        _CASES[key] = rec
        f = lambda v: ' / '.join(f'{a:.2e}' for a in v[:3])
        ratio = rec['dev'][0] / ref['dev32'][0] if ref['dev32'][0] else float('nan')
        print(f"\nplms {pc.setting_name(setting)} {pc.case_name(B, T, ref['lens'])}: hip {f(rec['dev'])} | fp32 oracle on the GPU {f(ref['dev32'])}"
              + (f" on the CPU {f(ref['cpu32'])}" if ref['cpu32'] else '') + f" | bar {ref['bar']:.2e} | hip / fp32 {ratio:.2f}"
              + (' (> 2)' if ratio > 2 else '') + f" | max |want| {np.abs(ref['want']).max():.1f} | {path}, chains / groups {rec['launch']} | {time.time() - _T0:.0f} s")
    return _CASES[key], _REF[key]


def _assert_parity(tag, rec, ref):
    assert rec['finite'], tag
    for name, dev in zip(('whole batch', 'row ends', 'tile seams'), rec['dev']):
        assert dev <= ref['bar'], (tag, name, dev, ref['bar'], rec['path'])


def test_device_float64_equals_cpu(sds):
    """What 'adds no term to the bound' rests on: the float64 reference evaluated by torch on the GPU is the one of the CPU, to 1e-12."""
    x, cond = pc.inputs(2, 31)
    cpu = pc.trajectory(sds['cpu'], x, cond, pc.MAIN, F64)
    dev = pc.trajectory(sds['cuda'], x, cond, pc.MAIN, F64, 'cuda')
    d = float(np.abs(cpu - dev).max())
    print(f'\nfloat64 oracle trajectory 2x31 at 100 / 5, GPU against CPU: {d:.2e} (max |x| {np.abs(cpu).max():.1f})')
    assert d <= 1e-12


@pytest.mark.parametrize('B,T', pc.SHAPES)
def test_default_path_vs_fp64(B, T, models, sds):
    rec, ref = _case(models, sds, pc.MAIN, B, T)
    _assert_parity(f'100/5 {B}x{T}', rec, ref)
    assert rec['path'].startswith('stack_h2'), rec['path']      # the default path is a split-fp16 stack launch at every shape of the list


REQUIRED = ['stack_h2_quad', 'stack_h2_quad64', 'stack_h2_pair64', 'stack_h2q_tail']


def test_default_path_covers_every_launch_form(models, sds):
    """The union of last_path over SHAPES holds every form of the default path, the tail form with one launch group (B x ceil(T / 64) tiles
    <= CUs) and with several, the count read from the handle; cases the parametrised test has run are taken from its record.  The
    half-batch chains are no form of the default path (every shape has a stack plan and runs as one chain, asserted here); they are
    required of test_fallback_and_switch_forms_vs_fp64, under the per-layer launches."""
    cases = {s: _case(models, sds, pc.MAIN, *s)[0] for s in pc.SHAPES}
    reached = {}
    for (B, T), r in cases.items():
        reached.setdefault(r['path'], []).append((B, T))
        if r['path'] == 'stack_h2q_tail':      # the group count is the handle's (bsg_diffnet_last_launch), not plan_stack's arithmetic restated
            assert r['launch'][1] >= 1, (B, T, r['launch'])
            reached.setdefault('stack_h2q_tail, one launch group' if r['launch'][1] == 1 else 'stack_h2q_tail, several launch groups', []).append((B, T))
        assert r['launch'][0] == 1, (B, T, r['launch'])      # a stack plan: dual_fork leaves it alone
    print('\nforms reached:')
    for k, v in sorted(reached.items()):
        print(f'  {k}: {v}')
    print('  10 x 900, 5 x 1000, 8 x 1000, 7 x 129 ran as', [cases[s]['path'] for s in ((10, 900), (5, 1000), (8, 1000), (7, 129))],
          '(a stack form: one chain, dual_fork needs a plan without a stack form)')
    missing = [f for f in REQUIRED + ['stack_h2q_tail, one launch group', 'stack_h2q_tail, several launch groups'] if f not in reached]
    assert not missing, f'launch forms no shape reached: {missing}; reached {sorted(reached)}'


@pytest.mark.parametrize('B,T', pc.EDGE_SHAPES)
@pytest.mark.parametrize('K_step,interval', pc.EDGES)
def test_history_depth_and_schedule_edges_vs_fp64(K_step, interval, B, T, models, sds):
    setting = (100, K_step, interval)
    rec, ref = _case(models, sds, setting, B, T)
    _assert_parity(f'{K_step}/{interval} {B}x{T}', rec, ref)
    moved = float(np.abs(ref['want'] - ref['x'].double().numpy()).max())
    assert (moved == 0.0) == (K_step <= interval), (K_step, interval, moved)      # a single iteration at i = 0 leaves x_T; every other loop moves x


@pytest.mark.parametrize('B,T', pc.SHIPPED_SHAPES)
def test_shipped_schedule_vs_fp64(B, T, models, sds):
    rec, ref = _case(models, sds, pc.SHIPPED, B, T)
    _assert_parity(f'1000/5 {B}x{T}', rec, ref)


def test_ragged_vs_fp64(models, sds):
    rec, ref = _case(models, sds, pc.MAIN, pc.RAGGED_B, pc.RAGGED_T, True)
    _assert_parity('ragged', rec, ref)
    assert rec['path'] == 'stack_h2q_ragged_tail', rec['path']
    x = ref['x'].double().numpy()
    for b, n in enumerate(ref['lens']):
        assert np.array_equal(rec['got'][b, :, :, n:], x[b, :, :, n:]), f'row {b}: x beyond its {n} frames was written'


# ------------------------------------------------------------------------------------------------------------------
# the fallback and switch forms, one child process per switch set
# ------------------------------------------------------------------------------------------------------------------
CHILD = r'''
import sys, json, warnings, torch, numpy as np
sys.path.insert(0, %r)
from tests import plms_cases as pc
from tests import test_gpu_plms_shapes as me
torch.set_grad_enabled(False)
model = me._build(100)
out = {}
for tag, setting, B, T in json.loads(sys.argv[2]):
    x, cond = pc.inputs(B, T)
    got, path = me._sample(model, tuple(setting), x, cond)
    np.save(sys.argv[1] + '/' + tag + '.npy', got)
    out[tag] = [path, list(model.last_plms_launch)]
print(json.dumps(out))
''' % ROOT

SWITCH_SETS = [
    ('h2_32row', {'BSG_H2_Q': '0'}),                       # 32-row launch and its tail
    ('no_part', {'BSG_H2_PART': '0'}),                     # one workgroup per tile at small B; also reaches NCT = 1
    ('tail_own_launch', {'BSG_H2_TAIL': '0'}),             # the tail as its own launch
    ('no_fused_tail', {'BSG_NO_FUSED_TAIL': '1'}),         # every iteration through plms_step_kernel
    ('f43', {'BSG_H2': '0'}),                              # F(4,3) / per-layer forms with step_tail_kernel<.., true>
    ('f23', {'BSG_H2': '0', 'BSG_WINO': '1'}),             # per-layer F(2,3) launches: the half-batch chains at 16 x 1000
    ('no_dual', {'BSG_DUAL': '0'}),
    ('f23_no_dual', {'BSG_H2': '0', 'BSG_WINO': '1', 'BSG_DUAL': '0'}),      # the same launches in one chain
]
BITS_ONLY = ('no_fused_tail',)      # a switch that keeps last_path: its effect is looked for in the output bits


def test_fallback_and_switch_forms_vs_fp64(tmp_path, models, sds):
    """Each set against the float64 references and the bars of the default path, at the short list at 100 / 5 and (15, 5) at 3 x 77;
    nothing is started after a child that failed.  A set must have changed last_path on some shape, or (no_fused_tail) the output bits.
    BSG_DUAL's effect is the chain count, which the handle reports (DiffNet.last_launch): 2 under the per-layer launches at 16 x 1000,
    1 with BSG_DUAL=0 beside them and at every other shape; alone, on the default path, the switch must change nothing (every shape of
    the list has a stack plan, which dual_fork leaves alone).  Whether the chains change bits is printed: rows are independent."""
    jobs = [(f'{B}x{T}', pc.MAIN, B, T) for B, T in pc.SHORT_LIST] + [('edge', pc.SHORT_EDGE[1], *pc.SHORT_EDGE[0])]
    default = {tag: _case(models, sds, tuple(s), B, T) for tag, s, B, T in jobs}
    results = {}
    for name, env in SWITCH_SETS:
        d = tmp_path / name
        d.mkdir()
        res = subprocess.run([sys.executable, '-c', CHILD, str(d), json.dumps(jobs)], env=dict(os.environ, **env), capture_output=True,
                             text=True, timeout=600)
        assert res.returncode == 0, (name, res.stderr[-2000:])
        paths = json.loads(res.stdout.strip().splitlines()[-1])
        changed_path, changed_bits = [], []
        for tag, s, B, T in jobs:
            rec0, ref = default[tag]
            got = np.load(str(d / f'{tag}.npy'))
            rec = dict(path=paths[tag][0], launch=tuple(paths[tag][1]), finite=bool(np.isfinite(got).all()), dev=pc.deviations(got, ref['want']),
                       got=got)
            print(f"\nplms {name} {pc.setting_name(tuple(s))} {B}x{T}: hip {' / '.join('%.2e' % v for v in rec['dev'])} | fp32 oracle "
                  f"{ref['dev32'][0]:.2e} | bar {ref['bar']:.2e} | {rec['path']}, chains / groups {rec['launch']} (default {rec0['path']}, {rec0['launch']})")
            _assert_parity(f'{name} {tag}', rec, ref)
            if rec['path'] != rec0['path']:
                changed_path.append(tag)
            if not np.array_equal(got, rec0['got']):
                changed_bits.append(tag)
            results[(name, tag)] = rec
        print(f'  {name}: last_path changed at {changed_path}, bits changed at {changed_bits}')
        chains = {tag: results[(name, tag)]['launch'][0] for tag, *_ in jobs}
        if name == 'f23':
            # the only place of this file where the second half batch's history offsets (subs[1].off * M * T) are exercised: the fork
            # must have happened, and its result has just met the bar over the whole batch, rows of the second half included
            assert chains['16x1000'] == 2, ('half-batch chains not reached', chains)
        elif name == 'no_dual':
            # every shape of the list has a stack plan on the default path, which dual_fork leaves alone: the switch has nothing to take
            # there, and must change nothing
            assert not changed_path and not changed_bits and set(chains.values()) == {1}, (name, changed_path, changed_bits, chains)
        elif name == 'f23_no_dual':
            # ... its effect is asserted where the chains run: one chain instead of two at 16 x 1000, the same launches otherwise
            assert results[('f23', '16x1000')]['launch'][0] == 2 and set(chains.values()) == {1}, (name, chains)
            assert all(results[(name, tag)]['path'] == results[('f23', tag)]['path'] for tag, *_ in jobs)
            same = [tag for tag, *_ in jobs if np.array_equal(results[(name, tag)]['got'], results[('f23', tag)]['got'])]
            print(f'  f23 with and without the half-batch chains: bit-identical at {same}')
        elif name in BITS_ONLY:
            assert changed_bits, (name, 'the switch changed nothing')
        else:
            assert changed_path, (name, 'the switch changed no launch form')


def test_state_left_on_the_handle(models):
    """A long call leaves the history ring, xpred and xa full of another batch's values; a short call behind it on the same handle must be
    bit-identical to the same call on a fresh handle."""
    jobs = [(pc.MAIN, 16, 1000), ((100, 15, 5), 3, 77), ((100, 5, 5), 2, 5)]
    used = [_sample(models[100], s, *pc.inputs(B, T))[0] for s, B, T in jobs]
    for (s, B, T), got in list(zip(jobs, used))[1:]:
        fresh = _build(100)
        want = _sample(fresh, s, *pc.inputs(B, T))[0]
        fresh.denoise_fn.release()
        assert np.array_equal(got, want), (s, B, T, float(np.abs(got - want).max()))


@pytest.mark.parametrize('B,T', [(3, 77), (16, 1000)])
def test_plms_loop_replays_from_a_graph(models, B, T):
    """One PLMS call captured behind an eager warm-up, as test_sampler_loop_is_graph_capturable does for DDPM: three replays, each
    bit-identical to the eager result.  The default queue count is kept."""
    model = models[100]
    x0, cond = pc.inputs(B, T)
    x0, cond = x0.cuda(), cond.cuda()
    hparams['pndm_speedup'] = 5
    try:
        eager = model.sample(cond, x0.clone()).clone()
        torch.cuda.synchronize()
        eager_path = model.denoise_fn.last_path()
        xg = x0.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                model.sample(cond, xg)
            assert model.denoise_fn.last_path() == eager_path
        torch.cuda.current_stream().wait_stream(side)
        for _ in range(3):
            xg.copy_(x0)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(xg, eager)
    finally:
        hparams['pndm_speedup'] = 0
    assert model.denoise_fn.take_handoff_timeouts() == 0
