"""GPU parity of the DDPM sampler (bsg_ddpm_sample, the loop that bench.py, configs[0] and the ragged decoder run) on every form of its
step tail, against the float64 evaluation of the CPU oracle: oracle.diffusion.p_sample over oracle.diffnet.diffnet_forward(dtype=float64).
The DDPM twin of tests/test_gpu_plms_shapes.py.  What it exposed, and what was changed for it: a window of steps run as two calls was not
the same window run as one call, bit for bit (below: "What the sweep found"); bsg_ddpm_sample now computes a call's first input projection
with the arithmetic of the split-fp16 tails' head (in_proj_h2_kernel).  No tail and no stack launch was changed.

Why windows.  p_sample clamps x_recon to [-1, 1], and a clamped element's new x does not depend on eps.  From x_T ~ N(0, 1), 84 % of the
elements are clamped at t = 99 and 81 % at t = 90, so the suite's "10 sampler steps from t = 99" hide a wrong halo, tile seam or row offset
in eps on four elements of five.  A case here is a window of six steps from a scaled x at a step where eps reaches x (tests/ddpm_cases.py):
LOW t = 5 .. 0 (ends in the sigma[0] = 0 step, no head), MID t = 40 .. 35 (last step with noise and no head), clamp share <= 0.10 / 0.20 at
every step, a CONDITION asserted on the CPU record and here again on the reference this test computes.  HIGH t = 99 .. 94 is the clamp
branch itself (share 0.83) and EXEMPT from the cap, which is why it cannot stand alone: it runs at 3 x 77, 16 x 1000 and in the switch sets.

  * the shapes (plms_cases.SHAPES) x {LOW, MID} walk plan_stack's map; WHICH form ran is read from DiffNet.last_path() and last_launch()
    behind the call, never restated from thresholds; every call asserts handoff_timeouts() == 0 and that no range-guard warning fired;
  * API edges at 3 x 77 and 9 x 1000: n_steps = 0 leaves x bit for bit; one step at t = 0 (only the sigma = 0 step, no head) and at t = 99
    against float64 (windows T0, T99 with bars of their own); LOW in two calls (t = 5 .. 3, then 2 .. 0) meets the same bar, and is
    one call bit for bit (it was not before this file: below); steps below 0 or a start at or beyond the schedule's end
    are refused with x untouched;
  * ragged batches (stack_h2q_ragged_tail): B = 6, T = 200, lengths [200, 1, 63, 64, 65, 129] in LOW and MID, test_gpu_ragged.SAMPLE_LENS
    at T = 1000 (several launch groups) in LOW; every row against its own float64 window at T = len with the batch's noise sliced, x beyond
    every length bit-identical to the caller's;
  * Philox mode at 3 x 77, 5 x 333, 32 x 997 (T % 4 != 0: quads that straddle rows) and 16 x 1000 in MID, at row0 = 0 and at row0 = 2 of
    B + 2: the float64 reference is fed the device's own stream (bsg_philox_normal, stream id i + 1, offset row0 x 80 x T, one buffer per
    step); same bar; a second seed must move x by more than 1e-3.  Whether the in-kernel draw is bit-identical to the stand-alone kernel's
    (the supplied-noise call fed that buffer) is printed, not asserted;
  * the fallback and switch forms, one child process per set of test_gpu_plms_shapes.SWITCH_SETS: SHORT_LIST x {LOW, MID}, HIGH at 3 x 77,
    MID in Philox mode at 3 x 77 and 16 x 1000, against the same references and bars; nothing is started after a child that failed.  f23
    reaches the two half-batch chains at 16 x 1000, the only place where the second half's noise offset and quad_row0 are exercised;
  * state: MID at 16 x 1000, then LOW at 2 x 5 on the same handle, equals a fresh handle bit for bit.
  Every child has its own timeout; every in-process sampler call and reference runs under a watchdog that ends the process.  No retries.

Reference and bar.  Every supplied-noise case has the float64 and the fp32 oracle window computed on the CPU by tools/ddpm_yardsticks.py
BEFORE any kernel ran (tests/golden/ddpm_yardsticks.json; tests/test_ddpm_cases_cpu.py ties the file to the oracle and shows that each bar
catches 3e-4 planted in eps on one edge frame at any step).  The bar of a window is 4 x the largest whole-batch fp32-against-float64
deviation over the window's cases, in normalised units, the project's convention; row ends and tile seams meet the same number, and so do
the fallback forms and the Philox cases.  The float64 window itself is evaluated again by torch on the GPU inside this test
(test_gpu_plms_shapes.test_device_float64_equals_cpu holds that evaluation to the CPU's to 1e-12); the fp32 figure beside it is printed.

Yardsticks computed on the CPU (fp32 oracle against float64, whole batch; largest clamp share) and the bars they give:

  LOW   1 x 1 2.09e-7   2 x 5 2.20e-7   3 x 17 2.31e-7   2 x 31 2.32e-7   3 x 65 2.76e-7   3 x 77 2.98e-7   7 x 129 3.32e-7   1 x 1000 3.03e-7
        5 x 333 3.45e-7   2 x 1000 4.09e-7   1 x 2500 3.17e-7   4 x 1000 3.35e-7   5 x 1000 3.77e-7   8 x 1000 3.64e-7   9 x 1000 3.79e-7
        10 x 900 3.57e-7   16 x 1000 3.46e-7   20 x 777 3.65e-7   32 x 997 3.86e-7   ragged 6 x 200 3.37e-7   ragged 21 x 1000 3.78e-7
        clamp share <= 0.050 (cap 0.10), max |x| 1 (the t = 0 step returns the clamped x_recon) .. 2.4                -> bar 1.64e-6
  MID   1 x 1 1.36e-7   2 x 5 2.08e-7   3 x 17 3.00e-7   2 x 31 3.46e-7   3 x 65 3.61e-7   3 x 77 3.49e-7   7 x 129 3.73e-7   1 x 1000 3.81e-7
        5 x 333 4.26e-7   2 x 1000 4.46e-7   1 x 2500 4.30e-7   4 x 1000 4.37e-7   5 x 1000 4.11e-7   8 x 1000 4.71e-7   9 x 1000 4.20e-7
        10 x 900 4.54e-7   16 x 1000 4.63e-7   20 x 777 4.57e-7   32 x 997 4.92e-7   ragged 6 x 200 3.89e-7
        clamp share <= 0.144 (cap 0.20; the batch's own elements: the 80 elements of the ragged batch's 1-frame row alone reach 0.225),
        max |x| 1.3 .. 2.6                                                                                          -> bar 1.97e-6
  HIGH  3 x 77 7.46e-7   16 x 1000 1.02e-6   clamp share 0.83 (exempt), max |x| 4.8                                  -> bar 4.07e-6
  T0    3 x 77 7.78e-8   9 x 1000 8.83e-8    clamp share 0.045                                                       -> bar 3.53e-7
  T99   3 x 77 3.33e-7   9 x 1000 4.69e-7    clamp share 0.83                                                        -> bar 1.88e-6
  planted 3e-4 in eps on the last frame of 3 x 77 moves x_final by 3.0e-6 (the t = 0 step) .. 9.7e-6 in LOW, 1.14e-5 .. 1.25e-5 in MID

Every case prints "ddpm <window> <B>x<T>: hip whole / ends / seams | fp32 oracle on the GPU (and the CPU record) | bar | hip / fp32 |
clamp share | max |want| | the form read from last_path, chains / launch groups".  The HIP side (figure per window, the worst hip / fp32
ratio, the forms reached), copied from the printed lines of an MI355X run:

  window          default path (worst case)        hip / fp32 (worst)   fallback and switch forms (worst)
  LOW             3.57e-7 (20 x 777)               1.09 (1 x 1000)      3.40e-7 (f23 16 x 1000)
  MID             4.92e-7 (32 x 997)               1.00                 4.84e-7 (no_fused_tail 16 x 1000)
  MID, Philox     5.59e-7 (16 x 1000, row0 = 2)    1.01                 4.23e-7
  HIGH            1.02e-6 (16 x 1000)              1.00                 7.46e-7 (3 x 77)
  T0 / T99        8.40e-8 / 4.69e-7 (9 x 1000)     1.00
  ragged          LOW 2.61e-7 (6 x 200) 3.89e-7 (21 x 1000, 2 launch groups)   MID 3.89e-7 (6 x 200)    hip / fp32 <= 1.10
  No ratio exceeds 2.  In MID, HIGH and T99 the HIP figure IS the fp32 oracle's to three digits: the largest deviation sits on an element
  of large |x| and is the rounding of mean + sigma x noise in fp32, which the tails evaluate in the oracle's order; the eps error below it
  does not show in the maximum.  What the bar is worth is therefore what the planted error says, not the ratio.
  Forms reached on the default path, in LOW and in MID alike: stack_h2_quad (1 x 1 .. 2 x 1000, 7 x 129), stack_h2_quad64 (4 x 1000,
  1 x 2500), stack_h2_pair64 (5 x 1000, 8 x 1000), stack_h2q_tail with one launch group (9 x 1000, 16 x 1000, 10 x 900) and with two
  (20 x 777, 32 x 997), stack_h2q_ragged_tail with one and two groups; always one chain.  Under the switches: h2_32row stack_h2_tail;
  no_part stack_h2q_tail at every shape; tail_own_launch and no_fused_tail stack_h2q at 16 x 1000 (bits change at every shape); f43
  stack_f43 / split4; f23 split4 / layer with 2 chains at 16 x 1000 in LOW, MID and Philox mode, bit-identical to f23_no_dual's one
  chain at every case; no_dual changes neither path nor bits.
  The in-kernel Philox draw was bit-identical to the supplied-noise call fed bsg_philox_normal's buffer at all four shapes, row0 = 0 and 2.

What the sweep found.  LOW in two calls (t = 5 .. 3, then 2 .. 0) was NOT one call bit for bit on the fused loop: max |two calls - one
call| 1.19e-7 at 3 x 77 (stack_h2_quad), 1.79e-7 at 9 x 1000 (stack_h2q_tail), with both inside the float64 bar and the unfused loop
(BSG_NO_FUSED_TAIL=1) bit-identical.  Cause: a call's FIRST input projection was the generic GEMM (conv1x1), every later one is the head of
the previous step's tail (the hi / lo planes of the updated x against the tail's fragments, six k-steps on the 16-bit matrix pipe: another
summation order), and the second call starts where the one call's third tail had its head.  Fix: in front of the split-fp16 tails (inside
the stack launch, or step_tail_h2_kernel behind a part launch) bsg_ddpm_sample projects the first x with in_proj_h2_kernel, the head's
GEMM on its own; the two calls are now one call bit for bit at both shapes (0.0 printed), and every figure above is from the run with it.
In front of the fp32-pipe and bf16 tails the first projection is still the generic GEMM; two calls there agree with one to rounding.
"""
import contextlib
import faulthandler
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np
import pytest
import torch

from bisinger_amd import _lib
from bisinger_amd.hparams import hparams
from tests import ddpm_cases as dc
from tests import plms_cases as pc
from tests import test_gpu_plms_shapes as plms
from tests.util import ROOT, cpu_sd

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

F64, F32 = torch.float64, torch.float32
CALL_LIMIT = 120      # seconds a sampler call may take before the watchdog ends the process (a call of this file takes well under one)
REF_LIMIT = 300       # ... and a reference (twelve oracle evaluations by torch on the GPU, row by row for a ragged batch)
CHILD_LIMIT = 600
_REF = {}             # (window, case name) -> references
_CASES = {}           # (window, case name) -> figures of the default path
_PHILOX = {}          # (B, T, row0) -> reference fed the device's own stream, and the default path's result
_T0 = time.time()


@contextlib.contextmanager
def _limit(seconds):
    """A hang must end the run, not wait for whoever started it: past `seconds` every thread's traceback is written and the process exits."""
    faulthandler.dump_traceback_later(seconds, exit=True, file=sys.__stderr__)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope='module')
def model():
    """GaussianDiffusion over the WaveNet denoiser on the formula weights, 100 steps to beta 0.06, as test_gpu_plms_shapes builds it."""
    return plms._build(100)


@pytest.fixture(scope='module')
def sds(model):
    sd = cpu_sd(model)
    return {'cpu': sd, 'cuda': {k: v.cuda() for k, v in sd.items()}}


def _sample(model, window, x, cond, noise=None, lens=None, steps=None, **kw):
    """One sampler call over the window's steps (or `steps` = (t_start, n)) from a copy of x; (x as float64 numpy, last_path,
    (chains, launch groups)).  No warning may fire and no hand-off may give up."""
    t_start, n = dc.WINDOWS[window][:2] if steps is None else steps
    xd = x.detach().clone().cuda().contiguous()
    hparams['pndm_speedup'] = 0
    model.K_step = t_start + 1
    try:
        with _limit(CALL_LIMIT), warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            out = model.sample(cond.cuda().contiguous(), xd, noise=None if noise is None else noise.cuda().contiguous(), n_steps=n,
                               lengths=lens, **kw)
            torch.cuda.synchronize()
            path, launch = model.denoise_fn.last_path(), model.denoise_fn.last_launch()
    finally:
        model.K_step = model.num_timesteps
    assert not caught, [str(w.message) for w in caught]
    assert model.denoise_fn.handoff_timeouts() == 0
    return out.double().cpu().numpy(), path, tuple(launch)


def _reference(sds, window, x, cond, noise, lens=None):
    """(float64 window, the fp32 oracle's deviations from it, the largest clamp share), evaluated by torch on the GPU; the cap of the
    window is asserted on this reference."""
    with _limit(REF_LIMIT):
        want, shares = dc.reference(sds['cuda'], window, x, cond, noise, F64, 'cuda', lens)
        dev32 = pc.deviations(dc.reference(sds['cuda'], window, x, cond, noise, F32, 'cuda', lens)[0], want, lens)
    if window in dc.CLAMP_CAP:
        assert max(shares) <= dc.CLAMP_CAP[window], (window, shares)
    return want, dev32, max(shares)


def _ref(sds, window, B, T, ragged=None):
    key = (window, dc.case_name(B, T, ragged is not None))
    if key not in _REF:
        x, cond, noise = dc.inputs(window, B, T)
        want, dev32, clamp = _reference(sds, window, x, cond, noise, ragged)
        rec = dc.load_yardsticks()[window].get(key[1])
        assert rec is not None, (key, 'tests/golden/ddpm_yardsticks.json is stale: tools/ddpm_yardsticks.py')
        _REF[key] = dict(x=x, cond=cond, noise=noise, lens=ragged, want=want, dev32=dev32, clamp=clamp, cpu32=rec['dev'], bar=dc.bar(window))
    return _REF[key]


def _line(tag, rec, ref):
    f = lambda v: ' / '.join(f'{a:.2e}' for a in v[:3])
    ratio = rec['dev'][0] / ref['dev32'][0] if ref['dev32'][0] else float('nan')
    print(f"\nddpm {tag}: hip {f(rec['dev'])} | fp32 oracle on the GPU {f(ref['dev32'])}" + (f" on the CPU {f(ref['cpu32'])}" if ref.get('cpu32') else '')
          + f" | bar {ref['bar']:.2e} | hip / fp32 {ratio:.2f}" + (' (> 2)' if ratio > 2 else '') + f" | clamp share {ref['clamp']:.3f}"
          + f" | max |want| {np.abs(ref['want']).max():.2f} | {rec['path']}, chains / groups {rec['launch']} | {time.time() - _T0:.0f} s")


def _record(got, path, launch, ref):
    return dict(path=path, launch=launch, finite=bool(np.isfinite(got).all()), dev=pc.deviations(got, ref['want'], ref.get('lens')), got=got)


def _case(model, sds, window, B, T, ragged=None):
    key = (window, dc.case_name(B, T, ragged is not None))
    if key not in _CASES:
        ref = _ref(sds, window, B, T, ragged)
        _CASES[key] = _record(*_sample(model, window, ref['x'], ref['cond'], ref['noise'], ragged), ref)
        _line(' '.join(key), _CASES[key], ref)
    return _CASES[key], _REF[key]


def _assert_parity(tag, rec, ref):
    assert rec['finite'], tag
    for name, dev in zip(('whole batch', 'row ends', 'tile seams'), rec['dev']):
        assert dev <= ref['bar'], (tag, name, dev, ref['bar'], rec['path'])


# ------------------------------------------------------------------------------------------------------------------
# the default path
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,T', pc.SHAPES)
@pytest.mark.parametrize('window', dc.SWEEP)
def test_default_path_vs_fp64(window, B, T, model, sds):
    rec, ref = _case(model, sds, window, B, T)
    _assert_parity(f'{window} {B}x{T}', rec, ref)
    assert rec['path'].startswith('stack_h2'), rec['path']      # the default path is a split-fp16 stack launch at every shape of the list


def test_default_path_covers_every_launch_form(model, sds):
    """The union of last_path over SHAPES x {LOW, MID} holds every form of the default path, the tail form with one launch group and with
    several, the count read from the handle; cases the parametrised test has run are taken from its record."""
    reached = {}
    for window in dc.SWEEP:
        for B, T in pc.SHAPES:
            r = _case(model, sds, window, B, T)[0]
            names = [r['path']]
            if r['path'] == 'stack_h2q_tail':
                assert r['launch'][1] >= 1, (B, T, r['launch'])
                names.append('stack_h2q_tail, one launch group' if r['launch'][1] == 1 else 'stack_h2q_tail, several launch groups')
            for name in names:
                reached.setdefault((window, name), []).append((B, T))
            assert r['launch'][0] == 1, (B, T, r['launch'])      # a stack plan: dual_fork leaves it alone
    print('\nforms reached:')
    for k, v in sorted(reached.items()):
        print(f'  {k[0]} {k[1]}: {v}')
    required = plms.REQUIRED + ['stack_h2q_tail, one launch group', 'stack_h2q_tail, several launch groups']
    missing = [(w, f) for w in dc.SWEEP for f in required if (w, f) not in reached]
    assert not missing, f'launch forms no shape reached: {missing}; reached {sorted(reached)}'


@pytest.mark.parametrize('B,T', dc.HIGH_SHAPES)
def test_high_window_vs_fp64(B, T, model, sds):
    """The clamp branch and the largest coefficients.  Most of x_recon is clamped here (asserted), so this window says little about eps."""
    rec, ref = _case(model, sds, 'HIGH', B, T)
    _assert_parity(f'HIGH {B}x{T}', rec, ref)
    assert ref['clamp'] > 0.5, ref['clamp']


# ------------------------------------------------------------------------------------------------------------------
# API edges
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,T', dc.EDGE_SHAPES)
def test_zero_steps_leave_x(B, T, model):
    x, cond, _ = dc.inputs('LOW', B, T)
    for t_start in (5, 0, 99):
        got, _, _ = _sample(model, 'LOW', x, cond, steps=(t_start, 0))
        assert np.array_equal(got, x.double().numpy()), t_start


@pytest.mark.parametrize('B,T', dc.EDGE_SHAPES)
@pytest.mark.parametrize('window', ['T0', 'T99'])
def test_single_step_vs_fp64(window, B, T, model, sds):
    """One call of one step: do_head is false at once.  At t = 0 sigma is 0 and the draw must not reach x: the float64 window multiplies
    it by 0, and a second call with other draws gives the same bits."""
    rec, ref = _case(model, sds, window, B, T)
    _assert_parity(f'{window} {B}x{T}', rec, ref)
    other = _sample(model, window, ref['x'], ref['cond'], -3.0 * ref['noise'])[0]
    assert np.array_equal(other, rec['got']) == (window == 'T0'), window


def _two_calls(model, ref):
    """LOW as t = 5 .. 3, then t = 2 .. 0 from the first call's x: (x, the two paths)."""
    half, path1, _ = _sample(model, 'LOW', ref['x'], ref['cond'], ref['noise'][:3], steps=(5, 3))
    got, path2, launch = _sample(model, 'LOW', torch.from_numpy(half).float(), ref['cond'], ref['noise'][3:], steps=(2, 3))
    return got, path1, path2, launch


@pytest.mark.parametrize('B,T', dc.EDGE_SHAPES)
def test_window_in_two_calls_vs_fp64(B, T, model, sds):
    """What holds of a window in two calls on every form: the same float64 window within the same bar."""
    one, ref = _case(model, sds, 'LOW', B, T)
    got, path1, path2, launch = _two_calls(model, ref)
    assert path1 == path2 == one['path']
    rec = _record(got, path2, launch, ref)
    _line(f'LOW {B}x{T} in two calls', rec, ref)
    _assert_parity(f'LOW {B}x{T} in two calls', rec, ref)


@pytest.mark.parametrize('B,T', dc.EDGE_SHAPES)
def test_window_in_two_calls_is_one_call(B, T, model, sds):
    """A call that continues where another stopped computes what one call over all the steps computes.  Before in_proj_h2_kernel this
    failed by 1.19e-7 at 3 x 77 (stack_h2_quad) and 1.79e-7 at 9 x 1000 (stack_h2q_tail): a call's first input projection was the
    generic GEMM, every later one the head of the previous step's tail, which sums in another order (the module docstring)."""
    one, ref = _case(model, sds, 'LOW', B, T)
    got = _two_calls(model, ref)[0]
    d = float(np.abs(got - one['got']).max())
    print(f"\nddpm LOW {B}x{T} as t = 5 .. 3, then 2 .. 0: max |two calls - one call| {d:.2e} ({one['path']})")
    assert np.array_equal(got, one['got']), d


TWO_CALLS_CHILD = r'''
import sys, json, torch, numpy as np
sys.path.insert(0, %r)
from tests import ddpm_cases as dc
from tests import test_gpu_ddpm_shapes as me
torch.set_grad_enabled(False)
model = me.plms._build(100)
out = {}
for B, T in dc.EDGE_SHAPES:
    x, cond, noise = dc.inputs('LOW', B, T)
    one, path, _ = me._sample(model, 'LOW', x, cond, noise)
    two = me._two_calls(model, dict(x=x, cond=cond, noise=noise))[0]
    out['%%dx%%d' %% (B, T)] = [path, float(np.abs(two - one).max()), bool(np.array_equal(two, one))]
print(json.dumps(out))
''' % ROOT


def test_two_calls_are_one_call_in_the_unfused_loop():
    """BSG_NO_FUSED_TAIL=1: forward_impl + ddpm_step_kernel per step, every input projection by the same launch.  The per-step slice of
    the supplied noise, the coefficients of the steps and the start of a call then leave no other difference: bit-identical."""
    res = subprocess.run([sys.executable, '-c', TWO_CALLS_CHILD], env=dict(os.environ, BSG_NO_FUSED_TAIL='1'), capture_output=True, text=True,
                         timeout=CHILD_LIMIT)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    print('\nunfused loop, LOW in two calls against one call [path, max |diff|, bit-identical]:', out)
    assert len(out) == len(dc.EDGE_SHAPES) and all(v[2] for v in out.values()), out


@pytest.mark.parametrize('B,T', dc.EDGE_SHAPES)
def test_refusals(B, T, model, sds):
    rec, ref = _case(model, sds, 'LOW', B, T)
    xd, cond, noise = ref['x'].cuda(), ref['cond'].cuda(), ref['noise'].cuda()
    keep = xd.clone()
    try:
        for K_step in (3, 5, 101, 150):      # steps 2 .. -3 and 4 .. -1; a start at and beyond the schedule's end
            model.K_step = K_step
            with pytest.raises(_lib.BsgError, match='outside the schedule'):
                model.sample(cond, xd, noise=noise, n_steps=6)
            torch.cuda.synchronize()
            assert torch.equal(xd, keep), K_step
    finally:
        model.K_step = model.num_timesteps
    assert np.array_equal(_sample(model, 'LOW', ref['x'], ref['cond'], ref['noise'])[0], rec['got'])      # the handle is as good as before


# ------------------------------------------------------------------------------------------------------------------
# ragged batches
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,window', [(n, w) for n, c in dc.RAGGED.items() for w in c[3]])
def test_ragged_vs_fp64(name, window, model, sds):
    from tests import test_gpu_ragged
    assert dc.SAMPLE_LENS == test_gpu_ragged.SAMPLE_LENS
    B, T, lens, _ = dc.RAGGED[name]
    rec, ref = _case(model, sds, window, B, T, lens)
    _assert_parity(f'{window} {name}', rec, ref)
    assert rec['path'] == 'stack_h2q_ragged_tail', rec['path']
    if name == '21x1000r':
        assert rec['launch'][1] > 1, rec['launch']      # several launch groups, read from the handle
    x = ref['x'].double().numpy()
    for b, n in enumerate(lens):
        assert np.array_equal(rec['got'][b, :, :, n:], x[b, :, :, n:]), f'row {b}: x beyond its {n} frames was written'


# ------------------------------------------------------------------------------------------------------------------
# Philox mode
# ------------------------------------------------------------------------------------------------------------------
def _philox_ref(model, sds, B, T, row0):
    """The float64 MID window fed the device's own stream: one buffer per step from bsg_philox_normal at stream id i + 1, offset
    row0 x 80 x T."""
    key = (B, T, row0)
    if key not in _PHILOX:
        t_start, n, _ = dc.WINDOWS['MID']
        x, cond, _ = dc.inputs('MID', B, T)
        noise = torch.stack([model.philox_normal((B, 80, T), 'cuda', dc.PHILOX_SEEDS[0], t_start - k + 1, row0 * 80 * T) for k in range(n)]).cpu()
        want, dev32, clamp = _reference(sds, 'MID', x, cond, noise)
        _PHILOX[key] = dict(x=x, cond=cond, noise=noise, want=want, dev32=dev32, clamp=clamp, bar=dc.bar('MID'))
    return _PHILOX[key]


@pytest.mark.parametrize('B,T', dc.PHILOX_SHAPES)
def test_philox_mode_vs_fp64(B, T, model, sds):
    for row0 in (0, 2):
        ref = _philox_ref(model, sds, B, T, row0)
        kw = dict(seed=dc.PHILOX_SEEDS[0], row0=row0, B_total=B + row0)
        rec = _record(*_sample(model, 'MID', ref['x'], ref['cond'], **kw), ref)
        fed = _sample(model, 'MID', ref['x'], ref['cond'], ref['noise'])[0]
        _line(f'MID {B}x{T} philox row0 = {row0}', rec, ref)
        print(f"  the in-kernel draw against the supplied-noise call fed bsg_philox_normal's buffer: "
              + ('bit-identical' if np.array_equal(fed, rec['got']) else f"max |diff| {np.abs(fed - rec['got']).max():.2e}"))
        _assert_parity(f'MID {B}x{T} philox row0 = {row0}', rec, ref)
        if row0 == 0:
            ref['default'] = rec
            other = _sample(model, 'MID', ref['x'], ref['cond'], seed=dc.PHILOX_SEEDS[1])[0]
            assert float(np.abs(other - rec['got']).max()) > 1e-3
        else:
            assert float(np.abs(rec['got'] - _PHILOX[(B, T, 0)]['default']['got']).max()) > 1e-3      # other rows of the stream


# ------------------------------------------------------------------------------------------------------------------
# the fallback and switch forms, one child process per switch set
# ------------------------------------------------------------------------------------------------------------------
CHILD = r'''
import sys, json, torch, numpy as np
sys.path.insert(0, %r)
from tests import ddpm_cases as dc
from tests import test_gpu_ddpm_shapes as me
torch.set_grad_enabled(False)
model = me.plms._build(100)
out = {}
for tag, window, B, T, philox in json.loads(sys.argv[2]):
    x, cond, noise = dc.inputs(window, B, T)
    got, path, launch = me._sample(model, window, x, cond, seed=dc.PHILOX_SEEDS[0]) if philox else me._sample(model, window, x, cond, noise)
    np.save(sys.argv[1] + '/' + tag + '.npy', got)
    out[tag] = [path, list(launch)]
print(json.dumps(out))
''' % ROOT

SWITCH_PHILOX = [(3, 77), (16, 1000)]


def test_fallback_and_switch_forms_vs_fp64(tmp_path, model, sds):
    """Each set against the float64 references and the bars of the default path; nothing is started after a child that failed.  A set
    must have changed last_path on some case, or (no_fused_tail) the output bits.  f23 must reach 2 chains at 16 x 1000 in every window
    and in Philox mode: the second half's noise offset (noise + k n + mo) and quad_row0 have then met the bar over the whole batch.
    no_dual changes nothing on the default path; f23_no_dual runs f23's launches in one chain."""
    jobs = [(f'{w}_{B}x{T}', w, B, T, False) for w in dc.SWEEP for B, T in pc.SHORT_LIST] + [('HIGH_3x77', 'HIGH', 3, 77, False)]
    jobs += [(f'philox_{B}x{T}', 'MID', B, T, True) for B, T in SWITCH_PHILOX]
    default = {}
    for tag, w, B, T, philox in jobs:
        if philox:
            ref = _philox_ref(model, sds, B, T, 0)
            if 'default' not in ref:
                ref['default'] = _record(*_sample(model, 'MID', ref['x'], ref['cond'], seed=dc.PHILOX_SEEDS[0]), ref)
            default[tag] = (ref['default'], ref)
        else:
            default[tag] = _case(model, sds, w, B, T)
    results = {}
    for name, env in plms.SWITCH_SETS:
        d = tmp_path / name
        d.mkdir()
        res = subprocess.run([sys.executable, '-c', CHILD, str(d), json.dumps(jobs)], env=dict(os.environ, **env), capture_output=True,
                             text=True, timeout=CHILD_LIMIT)
        assert res.returncode == 0, (name, res.stderr[-2000:])
        paths = json.loads(res.stdout.strip().splitlines()[-1])
        changed_path, changed_bits = [], []
        for tag, *_ in jobs:
            rec0, ref = default[tag]
            rec = _record(np.load(str(d / f'{tag}.npy')), paths[tag][0], tuple(paths[tag][1]), ref)
            _line(f'{name} {tag}', rec, ref)
            print(f"  (default {rec0['path']}, {rec0['launch']})")
            _assert_parity(f'{name} {tag}', rec, ref)
            if rec['path'] != rec0['path']:
                changed_path.append(tag)
            if not np.array_equal(rec['got'], rec0['got']):
                changed_bits.append(tag)
            results[(name, tag)] = rec
        print(f'  {name}: last_path changed at {changed_path}, bits changed at {changed_bits}')
        chains = {tag: results[(name, tag)]['launch'][0] for tag, *_ in jobs}
        big = [tag for tag, _, B, T, _ in jobs if (B, T) == (16, 1000)]
        if name == 'f23':
            assert len(big) == 3 and all(chains[tag] == 2 for tag in big), ('half-batch chains not reached', chains)
        elif name == 'no_dual':
            assert not changed_path and not changed_bits and set(chains.values()) == {1}, (name, changed_path, changed_bits, chains)
        elif name == 'f23_no_dual':
            assert set(chains.values()) == {1}, (name, chains)
            assert all(results[(name, tag)]['path'] == results[('f23', tag)]['path'] for tag, *_ in jobs)
            same = [tag for tag, *_ in jobs if np.array_equal(results[(name, tag)]['got'], results[('f23', tag)]['got'])]
            print(f'  f23 with and without the half-batch chains: bit-identical at {same}')
        elif name in plms.BITS_ONLY:
            assert changed_bits, (name, 'the switch changed nothing')
        else:
            assert changed_path, (name, 'the switch changed no launch form')


# ------------------------------------------------------------------------------------------------------------------
# state
# ------------------------------------------------------------------------------------------------------------------
def test_state_left_on_the_handle(model):
    """A large call leaves xa, the skip sums and the hand-off flags full of another batch's values; a small call behind it on the same
    handle must be bit-identical to the same call on a fresh handle."""
    jobs = [('MID', 16, 1000), ('LOW', 2, 5)]
    used = [_sample(model, w, *dc.inputs(w, B, T))[0] for w, B, T in jobs]
    fresh = plms._build(100)
    w, B, T = jobs[1]
    want = _sample(fresh, w, *dc.inputs(w, B, T))[0]
    fresh.denoise_fn.release()
    assert np.array_equal(used[1], want), float(np.abs(used[1] - want).max())
