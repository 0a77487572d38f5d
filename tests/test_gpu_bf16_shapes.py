"""GPU: every launch form of the bf16-operand configuration (set_compute('bf16'), BASELINE configs[2]) at its tile seams and shape
edges, against the float64 evaluation of the rounding-emulating oracle (oracle.diffnet.diffnet_forward(operand_bf16=True, dtype=float64);
cases, inputs, classes and statistics: tests/bf16_cases.py).

Why per class.  A 1e-7 difference ahead of a bf16 rounding flips an operand by one ulp and the following layers carry the flip forward, so
two correct implementations agree only statistically and a whole-tensor bar has to sit above that noise; an error confined to the 16 frames
around a tile seam or to a row's last frames can hide under it.  The noise does not depend on position, a seam error does: every case is
judged per position class (start, end, seam, interior, all; `group` for the rows on both sides of a launch-group boundary) on two
statistics (rms; frame_max, the largest per-frame rms over the 80 bins), on short stacks (L = 1, 2, 5: far less chaotic) and the shipped one.

Reference and bar.  The reference is the emulation in float64, computed here on the CPU.  The yardstick is the SAME emulation in float32
against float64, computed on the CPU by tools/make_golden_bf16_yardsticks.py before any kernel ran (tests/golden/bf16_yardsticks.json; no
bar is taken from a HIP run); the bar is 4 x the yardstick per case, class and statistic, the margin tests/test_gpu_fs2_shapes.py and
tests/test_gpu_plms_shapes.py give a kernel over the oracle's own deviation.  That bar holds unchanged for every case whose record is
dense: L >= 5, the samplers, the ragged forms, the launch groups and the switch sets.

The exception (bf16_cases.bars, SPARSE_L): the single evaluations at L = 1 and L = 2.  There a class is held to 4 x the largest `all`
yardstick over the cases of the same L where that is larger than its own: L = 1: 4 x (4.86e-5 / 3.84e-4) = 1.94e-4 / 1.54e-3;
L = 2: 4 x (8.04e-5 / 3.76e-4) = 3.22e-4 / 1.50e-3.  In so short a stack the yardstick is a sample of a few flips: a flip of the
once-rounded skip sum moves one frame by 1e-4 .. 4e-4 rms, the float32 emulation flips in 1 .. 10 frames of a case, and the 16 .. 24
frames of `start` or `end` often hold none, so their record is plain float32 rounding (6e-8).  The kernel's flips fall elsewhere (its
gate runs on the hardware's exp2 / rcp ahead of the same roundings).  Measured on an MI355X, eval/L1/2x72, stack_bf16, 1 group
(class: HIP rms / frame_max | yardstick | ratio):
    start     4.45e-05 / 1.11e-04 | 5.80e-08 / 7.04e-08 | 768 / 1577      end    2.27e-07 / 8.96e-07 | 5.93e-08 / 7.33e-08 | 3.82 / 12.2
    seam      1.31e-05 / 5.25e-05 | 6.09e-08 / 7.67e-08 | 215 / 684       all    4.30e-05 / 2.59e-04 | 8.91e-06 / 1.07e-04 | 4.82 / 2.43
    interior  4.91e-05 / 2.59e-04 | 1.09e-05 / 1.07e-04 | 4.50 / 2.43
That case's float32 emulation flipped in exactly ONE frame (8.91e-6 = 1.07e-4 / sqrt(144)); the HIP figure is what the emulation shows
where it happened to flip more often (eval/L1/3x65: 4.86e-5), 11 x below what the roundings cost (4.98e-4) and 370 x below a halo slip
(1.6e-2 at L = 2).  Nothing is wrong there; against the pooled bar the largest figure of the case is 0.25 (interior rms).
tests/test_oracle_golden.py::test_bf16_bars_catch_a_one_frame_halo_slip holds the bars of this file to a planted one-frame halo slip: it
exceeds them in the seam class by 46 x / 32 x (rms / frame_max) at L = 2 (pooled bars), 10.4 x / 15.8 x at L = 5 and 4.0 x / 7.7 x at
L = 20 (the class's own bars).

Every case asserts: last_path() is the form it names, a second call repeats bit for bit, handoff_timeouts() == 0, last_launch() gives the
group count the case is about, the outputs are finite.  Every test prints "bf16 <case> <class>: hip rms / frame_max | yardstick | ratio |
cost of the roundings | path, groups".

PLMS.  bsg_plms_sample runs its first iteration unfused (two evaluations through bsg_diffnet's own fp32 projections) and projects x
for the first fused iteration with the fp32 conv1x1, so the emulation takes tail_bf16 from the third evaluation and in_bf16 from the
fourth on (bf16_cases._emulate_rows), not "from the second" as in the DDPM loop.

Measured.  The lines above are the only MI355X figures this file has been seen to print; the full table (case, class, HIP |
yardstick | ratio, path, groups), the largest ratio and whether any other form deviates are still to be copied from the printed lines
of a complete run, and until then neither "nothing deviates" nor a further deviation is claimed.  No kernel and no launch was changed.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bisinger_amd.hparams import hparams
from tests import bf16_cases as bc
from tests.util import ROOT, cpu_sd, load_formula_weights

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

_NETS, _MODELS, _SDS, _REF, _GOT = {}, {}, {}, {}, {}


class _Enc:
    def __len__(self):
        return 65

    def pad(self):
        return 0


def sd_of(L):
    if L not in _SDS:
        _SDS[L] = bc.state_dict(L)
    return _SDS[L]


def net_of(L):
    """DiffNet of L layers in the bf16 configuration."""
    if L not in _NETS:
        _NETS[L] = bc.build_net(L).cuda()
        _NETS[L].set_compute('bf16')
    return _NETS[L]


def model_of(L):
    """GaussianDiffusion (100 steps to beta 0.06) over a DiffNet of L layers in the bf16 configuration, on the weights of bc.state_dict."""
    if L not in _MODELS:
        from bisinger_amd import synth
        from bisinger_amd.diffusion import GaussianDiffusion
        m = GaussianDiffusion(_Enc(), 80, bc.build_net(L), timesteps=100, K_step=100, spec_min=hparams['spec_min'], spec_max=hparams['spec_max'])
        load_formula_weights(m, 0, synth.DIFFNET_GAIN)
        sd, want = cpu_sd(m), sd_of(L)
        assert all(torch.equal(sd[k], v) for k, v in want.items())
        m = m.cuda().eval()
        m.denoise_fn.set_compute('bf16')
        _MODELS[L] = m
    return _MODELS[L]


def run_case(case):
    """The HIP side of a case, twice -> (float64 numpy [B, 1, 80, T], last_path, launch groups, second call bit-identical, give-ups)."""
    inp, lens = bc.inputs(case), bc.lengths_of(case)
    x, cond = inp['x'].cuda(), inp['cond'].cuda()
    kind = case.kind.replace('ragged_', '')
    if kind in ('eval', 'eval_running', 'group'):
        net = net_of(case.L)
        call = lambda: net(x, inp['t'].cuda(), cond, lengths=lens).clone()
    else:
        m = model_of(case.L)
        net = m.denoise_fn
        noise = inp['noise'].cuda()

        def call():
            if kind == 'plms':
                keep = hparams.get('pndm_speedup'), m.K_step
                hparams['pndm_speedup'], m.K_step = bc.PLMS[2], bc.PLMS[1]
                try:
                    return m.sample(cond, x.clone(), lengths=lens).clone()
                finally:
                    hparams['pndm_speedup'], m.K_step = keep
            return m.sample(cond, x.clone(), noise=noise, n_steps=bc.DDPM_STEPS, lengths=lens).clone()
    a = call()
    torch.cuda.synchronize()
    path, groups = net.last_path(), net.last_launch()[1]
    b = call()
    torch.cuda.synchronize()
    return a.double().cpu().numpy(), path, groups, bool(torch.equal(a, b)), net.handoff_timeouts()


def reference(case):
    if case not in _REF:
        _REF[case] = bc.emulate(sd_of(case.L), case, bc.inputs(case), torch.float64)
    return _REF[case]


def judge(tag, case, got, path, groups, same, giveups, want_path, want_groups):
    """Print every figure, then assert the form, the repeat, the hand-offs, the group count, finiteness and every bar."""
    want, masks, rec = reference(case), bc.masks_of(case), bc.load_yardsticks()[bc.name(case)]
    dev, bars = bc.stats(got, want, masks), bc.bars(case)
    assert set(rec) == set(masks), (tag, 'tests/golden/bf16_yardsticks.json is stale: tools/make_golden_bf16_yardsticks.py')
    worst = 0.0
    for k in masks:
        y, c = rec[k]['yard'], rec[k]['cost']
        r = [dev[k][i] / y[i] if y[i] else float('inf') for i in (0, 1)]
        worst = max(worst, max(dev[k][i] / bars[k][i] for i in (0, 1)))
        print(f'bf16 {tag} {k}: hip {dev[k][0]:.2e} / {dev[k][1]:.2e} | yardstick {y[0]:.2e} / {y[1]:.2e} | ratio {r[0]:.2f} / {r[1]:.2f} | '
              f'roundings cost {c[0]:.2e} / {c[1]:.2e} | {path}, {groups} groups')
    print(f'bf16 {tag}: largest hip / bar {worst:.2f}')
    assert path == want_path, (tag, path)
    assert same, (tag, 'a second call does not repeat bit for bit')
    assert giveups == 0, (tag, giveups)
    assert want_groups(groups), (tag, 'launch groups', groups)
    assert np.isfinite(got).all(), tag
    for k in masks:
        for i, stat in enumerate(('rms', 'frame_max')):
            assert dev[k][i] <= bars[k][i], (tag, k, stat, dev[k][i], bars[k][i], path)


def default_case(case, want_path='stack_bf16', want_groups=lambda g: g == 1):
    if case not in _GOT:
        _GOT[case] = run_case(case)
    judge(bc.name(case), case, *_GOT[case], want_path, want_groups)
    return _GOT[case][0]


@pytest.mark.parametrize('case', bc.eval_cases(), ids=bc.name)
def test_single_evaluation(case):
    """DiffNet.forward through the stack launch: rows shorter than, equal to and one past a halo; one partial tile, one tile, a second tile
    of 1, 7, 8, 9 frames; the same one tile further; three tiles with a last tile of 8; each at 1, 2, 5 and 20 layers."""
    default_case(case)


def test_launch_groups():
    """26 x 640 at L = 5: 10 tiles per row, so 25 rows fill a launch group of 256 CUs and row 25 starts the second.  The count is the
    handle's (last_launch); on a device whose CU count makes this one group the assertion fails and says so."""
    got = run_case(bc.GROUP)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert got[2] >= 2, f'26 x 640 ran as {got[2]} launch group(s) on {cus} CUs: this case needs a device on which it splits (256 CUs)'
    judge(bc.name(bc.GROUP), bc.GROUP, *got, 'stack_bf16', lambda g: g >= 2)


@pytest.mark.parametrize('case', bc.sampler_cases(), ids=bc.name)
def test_sampler_forms(case):
    """Three fused DDPM steps with supplied noise, and PLMS through the warm-up pair and five multistep iterations (the four-term formula
    acts twice), both with the bf16 step tail; the final x by class."""
    default_case(case)


@pytest.mark.parametrize('case', bc.ragged_cases(), ids=bc.name)
def test_ragged(case):
    """stack_bf16_ragged and the ragged bf16 tail: rows of 200, 129, 65, 64 and 1 frames, each against the emulation of that row alone
    with classes from its own length; beyond a row's length exactly what the ragged contract documents: eps 0, x as the caller gave it."""
    got = default_case(case, 'stack_bf16_ragged')
    x = bc.inputs(case)['x'].double().numpy()
    for b, n in enumerate(bc.RAGGED_LENS):
        pad = got[b, :, :, n:]
        assert np.array_equal(pad, np.zeros_like(pad) if case.kind == 'ragged_eval' else x[b, :, :, n:]), (bc.name(case), b, n)


# ------------------------------------------------------------------------------------------------------------------
# switch sets: one child process each (the switches are read once per process)
# ------------------------------------------------------------------------------------------------------------------
CHILD = r'''
import sys, json, numpy as np, torch
sys.path.insert(0, %r)
torch.set_grad_enabled(False)
from tests import bf16_cases as bc
from tests import test_gpu_bf16_shapes as me
out = {}
for i, c in enumerate(json.loads(sys.argv[2])):
    got, path, groups, same, giveups = me.run_case(bc.Case(*c))
    np.save(sys.argv[1] + '/%%d.npy' %% i, got)
    out[i] = [path, groups, same, giveups]
print(json.dumps(out))
''' % ROOT

SWITCH_SETS = [
    # name, environment, last_path, launch groups
    ('stack_off', {'BSG_STACK_BF16': '0'}, 'bf16', 0),               # per-layer launches: the running skip sum rounded after every layer
    ('cond_indirect', {'BSG_COND_BF16_DIRECT': '0'}, 'stack_bf16', 1),   # the conditioner term through the fp32 copy and a conversion launch
    ('tail_f32', {'BSG_TAIL_BF16': '0'}, 'stack_bf16', 1),           # the fp32 step tail behind the bf16 stack launch
]


def test_switch_sets(tmp_path):
    """Each set at T = 65, 129, 200, L = 5 against the emulation of what it computes.  last_path shows that BSG_STACK_BF16=0 left the
    stack launch and that the other two kept it; BSG_TAIL_BF16=0 must change the bits of the DDPM result, BSG_COND_BF16_DIRECT=0 rounds
    the same fp32 term to bf16 in another launch (whether the bits agree is printed).  Nothing is started after a child that failed."""
    for name, env, want_path, want_groups in SWITCH_SETS:
        cases = bc.switch_cases()[name]
        d = tmp_path / name
        d.mkdir()
        res = subprocess.run([sys.executable, '-c', CHILD, str(d), json.dumps([list(c) for c in cases])], env=dict(os.environ, **env),
                             capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, (name, res.stderr[-2000:])
        out = json.loads(res.stdout.strip().splitlines()[-1])
        for i, case in enumerate(cases):
            got = np.load(str(d / f'{i}.npy'))
            judge(f'{name} {bc.name(case)}', case, got, *out[str(i)], want_path, lambda g: g == want_groups)
            twin = {'cond_indirect': case, 'tail_f32': bc.Case('ddpm', case.L, case.B, case.T)}.get(name)
            if twin is not None:
                if twin not in _GOT:
                    _GOT[twin] = run_case(twin)
                equal = np.array_equal(got, _GOT[twin][0])
                print(f'bf16 {name} {bc.name(case)}: bit-identical to the default form: {equal}')
                assert name != 'tail_f32' or not equal, (name, bc.name(case), 'the switch changed nothing')
