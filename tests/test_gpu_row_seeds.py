"""GPU: row-keyed sampler noise (ABI v22) — a batched row draws what it draws alone.

  1. the fill (bsg_philox_normal_rows), bit for bit: every row's live part is bsg_philox_normal over M n_b values under that row's seed,
     everything beyond is 0 in a buffer pre-filled with NaN; odd T (rows start unaligned), the flat layout (M = 1), lengths NULL, 33 rows
     (two launches);
  2. the loop reads what the fill wrote: sample(row_seeds=) equals, bit for bit, sample(noise=N) with N[k] the fill at the step's stream id,
     on the same launch form; ragged, padded, and in the bf16 configuration;
  3. the row is the lone call: row b of the ragged result against sample(seed=s[b]) of that row alone at T = n_b (a child process with
     BSG_H2_NCT=2, as tests/test_gpu_ragged.py::test_sampling_matches_each_row_alone runs its lone rows), at that test's bounds for the
     supplied-noise comparison — the draws are identical now, nothing else has changed: 1e-6 DDPM, 4e-6 PLMS; the row-by-row fallback
     within 1e-5 of the native path, as test_fallback_row_by_row holds it;
  4. the vocoders: NSF HiFi-GAN forward(lengths=, row_seeds=) row b against the lone forward(seed=s[b]) at twice the bar
     tests/test_gpu_hifigan_ragged.py holds a ragged row to against float64 (both sides are within it of the same float64 result);
     Parallel WaveGAN forward_ragged(row_seeds=) row b equals the lone forward(seed=s[b]) bit for bit;
  5. end to end: forward_batch(items, seeds=S, max_sentences=3, every ragged switch) against forward_model(items[i], seed=S[i]) for every
     item at twice the composed bars of tests/test_gpu_e2e_ragged.py; the shortest item against the float64 alone chain at row place 0 of
     a bucket of one under its own seed, at the bar itself; the same list with max_sentences=2 (other buckets, other row places) within
     the doubled bar of the first run.
     Planted once, then reverted: the bucket's seeds handed over in bucket order (seeds[:len(bucket)]) instead of item order -> 5 fails
     (the shortest item 0.94 from its float64 chain).

Measured on the MI355X (every test passed): 2. bit-identical on stack_h2q_ragged_tail, stack_bf16_ragged, stack_h2_quad, stack_bf16;
3. DDPM 0 on all three rows, PLMS 0 / 2.4e-7 / 4.8e-7 (n = 128 / 65 / 29), fallback 2.4e-7 .. 3.6e-7; 4. NSF 0 (bar 1.08e-5);
5. against forward_model: plain 7.8e-7 .. 9.2e-7 (bar 9.6e-6), nsf 1.1e-6 .. 2.0e-6 (bar 1.28e-5); re-bucketed: bit-identical; the
shortest item against float64: 9.2e-7 (bar 4.8e-6) plain, 1.5e-6 (bar 6.4e-6) nsf.
"""
import os
import subprocess
import sys
from ctypes import c_int32, c_uint64

import numpy as np
import pytest
import torch

from bisinger_amd import _lib
from tests import e2e_ragged_cases as E
from tests.test_gpu_ddpm_shapes import _limit
from tests.test_gpu_e2e_ragged import switches
from tests.test_gpu_f2_fullsize import nsf  # noqa: F401  (the module-scoped NSF generator fixture of that file)
from tests.test_gpu_hifigan_ragged import _f0
from tests.test_gpu_hifigan_shapes import BAR
from tests.test_gpu_infer import workdir  # noqa: F401  (the synthetic checkpoint directory of the inference tests)
from tests.test_gpu_pe_ragged import nsf_workdir  # noqa: F401  (the pe_enable + use_nsf set-up)
from tests.util import ROOT, maxabs

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

HOP, NH = 256, 9
NSF_STREAM, PWG_STREAM = 0x4E5346, 0x505747
SEEDS3 = [20240917, 5, 0xFFFFFFFF00000003]      # (one beyond 32 bits: both key words are the row's)
LENS, T_S, STEPS = [128, 65, 29], 128, 3


# ------------------------------------------------------------------------------------------------------------------
# 1. the fill, bit for bit
# ------------------------------------------------------------------------------------------------------------------
def lone_fill(n, seed, stream):
    y = torch.empty(n, device='cuda')
    _lib.check(_lib.load().bsg_philox_normal(_lib.ptr(y), n, seed, stream, 0, _lib.stream_ptr()), 'bsg_philox_normal')
    return y


def rows_fill(B, M, T, lens, seeds, stream):
    x = torch.full((B, M, T), float('nan'), device='cuda')
    larr = None if lens is None else (c_int32 * B)(*lens)
    _lib.check(_lib.load().bsg_philox_normal_rows(_lib.ptr(x), B, M, T, larr, (c_uint64 * B)(*seeds), stream, _lib.stream_ptr()),
               'bsg_philox_normal_rows')
    return x


@pytest.mark.parametrize('B,M,T,lens', [(3, 80, 13, [13, 1, 6]), (3, 1, 36, [36, 4, 20]), (3, 80, 13, None), (3, 1, 36, None),
                                        (33, 80, 4, [1 + b % 4 for b in range(33)])],
                         ids=['80x13', 'flat36', '80x13-null', 'flat36-null', '33rows'])
def test_fill_is_every_rows_lone_stream(B, M, T, lens):
    seeds = (SEEDS3 if B == 3 else [1000 + 7 * b for b in range(B)])
    x = rows_fill(B, M, T, lens, seeds, 7)
    for b in range(B):
        n = T if lens is None else lens[b]
        want = lone_fill(M * n, seeds[b], 7).reshape(M, n)
        assert torch.equal(x[b, :, :n], want), (b, n)
        assert bool((x[b, :, n:] == 0).all()), (b, n, 'not 0 beyond the row')
    assert len({float(x[b, 0, 0]) for b in range(B)}) == B      # the rows' streams differ


# ------------------------------------------------------------------------------------------------------------------
# 2., 3. the sampler
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model():
    from tests.test_gpu_fs2_ragged import _diffusion
    return _diffusion(False)      # the timesteps-4 WaveNet model of the ragged front's tests


def inputs():
    g = torch.Generator().manual_seed(41)
    cond = torch.randn(3, 256, T_S, generator=g).cuda()
    x = torch.randn(3, 1, 80, T_S, generator=g).cuda()
    return cond, x


def step_noise(model, lens):
    """N[k]: the fill at the stream id i + 1 of step k (i = K_step - 1 - k)."""
    return torch.stack([rows_fill(3, 80, T_S, lens, SEEDS3, model.K_step - 1 - k + 1) for k in range(STEPS)])


@pytest.mark.parametrize('compute', ['fp32', 'bf16'])
@pytest.mark.parametrize('ragged', [True, False], ids=['ragged', 'padded'])
def test_loop_reads_what_the_fill_wrote(model, ragged, compute):
    net = model.denoise_fn
    lens = LENS if ragged else None
    cond, x = inputs()
    net.set_compute(compute)
    try:
        N = step_noise(model, lens)
        assert bool(torch.isfinite(N).all())
        want = model.sample(cond, x.clone(), noise=N, n_steps=STEPS, lengths=lens)
        want_path = net.last_path()
        got = model.sample(cond, x.clone(), row_seeds=SEEDS3, n_steps=STEPS, lengths=lens)
        assert net.last_path() == want_path, (net.last_path(), want_path)
        print(f'  {compute} {"ragged" if ragged else "padded"}: {want_path}')
    finally:
        net.set_compute('fp32')
    assert ('ragged' in want_path) == ragged
    assert torch.equal(got, want)
    assert not torch.equal(got, x) and bool(torch.isfinite(got).all())
    for b, n in enumerate(lens or []):
        assert torch.equal(got[b, :, :, n:], x[b, :, :, n:]), b


_CHILD = r'''
import sys, torch
sys.path.insert(0, sys.argv[1])
torch.set_grad_enabled(False)
from bisinger_amd.hparams import hparams
from tests.test_gpu_fs2_ragged import _diffusion
d = torch.load(sys.argv[2])
model = _diffusion(False)
out = {'ddpm': [], 'plms': [], 'path': []}
for b, n in enumerate(d['lens']):
    cond = d['cond'][b:b + 1, :, :n].cuda().contiguous()
    x = d['x'][b:b + 1, :, :, :n].cuda().contiguous()
    out['ddpm'].append(model.sample(cond, x.clone(), seed=d['seeds'][b], n_steps=d['steps']).cpu())
    out['path'].append(model.denoise_fn.last_path())
    hparams['pndm_speedup'] = 1
    out['plms'].append(model.sample(cond, x.clone(), seed=d['seeds'][b]).cpu())
    hparams['pndm_speedup'] = 0
torch.save(out, sys.argv[3])
'''


def test_row_is_the_lone_call(model, tmp_path):
    from bisinger_amd.hparams import hparams
    net = model.denoise_fn
    cond, x = inputs()
    xd = model.sample(cond, x.clone(), row_seeds=SEEDS3, n_steps=STEPS, lengths=LENS)
    assert net.last_path() == 'stack_h2q_ragged_tail'
    hparams['pndm_speedup'] = 1
    try:
        xp = model.sample(cond, x.clone(), row_seeds=SEEDS3, lengths=LENS)
    finally:
        hparams['pndm_speedup'] = 0
    # the fallback: every row through the lone entry under its own seed
    net.set_q_launch(False)
    try:
        assert not net.ragged_native(3, T_S)
        rows = model.sample(cond, x.clone(), row_seeds=SEEDS3, n_steps=STEPS, lengths=LENS)
        assert not net.last_path().startswith('stack_h2q')
    finally:
        net.set_q_launch(True)
    for b, n in enumerate(LENS):
        e = maxabs(rows[b, :, :, :n], xd[b, :, :, :n])
        print(f'  row {b} (n={n}): fallback against the native path {e:.2e} (allowed 1e-5)')
        assert e <= 1e-5, b
        assert torch.equal(rows[b, :, :, n:], x[b, :, :, n:])
    src, dst = tmp_path / 'in.pt', tmp_path / 'out.pt'
    torch.save({'lens': LENS, 'cond': cond.cpu(), 'x': x.cpu(), 'seeds': SEEDS3, 'steps': STEPS}, src)
    p = subprocess.run([sys.executable, '-c', _CHILD, ROOT, str(src), str(dst)], env=dict(os.environ, BSG_H2_NCT='2'), capture_output=True,
                       text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    alone = torch.load(dst)
    assert all(q.startswith('stack_h2q') for q in alone['path']), alone['path']
    for b, n in enumerate(LENS):
        ed, ep = maxabs(xd[b:b + 1, :, :, :n], alone['ddpm'][b]), maxabs(xp[b:b + 1, :, :, :n], alone['plms'][b])
        print(f'  row {b} (n={n}): against the row alone under seed {SEEDS3[b]}: ddpm {ed:.2e} (allowed 1e-6)  plms {ep:.2e} (allowed 4e-6)')
        assert ed <= 1e-6 and ep <= 4e-6, (b, ed, ep)
        assert n % 4 or (ed == 0 and ep == 0), (b, 'a row of n % 4 == 0 takes the same GEMM forms alone: bit for bit')
        assert torch.equal(xd[b, :, :, n:], x[b, :, :, n:]) and torch.equal(xp[b, :, :, n:], x[b, :, :, n:])


# ------------------------------------------------------------------------------------------------------------------
# 4. the vocoders
# ------------------------------------------------------------------------------------------------------------------
def test_nsf_row_is_the_lone_call(nsf):  # noqa: F811
    gen, _sd, _cfg = nsf
    B, T, lens = 2, 5, [5, 2]
    rs = np.random.RandomState(500 * B + T)
    mel = torch.from_numpy((rs.standard_normal((B, 80, T)) * 1.5 - 3.0).astype(np.float32)).cuda()
    f0 = torch.from_numpy(_f0(rs, B, T)).cuda()
    seeds = SEEDS3[:B]
    for ln in (lens, None):
        got = gen(mel, f0, row_seeds=seeds, **({} if ln is None else {'lengths': ln}))
        for b in range(B):
            n = T if ln is None else ln[b]
            lone = gen(mel[b:b + 1, :, :n].contiguous(), f0[b:b + 1, :n].contiguous(), seed=seeds[b])[0, 0]
            bar = 2 * BAR * max(1.0, float(lone.abs().max()))
            e = maxabs(got[b, 0, :n * HOP], lone)
            print(f'  nsf row {b} (n={n}, lengths={ln}): against the lone call {e:.2e} (allowed {bar:.2e})')
            assert e <= bar, (b, e, bar)
            assert not bool(got[b, 0, n * HOP:].any())
    # the draws themselves: the flat fill on the NSF stream is the lone call's noise
    nz = rows_fill(B, 1, T * HOP * NH, [n * HOP * NH for n in lens], seeds, NSF_STREAM)
    assert torch.equal(nz[1, 0, :lens[1] * HOP * NH], lone_fill(lens[1] * HOP * NH, seeds[1], NSF_STREAM))


def test_pwg_row_is_the_lone_call_bit_for_bit():
    from collections import OrderedDict
    from bisinger_amd import synth
    from bisinger_amd.pwg import ParallelWaveGANGenerator
    from tests import pwg_ref as ref
    from tests.test_gpu_pwg_ragged import CASE2, HOP300_SCALES, edge
    q = ref.params(False, layers=6, stacks=2, upsample_params={'upsample_scales': HOP300_SCALES})      # the small hop-300 generator
    g = ParallelWaveGANGenerator(**q)
    spec = OrderedDict((k, tuple(v.shape)) for k, v in g.state_dict().items())
    g.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(spec, 23).items()}, strict=True)
    g = g.cuda().eval()
    g.remove_weight_norm()
    B, T, lens = CASE2
    hop = g.hop_size
    assert hop == 300
    _, mel, _ = ref.make_inputs(B, T, 7000 + 10 * B + T, 0, False, hop=hop)
    seeds = [11, 12, 2 ** 40 + 13, 14]
    got = g.forward_ragged(None, torch.from_numpy(mel), lengths=list(lens), row_seeds=seeds)
    for b, n in enumerate(lens):
        lone = g(None, torch.from_numpy(edge(mel[b:b + 1], n)), seed=seeds[b])
        assert torch.equal(got[b, 0, :n * hop], lone[0, 0]), (b, n)
        assert not bool(got[b, 0, n * hop:].any())
    assert bool(torch.isfinite(got).all()) and bool(got[1, 0, :hop].any())


# ------------------------------------------------------------------------------------------------------------------
# 5. end to end
# ------------------------------------------------------------------------------------------------------------------
S = (101, 2024, 7, 99991, 31337)      # one seed per item, in the order the items are given


@pytest.mark.parametrize('setup', E.SETUPS)
def test_forward_batch_item_is_forward_model_under_its_seed(setup, request):
    request.getfixturevalue('workdir' if setup == 'plain' else 'nsf_workdir')
    from bisinger_amd.hparams import hparams, set_hparams
    from bisinger_amd.infer import DiffSingerE2EInfer
    E.raise_checkpoint('checkpoints/exp_diff_e2e/model_ckpt_steps_1000.ckpt')
    set_hparams('exp.yaml' if setup == 'plain' else 'exp2.yaml', exp_name='exp_diff_e2e', print_hparams=False, hparams_str='seed=4321')
    infer = DiffSingerE2EInfer(hparams)
    items = E.items()
    bar = 4 * E.YARD_COMPOSED[setup]['wav']      # the composed bar of tests/test_gpu_e2e_ragged.py
    f0s = []
    if setup == 'nsf':
        inner = infer.pe.forward

        def recording(mel, *a, **k):
            out = inner(mel, *a, **k)
            f0s.append(out['f0_denorm_pred'].cpu().numpy())
            return out
        infer.pe.forward = recording
    with _limit(120):
        first = infer.forward_batch(items, seeds=S, max_sentences=E.MAX_SENTENCES, **switches(setup))
        st = dict(infer.last_batch_stats)
        assert tuple(map(tuple, st['buckets'])) == E.BUCKETS and tuple(st['frames']) == E.FRAMES
        assert infer.model.denoise_fn.last_path() == 'stack_h2q_ragged_tail'
        batch_f0 = list(f0s)
        lone = [infer.forward_model(it, seed=s) for it, s in zip(items, S)]
        second = infer.forward_batch(items, seeds=S, max_sentences=2, **switches(setup))
        assert tuple(map(tuple, infer.last_batch_stats['buckets'])) != E.BUCKETS and len(infer.last_batch_stats['buckets']) == 3
    if setup == 'nsf':
        infer.pe.forward = inner
    bad = []
    for i, n in enumerate(E.FRAMES):
        assert first[i].shape == second[i].shape == lone[i].shape == (n * HOP,)
        a, b = E.norm_dev(first[i], lone[i]), E.norm_dev(second[i], first[i])
        print(f'  {setup} item {i} (n={n}, seed {S[i]}): against forward_model {a:.2e}  re-bucketed against the first run {b:.2e}  (allowed {2 * bar:.2e})')
        if not (a <= 2 * bar and b <= 2 * bar):
            bad.append((i, a, b, 2 * bar))
    i = int(np.argmin(E.FRAMES))
    n = E.FRAMES[i]
    feed = None
    if setup == 'nsf':      # (the chain fed the device's f0 of that row, as the sine source integrates f0)
        k = next(k for k, bk in enumerate(st['buckets']) if i in bk)
        feed = {'f0': batch_f0[k][list(st['buckets'][k]).index(i), :n]}
    with _limit(600):
        want = E.alone_chain(E.state_dicts(setup), items[i], 0, 1, n, S[i], E.F64, feed=feed)
    dev = E.norm_dev(first[i], want['wav'])
    print(f'  {setup} item {i} (n={n}): against the float64 chain of the item alone under seed {S[i]} {dev:.2e} (allowed {bar:.2e})')
    assert dev <= bar, (dev, bar)
    assert not bad, bad
