"""GPU: ragged batches — every row decoded at its own length (bsg_diffnet_prepare_ragged, the ragged 16-row stack launch), against the
padded launch, the oracle, the same rows run alone, and the row-by-row fallback."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bisinger_amd import _lib, synth
from bisinger_amd.diffnet import ragged_plan
from tests.util import ROOT, cpu_sd, maxabs

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# 15 x 16 + 13 + 9 + 5 + 2 + 1 + 1 = 271 tiles of 64 frames: two launch groups on 256 CUs
SAMPLE_LENS = [1000] * 15 + [777, 517, 300, 65, 64, 1]


@pytest.fixture(scope='module')
def model():
    import bench
    return bench.build_model(torch.device('cuda', 0))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _inputs(B, T, seed, steps=None):
    g = torch.Generator().manual_seed(seed)
    cond = torch.randn(B, 256, T, generator=g).cuda()
    x = torch.randn(B, 1, 80, T, generator=g).cuda()
    noise = None if steps is None else torch.randn(steps, B, 80, T, generator=g).cuda()
    return cond, x, noise


@pytest.mark.parametrize('B,T', [(16, 1000), (20, 777)])
def test_all_rows_full_length_is_the_padded_call_bit_for_bit(model, B, T):
    """lengths = T everywhere: the ragged launch computes what the padded one does (Philox draws, the whole 100-step DDPM loop)."""
    cond, x, _ = _inputs(B, T, B)
    want = model.sample(cond, x.clone(), seed=11)
    assert model.denoise_fn.last_path() == 'stack_h2q_tail'
    got = model.sample(cond, x.clone(), seed=11, lengths=[T] * B)
    assert model.denoise_fn.last_path() == 'stack_h2q_ragged_tail'
    assert torch.equal(got, want)


def test_one_evaluation_matches_each_row_alone(model):
    """eps of a ragged batch at frames < len equals the float64 oracle DiffNet on that row alone at T = len; 0 beyond.  The padding holds
    values the 16-row launch's range guard would trip on (|x| >= 3750 after the input projection) if it read them: it does not."""
    from oracle import diffnet as odn
    net = model.denoise_fn
    lens, T = [1000, 1, 63, 64, 65, 517], 1000
    B = len(lens)
    cond, x, _ = _inputs(B, T, 3)
    t = torch.tensor([0, 99, 7, 50, 33, 64], device='cuda')
    for b, n in enumerate(lens):
        x[b, :, :, n:] = 3000.0
        cond[b, :, n:] = 40.0
    eps = net(x, t, cond, lengths=lens)
    assert net.last_path() == 'stack_h2q_ragged'
    assert not getattr(net, '_h2q_range_off', False) and not getattr(net, '_h2_range_off', False)
    sd = cpu_sd(net, 'denoise_fn.')
    for b, n in enumerate(lens):
        ref = odn.diffnet_forward(sd, x[b:b + 1, :, :, :n].cpu(), t[b:b + 1].cpu(), cond[b:b + 1, :, :n].cpu(), 'denoise_fn.',
                                  dtype=torch.float64)
        assert maxabs(eps[b:b + 1, :, :, :n], ref) <= 2e-5, (b, n)
        assert bool((eps[b, :, :, n:] == 0).all())


_CHILD = r'''
import sys, torch
sys.path.insert(0, sys.argv[1])
torch.set_grad_enabled(False)
import bench
from bisinger_amd.hparams import hparams
d = torch.load(sys.argv[2])
model = bench.build_model(torch.device('cuda', 0))
out = {'ddpm': [], 'plms': [], 'path': []}
for b, n in enumerate(d['lens']):
    cond = d['cond'][b:b + 1, :, :n].cuda().contiguous()
    x = d['x'][b:b + 1, :, :, :n].cuda().contiguous()
    noise = d['noise'][:, b:b + 1, :, :n].cuda().contiguous()
    out['ddpm'].append(model.sample(cond, x.clone(), noise=noise, n_steps=noise.shape[0]).cpu())
    out['path'].append(model.denoise_fn.last_path())
    hparams['pndm_speedup'] = d['interval']
    out['plms'].append(model.sample(cond, x.clone()).cpu())
    hparams['pndm_speedup'] = 0
torch.save(out, sys.argv[3])
'''


def test_sampling_matches_each_row_alone(model, tmp_path):
    """DDPM (supplied noise, 20 steps) and PLMS on a batch of two launch groups: each row equals the same row sampled alone at T = len in a
    child process with BSG_H2_NCT=2 (the 16-row launch on 64-frame tiles, no part form); x beyond len is untouched.
    Bit for bit where len is a multiple of 4.  The shape-dependent launch is the projection GEMM outside the residual stack (conv1x1 ->
    launch_gemm, csrc/gemm.hip): a row ALONE at T = len with len % 4 != 0 has rows that are not 16-byte aligned and takes gemm_f32_kernel
    (fp32 FMAs) instead of the split-fp16 GEMM the batch (T = 1000) takes — for the input projection of x (DDPM: once per call; measured
    <= 3.6e-7) and, in PLMS's unfused first iteration, for the skip / output projections too (measured <= 1.9e-6 after the 5 iterations)."""
    from bisinger_amd.hparams import hparams
    lens, T, steps, interval = SAMPLE_LENS, 1000, 20, 20
    B = len(lens)
    assert ragged_plan(lens, _cus())[1] >= 2
    cond, x, noise = _inputs(B, T, 21, steps)
    xd = model.sample(cond, x.clone(), noise=noise, n_steps=steps, lengths=lens)
    assert model.denoise_fn.last_path() == 'stack_h2q_ragged_tail'
    hparams['pndm_speedup'] = interval
    try:
        xp = model.sample(cond, x.clone(), lengths=lens)
    finally:
        hparams['pndm_speedup'] = 0
    assert model.denoise_fn.last_path() == 'stack_h2q_ragged_tail'
    for b, n in enumerate(lens):
        assert torch.equal(xd[b, :, :, n:], x[b, :, :, n:]) and torch.equal(xp[b, :, :, n:], x[b, :, :, n:])
    src, dst = tmp_path / 'in.pt', tmp_path / 'out.pt'
    torch.save({'lens': lens, 'cond': cond.cpu(), 'x': x.cpu(), 'noise': noise.cpu(), 'interval': interval}, src)
    env = dict(os.environ, BSG_H2_NCT='2')
    p = subprocess.run([sys.executable, '-c', _CHILD, ROOT, str(src), str(dst)], env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    alone = torch.load(dst)
    assert all(q.startswith('stack_h2q') for q in alone['path']), alone['path']
    worst = {}
    for b, n in enumerate(lens):
        for kind, got in (('ddpm', xd), ('plms', xp)):
            e = maxabs(got[b:b + 1, :, :, :n], alone[kind][b])
            if e:
                worst[(kind, b, n)] = e
    print('rows not bit-identical to the row alone:', worst)
    assert all(n % 4 for _, _, n in worst), worst
    assert max((e for (k, _, _), e in worst.items() if k == 'ddpm'), default=0.0) <= 1e-6, worst
    assert max(worst.values(), default=0.0) <= 4e-6, worst


def test_fallback_row_by_row(model):
    """Off the 16-row launch (bsg_diffnet_set_h2q(h, 0)) the handle has no ragged launch: the call decodes the rows one by one at their
    own lengths, within 1e-5 of the ragged launch (supplied noise: the same draws on both paths)."""
    net = model.denoise_fn
    lens, T, steps = [1000, 517, 65, 1], 1000, 20
    B = len(lens)
    cond, x, noise = _inputs(B, T, 31, steps)
    native = model.sample(cond, x.clone(), noise=noise, n_steps=steps, lengths=lens)
    assert net.ragged_native(B, T)
    net.set_q_launch(False)
    try:
        assert not net.ragged_native(B, T)
        rows = model.sample(cond, x.clone(), noise=noise, n_steps=steps, lengths=lens)
        assert not net.last_path().startswith('stack_h2q')
        eps_rows = net(x, torch.full((B,), 9, device='cuda'), cond, lengths=lens)
    finally:
        net.set_q_launch(True)
    eps_native = net(x, torch.full((B,), 9, device='cuda'), cond, lengths=lens)
    assert net.last_path() == 'stack_h2q_ragged'
    for b, n in enumerate(lens):
        assert maxabs(rows[b, :, :, :n], native[b, :, :, :n]) <= 1e-5, b
        assert torch.equal(rows[b, :, :, n:], x[b, :, :, n:])
    assert maxabs(eps_rows, eps_native) <= 1e-5
    assert bool(torch.isfinite(rows).all())


def test_refusals(model):
    net = model.denoise_fn
    cond, x, _ = _inputs(2, 64, 5)
    with pytest.raises(ValueError):
        net.prepare(cond, lengths=[64, 65])
    with pytest.raises(_lib.BsgError, match='launch group holds'):
        net.prepare(torch.zeros(1, 256, 64 * (_cus() + 1), device='cuda'), lengths=[64 * (_cus() + 1)])
    with pytest.raises(NotImplementedError):
        model(torch.zeros(2, 8, dtype=torch.long, device='cuda'), infer=True, ragged=True, rows=slice(0, 1))


def test_end_to_end_forward_ragged(model):
    """GaussianDiffusion.forward(ragged=True): lengths from mel2ph, mel_out 0 beyond each row's frames, everything finite.
    (The values of mel_out, row by row against float64 with the row's own Philox draws: tests/test_gpu_e2e_ragged.py.)"""
    B, T_txt, T = 4, 12, 300
    inp = synth.synth_inputs(B, T_txt, T, seed=2, ragged=True)
    d = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    kw = {k: d[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')}
    out = model(d['txt_tokens'], mel2ph=d['mel2ph'], spk_embed=d['spk_embed'], infer=True, seed=5, ragged=True, **kw)
    assert model.denoise_fn.last_path() == 'stack_h2q_ragged_tail'
    mel = out['mel_out']
    lens = (d['mel2ph'] > 0).sum(-1).tolist()
    assert len(set(lens)) > 1
    assert bool(torch.isfinite(mel).all())
    for b, n in enumerate(lens):
        assert bool((mel[b, n:] == 0).all()) and bool((mel[b, :n] != 0).any())
    bad = d['mel2ph'].clone()
    bad[1, 3] = 0
    with pytest.raises(ValueError, match='row 1'):
        model(d['txt_tokens'], mel2ph=bad, spk_embed=d['spk_embed'], infer=True, seed=5, ragged=True, **kw)


from tests.test_gpu_infer import _item, workdir  # noqa: E402,F401  (the synthetic checkpoint directory of the inference tests)


def test_forward_batch_ragged(workdir):
    # (shapes and launch groups only; the values, every row against float64 on the utterance alone: tests/test_gpu_e2e_ragged.py)
    from bisinger_amd.hparams import set_hparams, hparams
    from bisinger_amd.infer import DiffSingerE2EInfer
    set_hparams('exp.yaml', exp_name='exp_diff_e2e', print_hparams=False, hparams_str='seed=4321')
    infer = DiffSingerE2EInfer(hparams)
    items = [infer.preprocess_input(_item(n, s), 'phoneme') for n, s in ((9, 1), (6, 2), (11, 3), (4, 4), (7, 5))]
    wavs = infer.forward_batch(items, seed=77, max_sentences=3, ragged=True)
    st = infer.last_batch_stats
    assert len(st['buckets']) == 2
    want_groups = sum(ragged_plan([st['frames'][i] for i in bk], _cus())[1] for bk in st['buckets'])
    assert st['launch_groups'] == want_groups
    assert st['tiles'] == sum(-(-n // 64) for n in st['frames'])
    for w, n in zip(wavs, st['frames']):
        assert w.shape == (n * 256,) and np.isfinite(w).all()
    with pytest.raises(ValueError):
        infer.forward_batch(items, max_frames=5000, ragged=True)
