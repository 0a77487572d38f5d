"""GPU: ragged batches in the bf16-operand configuration (diff_compute_dtype bf16) — every row decoded at its own length by the ragged form
of the bf16 stack launch (residual_stack_bf16_varlen_kernel) and of the bf16 step tail, against the padded launch, the bf16-emulating
oracle, the same rows run alone, and the row-by-row fallback."""
import subprocess
import sys
from ctypes import c_int32

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
    m = bench.build_model(torch.device('cuda', 0))
    m.denoise_fn.set_compute('bf16')
    return m


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _inputs(B, T, seed, steps=None):
    g = torch.Generator().manual_seed(seed)
    cond = torch.randn(B, 256, T, generator=g).cuda()
    x = torch.randn(B, 1, 80, T, generator=g).cuda()
    noise = None if steps is None else torch.randn(steps, B, 80, T, generator=g).cuda()
    return cond, x, noise


@pytest.mark.parametrize('B,T,steps', [(16, 1000, None), (20, 777, None), (64, 1000, 10)])
def test_all_rows_full_length_is_the_padded_call_bit_for_bit(model, B, T, steps):
    """lengths = T everywhere: the ragged bf16 launch computes what the padded one does (Philox draws; the whole 100-step DDPM loop, 10
    steps at B = 64)."""
    cond, x, _ = _inputs(B, T, B)
    want = model.sample(cond, x.clone(), seed=11, n_steps=steps)
    assert model.denoise_fn.last_path() == 'stack_bf16'
    got = model.sample(cond, x.clone(), seed=11, n_steps=steps, lengths=[T] * B)
    assert model.denoise_fn.last_path() == 'stack_bf16_ragged'
    assert torch.equal(got, want)


def test_one_evaluation_matches_each_row_alone(model):
    """eps of a ragged bf16 batch at frames < len against the bf16-emulating oracle on each row alone at T = len (the stack launch's
    roundings: operands of both GEMMs, the skip sum once); 0 beyond.  The criterion of test_config2_bf16_full_size_vs_emulating_oracle over
    the real frames of all rows: rms no larger than the roundings' own rms (emulation vs fp32 oracle), max-abs at most twice theirs.  The
    padding holds x = 3000 and cond = 40, which no real frame may see."""
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
    assert net.last_path() == 'stack_bf16_ragged'
    assert not getattr(net, '_h2q_range_off', False) and not getattr(net, '_h2_range_off', False)
    assert net.handoff_timeouts() == 0
    sd = cpu_sd(net, 'denoise_fn.')
    got, emu, f32 = [], [], []
    for b, n in enumerate(lens):
        xb, tb, cb = x[b:b + 1, :, :, :n].cpu(), t[b:b + 1].cpu(), cond[b:b + 1, :, :n].cpu()
        got.append(eps[b:b + 1, :, :, :n].cpu().flatten())
        emu.append(odn.diffnet_forward(sd, xb, tb, cb, 'denoise_fn.', operand_bf16=True, skip_rounding='final').flatten())
        f32.append(odn.diffnet_forward(sd, xb, tb, cb, 'denoise_fn.').flatten())
        assert bool((eps[b, :, :, n:] == 0).all()), b
    got, emu, f32 = torch.cat(got), torch.cat(emu), torch.cat(f32)
    e, q = maxabs(got, emu), maxabs(emu, f32)
    rms, rms_q, rms_eps = [float(v.pow(2).mean().sqrt()) for v in (got - emu, emu - f32, f32)]
    print(f'ragged bf16 eps (rms {rms_eps:.3f}): vs bf16-emulating oracle max-abs {e:.3e}, rms {rms:.2e}; the roundings themselves '
          f'max-abs {q:.3e}, rms {rms_q:.2e}')
    assert rms <= rms_q and e <= 2.0 * q and e <= 0.1 * rms_eps


_CHILD = r'''
import sys, torch
sys.path.insert(0, sys.argv[1])
torch.set_grad_enabled(False)
import bench
from bisinger_amd.hparams import hparams
d = torch.load(sys.argv[2])
model = bench.build_model(torch.device('cuda', 0))
model.denoise_fn.set_compute('bf16')
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
    """DDPM (supplied noise, 20 steps) and PLMS on a batch of two launch groups: each row against the same row sampled alone at T = len
    in a child process in the bf16 configuration; x beyond len is untouched.  Bit for bit where len is a multiple of 4.  Elsewhere the
    projection GEMMs outside the stack take another kernel for a row alone (tests/test_gpu_ragged.py explains the alignment exception),
    and in bf16 a 1e-7 difference flips an operand by one bf16 ulp now and then, which the following layers and steps carry forward
    (measured on x, whose values are O(1): DDPM <= 4.9e-4, PLMS <= 3.1e-3).  Bounds: 2e-3 for DDPM, 1e-2 for PLMS."""
    from bisinger_amd.hparams import hparams
    lens, T, steps, interval = SAMPLE_LENS, 1000, 20, 20
    B = len(lens)
    assert ragged_plan(lens, _cus())[1] >= 2
    cond, x, noise = _inputs(B, T, 21, steps)
    xd = model.sample(cond, x.clone(), noise=noise, n_steps=steps, lengths=lens)
    assert model.denoise_fn.last_path() == 'stack_bf16_ragged'
    hparams['pndm_speedup'] = interval
    try:
        xp = model.sample(cond, x.clone(), lengths=lens)
    finally:
        hparams['pndm_speedup'] = 0
    assert model.denoise_fn.last_path() == 'stack_bf16_ragged'
    for b, n in enumerate(lens):
        assert torch.equal(xd[b, :, :, n:], x[b, :, :, n:]) and torch.equal(xp[b, :, :, n:], x[b, :, :, n:])
    src, dst = tmp_path / 'in.pt', tmp_path / 'out.pt'
    torch.save({'lens': lens, 'cond': cond.cpu(), 'x': x.cpu(), 'noise': noise.cpu(), 'interval': interval}, src)
    p = subprocess.run([sys.executable, '-c', _CHILD, ROOT, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    alone = torch.load(dst)
    assert all(q == 'stack_bf16' for q in alone['path']), alone['path']
    worst = {}
    for b, n in enumerate(lens):
        for kind, got in (('ddpm', xd), ('plms', xp)):
            e = maxabs(got[b:b + 1, :, :, :n], alone[kind][b])
            if e:
                worst[(kind, b, n)] = e
    print('rows not bit-identical to the row alone:', worst)
    assert all(n % 4 for _, _, n in worst), worst
    assert max((e for (k, _, _), e in worst.items() if k == 'ddpm'), default=0.0) <= 2e-3, worst
    assert max(worst.values(), default=0.0) <= 1e-2, worst


def test_fallback_row_by_row(model):
    """After a split demotion (bsg_diffnet_set_split(h, 0), the self-heal path after a give-up) the bf16 handle has no ragged launch: the
    call decodes the rows one by one at their own lengths through the per-layer bf16 launches.  Supplied noise: the same draws on both
    paths; the per-layer launches round the running skip sum to bf16 after every layer (the stack once), so the bound is the one
    tests/test_gpu_bf16.py holds the two launches to on eps (measured: 3.9e-3 max-abs, 5.0e-4 rms), and 1e-2 on x after 20 steps
    (measured 1.1e-3)."""
    net = model.denoise_fn
    lib = _lib.load()
    lens, T, steps = [1000, 517, 65, 1], 1000, 20
    B = len(lens)
    cond, x, noise = _inputs(B, T, 31, steps)
    native = model.sample(cond, x.clone(), noise=noise, n_steps=steps, lengths=lens)
    assert net.last_path() == 'stack_bf16_ragged'
    eps_native = net(x, torch.full((B,), 9, device='cuda'), cond, lengths=lens)
    assert net.ragged_native(B, T)
    _lib.check(lib.bsg_diffnet_set_split(net.handle(), 0), 'bsg_diffnet_set_split')
    try:
        assert not net.ragged_native(B, T)
        rows = model.sample(cond, x.clone(), noise=noise, n_steps=steps, lengths=lens)
        assert net.last_path() == 'bf16'
        eps_rows = net(x, torch.full((B,), 9, device='cuda'), cond, lengths=lens)
    finally:
        _lib.check(lib.bsg_diffnet_set_split(net.handle(), 1), 'bsg_diffnet_set_split')
    assert net.ragged_native(B, T)
    assert bool(torch.isfinite(rows).all())
    for b, n in enumerate(lens):
        assert torch.equal(rows[b, :, :, n:], x[b, :, :, n:])
        assert bool((eps_rows[b, :, :, n:] == 0).all())
    real = [(rows[b, :, :, :n], native[b, :, :, :n]) for b, n in enumerate(lens)]
    dx = max(maxabs(a, c) for a, c in real)
    de, rms_e = maxabs(eps_rows, eps_native), float((eps_rows - eps_native).pow(2).mean().sqrt())
    print(f'bf16 fallback vs ragged launch: x max-abs {dx:.2e}; eps max-abs {de:.2e}, rms {rms_e:.2e}')
    assert de <= 2e-2 and rms_e <= 2e-3
    assert dx <= 1e-2


def test_refusals(model):
    """Kept in the bf16 configuration: a ragged binding or call under stream capture, a row longer than one launch group, lengths
    outside 1..T, rows= with ragged=True."""
    net = model.denoise_fn
    lib = _lib.load()
    cond, x, _ = _inputs(2, 64, 5)
    with pytest.raises(ValueError):
        net.prepare(cond, lengths=[64, 65])
    with pytest.raises(_lib.BsgError, match='launch group holds'):
        net.prepare(torch.zeros(1, 256, 64 * (_cus() + 1), device='cuda'), lengths=[64 * (_cus() + 1)])
    with pytest.raises(NotImplementedError):
        model(torch.zeros(2, 8, dtype=torch.long, device='cuda'), infer=True, ragged=True, rows=slice(0, 1))
    # capture: the bound ragged batch's compute call and a new ragged binding are refused before anything is enqueued
    net.prepare(cond, lengths=[64, 9])
    xs, t, eps = x[:, 0].contiguous(), torch.zeros(2, dtype=torch.long, device='cuda'), torch.empty(2, 80, 64, device='cuda')
    lens = (c_int32 * 2)(64, 9)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            rc_fwd = lib.bsg_diffnet_forward(net.handle(), _lib.ptr(xs), _lib.ptr(t), _lib.ptr(eps), 2, 64, _lib.stream_ptr())
            rc_bind = lib.bsg_diffnet_prepare_ragged(net.handle(), _lib.ptr(cond), lens, 2, 64, _lib.stream_ptr())
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert rc_fwd != 0 and rc_bind != 0
    eps2 = net(x, t, cond, lengths=[64, 9])   # the handle still decodes the ragged batch eagerly
    assert net.last_path() == 'stack_bf16_ragged' and bool(torch.isfinite(eps2).all())


def test_end_to_end_forward_ragged(model):
    """GaussianDiffusion.forward(ragged=True) on a bf16 model: lengths from mel2ph, mel_out 0 beyond each row's frames, finite."""
    B, T_txt, T = 4, 12, 300
    inp = synth.synth_inputs(B, T_txt, T, seed=2, ragged=True)
    d = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    kw = {k: d[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')}
    out = model(d['txt_tokens'], mel2ph=d['mel2ph'], spk_embed=d['spk_embed'], infer=True, seed=5, ragged=True, **kw)
    assert model.denoise_fn.last_path() == 'stack_bf16_ragged'
    mel = out['mel_out']
    lens = (d['mel2ph'] > 0).sum(-1).tolist()
    assert len(set(lens)) > 1
    assert bool(torch.isfinite(mel).all())
    for b, n in enumerate(lens):
        assert bool((mel[b, n:] == 0).all()) and bool((mel[b, :n] != 0).any())


from tests.test_gpu_infer import _item, workdir  # noqa: E402,F401  (the synthetic checkpoint directory of the inference tests)


def test_forward_batch_ragged(workdir):
    # (shapes and launch groups only; the values of the fp32 configuration's ragged forward_batch: tests/test_gpu_e2e_ragged.py)
    from bisinger_amd.hparams import set_hparams, hparams
    from bisinger_amd.infer import DiffSingerE2EInfer
    set_hparams('exp.yaml', exp_name='exp_diff_e2e', print_hparams=False, hparams_str='seed=4321')
    infer = DiffSingerE2EInfer(hparams)
    infer.model.denoise_fn.set_compute('bf16')
    items = [infer.preprocess_input(_item(n, s), 'phoneme') for n, s in ((9, 1), (6, 2), (11, 3), (4, 4), (7, 5))]
    wavs = infer.forward_batch(items, seed=77, max_sentences=3, ragged=True)
    assert infer.model.denoise_fn.last_path() == 'stack_bf16_ragged'
    st = infer.last_batch_stats
    assert len(st['buckets']) == 2
    want_groups = sum(ragged_plan([st['frames'][i] for i in bk], _cus())[1] for bk in st['buckets'])
    assert st['launch_groups'] == want_groups
    assert st['tiles'] == sum(-(-n // 64) for n in st['frames'])
    for w, n in zip(wavs, st['frames']):
        assert w.shape == (n * 256,) and np.isfinite(w).all()
