"""GPU: ragged batches through the FFT denoiser (diff_decoder_type: fft) — every row decoded as the row alone.

Reference: the float64 oracle on each row's own slice (tests/fftden_ragged_cases.py), bounds from that module (4 x the float32 oracle's own
figure x max(1, max |want|)); its CPU test shows that the reference's padded evaluation of a short row lies at least 1000 bounds away.

  forward   every case of FWD_CASES: each row against float64 on it alone, eps exactly 0 beyond a row's end, unchanged bit for bit with NaN
            in x and cond beyond the ends, the attention form and the set of GEMM forms read from bsg_fftden_last_path (the record starts with
            den.ragged); the all-full batch against the padded call; a stale, poisoned workspace; the capture rules
  DDPM      sample(lengths=) — bsg_fftden_ddpm_sample, the fused step tail — with supplied noise, row_seeds (two batch compositions, and
            the lone call under the row's seed) and seed; the entry itself on a padded binding
  PLMS      sample(lengths=) with pndm_speedup — bsg_fftden_plms_sample — and the entry on a padded binding
  top       GaussianDiffusion.forward(ragged=True) and DiffSingerE2EInfer.forward_batch(ragged=True, seeds=) with the FFT denoiser

At the parent commit every test here fails: sample(lengths=) raises NotImplementedError, FFT.forward takes no lengths, the symbols are missing.
"""
from ctypes import byref, c_int32

import numpy as np
import pytest
import torch

from bisinger_amd import _lib
from bisinger_amd.hparams import hparams
from tests import fftden_ragged_cases as RC
from tests.util import use_config

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
T_ = torch.from_numpy
EINVAL = -22


class _Enc:
    def __len__(self):
        return 65

    def pad(self):
        return 0


def _model(gain=None):
    from bisinger_amd.diffusion import GaussianDiffusion
    net = RC.build_net(gain)
    use_config('diff_decoder_type=fft')
    try:
        m = GaussianDiffusion(_Enc(), 80, net, timesteps=100, K_step=100, spec_min=hparams['spec_min'], spec_max=hparams['spec_max'])
    finally:
        use_config()
    return m.cuda().eval()


@pytest.fixture(scope='module')
def model():
    return _model()


@pytest.fixture(scope='module')
def model_plms():
    return _model(RC.PLMS_GAIN)


@pytest.fixture(scope='module')
def sd():
    return RC.oracle_sd()


def _clean(before, net):
    assert _lib.range_retries == before and net.gemm_range_peek() == 0, 'a range event fired: the call was repeated on the fp32 matrix pipe'


def _check_row(kind, tag, b, n, got_row, want):
    d, bar = float(np.abs(got_row.astype(np.float64) - want).max()), RC.bound(kind, want)
    print(f'  {tag} row {b} (n={n}): {kind} {d:.2e} (allowed {bar:.2e}; max |want| {np.abs(want).max():.2f})')
    assert np.isfinite(got_row).all() and d <= bar, (tag, b, n, d, bar)


def _nan_beyond(a, lens):
    a = a.copy()
    for b, n in enumerate(lens):
        a[b, ..., n:] = np.nan
    return a


# ------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(RC.FWD_CASES)), ids=[RC.name(c) for c in RC.FWD_CASES])
def test_forward_each_row_vs_fp64_alone(i, model):
    net = model.denoise_fn
    case = RC.FWD_CASES[i]
    lens, T, attn, gemm = case
    x, t, cond = RC.fwd_inputs(case)
    before = _lib.range_retries
    eps = net(T_(x).cuda(), T_(t).cuda(), T_(cond).cuda(), lengths=lens)
    path = net.last_path().split()
    _clean(before, net)
    assert path[0] == 'den.ragged' and all(p.startswith('den.') for p in path), path
    assert f'den.attn:{attn}' in path, (path, attn)
    assert {p for p in path if p.startswith('den.gemm:')} == {'den.gemm:' + g for g in gemm}, (path, gemm)
    assert tuple(eps.shape) == (len(lens), 1, RC.M, T)
    got = eps[:, 0].cpu().numpy()
    for b, n in enumerate(lens):
        _check_row('eps', RC.name(case), b, n, got[b, :, :n], RC.eps_alone_case(i, b, RC.F64))
        assert not got[b, :, n:].any(), (b, n, 'eps is not exactly 0 beyond the row')
    # nothing at or beyond a row's end is read
    eps_nan = net(T_(_nan_beyond(x, lens)).cuda(), T_(t).cuda(), T_(_nan_beyond(cond, lens)).cuda(), lengths=lens)
    assert torch.equal(eps_nan, eps)
    if all(n == T for n in lens):      # every row full: the padded call (whose record has no den.ragged token)
        padded = net(T_(x).cuda(), T_(t).cuda(), T_(cond).cuda())[:, 0].cpu().numpy()
        assert 'den.ragged' not in net.last_path().split()
        for b in range(len(lens)):
            _check_row('eps', RC.name(case) + ' against the padded call', b, T, got[b], padded[b].astype(np.float64))


def test_stale_workspace(model, sd):
    """A padded (2, 301) call, NaN bytes over every workspace, then lengths [5, 1] at T = 9: within the bound, and the same bits again."""
    net = model.denoise_fn
    B, T = RC.STALE['padded']
    rs = np.random.RandomState(5)
    long_ = net(T_(rs.standard_normal((B, 1, RC.M, T)).astype(np.float32)).cuda(), torch.tensor([3, 60]).cuda(),
                T_(rs.standard_normal((B, RC.H, T)).astype(np.float32)).cuda())
    assert bool(torch.isfinite(long_).all())
    net.poison_workspace()
    case = (RC.STALE['lens'], RC.STALE['T'], None)
    x, t, cond = RC.fwd_inputs(case)
    first = net(T_(x).cuda(), T_(t).cuda(), T_(cond).cuda(), lengths=case[0])
    for b, n in enumerate(case[0]):
        _check_row('eps', 'stale', b, n, first[b, 0, :, :n].cpu().numpy(), RC.eps_alone(sd, x, t, cond, b, n, RC.F64))
        assert not bool(first[b, 0, :, n:].any())
    net.poison_workspace()
    again = net(T_(x).cuda(), T_(t).cuda(), T_(cond).cuda(), lengths=case[0])
    assert torch.equal(again, first)


def test_forward_refuses_another_shape_than_the_binding(model):
    net = model.denoise_fn
    lib = _lib.load()
    cond = torch.randn(2, RC.H, 9).cuda()
    net.prepare(cond, (9, 4))
    x, eps, t = torch.randn(2, RC.M, 9).cuda(), torch.empty(2, RC.M, 9).cuda(), torch.tensor([1, 2]).cuda()
    for B, T in ((2, 8), (1, 9)):
        assert lib.bsg_fftden_forward(net._h, _lib.ptr(x), _lib.ptr(t), _lib.ptr(eps), B, T, _lib.stream_ptr()) == EINVAL
        assert 'does not match' in lib.bsg_last_error().decode()
    s, _keep = model._schedule()
    assert lib.bsg_fftden_ddpm_sample(net._h, byref(s), _lib.ptr(x), None, 0, None, 99, 1, 2, 8, 0, 2, _lib.stream_ptr()) == EINVAL
    assert lib.bsg_fftden_prepare_ragged(net._h, _lib.ptr(cond), (c_int32 * 2)(9, 10), 2, 9, _lib.stream_ptr()) == EINVAL
    torch.cuda.synchronize()


def test_capture_refuses_a_new_binding_and_takes_a_bound_sample(model):
    """The capture rules: a new ragged binding inside a capture is refused (BSG_ESTATE, nothing enqueued: the capture ends normally with
    its one marker node), and sample(lengths=) on the handle as it is already bound is captured; every replay gives the eager call's bits."""
    net = model.denoise_fn
    c = RC.DDPM
    cond, noise = RC.ddpm_inputs(c)
    condg, x0 = T_(cond).cuda(), T_(noise[0][:, None]).cuda().contiguous()
    eager = model.sample(condg, x0.clone(), seed=7, n_steps=2, lengths=c['lens'])      # binds condg with the lengths, sizes every workspace
    torch.cuda.synchronize()
    other = torch.randn(2, RC.H, 12).cuda()
    marker = torch.zeros(4, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        marker.fill_(1.0)
        with pytest.raises(_lib.BsgError, match='cannot be bound under stream capture'):
            net.prepare(other, (12, 3))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    # the refused call left the binding as it was: the same tensor and lengths, no new prepare
    xg = x0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=side):
        model.sample(condg, xg, seed=7, n_steps=2, lengths=c['lens'])
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        xg.copy_(x0)
        g2.replay()
        torch.cuda.synchronize()
        assert torch.equal(xg, eager)


# ------------------------------------------------------------------------------------------------------------------
# DDPM
# ------------------------------------------------------------------------------------------------------------------
def _ddpm_rows(tag, got, x0, lens, wants):
    for b, n in enumerate(lens):
        _check_row('ddpm', tag, b, n, got[b, 0, :, :n].cpu().numpy(), wants[b])
        assert torch.equal(got[b, :, :, n:], x0[b, :, :, n:]), (tag, b, 'x beyond the row changed')


def test_ddpm_supplied_noise(model, sd):
    c = RC.DDPM
    cond, noise = RC.ddpm_inputs(c)
    x0 = T_(noise[0][:, None]).cuda().contiguous()
    before = _lib.range_retries
    got = model.sample(T_(cond).cuda(), x0.clone(), noise=T_(noise[1:]).cuda(), n_steps=c['steps'], lengths=c['lens'])
    _clean(before, model.denoise_fn)
    assert model.denoise_fn.last_path().split()[0] == 'den.ragged'
    _ddpm_rows('noise', got, x0, c['lens'],
               [RC.ddpm_alone(sd, cond, noise[0][b], noise[1:, b, :, :n], b, n, c, RC.F64) for b, n in enumerate(c['lens'])])


def test_ddpm_row_seeds_two_compositions(model, sd):
    """Row b draws from the stream of its own seed at its own length: against the oracle fed the draws of bsg_philox_normal_rows, against
    the lone call sample(seed=row_seeds[b]) at T = n_b, and the same in another batch."""
    c = RC.DDPM
    lens, T, seeds = c['lens'], c['T'], list(RC.ROW_SEEDS)
    cond, noise = RC.ddpm_inputs(c)
    x0 = T_(noise[0][:, None]).cuda().contiguous()
    condg = T_(cond).cuda()
    got = model.sample(condg, x0.clone(), row_seeds=seeds, n_steps=c['steps'], lengths=lens)
    draws = torch.stack([_lib.philox_normal_rows(torch.empty(len(lens), RC.M, T, device='cuda'), RC.M, T, lens, seeds, c['t_start'] - k + 1)
                         for k in range(c['steps'])]).cpu().numpy()
    _ddpm_rows('row_seeds', got, x0, lens,
               [RC.ddpm_alone(sd, cond, noise[0][b], draws[:, b, :, :n], b, n, c, RC.F64) for b, n in enumerate(lens)])
    for b, n in enumerate(lens):      # the lone call under the row's seed (the padded loop, B = 1, T = n_b)
        lone = model.sample(condg[b:b + 1, :, :n].contiguous(), x0[b:b + 1, :, :, :n].contiguous(), seed=seeds[b], n_steps=c['steps'])
        _check_row('ddpm', 'against the lone call', b, n, got[b, 0, :, :n].cpu().numpy(), lone[0, 0].cpu().double().numpy())
    # another composition: rows 2 and 0 in other places, beside a row of another length
    o = RC.DDPM_OTHER
    rs = np.random.RandomState(99)
    n_x = o['extra_len']
    cond2 = np.concatenate([cond[list(o['order'])], rs.standard_normal((1, RC.H, T)).astype(np.float32)])
    x2 = np.concatenate([noise[0][list(o['order'])], rs.standard_normal((1, RC.M, T)).astype(np.float32)])[:, None]
    lens2 = [lens[i] for i in o['order']] + [n_x]
    seeds2 = [seeds[i] for i in o['order']] + [o['extra_seed']]
    got2 = model.sample(T_(cond2).cuda(), T_(x2).cuda().contiguous(), row_seeds=seeds2, n_steps=c['steps'], lengths=lens2)
    for place, b in enumerate(o['order']):
        n = lens[b]
        _check_row('ddpm', f'row {b} at place {place} of another batch', b, n, got2[place, 0, :, :n].cpu().numpy(),
                   got[b, 0, :, :n].cpu().double().numpy())
        _check_row('ddpm', f'row {b} at place {place} against float64', b, n, got2[place, 0, :, :n].cpu().numpy(),
                   RC.ddpm_alone(sd, cond, noise[0][b], draws[:, b, :, :n], b, n, c, RC.F64))


def test_ddpm_seed_draws_by_padded_index(model, sd):
    c = RC.DDPM
    lens, T = c['lens'], c['T']
    cond, noise = RC.ddpm_inputs(c)
    x0 = T_(noise[0][:, None]).cuda().contiguous()
    seed, row0, B_total = 4321, 1, 5
    got = model.sample(T_(cond).cuda(), x0.clone(), seed=seed, row0=row0, B_total=B_total, n_steps=c['steps'], lengths=lens)
    draws = torch.stack([model.philox_normal((len(lens), RC.M, T), 'cuda', seed, c['t_start'] - k + 1, row0 * RC.M * T)
                         for k in range(c['steps'])]).cpu().numpy()
    _ddpm_rows('seed', got, x0, lens,
               [RC.ddpm_alone(sd, cond, noise[0][b], draws[:, b, :, :n], b, n, c, RC.F64) for b, n in enumerate(lens)])


def test_ddpm_entry_on_a_padded_binding(model, sd):
    """bsg_fftden_ddpm_sample called directly on a padded binding (2 x 40): the fused tail where no row ends."""
    c = RC.DDPM_PADDED
    B, T = c['B'], c['T']
    net, lib = model.denoise_fn, _lib.load()
    cond, noise = RC.ddpm_inputs(c, B)
    condg, x = T_(cond).cuda(), T_(noise[0][:, None]).cuda().contiguous()
    nz = T_(noise[1:]).cuda().contiguous()
    net.prepare(condg)
    s, _keep = model._schedule()
    before = _lib.range_retries
    _lib.check(lib.bsg_fftden_ddpm_sample(net._h, byref(s), _lib.ptr(x), _lib.ptr(nz), 0, None, c['t_start'], c['steps'], B, T, 0, B,
                                          _lib.stream_ptr()), 'bsg_fftden_ddpm_sample')
    torch.cuda.synchronize()
    _clean(before, net)
    assert 'den.ragged' not in net.last_path().split()
    for b in range(B):
        _check_row('ddpm', 'padded binding', b, T, x[b, 0].cpu().numpy(), RC.ddpm_alone(sd, cond, noise[0][b], noise[1:, b], b, T, c, RC.F64))


# ------------------------------------------------------------------------------------------------------------------
# PLMS
# ------------------------------------------------------------------------------------------------------------------
def test_plms_ragged_and_padded_binding(model_plms):
    c = RC.PLMS
    lens, T = c['lens'], c['T']
    sdp = RC.oracle_sd(RC.PLMS_GAIN)
    net, lib = model_plms.denoise_fn, _lib.load()
    cond, xT = RC.plms_inputs()
    condg, x0 = T_(cond).cuda(), T_(xT[:, None]).cuda().contiguous()
    prev = hparams.get('pndm_speedup')
    hparams['pndm_speedup'] = c['interval']
    try:
        before = _lib.range_retries
        got = model_plms.sample(condg, x0.clone(), lengths=lens)
        _clean(before, net)
    finally:
        hparams['pndm_speedup'] = prev
    assert net.last_path().split()[0] == 'den.ragged'
    for b, n in enumerate(lens):
        _check_row('plms', 'ragged', b, n, got[b, 0, :, :n].cpu().numpy(), RC.plms_alone(sdp, cond, xT, b, n, c, RC.F64))
        assert torch.equal(got[b, :, :, n:], x0[b, :, :, n:]), (b, 'x beyond the row changed')
    # the entry on a padded binding: every row at T
    net.prepare(condg)
    x = x0.clone()
    s, _keep = model_plms._schedule()
    _lib.check(lib.bsg_fftden_plms_sample(net._h, byref(s), _lib.ptr(x), c['K_step'], c['interval'], len(lens), T, _lib.stream_ptr()),
               'bsg_fftden_plms_sample')
    torch.cuda.synchronize()
    _clean(before, net)
    for b in range(len(lens)):
        _check_row('plms', 'padded binding', b, T, x[b, 0].cpu().numpy(), RC.plms_alone(sdp, cond, xT, b, T, c, RC.F64))


# ------------------------------------------------------------------------------------------------------------------
# through the top
# ------------------------------------------------------------------------------------------------------------------
def test_forward_ragged_each_row_vs_fp64_pipeline(gd_sd):
    """GaussianDiffusion.forward(infer=True, ragged=True, noise=) with diff_decoder_type=fft on 2 rows of 40 and 25 frames: each row's
    mel_out against the float64 pipeline with the diffusion on that row alone (RC.top_reference), at RC.TOP_BAR — the derived bar
    (4 x the float32 pipeline's 1.52e-6 x max |want| 6.0 = 3.6e-5) lies below the project's 1e-3 for sampled mels, so 1e-3 it is."""
    from bisinger_amd.diffnet import DIFF_DECODERS
    from bisinger_amd.diffusion import GaussianDiffusion
    full = RC.top_state_dict(gd_sd)
    use_config('diff_decoder_type=fft')
    try:
        m = GaussianDiffusion(_Enc(), 80, DIFF_DECODERS[hparams['diff_decoder_type']](hparams), timesteps=100, K_step=100,
                              spec_min=hparams['spec_min'], spec_max=hparams['spec_max'])
        missing, unexpected = m.load_state_dict(full, strict=False)
        assert not unexpected and all(k.endswith('_float_tensor') for k in missing), (missing, unexpected)
        m = m.cuda().eval()
        inp, noise = RC.top_inputs()
        d = {k: T_(v).cuda() for k, v in inp.items()}
        kw = {k: d[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')}
        before = _lib.range_retries
        out = m(d['txt_tokens'], mel2ph=d['mel2ph'], spk_embed=d['spk_embed'], infer=True, noise=T_(noise).cuda(), ragged=True, **kw)
        assert _lib.range_retries == before
        assert m.denoise_fn.last_path().split()[0] == 'den.ragged'
        with pytest.raises(NotImplementedError):      # rows= with ragged=True stays refused
            m(d['txt_tokens'], mel2ph=d['mel2ph'], spk_embed=d['spk_embed'], infer=True, ragged=True, rows=slice(0, 1), **kw)
    finally:
        use_config()
    mel = out['mel_out'].cpu().numpy()
    want = RC.top_reference(full, inp, noise, RC.F64)
    for b, n in enumerate(RC.TOP['lens']):
        dev = float(np.abs(mel[b, :n].astype(np.float64) - want[b]).max())
        print(f'  top row {b} (n={n}): mel_out {dev:.2e} (allowed {RC.TOP_BAR:.0e}; derived {4 * RC.MEASURED_F32_TOP * np.abs(want[b]).max():.1e})')
        assert np.isfinite(mel[b]).all() and dev <= RC.TOP_BAR, (b, dev)
        assert not mel[b, n:].any(), (b, 'mel_out is not 0 beyond the row')


@pytest.fixture
def fft_workdir(tmp_path, gd_sd, hifigan_sd, monkeypatch):
    """The synthetic checkpoint directory of tests/test_gpu_infer.py with the FFT denoiser in the model checkpoint and the config."""
    import json
    import os

    import yaml

    from tests.util import ROOT
    monkeypatch.chdir(tmp_path)
    os.makedirs('checkpoints/exp_fft')
    os.makedirs('checkpoints/hifigan')
    os.makedirs('data/binary')
    full = RC.top_state_dict(gd_sd)
    full['fs2.decoder.embed_positions._float_tensor'] = torch.zeros(1)
    full['denoise_fn.embed_positions._float_tensor'] = torch.zeros(1)
    torch.save({'state_dict': {'model.' + k: v for k, v in full.items()}, 'global_step': 1000}, 'checkpoints/exp_fft/model_ckpt_steps_1000.ckpt')
    torch.save({'state_dict': {'model_gen': hifigan_sd}}, 'checkpoints/hifigan/model_ckpt_steps_5.ckpt')
    hcfg = yaml.safe_load(open(f'{ROOT}/bisinger_amd/configs/hifigan.yaml'))
    yaml.safe_dump(hcfg, open('checkpoints/hifigan/config.yaml', 'w'))
    json.dump(['<AP>', '<SP>'] + [f'p{i}' for i in range(60)], open('data/binary/phone_set.json', 'w'))
    json.dump({'Tenor-1': 3, 'Alto-2': 7}, open('data/binary/spk_map.json', 'w'))
    cfg = {'base_config': f'{ROOT}/bisinger_amd/configs/bisinger_diff100.yaml', 'binary_data_dir': 'data/binary', 'diff_decoder_type': 'fft',
           'vocoder_ckpt': 'checkpoints/hifigan', 'pe_enable': False, 'use_nsf': False, 'max_frames': 5000}
    yaml.safe_dump(cfg, open('exp.yaml', 'w'))
    return tmp_path


def test_forward_batch_same_item_same_seed_in_two_buckets(fft_workdir):
    """forward_batch(items, ragged=True, ragged_front=True, seeds=) with diff_decoder_type=fft: bucketed by 3 and by 2, every item lands in
    another bucket and row place and keeps its mel.  Both runs are the row alone under its own seed, each within 4 x MEASURED_F32_TOP x max |mel| of the float64 pipeline
    (the derived bar of the test above), so the two lie within twice that of each other: about 7e-5."""
    from bisinger_amd.candidate_decoder import FFT
    from bisinger_amd.hparams import set_hparams
    from bisinger_amd.infer import DiffSingerE2EInfer
    from tests import e2e_ragged_cases as E
    try:
        E.raise_checkpoint('checkpoints/exp_fft/model_ckpt_steps_1000.ckpt')      # (the duration predictor's bias: every item gets frames)
        set_hparams('exp.yaml', exp_name='exp_fft', print_hparams=False, hparams_str='seed=4321')
        infer = DiffSingerE2EInfer(hparams)
        assert isinstance(infer.model.denoise_fn, FFT)
        items = E.items()
        seeds = (101, 2024, 7, 99991, 31337)
        mels, inner = [], infer.model.forward

        def recording(*a, **k):
            out = inner(*a, **k)
            mels.append(out['mel_out'].cpu().numpy())
            return out
        infer.model.forward = recording
        runs = []
        for ms in (3, 2):
            del mels[:]
            wavs = infer.forward_batch(items, seeds=seeds, max_sentences=ms, ragged=True, ragged_front=True)
            st = infer.last_batch_stats
            assert infer.model.denoise_fn.last_path().split()[0] == 'den.ragged'
            assert len(mels) == len(st['buckets']) and all(np.isfinite(w).all() for w in wavs)
            per_item = {}
            for k, bk in enumerate(st['buckets']):
                for row, i in enumerate(bk):
                    per_item[i] = mels[k][row, :st['frames'][i]]
                    assert not mels[k][row, st['frames'][i]:].any()
            runs.append((per_item, [tuple(b) for b in st['buckets']]))
        infer.model.forward = inner
    finally:
        use_config()
    assert runs[0][1] != runs[1][1] and len(runs[0][1]) == 2 and len(runs[1][1]) == 3
    for i in range(len(items)):
        a, b = runs[0][0][i], runs[1][0][i]
        dev = float(np.abs(a.astype(np.float64) - b).max())
        bar = 2 * 4 * RC.MEASURED_F32_TOP * max(1.0, float(np.abs(a).max()))
        print(f'  item {i} (n={a.shape[0]}): mel in buckets {runs[0][1]} against {runs[1][1]}: {dev:.2e} (allowed {bar:.1e})')
        assert a.shape == b.shape and dev <= bar, (i, dev, bar)
