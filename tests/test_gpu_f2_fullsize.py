"""GPU parity at production length, SURVEY.md §8 row f2: the NSF harmonic source, NSF-HiFiGAN and the PitchExtractor against the
float64 evaluation of the CPU oracle (oracle/nsf.py, oracle/pe.py).  The float32 evaluation of the same oracle is the yardstick: each
kernel may deviate from float64 by twice what the fp32 oracle does, plus a small floor.  tests/test_gpu_f2.py pins the same modules to
the reference's goldens at toy sizes (T <= 133); here the lengths are the ones production runs (T = 1000 .. 4000 frames, up to
1 024 000 samples per harmonic), where the source's two cumulative sums over T*hop samples lose precision if their phase is not kept
bounded."""
from collections import OrderedDict

import numpy as np
import pytest
import torch
import yaml

from bisinger_amd import _lib, synth
from oracle import nsf as onsf, pe as ope
from tests import pe_cases
from tests.util import ROOT

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SR, HOP, NH = 22050, 256, 9
F64, F32 = torch.float64, torch.float32


def _maxabs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def notes_f0(rs, T):
    """A sung contour: notes of 80..1100 Hz with vibrato, some separated by unvoiced gaps; the first frame unvoiced, the last voiced."""
    fps = SR / HOP
    f0 = np.zeros(T)
    t = int(rs.randint(1, 12))
    while t < T:
        n = min(int(rs.randint(15, 160)), T - t)
        base = np.exp(rs.uniform(np.log(85), np.log(1050)))
        depth, rate, ph = rs.uniform(0.005, 0.03), rs.uniform(4.5, 7.0), rs.uniform(0, 2 * np.pi)
        f0[t:t + n] = base * (1 + depth * np.sin(2 * np.pi * rate * np.arange(n) / fps + ph))
        t += n
        if rs.rand() < 0.5:
            t += int(rs.randint(3, 30))
    f0[0] = 0
    if f0[-1] == 0:
        f0[-5:] = 220.0
    return np.clip(f0, 0, 1100).astype(np.float32)


@pytest.fixture(scope='module')
def nsf(sd_spec):
    """NSF-HiFiGAN on formula weights of seed 13 (as tests/test_gpu_f2.py), weight norm folded; with the checkpoint-layout state dict."""
    from bisinger_amd.hifigan import HifiGanGenerator
    cfg = yaml.safe_load(open(f'{ROOT}/bisinger_amd/configs/hifigan.yaml'))
    cfg['use_pitch_embed'] = True
    spec = OrderedDict((k, tuple(s)) for k, s in sd_spec['HifiGanGenerator_nsf_weight_norm'])
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(spec, seed=13).items()}
    gen = HifiGanGenerator(cfg)
    gen.load_state_dict(sd, strict=True)
    gen = gen.cuda()
    gen.remove_weight_norm()
    return gen, sd, cfg


@pytest.fixture(scope='module')
def pitch_ext(sd_spec):
    """PitchExtractor on formula weights of seed 11 with tests/test_gpu_f2.py's running statistics."""
    pe = pe_cases.pitch_extractor(sd_spec).cuda()
    return pe, pe_cases.cpu_state_dict(pe)


def hip_source(f0, rand_ini, noise, lin_w, lin_b, HOP=HOP):
    """bsg_nsf_source: (har [B,L], sines [B,NH,L]) as float64 numpy; NH from rand_ini."""
    B, T = f0.shape
    NH = rand_ini.shape[1]
    L = T * HOP
    dev = torch.device('cuda')
    f0_d, ri_d, nz_d = (torch.from_numpy(a).to(dev).contiguous() for a in (f0, rand_ini, noise))
    w_d, b_d = lin_w.to(dev, F32).contiguous(), lin_b.to(dev, F32).contiguous()
    har = torch.full((B, L), float('nan'), device=dev)
    sines = torch.full((B, NH, L), float('nan'), device=dev)
    _lib.check(_lib.load().bsg_nsf_source(_lib.ptr(f0_d), _lib.ptr(ri_d), _lib.ptr(nz_d), _lib.ptr(w_d), _lib.ptr(b_d), _lib.ptr(har),
                                          _lib.ptr(sines), B, T, HOP, NH, SR, _lib.stream_ptr()), 'bsg_nsf_source')
    torch.cuda.synchronize()
    har2 = torch.full((B, L), float('nan'), device=dev)      # without `sines`: its own workspace, the same arithmetic
    _lib.check(_lib.load().bsg_nsf_source(_lib.ptr(f0_d), _lib.ptr(ri_d), _lib.ptr(nz_d), _lib.ptr(w_d), _lib.ptr(b_d), _lib.ptr(har2),
                                          None, B, T, HOP, NH, SR, _lib.stream_ptr()), 'bsg_nsf_source')
    torch.cuda.synchronize()
    assert torch.equal(har, har2)
    return har.double().cpu().numpy(), sines.double().cpu().numpy()


# B = 3 rows: a sung contour; f0 = sr/4 throughout, so every harmonic's rad is a multiple of 1/4 and the first cumsum lands on exact
# integers (the wrap test sees cur == 0); all unvoiced (noise only).  T = 1: one sample per thread, most of the 256 threads empty.
@pytest.mark.parametrize('B,T', [(1, 1000), (3, 1000), (1, 4000), (3, 4000), (3, 1)])
def test_nsf_source_vs_fp64(B, T, nsf):
    _, sd, _ = nsf
    rs = np.random.RandomState(1000 * B + T)
    f0 = np.zeros((B, T), np.float32)
    f0[0] = notes_f0(rs, T) if T > 1 else 440.0
    if B > 1:
        f0[1] = SR / 4
        f0[2] = 0
    _check_source(f'nsf_source B={B} T={T}', rs, f0, sd, HOP, NH)


def _check_source(tag, rs, f0, sd, hop, nh):
    """bsg_nsf_source on f0 [B, T] at `hop` samples per frame and `nh` harmonics against oracle.nsf.sine_waves in float64."""
    B, T = f0.shape
    rand_ini = rs.uniform(0, 1, size=(B, nh)).astype(np.float32)
    noise = rs.standard_normal((B, T * hop, nh)).astype(np.float32)
    lin_w, lin_b = sd['m_source.l_linear.weight'][:, :nh].contiguous(), sd['m_source.l_linear.bias']
    har, sines = hip_source(f0, rand_ini, noise, lin_w, lin_b, hop)
    assert np.isfinite(har).all() and np.isfinite(sines).all()
    dev = np.zeros(nh)
    dev32 = np.zeros(nh)
    dev_har = dev32_har = 0.0
    for b in range(B):        # the oracle one row at a time: at T = 4000 a row is 9 x 1 024 000 samples
        args = (torch.from_numpy(f0[b:b + 1]), torch.from_numpy(rand_ini[b:b + 1]), torch.from_numpy(noise[b:b + 1]), SR, hop, nh - 1)
        w64 = onsf.sine_waves(*args, dtype=F64)
        w32 = onsf.sine_waves(*args, dtype=F32)
        h64 = torch.tanh(torch.nn.functional.linear(w64, lin_w.double(), lin_b.double()))[0, :, 0].numpy()
        h32 = torch.tanh(torch.nn.functional.linear(w32, lin_w, lin_b))[0, :, 0].double().numpy()      # oracle.nsf.sine_source in fp32
        w64, w32 = w64[0].T.numpy(), w32.double()[0].T.numpy()
        dev = np.maximum(dev, np.abs(sines[b] - w64).max(1))
        dev32 = np.maximum(dev32, np.abs(w32 - w64).max(1))
        dev_har = max(dev_har, _maxabs(har[b], h64))
        dev32_har = max(dev32_har, _maxabs(h32, h64))
    # per harmonic: 2 x the fp32 oracle's deviation, at least 2e-4 (0.2 % of the sine amplitude 0.1)
    bar = np.maximum(2 * dev32, 2e-4)
    # merged: the per-harmonic floor through l_linear (tanh' <= 1)
    bar_har = max(2 * dev32_har, 2e-4 * max(1.0, float(lin_w.abs().sum())))
    print(f'{tag}: per harmonic hip {np.array2string(dev, precision=2)} fp32 oracle {np.array2string(dev32, precision=2)}; '
          f'merged hip {dev_har:.2e} fp32 oracle {dev32_har:.2e}')
    assert (dev <= bar).all(), (dev, bar)
    assert dev_har <= bar_har, (dev_har, bar_har)
    # the kernel forms rad and carries the phase in fp64: only its fp32 sin, noise term and store round (a phase carried in fp32, or
    # rad rounded to fp32 as the fp32 oracle does, is 1e-5 .. 1e-4 off here)
    assert dev.max() <= 1e-6 and dev_har <= 1e-6, (dev, dev_har)


# hop != 256: a thread's share S = ceil(T * hop / 256) samples no longer ends on a frame boundary, and L is no multiple of 256.
# (3, 100): L = 300, S = 2, threads 150 .. 255 empty; (7, 300): the PWG hop, S = 9 over frames of 300; hop = 1: every sample its own
# frame, L = 255 (S = 1, one thread empty), L = 257 (S = 2, the last thread's share is one sample) and L = 5; NH = 1 and 2 harmonics.
@pytest.mark.parametrize('T,hop,nh', [(3, 100, 9), (7, 300, 9), (255, 1, 9), (257, 1, 1), (5, 1, 2)])
def test_nsf_source_odd_hops_vs_fp64(T, hop, nh, nsf):
    _, sd, _ = nsf
    rs = np.random.RandomState(T * 1000 + hop + nh)
    f0 = np.zeros((3, T), np.float32)
    f0[0] = notes_f0(rs, T) if T > 16 else np.resize(np.float32([0, 440, 523.25, 0, 87.3, 1046.5, 330]), T)
    f0[1] = SR / 4
    f0[2, T // 2:] = 220.0        # unvoiced, then voiced from the middle frame on
    _check_source(f'nsf_source T={T} hop={hop} NH={nh}', rs, f0, sd, hop, nh)


@pytest.mark.parametrize('B', [1, 8])
def test_nsf_hifigan_fullsize_vs_fp64(B, nsf):
    """The whole NSF generator at T = 1000 in its default forms: the source and nsf_source_add_kernel at the 64/32/16/8-channel stages on
    top of the tile forms tests/test_gpu_hifigan.py's throughput test covers for the plain generator."""
    gen, sd, cfg = nsf
    T = 1000
    rs = np.random.RandomState(77 + B)
    mel = (rs.standard_normal((B, 80, T)) * 1.5 - 3.0).astype(np.float32)
    f0 = np.stack([notes_f0(rs, T) for _ in range(B)])
    rand_ini = rs.uniform(0, 1, size=(B, NH)).astype(np.float32)
    noise = rs.standard_normal((B, T * HOP, NH)).astype(np.float32)
    got = gen(torch.from_numpy(mel).cuda(), torch.from_numpy(f0).cuda(), rand_ini=torch.from_numpy(rand_ini),
              noise=torch.from_numpy(noise)).double().cpu().numpy()
    assert got.shape == (B, 1, T * HOP) and np.isfinite(got).all()
    _check_generator(f'nsf_hifigan B={B} T={T}', got, sd, cfg, mel, f0, rand_ini, noise)


def _check_generator(tag, got, sd, cfg, mel, f0, rand_ini, noise):
    dev = dev32 = 0.0
    scale = 1.0
    for b in range(got.shape[0]):
        args = (sd, torch.from_numpy(mel[b:b + 1]), torch.from_numpy(f0[b:b + 1]), torch.from_numpy(rand_ini[b:b + 1]),
                torch.from_numpy(noise[b:b + 1]), cfg)
        want = onsf.nsf_hifigan_forward(*args, dtype=F64).numpy()
        w32 = onsf.nsf_hifigan_forward(*args, dtype=F32).double().numpy()
        scale = max(scale, float(np.abs(want).max()))
        dev = max(dev, _maxabs(got[b:b + 1], want))
        dev32 = max(dev32, _maxabs(w32, want))
    print(f'{tag}: hip {dev:.2e} fp32 oracle {dev32:.2e} (scale {scale:.2f})')
    assert dev <= 2 * dev32 + 5e-5 * scale, (dev, dev32)
    # the fp32 oracle's own deviation is mostly its fp32 source amplified by the noise convs; with the source at fp32 rounding the NSF
    # generator meets the plain generator's bar (tests/test_gpu_hifigan.py) as well
    assert dev <= 5e-5 * scale, (dev, dev32)


def _check_pitch(tag, r, sd, mel, lens):
    """pitch_pred within 2 x the fp32 oracle's deviation + 2e-5 of its scale; f0 where the voicing logit is clear of 0; 0 past each row."""
    want = ope.pitch_extractor_forward(sd, torch.from_numpy(mel), dtype=F64)
    w32 = ope.pitch_extractor_forward(sd, torch.from_numpy(mel), dtype=F32)
    pp, pp64 = r['pitch_pred'].double().cpu().numpy(), want['pitch_pred'].numpy()
    dev, dev32 = _maxabs(pp, pp64), _maxabs(w32['pitch_pred'].double().numpy(), pp64)
    scale = max(1.0, float(np.abs(pp64).max()))
    bar = 2 * dev32 + 2e-5 * scale
    print(f'{tag}: pitch_pred hip {dev:.2e} fp32 oracle {dev32:.2e} (scale {scale:.2f})')
    assert dev <= bar, (dev, dev32)
    f0, f064 = r['f0_denorm_pred'].double().cpu().numpy(), want['f0_denorm_pred'].numpy()
    clear = np.abs(pp64[..., 1]) > 10 * bar          # voicing decided by a sign test: frames within 10 bars of 0 may flip
    assert clear.mean() > 0.9 and (f064[clear] > 0).any()
    assert ((f0 > 0) == (f064 > 0))[clear].all()
    rel = np.abs(f0 - f064)[clear] / np.maximum(f064[clear], 1e-30)
    assert (rel[f064[clear] > 0] <= 2 ** bar - 1 + 1e-6).all(), float(rel.max())
    for b, n in enumerate(lens):
        assert (f0[b, n:] == 0).all() and (f064[b, n:] == 0).all()
    return f0.astype(np.float32)


def _mel(rs, B, T, lens):
    mel = (rs.standard_normal((B, T, 80)) * 1.5 - 3.0).astype(np.float32)
    for b, n in enumerate(lens):
        mel[b, n:] = 0
    return mel


@pytest.mark.parametrize('B,T', [(16, 1000), (1, 3000)])
def test_pitch_extractor_fullsize_vs_fp64(B, T, pitch_ext):
    """B = 16 padded to T = 1000 (rows of different lengths, mel exactly 0 past each): GroupNorm's statistics run over all T frames of a
    row, padding included, as in the reference, so the target is the oracle on the padded batch.  B = 1 at T = 3000."""
    pe, sd = pitch_ext
    rs = np.random.RandomState(5 + B)
    lens = [T] if B == 1 else [T] + sorted(rs.randint(120, T, size=B - 1).tolist(), reverse=True)
    mel = _mel(rs, B, T, lens)
    r = pe(torch.from_numpy(mel).cuda())
    _check_pitch(f'pitch_extractor B={B} T={T}', r, sd, mel, lens)


def test_f2_chain_fullsize_vs_fp64(pitch_ext, nsf):
    """mel -> HIP PitchExtractor -> f0 -> HIP NSF-HiFiGAN at B = 2, T = 1000; the NSF oracle is fed the GPU's f0 (as the e2e test does) so a
    voicing decision within rounding of 0 cannot flip a frame between the two sides."""
    pe, pe_sd = pitch_ext
    gen, sd, cfg = nsf
    B, T = 2, 1000
    rs = np.random.RandomState(2024)
    mel = _mel(rs, B, T, [T, T])
    mel_d = torch.from_numpy(mel).cuda()
    r = pe(mel_d)
    f0 = _check_pitch(f'f2 chain PE B={B} T={T}', r, pe_sd, mel, [T, T])
    assert (f0 > 0).any()
    rand_ini = rs.uniform(0, 1, size=(B, NH)).astype(np.float32)
    noise = rs.standard_normal((B, T * HOP, NH)).astype(np.float32)
    mel_t = mel.transpose(0, 2, 1).copy()
    got = gen(torch.from_numpy(mel_t).cuda(), r['f0_denorm_pred'], rand_ini=torch.from_numpy(rand_ini),
              noise=torch.from_numpy(noise)).double().cpu().numpy()
    _check_generator(f'f2 chain NSF B={B} T={T}', got, sd, cfg, mel_t, f0, rand_ini, noise)
