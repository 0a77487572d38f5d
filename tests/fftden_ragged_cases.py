"""Cases, inputs, weights and bounds of the ragged FFT-denoiser tests (tests/test_fftden_ragged_cpu.py, tests/test_gpu_fftden_ragged.py).  No GPU.

Reference of every test: ``oracle.candidate_decoder.fft_denoiser_forward(..., dtype=float64)`` on each row's OWN slice (B = 1, T = n_b) and
``oracle.diffusion`` for the loops — never the code under test.

Bounds.  For each compared quantity the float32 restatement of the oracle was evaluated against the float64 oracle on the CPU over every
case of this module (tests/test_fftden_ragged_cpu.py::test_bounds_cover_the_float32_restatement does it again and holds every figure to
bound / 4); MEASURED_F32 records the largest figure, rounded up in its third digit (float32 CPU kernels differ in their last bits with the
thread count).  Bound = 4 x that figure x max(1, max |want|): the margin this project gives a split-fp16, fp32-grade GPU path over an fp32
CPU restatement.  It is the float32 ORACLE's error, never the device's.

Separation (checked on the CPU): for every ragged case with a short row — eps of the forward cases, x after the DDPM run, x after the PLMS
run — the float64 PADDED result of that row (the reference's own behaviour: padded frames stay live) differs from its row-alone result by
at least 1000 x the bound, so no test here could pass on a padded evaluation.
"""
import json
import os
from collections import OrderedDict

import numpy as np
import torch

from bisinger_amd import synth
from oracle import candidate_decoder as ocd, diffusion as odf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
M, H = 80, 256

# A figure is max |got - want| / max(1, max |want|) of one row.  Largest float32-oracle figures over the cases below, over runs with 1, 2, 4
# and 8 CPU threads (where): eps 9.58e-7 (1537x64x32x8x2@1537 row 0 at 1 thread, max |want| 4.4; 9.21e-7 at 512x63x31x8x1@512 row 1 at 4
# and 8 threads, 9.19e-7 at 64x1@64 row 0 at 2), x after the 6 DDPM steps 3.03e-7 (the padded 2 x 40 binding, row 0, max |want| 4.4), x
# after the 21 PLMS evaluations 1.01e-7 (row 1 at T = 40, max |want| 0.31).
MEASURED_F32 = {'eps': 9.58e-7, 'ddpm': 3.03e-7, 'plms': 1.01e-7}
BOUND = {k: 4 * v for k, v in MEASURED_F32.items()}


def figure(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


def bound(kind, want):
    """The absolute bound on max |got - want| for this `want`."""
    return BOUND[kind] * max(1.0, float(np.abs(np.asarray(want)).max()))


# ---- forward: (row lengths, T, the attention token, the set of GEMM tokens) as bsg_fftden_last_path names them.
# Attention (csrc/fs2.hip plan_fft): the pre-split form ('planes') when 32 * ceil(T / 32) <= 3 T (T >= 11) and B * T >= 32, else
# 'split/nw2'; the keys of a query tile go over ks workgroups: ks doubles (up to 4) while units * ks * 2 <= 512 (units = ceil(T / 64) * B *
# heads) and ceil(T / 32) / (2 ks) >= 4.  At B <= 3 that is ks = 2 from T >= 225 and ks = 4 from T >= 481; at B = 5 the workgroup budget
# also counts: ks = 2 at T = 384 / 385 (ceil(T / 32) = 12 / 13), ks = 4 at 512 / 513, ks = 2 at 1536 .. 1600 (250 units) and ks = 1 from
# T = 1601 (260 units).
# GEMMs (csrc/gemm_h2w.hip launch_gemm_h2w, the forms with lengths): a product of one layer has ceil(T / 64) * (Wn / 128) * B workgroups
# of 64-row tiles; below 256 of them it runs on 32-row tiles ('h2w/32/deep', the k-tap FFN convolution 'h2w/32/ring16'), else on 64-row
# tiles ('h2w/64/ring8') while ceil(T / 128) * (Wn / 128) * B < 512, else on 128-row tiles ('h2w/128/ring4').  Wn / 128 is 8 for the FFN
# convolution, 6 for QKV, 2 for the two projections back to 256.  At B = 5 the thresholds in T are: 384 | 385 (FFN convolution leaves the
# 32-row tiles), 512 | 513 (QKV leaves them), 1536 | 1537 (FFN convolution reaches the 128-row tiles: the form of the B = 16, T = 1000
# benchmark shape), 1600 | 1601 (the projections leave the 32-row tiles).  The record is a SET of tokens per stack, so 512 | 513 changes
# no token (the projections still name 'h2w/32/deep'): that pair is run for its values.  Two further thresholds at B = 5 are left out for
# their cost on the CPU oracle: 2176 | 2177 (QKV on 128-row tiles, the same kernel as at 1537) and T >= 6529 for the projections, beyond
# the position table.  At B <= 3 every case below stays on the 32-row tiles (B = 3 leaves them at T >= 641).
# One batch on each side of every threshold; row lengths cover {1, 2, 8, 9, 10, 31, 32, 33, 63, 64, 65, 129, 130} (9: one FFN kernel;
# 32 / 64: the transposes' tile and the wave); B in {1, 2, 3, 5}.
G32 = ('h2w/32/deep', 'h2w/32/ring16')
G64 = ('h2w/32/deep', 'h2w/64/ring8')
FWD_CASES = [
    ((1,), 1, 'split/nw2', G32),
    ((31,), 31, 'split/nw2', G32),                      # B * T = 31 < 32
    ((32,), 32, 'planes/ks1', G32),
    ((33,), 40, 'planes/ks1', G32),                     # a lone row shorter than the pitch
    ((64, 1), 64, 'planes/ks1', G32),                   # one full row plus a 1-frame row
    ((9, 8), 9, 'split/nw2', G32),
    ((10, 2), 10, 'split/nw2', G32),                    # T = 10: 32 > 3 T
    ((15, 9), 15, 'split/nw2', G32),                    # T >= 11 but B * T = 30
    ((16, 10), 16, 'planes/ks1', G32),                  # B * T = 32
    ((10, 10, 10), 10, 'split/nw2', G32),
    ((11, 2, 1), 11, 'planes/ks1', G32),                # T = 11: 32 <= 3 T, B * T = 33
    ((32, 32, 32), 32, 'planes/ks1', G32),              # every row full: equals the padded call
    ((65, 63, 33), 65, 'planes/ks1', G32),
    ((130, 129, 64), 130, 'planes/ks1', G32),
    ((224, 129), 224, 'planes/ks1', G32),
    ((225, 224, 130, 9, 1), 225, 'planes/ks2', G32),
    ((480, 8), 480, 'planes/ks2', G32),
    ((481, 480, 65, 31, 2), 481, 'planes/ks4', G64),      # (B = 5: beyond 385 already)
    # B = 5 at the GEMM-form thresholds (the rows behind the long one are short: the oracle's cost is the long row's)
    ((384, 65, 33, 9, 1), 384, 'planes/ks2', G32),
    ((385, 64, 32, 10, 2), 385, 'planes/ks2', G64),
    ((512, 63, 31, 8, 1), 512, 'planes/ks4', G64),
    ((513, 130, 10, 2, 1), 513, 'planes/ks4', G64),
    ((1536, 129, 33, 9, 1), 1536, 'planes/ks2', G64),
    ((1537, 64, 32, 8, 2), 1537, 'planes/ks2', ('h2w/32/deep', 'h2w/64/ring8', 'h2w/128/ring4')),
    ((1600, 65, 31, 10, 1), 1600, 'planes/ks2', ('h2w/32/deep', 'h2w/64/ring8', 'h2w/128/ring4')),
    ((1601, 63, 9, 2, 1), 1601, 'planes/ks1', ('h2w/64/ring8', 'h2w/128/ring4')),
]
GEMM_FORMS = ('h2w/32/deep', 'h2w/32/ring16', 'h2w/64/ring8', 'h2w/128/ring4')      # every ragged form of launch_gemm_h2w
FULL_CASE = FWD_CASES[11]
STALE = dict(padded=(2, 301), lens=(5, 1), T=9)
DDPM = dict(lens=(77, 9, 1), T=77, t_start=99, steps=6, noise_seed=8)
DDPM_PADDED = dict(B=2, T=40, t_start=99, steps=6, noise_seed=9)
ROW_SEEDS = (20240917, 5, 0xFFFFFFFF00000003)      # (one beyond 32 bits: both key words are the row's)
# the second composition for the row-keyed draws: the same (row, seed) pairs in other places, beside another row
DDPM_OTHER = dict(order=(2, 0), extra_len=33, extra_seed=77)
PLMS = dict(lens=(40, 9), T=40, K_step=100, interval=5, xT_scale=1.0 / 128, noise_seed=10)
PLMS_GAIN = {'get_mel_out.weight': 0.02, 'get_mel_out.bias': 0.02}      # tests/cfg_fixtures.py SHIPPED: the mel stays O(10)
SCHEDULE = (100, 'linear', 0.06)


# ---- through the top: GaussianDiffusion.forward(ragged=True, noise=) with the FFT denoiser, 2 rows of 40 and 25 frames, the whole 100-step
# DDPM loop.  The float32 pipeline against the float64 one (top_reference) gives 1.52e-6 on mel_out (the 25-frame row) at max |want| 6.0, so the derived
# bar (4 x 1.52e-6 x 6.0 = 3.6e-5) lies BELOW the project's 1e-3 bar for sampled mels, and the tests use 1e-3 (the clamp of p_sample makes the
# loop contractive; 1e-3 is what tests/test_gpu_f4.py's generation holds the padded loop to on the same scale).
TOP = dict(B=2, T_txt=8, T=40, inp_seed=6, noise_seed=12, lens=(40, 25))
MEASURED_F32_TOP = 1.52e-6
TOP_BAR = 1e-3


def name(case):
    lens, T = case[:2]
    return 'x'.join(str(n) for n in lens) + f'@{T}'


def fft_spec():
    with open(os.path.join(ROOT, 'tests', 'golden', 'state_dict_spec.json')) as f:
        return OrderedDict((k, tuple(s)) for k, s in json.load(f)['FFT'])


def weights(gain=None):
    """Formula weights of seed 17 as numpy arrays (FFT.state_dict() keys but the computed position buffer)."""
    return synth.synth_state_dict(fft_spec(), seed=17, gain=gain)


def oracle_sd(gain=None):
    return {k: torch.from_numpy(v) for k, v in weights(gain).items()}


def build_net(gain=None):
    """The drop-in FFT denoiser with those weights (on the CPU; the caller moves it)."""
    from bisinger_amd.diffnet import DIFF_DECODERS
    from bisinger_amd.hparams import hparams
    from tests.util import use_config
    use_config('diff_decoder_type=fft')
    try:
        net = DIFF_DECODERS[hparams['diff_decoder_type']](hparams)
    finally:
        use_config()
    missing, unexpected = net.load_state_dict(oracle_sd(gain), strict=False)
    assert not unexpected and all(synth.is_computed_buffer(k) for k in missing), (missing, unexpected)
    return net


def fwd_inputs(case):
    """x [B,1,M,T], t [B], cond [B,H,T] of a forward case (numpy)."""
    lens, T = case[:2]
    B = len(lens)
    rs = np.random.RandomState(7000 + 31 * B + T)
    return (rs.standard_normal((B, 1, M, T)).astype(np.float32), np.array([7, 93, 50, 0, 99][:B], dtype=np.int64),
            rs.standard_normal((B, H, T)).astype(np.float32))


def eps_alone(sd, x, t, cond, b, n, dtype):
    """The denoiser on row b ALONE at T = n: [M, n] float64 numpy."""
    T_ = torch.from_numpy
    e = ocd.fft_denoiser_forward(sd, T_(x[b:b + 1, :, :, :n]), T_(t[b:b + 1]), T_(cond[b:b + 1, :, :n]), dtype=dtype)
    return e[0, 0].double().numpy()


_EPS = {}


def eps_alone_case(i, b, dtype):
    """eps_alone of row b of FWD_CASES[i] with the formula weights, computed once per process and shared by the tests (read only)."""
    key = (i, b, dtype)
    if key not in _EPS:
        x, t, cond = fwd_inputs(FWD_CASES[i])
        _EPS[key] = eps_alone(oracle_sd(), x, t, cond, b, FWD_CASES[i][0][b], dtype)
        _EPS[key].setflags(write=False)
    return _EPS[key]


def eps_padded(sd, x, t, cond, dtype=F64):
    """The reference's own padded evaluation of the whole batch: [B, M, T]."""
    T_ = torch.from_numpy
    return ocd.fft_denoiser_forward(sd, T_(x), T_(t), T_(cond), dtype=dtype)[:, 0].double().numpy()


def schedule():
    return odf.make_schedule(*SCHEDULE)


def ddpm_inputs(c, B=None):
    B = len(c['lens']) if B is None else B
    rs = np.random.RandomState(8100 + c['T'])
    cond = rs.standard_normal((B, H, c['T'])).astype(np.float32)
    noise = synth.synth_noise(c['steps'], B, M, c['T'], seed=c['noise_seed'])      # [steps + 1, B, M, T]: x_T, then the steps' draws
    return cond, noise


def ddpm_alone(sd, cond, xT, draws, b, n, c, dtype):
    """p_sample over the steps on row b alone at T = n.  xT [M, T'], draws [steps, M, n] (already cut and laid out for the row): [M, n]."""
    T_ = torch.from_numpy
    cb = T_(cond[b:b + 1, :, :n])
    den = lambda x_, t_: ocd.fft_denoiser_forward(sd, x_, t_, cb, dtype=dtype)
    sch = schedule()
    x = T_(np.ascontiguousarray(xT[None, None, :, :n])).to(dtype)
    for k in range(c['steps']):
        x = odf.p_sample(sch, den, x, torch.full((1,), c['t_start'] - k, dtype=torch.long), T_(np.ascontiguousarray(draws[k][None, None])).to(dtype))
    return x[0, 0].double().numpy()


def plms_inputs(c=PLMS):
    B = len(c['lens'])
    rs = np.random.RandomState(8200 + c['T'])
    cond = rs.standard_normal((B, H, c['T'])).astype(np.float32)
    xT = synth.synth_noise(1, B, M, c['T'], seed=c['noise_seed'])[0] * np.float32(c['xT_scale'])
    return cond, xT.astype(np.float32)


def plms_alone(sd, cond, xT, b, n, c, dtype):
    T_ = torch.from_numpy
    cb = T_(cond[b:b + 1, :, :n])
    den = lambda x_, t_: ocd.fft_denoiser_forward(sd, x_, t_, cb, dtype=dtype)
    x = odf.plms_sample(schedule(), den, T_(np.ascontiguousarray(xT[b:b + 1, None, :, :n])).to(dtype), c['K_step'], c['interval'])
    return x[0, 0].double().numpy()


# ---- through the top ---------------------------------------------------------------------------------------------------------
def top_state_dict(gd_sd):
    """The GaussianDiffusion state dict of the conftest fixture ``gd_sd`` (FS2 front, schedule, spec_min / spec_max) with the WaveNet
    denoiser's entries replaced by the FFT denoiser's formula weights of seed 17."""
    sd = {k: v for k, v in gd_sd.items() if not k.startswith('denoise_fn.')}
    sd.update({'denoise_fn.' + k: v for k, v in oracle_sd().items()})
    return sd


def top_inputs(c=TOP):
    inp = synth.synth_inputs(c['B'], c['T_txt'], c['T'], seed=c['inp_seed'], ragged=True)
    assert tuple(int(v) for v in (inp['mel2ph'] > 0).sum(-1)) == c['lens']
    return inp, synth.synth_noise(SCHEDULE[0], c['B'], M, c['T'], seed=c['noise_seed'])


def top_reference(sd, inp, noise, dtype):
    """mel_out of every row: the front as forward(ragged=True) runs it (the padded batch: without ragged_front the ESM attends over the
    batch axis), then the diffusion on the row ALONE — x_T, the draws and the condition cut to its frames — and the de-normalisation.
    -> list of [n_b, M] float64 numpy."""
    from oracle import fs2 as ofs2
    T_ = torch.from_numpy
    f = ofs2.fs2_forward(sd, {k: T_(v) for k, v in inp.items()}, 'fs2.', None, False, dtype)
    cond = f['decoder_inp'].transpose(1, 2)
    den_sd = {k[len('denoise_fn.'):]: v for k, v in sd.items() if k.startswith('denoise_fn.')}
    sch = schedule()
    nz = T_(noise).to(dtype)
    out = []
    for b, n in enumerate(int(v) for v in (T_(inp['mel2ph']) > 0).sum(-1)):
        cb = cond[b:b + 1, :, :n]
        den = lambda x_, t_: ocd.fft_denoiser_forward(den_sd, x_, t_, cb, dtype=dtype)
        x = odf.ddpm_sample(sch, den, nz[0][b:b + 1, None, :, :n], nz[1:][:, b:b + 1, None, :, :n], SCHEDULE[0])
        mel = odf.denorm_spec(x[:, 0].transpose(1, 2), sd['spec_min'].to(dtype), sd['spec_max'].to(dtype))
        out.append(mel[0].double().numpy())
    return out


# ---- the reference's own padded loops (the separation condition: a padded evaluation must lie far outside the bounds) --------------
def ddpm_padded(sd, cond, noise, c, dtype=F64):
    """p_sample over the steps on the whole padded batch, as the reference runs it: [B, M, T]."""
    T_ = torch.from_numpy
    cb = T_(cond)
    den = lambda x_, t_: ocd.fft_denoiser_forward(sd, x_, t_, cb, dtype=dtype)
    sch = schedule()
    x = T_(noise[0][:, None]).to(dtype)
    for k in range(c['steps']):
        x = odf.p_sample(sch, den, x, torch.full((x.shape[0],), c['t_start'] - k, dtype=torch.long), T_(noise[1 + k][:, None]).to(dtype))
    return x[:, 0].double().numpy()


def plms_padded(sd, cond, xT, c, dtype=F64):
    T_ = torch.from_numpy
    cb = T_(cond)
    den = lambda x_, t_: ocd.fft_denoiser_forward(sd, x_, t_, cb, dtype=dtype)
    return odf.plms_sample(schedule(), den, T_(xT[:, None]).to(dtype), c['K_step'], c['interval'])[:, 0].double().numpy()
