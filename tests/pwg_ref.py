"""Restatement of the Parallel WaveGAN generator forward (modules/parallel_wavegan/models/parallel_wavegan.py:135-168 with
layers/residual_block.py:91-129 and layers/upsample.py:106-183) from a state dict, in torch on the CPU, dtype-parametrised like
tests/wavden_ref.py: float64 is what the GPU tests compare the kernels with, float32 is what their tolerance is derived from.

Pinned against the reference's own run (tests/golden/pwg_*.npz, written by tools/make_golden_pwg.py): in float32 mode the largest
difference from the reference's output is 7.153e-07 (no-pitch form; 0 at B = 2, T = 40 and 7.153e-07 at B = 1, T = 3) and 1.490e-07 (pitch
form), asserted <= 1e-6 in tests/test_pwg_cpu.py.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from bisinger_amd import _lib

GENERATOR_PARAMS = dict(in_channels=1, out_channels=1, kernel_size=3, layers=30, stacks=3, residual_channels=64, gate_channels=128,
                        skip_channels=64, aux_channels=80, aux_context_window=2, dropout=0.0, use_weight_norm=True,
                        upsample_net='ConvInUpsampleNetwork', upsample_params={'upsample_scales': [4, 4, 4, 4]}, use_pitch_embed=False)
HOP = 256
GOLDEN_SEEDS = {'plain': 21, 'pitch': 22}                       # weights of tests/golden/pwg_<form>.npz (tools/make_golden_pwg.py)
GOLDEN_CASES = {'B2T40': (2, 40, 5), 'B1T3': (1, 3, 6)}         # tag -> (B, T, input seed)


def params(use_pitch_embed=False, **kw):
    p = dict(GENERATOR_PARAMS, upsample_params={'upsample_scales': [4, 4, 4, 4]}, use_pitch_embed=use_pitch_embed)
    p.update(kw)
    return p


def fold(sd):
    """remove_weight_norm on a state dict: weight = g v / ||v|| in float32, as torch folds it; `bias` stays in front of `weight`."""
    out = {}
    for k, v in sd.items():
        if k.endswith('.weight_g'):
            continue
        if k.endswith('.weight_v'):
            out[k[:-2]] = torch._weight_norm(v, sd[k[:-1] + 'g'], 0)
        else:
            out[k] = v
    return out


def make_inputs(B, T, seed, w=2, pitch=False, hop=HOP):
    """z [B, 1, T hop] N(0, 1), c [B, 80, T + 2 w] mel-like with the edge padding of vocoders/pwg.py:96 (, coarse pitch [B, T + 2 w])."""
    rs = np.random.RandomState(seed)
    z = rs.standard_normal((B, 1, T * hop)).astype(np.float32)
    mel = (rs.standard_normal((B, 80, T)) * 1.5 - 3.0).astype(np.float32)
    c = np.pad(mel, ((0, 0), (0, 0), (w, w)), 'edge')
    p = None
    if pitch:
        p = rs.randint(1, 256, size=(B, T)).astype(np.int64)
        p[:, T // 2:T // 2 + 2] = 1                      # an unvoiced stretch
        p = np.pad(p, ((0, 0), (w, w)), 'edge')
    return z, c, p


def _conv(x, w, b=None, d=1, pad=None):
    """Conv1d (zero padding `pad`, default `same`; dilation d) as F.conv1d — what the reference runs — except in float64 on a GPU, where the
    convolution libraries have no float64 form: there it is ONE matrix product over the stacked taps, the same sums."""
    K = w.shape[-1]
    pad = d * (K // 2) if pad is None else pad
    if not (x.is_cuda and x.dtype == torch.float64):
        return F.conv1d(x, w, b, padding=pad, dilation=d)
    xp = F.pad(x, (pad, pad)) if pad else x
    Lo = xp.shape[-1] - d * (K - 1)
    xs = xp if K == 1 else torch.cat([xp[:, :, k * d:k * d + Lo] for k in range(K)], dim=1)      # [B, K Cin, Lo], tap-major
    y = torch.matmul(w.permute(0, 2, 1).reshape(w.shape[0], -1), xs)
    return y if b is None else y + b[None, :, None]


def forward(sd, z, c, pitch=None, p=None, dtype=torch.float64, device='cpu', return_max=False, as_tensor=False, whole_batch=None):
    """sd: FOLDED state dict (tensors); z [B, 1, L], c [B, 80, T + 2 w], pitch [B, T + 2 w] int64 or None -> [B, 1, L] numpy in `dtype`.
    A small batch is evaluated in one piece, as the reference does it; a large one row by row (rows are independent, and a row of 1000
    frames already holds 128 x 256 000 pre-activations per layer); `whole_batch` = True / False decides it for the caller.
    `as_tensor`: the result stays a tensor on `device` (no copy to the host, no wait): what tools/bench_pwg.py times."""
    p = p or GENERATOR_PARAMS
    W = {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}
    z = torch.as_tensor(z).to(device=device, dtype=dtype)
    c = torch.as_tensor(c).to(device=device, dtype=dtype)
    if pitch is not None:
        pitch = torch.as_tensor(pitch).to(device)
    outs, big = [], 0.0
    step = z.shape[0] if (z.numel() <= 300000 if whole_batch is None else whole_batch) else 1
    for b in range(0, z.shape[0], step):
        y, m = _forward_row(W, z[b:b + step], c[b:b + step], None if pitch is None else pitch[b:b + step], p, return_max)
        outs.append(y)
        big = max(big, m)
    y = torch.cat(outs) if len(outs) > 1 else outs[0]
    if not as_tensor:
        y = y.cpu().numpy()
    return (y, big) if return_max else y


def _forward_row(W, z, c, pitch, p, return_max):
    big = 0.0
    if p.get('use_pitch_embed'):
        e = F.embedding(pitch, W['pitch_embed.weight'], padding_idx=0)
        c = F.linear(torch.cat([c.transpose(1, 2), e], -1), W['c_proj.weight'], W['c_proj.bias']).transpose(1, 2)
    c = _conv(c, W['upsample_net.conv_in.weight'], pad=0)
    B, A, _ = c.shape
    for i, s in enumerate(p['upsample_params']['upsample_scales']):
        c = torch.repeat_interleave(c, s, dim=-1)           # nearest stretch by an integer scale
        w = W[f'upsample_net.upsample.up_layers.{2 * i + 1}.weight'].reshape(1, 1, -1)
        c = _conv(c.reshape(B * A, 1, -1), w, pad=s).reshape(B, A, -1)
    assert c.shape[-1] == z.shape[-1], (c.shape, z.shape)
    x = _conv(z, W['first_conv.weight'], W['first_conv.bias'])
    skips = 0
    per = p['layers'] // p['stacks']
    for i in range(p['layers']):
        d = 2 ** (i % per)
        q = f'conv_layers.{i}.'
        y = _conv(x, W[q + 'conv.weight'], W[q + 'conv.bias'], d)
        ya, yb = y.split(y.shape[1] // 2, dim=1)
        a = _conv(c, W[q + 'conv1x1_aux.weight'])
        ca, cb = a.split(a.shape[1] // 2, dim=1)
        ya, yb = ya + ca, yb + cb
        if return_max:
            big = max(big, float(ya.abs().max()), float(yb.abs().max()), float(x.abs().max()))
        g = torch.tanh(ya) * torch.sigmoid(yb)
        skips = skips + _conv(g, W[q + 'conv1x1_skip.weight'], W[q + 'conv1x1_skip.bias'])
        x = (_conv(g, W[q + 'conv1x1_out.weight'], W[q + 'conv1x1_out.bias']) + x) * math.sqrt(0.5)
    skips = skips * math.sqrt(1.0 / p['layers'])
    y = F.relu(skips)
    y = F.relu(_conv(y, W['last_conv_layers.1.weight'], W['last_conv_layers.1.bias']))
    y = _conv(y, W['last_conv_layers.3.weight'], W['last_conv_layers.3.bias'])
    return y, big


def base_cfg():
    """bsg_pwg_cfg of configs/tts/pwg.yaml (no pitch front), for the tests that call bsg_pwg_create directly."""
    cfg = _lib.PwgCfg()
    for n, v in dict(in_channels=1, out_channels=1, kernel_size=3, layers=30, stacks=3, residual_channels=64, gate_channels=128,
                     skip_channels=64, aux_channels=80, aux_context_window=2, bias=1, use_causal_conv=0, upsample_net=0,
                     interpolate_nearest=1, freq_axis_kernel_size=1, n_scales=4, use_pitch_embed=0, n_pitch=0, hop_size=256).items():
        setattr(cfg, n, v)
    for i in range(4):
        cfg.upsample_scales[i] = 4
    return cfg
