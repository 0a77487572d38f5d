"""``ParallelWaveGANGenerator`` — drop-in for modules/parallel_wavegan/models/parallel_wavegan.py:18-201 (generator forward only) on
the HIP kernels of csrc/pwg.hip.

Constructed like the reference (``ParallelWaveGANGenerator(**config['generator_params'])``); parameters are registered with the
reference's state-dict keys, shapes and order in the weight-norm layout (``[bias,] weight_g, weight_v`` per convolution), so that a strict
``load_state_dict`` followed by ``remove_weight_norm()`` works as in vocoders/pwg.py:28-48; an already folded layout (``[bias,] weight``)
loads too.  What the kernels are built for (bsg_pwg_create refuses the rest with a message): kernel size 3, non-causal, residual = skip
= 64, gate = 128, aux = 80 channels, ``ConvInUpsampleNetwork`` with the nearest stretch.  The discriminator and the losses are
training-only and out of scope.
"""
from ctypes import byref, c_int32, c_void_p

import numpy as np
import torch
import torch.nn as nn

from . import _lib


class _WNConv(nn.Module):
    """Parameter holder for one weight-normed Conv1d / Conv2d (torch's weight_norm, dim=0), with or without a bias."""

    def __init__(self, weight_shape, bias, weight_norm=True, fill=None):
        super().__init__()
        self.weight_shape = tuple(weight_shape)
        if bias:
            self.bias = nn.Parameter(torch.zeros(weight_shape[0]))
        w = torch.empty(*weight_shape)
        if fill is None:
            nn.init.kaiming_normal_(w, nonlinearity='relu')      # residual_block.py:24
        else:
            w.fill_(fill)                                        # upsample.py:56
        if weight_norm:
            self.weight_g = nn.Parameter(w.reshape(w.shape[0], -1).norm(dim=1).reshape(self._g_shape()))
            self.weight_v = nn.Parameter(w)
        else:
            self.weight = nn.Parameter(w)

    def _g_shape(self):
        return (self.weight_shape[0],) + (1,) * (len(self.weight_shape) - 1)

    @property
    def folded(self):
        return 'weight' in self._parameters

    def _dev(self):
        return next(iter(self._parameters.values())).device

    def fold(self):
        """remove_weight_norm: weight = g * v / ||v|| (computed by the library on the GPU, by torch on the CPU)."""
        if self.folded:
            return
        g, v = self.weight_g.detach(), self.weight_v.detach()
        if v.is_cuda:
            w = torch.empty_like(v)
            with torch.cuda.device(v.device):
                _lib.check(_lib.load().bsg_weight_norm_fold(_lib.ptr(g.contiguous()), _lib.ptr(v.contiguous()), _lib.ptr(w),
                                                            v.shape[0], v[0].numel(), _lib.stream_ptr()), 'bsg_weight_norm_fold')
        else:
            w = torch._weight_norm(v, g, 0)
        del self._parameters['weight_g'], self._parameters['weight_v']
        self.register_parameter('weight', nn.Parameter(w))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kw):
        # accept the other layout than the one currently registered
        if prefix + 'weight' in state_dict and not self.folded:
            dev = self._dev()
            del self._parameters['weight_g'], self._parameters['weight_v']
            self.register_parameter('weight', nn.Parameter(torch.empty(self.weight_shape, device=dev)))
        elif prefix + 'weight_v' in state_dict and self.folded:
            dev = self._dev()
            del self._parameters['weight']
            self.register_parameter('weight_g', nn.Parameter(torch.ones(self._g_shape(), device=dev)))
            self.register_parameter('weight_v', nn.Parameter(torch.empty(self.weight_shape, device=dev)))
        super()._load_from_state_dict(state_dict, prefix, *args, **kw)


class _NoParams(nn.Module):
    """Place holder of a parameter-free reference module (Stretch2d, ReLU): it keeps the ModuleList indices of the state-dict keys."""


class UpsampleNetwork(nn.Module):
    """layers/upsample.py:61-122 (parameters only): per scale a stretch and a 1 x (2 scale + 1) single-channel Conv2d without bias."""

    def __init__(self, upsample_scales, weight_norm):
        super().__init__()
        self.up_layers = nn.ModuleList()
        for s in upsample_scales:
            self.up_layers += [_NoParams(), _WNConv((1, 1, 1, 2 * s + 1), False, weight_norm, fill=1.0 / (2 * s + 1))]


class ConvInUpsampleNetwork(nn.Module):
    """layers/upsample.py:125-183 (parameters only)."""

    def __init__(self, upsample_scales, aux_channels, aux_context_window, weight_norm):
        super().__init__()
        self.conv_in = _WNConv((aux_channels, aux_channels, 2 * aux_context_window + 1), False, weight_norm)
        self.upsample = UpsampleNetwork(upsample_scales, weight_norm)


class ResidualBlock(nn.Module):
    """layers/residual_block.py:39-89 (parameters only)."""

    def __init__(self, kernel_size, residual_channels, gate_channels, skip_channels, aux_channels, bias, weight_norm):
        super().__init__()
        self.conv = _WNConv((gate_channels, residual_channels, kernel_size), bias, weight_norm)
        self.conv1x1_aux = _WNConv((gate_channels, aux_channels, 1), False, weight_norm)
        self.conv1x1_out = _WNConv((residual_channels, gate_channels // 2, 1), bias, weight_norm)
        self.conv1x1_skip = _WNConv((skip_channels, gate_channels // 2, 1), bias, weight_norm)


class ParallelWaveGANGenerator(nn.Module, _lib.HandleOwner):
    DESTROY = 'bsg_pwg_destroy'
    LAST_PATH = 'bsg_pwg_last_path'      # the launches of the last forward in launch order (include/bisinger_hip.h, bsg_pwg_last_path)
    POISON = 'bsg_pwg_debug_poison_workspace'

    def __init__(self, in_channels=1, out_channels=1, kernel_size=3, layers=30, stacks=3, residual_channels=64, gate_channels=128,
                 skip_channels=64, aux_channels=80, aux_context_window=2, dropout=0.0, bias=True, use_weight_norm=True,
                 use_causal_conv=False, upsample_conditional_features=True, upsample_net='ConvInUpsampleNetwork',
                 upsample_params={'upsample_scales': [4, 4, 4, 4]}, use_pitch_embed=False):
        super().__init__()
        assert layers % stacks == 0
        if not upsample_conditional_features or upsample_net != 'ConvInUpsampleNetwork':
            raise NotImplementedError(f'upsample_net={upsample_net!r}, upsample_conditional_features={upsample_conditional_features}: '
                                      f'only ConvInUpsampleNetwork is built')
        up = dict(upsample_params)
        if up.get('nonlinear_activation') is not None:
            raise NotImplementedError(f"upsample_params['nonlinear_activation']={up['nonlinear_activation']!r} is not built")
        self.params = dict(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, layers=layers, stacks=stacks,
                           residual_channels=residual_channels, gate_channels=gate_channels, skip_channels=skip_channels,
                           aux_channels=aux_channels, aux_context_window=aux_context_window, bias=bool(bias),
                           use_causal_conv=bool(use_causal_conv), upsample_scales=[int(s) for s in up['upsample_scales']],
                           interpolate_mode=up.get('interpolate_mode', 'nearest'),
                           freq_axis_kernel_size=int(up.get('freq_axis_kernel_size', 1)), use_pitch_embed=bool(use_pitch_embed))
        self.in_channels, self.out_channels, self.aux_channels = in_channels, out_channels, aux_channels
        self.layers, self.stacks, self.kernel_size = layers, stacks, kernel_size
        self.aux_context_window = aux_context_window
        self.use_pitch_embed = bool(use_pitch_embed)
        wn = bool(use_weight_norm)
        self.first_conv = _WNConv((residual_channels, in_channels, 1), True, wn)
        self.upsample_net = ConvInUpsampleNetwork(self.params['upsample_scales'], aux_channels, aux_context_window, wn)
        self.conv_layers = nn.ModuleList(ResidualBlock(kernel_size, residual_channels, gate_channels, skip_channels, aux_channels, bias, wn)
                                         for _ in range(layers))
        self.last_conv_layers = nn.ModuleList([_NoParams(), _WNConv((skip_channels, skip_channels, 1), True, wn),
                                               _NoParams(), _WNConv((out_channels, skip_channels, 1), True, wn)])
        if use_pitch_embed:
            self.pitch_embed = nn.Embedding(300, aux_channels, 0)
            self.c_proj = nn.Linear(2 * aux_channels, aux_channels)

    @property
    def hop_size(self):
        return int(np.prod(self.params['upsample_scales']))

    @property
    def receptive_field_size(self):
        per = self.layers // self.stacks
        return (self.kernel_size - 1) * sum(2 ** (i % per) for i in range(self.layers)) + 1

    def remove_weight_norm(self):
        for m in self.modules():
            if isinstance(m, _WNConv):
                m.fold()
        self.forget_slots()

    # ------------------------------------------------------------------ handle
    def _before_weights(self):
        if not all(m.folded for m in self.modules() if isinstance(m, _WNConv)):
            raise _lib.BsgError('ParallelWaveGANGenerator is in the weight-norm layout: call remove_weight_norm() before the first forward '
                                '(vocoders/pwg.py:48)')

    def _create(self, ws, arr):
        q = self.params
        cfg = _lib.PwgCfg()
        for n in ('in_channels', 'out_channels', 'kernel_size', 'layers', 'stacks', 'residual_channels', 'gate_channels', 'skip_channels',
                  'aux_channels', 'aux_context_window', 'freq_axis_kernel_size'):
            setattr(cfg, n, int(q[n]))
        cfg.bias, cfg.use_causal_conv, cfg.use_pitch_embed = int(q['bias']), int(q['use_causal_conv']), int(q['use_pitch_embed'])
        cfg.upsample_net = 0
        cfg.interpolate_nearest = int(q['interpolate_mode'] == 'nearest')
        if len(q['upsample_scales']) > 8:
            raise _lib.BsgError(f"{len(q['upsample_scales'])} upsample_scales: at most 8 are built")
        cfg.n_scales = len(q['upsample_scales'])
        for i, s in enumerate(q['upsample_scales']):
            cfg.upsample_scales[i] = s
        cfg.n_pitch = self.pitch_embed.weight.shape[0] if self.use_pitch_embed else 0
        cfg.hop_size = self.hop_size
        hd = c_void_p()
        _lib.check(_lib.load().bsg_pwg_create(byref(hd), byref(cfg), arr, len(ws), _lib.stream_ptr()), 'bsg_pwg_create')
        return hd

    def last_tiles(self):
        """The 256-sample tiles one residual-layer launch of the last forward walked (bsg_pwg_last_tiles): B ceil(T hop / 256) after
        ``forward``, the sum of ceil(lengths[b] hop / 256) after ``forward_ragged``; 0 before the first."""
        return int(_lib.load().bsg_pwg_last_tiles(self._h)) if self._h is not None else 0

    @torch.no_grad()
    def forward_ragged(self, x, mel, pitch=None, *, lengths, seed=None, row_seeds=None):
        """A ragged batch: x [B,1,T*hop] noise (None: drawn on the device from the Philox stream of ``seed``), mel [B,80,T] UNPADDED,
        pitch [B,T] int64 with use_pitch_embed, ``lengths`` a list or tensor of B ints in 1 .. T -> [B,1,T*hop].

        Row b is the generator applied to that utterance alone, as vocoders/pwg.py:84-105 runs it: ``y[b, 0, :lengths[b]*hop]`` equals,
        bit for bit, ``forward(x[b:b+1, :, :lengths[b]*hop], edge_pad(mel[b:b+1, :, :lengths[b]], w), edge_pad(pitch[b:b+1, :lengths[b]], w))``;
        the rest of the row is 0, and nothing at or beyond a row's end is read.  A separate method, not a keyword of ``forward``: there
        ``c`` is the mel the caller already edge-padded, here the library pads each row at its own end.  With ``x=None`` the draws keep
        the index of the padded call at (B, T), element b*T*hop + t: a batched row with drawn noise is reproducible from the seed but
        is not the waveform of the lone call with that seed.  ``row_seeds`` (B ints; with ``x=None`` only) is the way out: row b's noise
        is the first lengths[b]*hop values of the Philox stream (row_seeds[b], 0x505747) — what ``forward(None, ..., seed=row_seeds[b])``
        draws for the utterance alone (``bsg_philox_normal_rows``) — so the row IS that lone call, bit for bit."""
        B, A, T = (int(v) for v in mel.shape)
        if row_seeds is not None:
            row_seeds = _lib.row_seeds_list(row_seeds, B, 'ParallelWaveGANGenerator.forward_ragged', {'x': x})
        # checked before the handle is built and before the output exists: without a GPU the refusal is the length's
        lengths = _lib.row_lengths(lengths, B, 'ParallelWaveGANGenerator.forward_ragged', T=T)
        hd = self.handle()
        dev = self.first_conv.weight.device
        mel = mel.to(dev, torch.float32).contiguous()
        assert A == self.aux_channels, (tuple(mel.shape), self.aux_channels)
        L = T * self.hop_size
        if x is not None:
            x = x.to(dev, torch.float32).contiguous()
            assert tuple(x.shape) == (B, 1, L), (tuple(x.shape), (B, 1, L))
        elif row_seeds is not None:
            x = _lib.philox_normal_rows(torch.empty(B, 1, L, device=dev), 1, L, [n * self.hop_size for n in lengths], row_seeds, 0x505747)
        elif seed is None:
            raise _lib.BsgError('ParallelWaveGANGenerator.forward_ragged: x=None needs seed= or row_seeds= (the noise is drawn on the device)')
        if self.use_pitch_embed:
            if pitch is None:
                raise _lib.BsgError('this generator has the pitch front (use_pitch_embed): pitch is required')
            pitch = pitch.to(dev, torch.int64).contiguous()
            assert tuple(pitch.shape) == (B, T), (tuple(pitch.shape), (B, T))
        elif pitch is not None:
            raise _lib.BsgError('pitch given but this generator was built without use_pitch_embed')
        y = torch.empty(B, 1, L, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().bsg_pwg_forward_ragged(hd, _lib.ptr(x), _lib.ptr(mel), _lib.ptr(pitch), (c_int32 * B)(*lengths), _lib.ptr(y),
                                                          B, T, int(seed or 0), _lib.stream_ptr()), 'bsg_pwg_forward_ragged')
        return y

    @torch.no_grad()
    def forward(self, x, c=None, pitch=None, seed=None, **kwargs):
        """x [B,1,T*hop] noise (None: drawn on the device from the Philox stream of ``seed``), c [B,80,T+2w] (edge-padded by the caller),
        pitch [B,T+2w] int64 with use_pitch_embed -> [B,1,T*hop]   (parallel_wavegan.py:135-168).  All products run on the fp32 matrix
        pipe: there is no operand range to guard."""
        if c is None:
            raise _lib.BsgError('ParallelWaveGANGenerator.forward without c (unconditional generation) is not built')
        hd = self.handle()
        dev = self.first_conv.weight.device
        c = c.to(dev, torch.float32).contiguous()
        B, A, Tp = c.shape
        T = Tp - 2 * self.aux_context_window
        assert A == self.aux_channels and T >= 1, (tuple(c.shape), self.aux_context_window)
        L = T * self.hop_size
        if x is not None:
            x = x.to(dev, torch.float32).contiguous()
            assert tuple(x.shape) == (B, 1, L), (tuple(x.shape), (B, 1, L))
        elif seed is None:
            raise _lib.BsgError('ParallelWaveGANGenerator.forward: x=None needs seed= (the noise is drawn on the device)')
        if self.use_pitch_embed:
            if pitch is None:
                raise _lib.BsgError('this generator has the pitch front (use_pitch_embed): pitch is required')
            pitch = pitch.to(dev, torch.int64).contiguous()
            assert tuple(pitch.shape) == (B, Tp), (tuple(pitch.shape), (B, Tp))
        elif pitch is not None:
            raise _lib.BsgError('pitch given but this generator was built without use_pitch_embed')
        y = torch.empty(B, 1, L, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().bsg_pwg_forward(hd, _lib.ptr(x), _lib.ptr(c), _lib.ptr(pitch), _lib.ptr(y), B, T, int(seed or 0),
                                                   _lib.stream_ptr()), 'bsg_pwg_forward')
        return y
