"""``PitchExtractor`` — drop-in for modules/fastspeech/pe.py:120-149 (mel -> f0), SURVEY.md §8 row f2, on HIP kernels.

Used by the inference harness when ``pe_enable`` is set to feed the NSF vocoder (a-*.py:600-603, :629-630).
Same module tree / ``state_dict`` (59 entries) as the reference; parameters only, the arithmetic is ``bsg_pitchext_*``.
"""
from ctypes import byref, c_int32, c_void_p

import torch
import torch.nn as nn

from . import _lib
from .fs2 import Linear, SinusoidalPositionalEmbedding, _Holder
from .hparams import hparams


class Prenet(_Holder):
    def __init__(self, in_dim=80, out_dim=256, kernel=5, n_layers=3):
        super().__init__()
        layers = []
        for _ in range(n_layers):
            layers.append(nn.Sequential(nn.Conv1d(in_dim, out_dim, kernel_size=kernel, padding=kernel // 2), nn.ReLU(),
                                        nn.BatchNorm1d(out_dim)))
            in_dim = out_dim
        self.layers = nn.ModuleList(layers)
        self.out_proj = nn.Linear(out_dim, out_dim)


class ConvNorm(_Holder):
    def __init__(self, cin, cout, kernel_size):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, kernel_size=kernel_size, padding=(kernel_size - 1) // 2)


class ConvBlock(_Holder):
    def __init__(self, idim, n_chans, kernel_size):
        super().__init__()
        self.conv = ConvNorm(idim, n_chans, kernel_size)
        self.norm = nn.GroupNorm(n_chans // 16, n_chans)


class ConvStacks(_Holder):
    def __init__(self, idim=80, n_layers=5, n_chans=256, odim=32, kernel_size=5):
        super().__init__()
        self.conv = nn.ModuleList()
        self.in_proj = Linear(idim, n_chans)
        for _ in range(n_layers):
            self.conv.append(ConvBlock(n_chans, n_chans, kernel_size))
        self.out_proj = Linear(n_chans, odim)


class PredictorLayerNorm(nn.LayerNorm):
    def __init__(self, nout):
        super().__init__(nout, eps=1e-12)


class PitchPredictor(_Holder):
    """tts_modules.py:194-231."""

    def __init__(self, idim, n_layers=5, n_chans=384, odim=2, kernel_size=5, dropout_rate=0.1):
        super().__init__()
        self.conv = nn.ModuleList()
        for i in range(n_layers):
            self.conv.append(nn.Sequential(
                nn.ConstantPad1d(((kernel_size - 1) // 2, (kernel_size - 1) // 2), 0),
                nn.Conv1d(idim if i == 0 else n_chans, n_chans, kernel_size, stride=1, padding=0),
                nn.ReLU(), PredictorLayerNorm(n_chans), nn.Dropout(dropout_rate)))
        self.linear = nn.Linear(n_chans, odim)
        self.embed_positions = SinusoidalPositionalEmbedding(idim, 0, init_size=4096)
        self.pos_embed_alpha = nn.Parameter(torch.Tensor([1]))


class PitchExtractor(nn.Module, _lib.HandleOwner, _lib.GemmGuarded):
    GUARD_KIND = 'pitchext'
    DESTROY = 'bsg_pitchext_destroy'
    POISON = 'bsg_pitchext_debug_poison_workspace'      # NaN bytes into every shape-sized buffer of the handle

    def __init__(self, n_mel_bins=80, conv_layers=2):
        super().__init__()
        self.hidden_size = 256
        self.n_mel_bins = n_mel_bins
        ph = hparams['predictor_hidden'] if hparams['predictor_hidden'] > 0 else self.hidden_size
        assert ph == 256 and hparams['ffn_padding'] == 'SAME'
        self.conv_layers = conv_layers
        self.predictor_kernel = hparams['predictor_kernel']
        self.mel_prenet = Prenet(n_mel_bins, self.hidden_size)
        if conv_layers > 0:
            self.mel_encoder = ConvStacks(idim=self.hidden_size, n_chans=self.hidden_size, odim=self.hidden_size, n_layers=conv_layers)
        self.pitch_predictor = PitchPredictor(self.hidden_size, n_chans=ph, n_layers=5, dropout_rate=0.5, odim=2,
                                              kernel_size=self.predictor_kernel)

    def _create(self, ws, arr):
        assert hparams.get('pitch_norm', 'log') == 'log', "only pitch_norm: log is on the BiSinger path"
        use_uv = int(hparams.get('pitch_type', 'frame') == 'frame' and bool(hparams.get('use_uv', True)))
        self._n_pos = max(4096, int(hparams.get('max_frames', 5000)) + 2)
        cfg = _lib.PitchextCfg(256, self.n_mel_bins, self.conv_layers, 5, self.predictor_kernel, use_uv, self._n_pos)
        lib = _lib.load()
        assert lib.bsg_pitchext_n_weights(byref(cfg)) == len(ws), (lib.bsg_pitchext_n_weights(byref(cfg)), len(ws))
        table = self.pitch_predictor.embed_positions.table(self._n_pos).to(ws[0].device).contiguous()
        h = c_void_p()
        _lib.check(lib.bsg_pitchext_create(byref(h), byref(cfg), arr, len(ws), _lib.ptr(table), _lib.stream_ptr()), 'bsg_pitchext_create')
        return h

    @torch.no_grad()
    def forward(self, mel_input=None, lengths=None):
        """mel [B,T,80] -> {'pitch_pred': [B,T,2], 'f0_denorm_pred': [B,T]}   (pe.py:136-149).

        ``lengths`` (list or tensor of B ints, 1 <= lengths[b] <= T): a ragged batch — row b runs at its own length, as the reference
        extracts the pitch of each utterance alone: ``pitch_pred[b, :lengths[b]]`` and ``f0_denorm_pred[b, :lengths[b]]`` are the extractor
        applied to ``mel_input[b:b+1, :lengths[b]]``, the rest of the row is 0, and nothing at or beyond a row's end is read (GroupNorm's
        statistics, the convolutions' padding and the predictor's positions all end with the row).  ``None``: the padded call, every row
        at T frames, padding included."""
        if lengths is not None:      # the count is checked before anything touches the GPU; the values by the library, before it enqueues anything
            lengths = _lib.row_lengths(lengths, int(mel_input.shape[0]), 'PitchExtractor.forward')
        # the guard's repeat (an operand beyond the fp16 range of the split-fp16 GEMMs) runs the same call, ragged or not, on the fp32 matrix pipe
        return _lib.range_guarded(lambda: self._forward(mel_input, lengths), 'PitchExtractor.forward', device=self, owners=(self,))

    def _forward(self, mel_input, lengths=None):
        h = self.handle()
        mel = mel_input.contiguous().float()
        B, T, M = mel.shape
        if T >= self._n_pos:
            raise _lib.BsgError(f'T={T} exceeds the position table ({self._n_pos})')
        pred = torch.empty(B, T, 2, device=mel.device)
        f0 = torch.empty(B, T, device=mel.device)
        lib = _lib.load()
        with torch.cuda.device(mel.device):
            if lengths is not None:
                _lib.check(lib.bsg_pitchext_forward_ragged(h, _lib.ptr(mel), (c_int32 * B)(*lengths), _lib.ptr(pred), _lib.ptr(f0), B, T,
                                                           _lib.stream_ptr()), 'bsg_pitchext_forward_ragged')
            else:
                _lib.check(lib.bsg_pitchext_forward(h, _lib.ptr(mel), _lib.ptr(pred), _lib.ptr(f0), B, T, _lib.stream_ptr()),
                           'bsg_pitchext_forward')
        return {'pitch_pred': pred, 'f0_denorm_pred': f0}
