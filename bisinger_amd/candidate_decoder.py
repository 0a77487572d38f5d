"""``FFT`` candidate denoiser — drop-in for usr/diff/candidate_decoder.py:39-100 (DIFF_DECODERS['fft']), SURVEY.md §8 row f4.

Same constructor ``FFT(hidden_size, num_layers, kernel_size, num_heads)``, state_dict (49 entries at 4 layers) and
``denoise_fn(spec [B,1,M,T], t [B], cond [B,H,T])`` contract as the reference; arithmetic in ``bsg_fftden_*``.
Not selected by any shipped BiSinger config (all use 'wavenet'), so its padded sampler loop is driven from Python:
one ``bsg_fftden_forward`` + ``bsg_ddpm_step`` per step (see GaussianDiffusion.sample).  A ragged batch (``prepare(cond, lengths)``) is
decoded row by row alone, and its loop runs in the library (``bsg_fftden_ddpm_sample`` / ``bsg_fftden_plms_sample``).
"""
from ctypes import byref, c_int32, c_void_p

import torch
import torch.nn as nn

from . import _lib
from .diffnet import Mish, SinusoidalPosEmb, _conv1d, ragged_lens
from .fs2 import FFTBlocks
from .hparams import hparams


class FFT(FFTBlocks, _lib.HandleOwner, _lib.GemmGuarded):
    GUARD_KIND = 'fftden'
    DESTROY = 'bsg_fftden_destroy'
    LAST_PATH = 'bsg_fftden_last_path'      # the launch forms of the last forward's FFT stack ('den.' tokens; include/bisinger_hip.h, bsg_fs2midi_last_path)
    POISON = 'bsg_fftden_debug_poison_workspace'      # NaN bytes over every activation workspace of the handle
    _bound = None
    _lengths = None        # row lengths of a ragged binding (prepare(cond, lengths))

    def __init__(self, hidden_size=None, num_layers=None, kernel_size=None, num_heads=None):
        num_heads = hparams['num_heads'] if num_heads is None else num_heads
        hidden_size = hparams['hidden_size'] if hidden_size is None else hidden_size
        kernel_size = hparams['dec_ffn_kernel_size'] if kernel_size is None else kernel_size
        num_layers = hparams['dec_layers'] if num_layers is None else num_layers
        super().__init__(hidden_size, num_layers, kernel_size, num_heads=num_heads)
        dim = hparams['residual_channels']
        assert dim == 256 and hidden_size == 256
        self.in_dims = hparams['audio_num_mel_bins']
        self.num_heads, self.kernel_size = num_heads, kernel_size
        self.max_steps = max(int(hparams.get('timesteps', 1000)), 1000)
        self.input_projection = _conv1d(self.in_dims, dim, 1)
        self.diffusion_embedding = SinusoidalPosEmb(dim)
        self.mlp = nn.Sequential(nn.Linear(dim, dim * 4), Mish(), nn.Linear(dim * 4, dim))
        self.get_mel_out = nn.Linear(hidden_size, 80, bias=True)
        self.get_decode_inp = nn.Linear(hidden_size + dim + dim, hidden_size)

    def _create(self, ws, arr):
        lib = _lib.load()
        assert lib.bsg_fftden_n_weights(self.num_layers) == len(ws), (lib.bsg_fftden_n_weights(self.num_layers), len(ws))
        dev = ws[0].device
        self._n_pos = max(2000, int(hparams.get('max_frames', 5000))) + 2
        step_table = self.diffusion_embedding.table(self.max_steps).to(dev).contiguous()
        pos_table = self.embed_positions.table(self._n_pos).to(dev).contiguous()
        h = c_void_p()
        _lib.check(lib.bsg_fftden_create(byref(h), self.in_dims, self.num_layers, self.num_heads, self.kernel_size, self.max_steps,
                                         self._n_pos, arr, len(ws), _lib.ptr(step_table), _lib.ptr(pos_table), _lib.stream_ptr()),
                   'bsg_fftden_create')
        return h

    def release(self):
        super().release()
        self._bound = None      # (handle() releases first: a new handle starts unbound)
        self._lengths = None

    def prepare(self, cond, lengths=None):
        """Bind ``cond`` [B,H,T]: hoists the condition part of the concat-Linear out of the step loop.
        ``lengths`` (B ints, 1..T): a ragged batch — the calls that follow decode row b on its first lengths[b] frames only, as if it were
        alone at T = lengths[b] (include/bisinger_hip.h bsg_fftden_prepare_ragged; INTEGRATION.md "Ragged batches")."""
        h = self.handle()
        cond = cond.contiguous().float()
        B, H, T = cond.shape
        lens = None if lengths is None else ragged_lens(lengths, B, T)
        with torch.cuda.device(cond.device):
            if lens is None:
                _lib.check(_lib.load().bsg_fftden_prepare(h, _lib.ptr(cond), B, T, _lib.stream_ptr()), 'bsg_fftden_prepare')
            else:
                _lib.check(_lib.load().bsg_fftden_prepare_ragged(h, _lib.ptr(cond), (c_int32 * B)(*lens), B, T, _lib.stream_ptr()),
                           'bsg_fftden_prepare_ragged')
        self._bound = (cond, cond._version, B, T)      # strong reference (see DiffNet._ensure_bound)
        self._lengths = lens
        return B, T

    def _ensure_bound(self, cond, lengths=None):
        """As DiffNet._ensure_bound: bind again unless ``cond`` IS the tensor bound last, unmodified, with the same row lengths."""
        b = self._bound
        lens = None if lengths is None else ragged_lens(lengths, cond.shape[0], cond.shape[2])
        if (self._h is None or self._key() != self._h_key or b is None or b[0] is not cond or b[1] != cond._version
                or not cond.is_contiguous() or cond.dtype != torch.float32 or self._lengths != lens):
            self.prepare(cond, lengths)
            if cond.is_contiguous() and cond.dtype == torch.float32:
                self._bound = (cond, cond._version, cond.shape[0], cond.shape[2])

    @torch.no_grad()
    def forward(self, spec, diffusion_step, cond, padding_mask=None, attn_mask=None, return_hiddens=False, lengths=None):
        """spec [B,1,M,T], diffusion_step [B], cond [B,H,T] -> eps [B,1,M,T].  ``lengths`` (B ints): a ragged batch (prepare()): row b's eps
        on frames < lengths[b] is the row's alone at T = lengths[b], 0 beyond; nothing of spec or cond at or beyond a row's end is read."""
        assert padding_mask is None and attn_mask is None and not return_hiddens, 'inference contract only'
        B, _, M, T = spec.shape
        x = spec[:, 0].contiguous().float()
        t = diffusion_step.to(device=x.device, dtype=torch.long).contiguous()
        eps = torch.empty_like(x)

        def run():
            self._ensure_bound(cond, lengths)
            with torch.cuda.device(x.device):
                _lib.check(_lib.load().bsg_fftden_forward(self._h, _lib.ptr(x), _lib.ptr(t), _lib.ptr(eps), B, T, _lib.stream_ptr()),
                           'bsg_fftden_forward')

        def again():
            self._bound = None          # the hoisted condition part was projected by the same GEMMs: bind again

        _lib.range_guarded(run, 'FFT denoiser forward', on_retry=again, device=self, owners=(self,))
        return eps[:, None, :, :]
