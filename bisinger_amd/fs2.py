"""``FastSpeech2MIDI`` — drop-in for modules/diffsinger_midi/fs2.py:80-197 (+ the base
modules/fastspeech/fs2.py:24-89 constructor), inference direction, on HIP kernels — and ``FastSpeech2``, the plain front the
reference builds when ``use_midi`` is absent or false (modules/fastspeech/fs2.py:24-240; usr/diff/shallow_diffusion_tts.py:76-79),
both with the frame-level pitch adaptor of ``use_pitch_embed: true`` (add_pitch, fs2.py:188-234).

The sub-modules below reproduce the reference's module tree so that ``state_dict()`` has exactly the
reference's 143 ``fs2.*`` entries (names, shapes, order — including the two aliased sub-trees
``encoder.esm``/``esm`` and ``encoder.embed_tokens``/``encoder_embed_tokens`` and the
``decoder.embed_positions._float_tensor`` buffer).  They only hold parameters: the arithmetic is
``bsg_fs2midi_*`` in libbisinger_hip (csrc/fs2.hip).
"""
import math
from ctypes import byref, c_int32, c_void_p

import torch
import torch.nn as nn

from . import _lib
from .hparams import hparams

DEFAULT_MAX_TARGET_POSITIONS = 2000


def Embedding(num_embeddings, embedding_dim, padding_idx=None):
    m = nn.Embedding(num_embeddings, embedding_dim, padding_idx=padding_idx)
    nn.init.normal_(m.weight, mean=0, std=embedding_dim ** -0.5)
    if padding_idx is not None:
        nn.init.constant_(m.weight[padding_idx], 0)
    return m


def Linear(in_features, out_features, bias=True):
    m = nn.Linear(in_features, out_features, bias)
    nn.init.xavier_uniform_(m.weight)
    if bias:
        nn.init.constant_(m.bias, 0.0)
    return m


class _Holder(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise _lib.BsgError(f'{type(self).__name__} only holds parameters; it runs inside libbisinger_hip')


class MultiheadAttention(_Holder):
    """common_layers.py:199-280 with bias=False: in_proj_weight [3C,C], out_proj.weight [C,C]."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=False)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.xavier_uniform_(self.out_proj.weight)


class TransformerFFNLayer(_Holder):
    """common_layers.py:598-644 (padding SAME, gelu)."""

    def __init__(self, hidden_size, filter_size, kernel_size):
        super().__init__()
        self.kernel_size = kernel_size
        self.ffn_1 = nn.Conv1d(hidden_size, filter_size, kernel_size, padding=kernel_size // 2)
        self.ffn_2 = Linear(filter_size, hidden_size)


class EncSALayer(_Holder):
    """common_layers.py:664-704."""

    def __init__(self, c, num_heads, kernel_size):
        super().__init__()
        self.layer_norm1 = nn.LayerNorm(c)
        self.self_attn = MultiheadAttention(c, num_heads)
        self.layer_norm2 = nn.LayerNorm(c)
        self.ffn = TransformerFFNLayer(c, 4 * c, kernel_size)


class TransformerEncoderLayer(_Holder):
    def __init__(self, hidden_size, kernel_size, num_heads):
        super().__init__()
        self.op = EncSALayer(hidden_size, num_heads, kernel_size)


class SinusoidalPositionalEmbedding(_Holder):
    """common_layers.py:106-179.  ``table`` builds the lookup the decoder kernels index by position."""

    def __init__(self, embedding_dim, padding_idx, init_size=1024):
        super().__init__()
        self.embedding_dim, self.padding_idx, self.init_size = embedding_dim, padding_idx, init_size
        self.register_buffer('_float_tensor', torch.zeros(1))

    def table(self, num):
        half = self.embedding_dim // 2
        e = math.log(10000) / (half - 1)
        e = torch.exp(torch.arange(half, dtype=torch.float) * -e)
        e = torch.arange(num, dtype=torch.float).unsqueeze(1) * e.unsqueeze(0)
        e = torch.cat([torch.sin(e), torch.cos(e)], dim=1).view(num, -1)
        if self.padding_idx is not None:
            e[self.padding_idx, :] = 0
        return e


class RelPositionalEncoding(_Holder):
    """espnet_positional_embedding.py:90-114 (reverse=True table of :25-46); no parameters."""

    def __init__(self, d_model, max_len=5000):
        super().__init__()
        self.d_model, self.max_len = d_model, max_len

    def table(self, length):
        pe = torch.zeros(length, self.d_model)
        pos = torch.arange(length - 1, -1, -1.0, dtype=torch.float32).unsqueeze(1)
        div = torch.exp(torch.arange(0, self.d_model, 2, dtype=torch.float32) * -(math.log(10000.0) / self.d_model))
        pe[:, 0::2] = torch.sin(pos * div)
        pe[:, 1::2] = torch.cos(pos * div)
        return pe


class FFTBlocks(_Holder):
    """tts_modules.py:253-282."""

    def __init__(self, hidden_size, num_layers, ffn_kernel_size=9, num_heads=2, use_pos_embed=True):
        super().__init__()
        self.num_layers, self.hidden_size, self.use_pos_embed = num_layers, hidden_size, use_pos_embed
        if use_pos_embed:
            self.padding_idx = 0
            self.pos_embed_alpha = nn.Parameter(torch.Tensor([1]))
            self.embed_positions = SinusoidalPositionalEmbedding(hidden_size, 0, init_size=DEFAULT_MAX_TARGET_POSITIONS)
        self.layers = nn.ModuleList([TransformerEncoderLayer(hidden_size, ffn_kernel_size, num_heads)
                                     for _ in range(num_layers)])
        self.layer_norm = nn.LayerNorm(hidden_size)


class FastspeechDecoder(FFTBlocks):
    def __init__(self):
        super().__init__(hparams['hidden_size'], hparams['dec_layers'], hparams['dec_ffn_kernel_size'], hparams['num_heads'])


class ESM(_Holder):
    """common_layers.py:832-846."""

    def __init__(self, d_model, nhead):
        super().__init__()
        self.mh = nn.MultiheadAttention(d_model, nhead)
        self.ffn = nn.Sequential(nn.Linear(d_model, d_model), nn.ReLU(), nn.Linear(d_model, d_model))
        self.ln1 = nn.LayerNorm(d_model)
        self.ln2 = nn.LayerNorm(d_model)


class FastspeechMIDIEncoder(FFTBlocks):
    """diffsinger_midi/fs2.py:14-17 on tts_modules.py:312-328."""

    def __init__(self, esm, embed_tokens):
        super().__init__(hparams['hidden_size'], hparams['enc_layers'], hparams['enc_ffn_kernel_size'],
                         hparams['num_heads'], use_pos_embed=False)
        self.embed_tokens = embed_tokens
        self.embed_scale = math.sqrt(hparams['hidden_size'])
        self.padding_idx = 0
        self.embed_positions = RelPositionalEncoding(hparams['hidden_size'])
        self.esm = esm


class PredictorLayerNorm(nn.LayerNorm):
    """tts_modules.py:39-58: LayerNorm over the channel axis of [B,C,T], eps = 1e-12."""

    def __init__(self, nout):
        super().__init__(nout, eps=1e-12)


class DurationPredictor(_Holder):
    """tts_modules.py:61-106 (dur_loss = mse)."""

    def __init__(self, idim, n_layers, n_chans, kernel_size):
        super().__init__()
        self.kernel_size = kernel_size
        self.conv = nn.ModuleList()
        for i in range(n_layers):
            self.conv.append(nn.Sequential(
                nn.ConstantPad1d(((kernel_size - 1) // 2, (kernel_size - 1) // 2), 0),
                nn.Conv1d(idim if i == 0 else n_chans, n_chans, kernel_size, stride=1, padding=0),
                nn.ReLU(), PredictorLayerNorm(n_chans), nn.Dropout(hparams['predictor_dropout'])))
        assert hparams['dur_loss'] == 'mse', 'only dur_loss: mse is on the BiSinger path'
        self.linear = nn.Linear(n_chans, 1)


class PitchPredictor(_Holder):
    """tts_modules.py:194-237 (odim = 2, padding SAME): state_dict order pos_embed_alpha, conv.i.1.*, conv.i.3.*, linear.*,
    embed_positions._float_tensor."""

    def __init__(self, idim, n_layers, n_chans, kernel_size):
        super().__init__()
        self.kernel_size, self.n_layers = kernel_size, n_layers
        self.conv = nn.ModuleList()
        for i in range(n_layers):
            self.conv.append(nn.Sequential(
                nn.ConstantPad1d(((kernel_size - 1) // 2, (kernel_size - 1) // 2), 0),
                nn.Conv1d(idim if i == 0 else n_chans, n_chans, kernel_size, stride=1, padding=0),
                nn.ReLU(), PredictorLayerNorm(n_chans), nn.Dropout(hparams['predictor_dropout'])))
        self.linear = nn.Linear(n_chans, 2)
        self.embed_positions = SinusoidalPositionalEmbedding(idim, 0, init_size=4096)
        self.pos_embed_alpha = nn.Parameter(torch.Tensor([1]))


class FastspeechEncoder(FFTBlocks):
    """tts_modules.py:312-349 without rel_pos: sqrt(H) * embed_tokens + SinusoidalPositionalEmbedding over the non-pad tokens."""

    def __init__(self, embed_tokens):
        super().__init__(hparams['hidden_size'], hparams['enc_layers'], hparams['enc_ffn_kernel_size'],
                         hparams['num_heads'], use_pos_embed=False)
        self.embed_tokens = embed_tokens
        self.embed_scale = math.sqrt(hparams['hidden_size'])
        self.padding_idx = 0
        self.embed_positions = SinusoidalPositionalEmbedding(hparams['hidden_size'], 0, init_size=DEFAULT_MAX_TARGET_POSITIONS)


def prefix_lengths(masks, whats, mins):
    """Row lengths of a ragged batch in ONE host read: for every boolean mask [B, n] (``txt_tokens > 0``, ``mel2ph > 0``) the count of each
    row as a list of ints.  ValueError (as diffusion.ragged_lengths) unless the set positions of each row are a prefix of it and the count
    is at least ``mins[i]``: a row with a hole has no length at which it could run alone."""
    cols = []
    for m, lo in zip(masks, mins):
        n = m.sum(-1)
        prefix = torch.arange(m.shape[-1], device=m.device)[None, :] < n[:, None]
        cols += [n, ((m != prefix).any(-1) | (n < lo)).long()]
    host = torch.stack(cols, 0).tolist()
    out = []
    for i, what in enumerate(whats):
        n, bad = host[2 * i], host[2 * i + 1]
        if any(bad):
            b = bad.index(1)
            raise ValueError(f'ragged batch: row {b} of {what} is not one run from position 0 (non-zero prefix, then zeros) or is shorter '
                             f'than {mins[i]}; it cannot run at its own length')
        out.append([int(v) for v in n])
    return out


def _refuse(key, what):
    raise NotImplementedError(f"{key}: {what} (INTEGRATION.md, 'The pitch adaptor and the plain front')")


def check_fs2_hparams(hp, plain):
    """The configurations neither front executes: NotImplementedError naming the key, at construction."""
    if hp.get('encoder_type', 'fft') != 'fft':
        _refuse('encoder_type', f"{hp['encoder_type']!r}: only the 'fft' encoder is built")
    if hp.get('decoder_type', 'fft') != 'fft':
        _refuse('decoder_type', f"{hp['decoder_type']!r}: only the 'fft' decoder is built")
    if hp.get('use_energy_embed'):
        _refuse('use_energy_embed', 'the energy embedding is not built')
    if hp.get('use_spk_embed'):
        _refuse('use_spk_embed', 'the speaker-embedding projection is not built; use_spk_id or no speaker')
    if hp.get('use_split_spk_id'):
        _refuse('use_split_spk_id', 'split speaker tables are not built')
    if plain and hp.get('rel_pos'):
        _refuse('rel_pos', 'the plain front is built with the sinusoidal token positions only')
    if hp.get('use_pitch_embed'):
        if hp.get('pitch_type', 'frame') != 'frame':
            _refuse('pitch_type', f"{hp['pitch_type']!r}: only the frame-level adaptor ('frame') is built")
        if hp.get('pitch_ar'):
            _refuse('pitch_ar', 'the autoregressive pitch predictor is not built')
        if hp.get('pitch_norm', 'log') != 'log':
            _refuse('pitch_norm', f"{hp['pitch_norm']!r}: only 'log' is built")


class _FastSpeech2Base(nn.Module, _lib.HandleOwner, _lib.GemmGuarded):
    """What FastSpeech2MIDI and FastSpeech2 share: the handle (one type for both fronts, bsg_fs2_create), the frame-level part and the
    reference's forward."""
    GUARD_KIND = 'fs2midi'
    FRONT = _lib.FS2_FRONT_MIDI
    DESTROY = 'bsg_fs2midi_destroy'
    # last_path() (test introspection): the launch forms of the last encode and of the decode after it, as blank-separated tokens in
    # launch order (include/bisinger_hip.h, bsg_fs2midi_last_path): 'esm:wave enc.qkv:fused enc.attn:planes/ks2 enc.gemm:h2w/32/deep ...
    # dec. ...'; 'none' before the first call
    LAST_PATH = 'bsg_fs2midi_last_path'
    POISON = 'bsg_fs2midi_debug_poison_workspace'      # NaN bytes over every activation workspace of the handle

    def _init_base(self, dictionary, out_dims):
        """fastspeech/fs2.py:27-81 in the reference's registration order, without the encoder (the subclass adds its own)."""
        hp = hparams
        self.dictionary = dictionary
        self.padding_idx = dictionary.pad()
        self.enc_layers, self.dec_layers = hp['enc_layers'], hp['dec_layers']
        self.hidden_size = H = hp['hidden_size']
        self.use_pitch_embed = bool(hp.get('use_pitch_embed'))
        self.use_uv = bool(hp.get('use_uv', True))
        self.encoder_embed_tokens = Embedding(len(dictionary), H, self.padding_idx)

    def _init_tail(self, out_dims):
        hp = hparams
        H = self.hidden_size
        self.decoder = FastspeechDecoder()
        self.out_dims = out_dims if out_dims is not None else hp['audio_num_mel_bins']
        self.mel_out = Linear(H, self.out_dims, bias=True)
        if hp.get('use_spk_id'):
            self.spk_embed_proj = Embedding(hp['num_spk'] + 1, H)
        ph = hp['predictor_hidden'] if hp['predictor_hidden'] > 0 else H
        if ph != H:
            _refuse('predictor_hidden', f'{ph}: the predictor kernels are built for hidden_size channels')
        self.dur_predictor = DurationPredictor(H, hp['dur_predictor_layers'], ph, hp['dur_predictor_kernel'])
        if self.use_pitch_embed:
            self.pitch_embed = Embedding(300, H, self.padding_idx)
            self.pitch_predictor = PitchPredictor(H, hp['predictor_layers'], ph, hp['predictor_kernel'])

    # ------------------------------------------------------------------ handle management
    def _token_table(self):
        raise NotImplementedError

    def _create(self, ws, arr):
        hp = hparams
        lib = _lib.load()
        self._n_pos = max(DEFAULT_MAX_TARGET_POSITIONS, int(hp.get('max_frames', 5000))) + 2
        dev = ws[0].device
        tok_table = self._token_table().to(dev).contiguous()
        self._n_rel = tok_table.shape[0]
        spk_rows = self.spk_embed_proj.num_embeddings if hasattr(self, 'spk_embed_proj') else 0
        base = _lib.Fs2Cfg(self.hidden_size, self.encoder_embed_tokens.num_embeddings, self.enc_layers, self.dec_layers,
                           hp['num_heads'], hp['enc_ffn_kernel_size'], hp['dec_ffn_kernel_size'], self.out_dims,
                           len(self.dur_predictor.conv), self.dur_predictor.kernel_size, spk_rows, 8, self._n_pos, self._n_rel)
        dec_table = self.decoder.embed_positions.table(self._n_pos).to(dev).contiguous()
        h = c_void_p()
        if self.FRONT == _lib.FS2_FRONT_MIDI and not self.use_pitch_embed:
            # the configuration of every BiSinger experiment: the entry it has always been created through
            assert lib.bsg_fs2midi_n_weights(byref(base)) == len(ws)
            _lib.check(lib.bsg_fs2midi_create(byref(h), byref(base), arr, len(ws), _lib.ptr(dec_table), _lib.ptr(tok_table),
                                              _lib.stream_ptr()), 'bsg_fs2midi_create')
        else:
            pit_table = None
            cfg = _lib.Fs2XCfg(base, self.FRONT, 0, 0, 0, 0, 0)
            if self.use_pitch_embed:
                pit_table = self.pitch_predictor.embed_positions.table(self._n_pos).to(dev).contiguous()
                cfg = _lib.Fs2XCfg(base, self.FRONT, 1, self.pitch_predictor.n_layers, self.pitch_predictor.kernel_size, int(self.use_uv),
                                   self._n_pos)
            n = lib.bsg_fs2_n_weights(byref(cfg))
            if n < 0:
                _lib.check(n, 'bsg_fs2_n_weights')
            assert n == len(ws), (n, len(ws))
            _lib.check(lib.bsg_fs2_create(byref(h), byref(cfg), arr, len(ws), _lib.ptr(dec_table), _lib.ptr(tok_table), _lib.ptr(pit_table),
                                          _lib.stream_ptr()), 'bsg_fs2_create')
        return h

    def last_rows(self):
        """-> (token rows the last encode ran its encoder on, rows of the last FFT stack): test introspection."""
        a, b = c_int32(), c_int32()
        _lib.check(_lib.load().bsg_fs2midi_last_rows(self._h if self._h is not None else self.handle(), byref(a), byref(b)), 'bsg_fs2midi_last_rows')
        return a.value, b.value

    @torch.no_grad()
    def regulate(self, enc, with_lengths=False):
        """LengthRegulator on the predicted durations (tts_modules.py:161-191); one host sync, as in the
        reference (the output length is data dependent, :182).  ``with_lengths``: -> (mel2ph, frames of every row) from that same read
        (a row's frames are a prefix by construction; a row may have none)."""
        dur, txt = enc['dur'], enc['txt']
        B, Tt = txt.shape
        per_row = [int(v) for v in (dur * (txt != 0)).sum(-1).tolist()]
        T = max(per_row)
        if T <= 0:
            raise _lib.BsgError('duration predictor produced an empty utterance')
        mel2ph = torch.empty(B, T, dtype=torch.long, device=txt.device)
        with torch.cuda.device(txt.device):
            _lib.check(_lib.load().bsg_length_regulator(_lib.ptr(dur), _lib.ptr(txt), _lib.ptr(mel2ph), B, Tt, T,
                                                        _lib.stream_ptr()), 'bsg_length_regulator')
        return (mel2ph, per_row) if with_lengths else mel2ph

    @torch.no_grad()
    def decode(self, enc_out, mel2ph, spk, speechsing, skip_decoder=False):
        """Frame-level part -> (decoder_inp, mel_out): decode_all() without the adaptor's inputs and outputs."""
        r = self.decode_all(enc_out, mel2ph, spk, speechsing, skip_decoder)
        return r['decoder_inp'], r.get('mel_out')

    @torch.no_grad()
    def decode_all(self, enc_out, mel2ph, spk, speechsing, skip_decoder=False, f0=None, uv=None, n_tok=None, n_frames=None):
        """Frame-level part: gather by mel2ph (+ the pitch adaptor, fs2.py:139-142, 201-234), +spk +style, mask; FFT decoder + mel_out
        (fs2.py:166-195).  ``f0`` / ``uv`` [B,T]: supplied values (neither is written: the reference zeroes the caller's f0 in place,
        fs2.py:230; this does not).  -> dict: decoder_inp, mel_out (unless skip_decoder) and, with the adaptor, pitch_pred [B,T,2],
        f0_denorm [B,T] and pitch_bin [B,T].  ``n_tok`` / ``n_frames`` (B ints each, together): a ragged batch (bsg_fs2_decode_ragged) — row b
        is what the B = 1 call gives on its first n_tok[b] tokens and n_frames[b] frames; beyond them every float is 0, pitch_bin is 1 and
        no input is read."""
        dev = enc_out.device
        h = self.handle()
        B, Tt, _ = enc_out.shape
        mel2ph = mel2ph.to(device=dev, dtype=torch.long).contiguous()
        T = mel2ph.shape[1]
        if T >= self._n_pos:
            raise _lib.BsgError(f'T={T} exceeds the decoder position table ({self._n_pos})')
        if speechsing is not None:
            speechsing = speechsing.to(device=dev, dtype=torch.long).contiguous()
        spk = None if spk is None else spk.contiguous()
        decoder_inp = torch.empty(B, T, self.hidden_size, device=dev)
        mel_out = None if skip_decoder else torch.empty(B, T, self.out_dims, device=dev)
        lib = _lib.load()
        if (n_tok is None) != (n_frames is None):
            raise _lib.BsgError('decode_all: n_tok and n_frames go together')
        rag = None if n_tok is None else ((c_int32 * B)(*n_tok), (c_int32 * B)(*n_frames))
        if not self.use_pitch_embed and self.FRONT == _lib.FS2_FRONT_MIDI:
            with torch.cuda.device(dev):
                if rag is None:
                    _lib.check(lib.bsg_fs2midi_decode(h, _lib.ptr(enc_out.contiguous()), _lib.ptr(mel2ph), _lib.ptr(spk),
                                                      _lib.ptr(speechsing), B, Tt, T, _lib.ptr(decoder_inp), _lib.ptr(mel_out),
                                                      _lib.stream_ptr()), 'bsg_fs2midi_decode')
                else:
                    _lib.check(lib.bsg_fs2_decode_ragged(h, _lib.ptr(enc_out.contiguous()), _lib.ptr(mel2ph), _lib.ptr(spk), _lib.ptr(speechsing),
                                                         None, None, rag[0], rag[1], B, Tt, T, None, None, None, _lib.ptr(decoder_inp),
                                                         _lib.ptr(mel_out), _lib.stream_ptr()), 'bsg_fs2_decode_ragged')
                # the same condition per token (row 0: padding): every frame of a token carries one vector, and the denoiser binds the
                # Tt + 1 rows instead of the T frames (DiffNet.prepare_tokens); cond_tok[b, mel2ph[b, f]] == decoder_inp[b, f] bit for bit
                cond_tok = torch.empty(B, Tt + 1, self.hidden_size, device=dev)
                _lib.check(lib.bsg_fs2midi_token_rows(h, _lib.ptr(enc_out.contiguous()), _lib.ptr(spk), _lib.ptr(speechsing), B, Tt,
                                                      _lib.ptr(cond_tok), _lib.stream_ptr()), 'bsg_fs2midi_token_rows')
            ret = dict(decoder_inp=decoder_inp, cond_tok=cond_tok)
            if not skip_decoder:
                ret['mel_out'] = mel_out
            return ret
        pred = f0d = bins = None
        if self.use_pitch_embed:
            f32 = lambda t: None if t is None else t.to(device=dev, dtype=torch.float32).contiguous()
            f0, uv = f32(f0), f32(uv)
            for n, t in (('f0', f0), ('uv', uv)):
                if t is not None and tuple(t.shape) != (B, T):
                    raise _lib.BsgError(f'{n} must be [B,T] = {(B, T)}, got {tuple(t.shape)}')
            pred = torch.empty(B, T, 2, device=dev)
            f0d = torch.empty(B, T, device=dev)
            bins = torch.empty(B, T, dtype=torch.long, device=dev)
        else:
            f0 = uv = None
        with torch.cuda.device(dev):
            if rag is None:
                _lib.check(lib.bsg_fs2_decode(h, _lib.ptr(enc_out.contiguous()), _lib.ptr(mel2ph), _lib.ptr(spk), _lib.ptr(speechsing),
                                              _lib.ptr(f0), _lib.ptr(uv), B, Tt, T, _lib.ptr(pred), _lib.ptr(f0d), _lib.ptr(bins),
                                              _lib.ptr(decoder_inp), _lib.ptr(mel_out), _lib.stream_ptr()), 'bsg_fs2_decode')
            else:
                _lib.check(lib.bsg_fs2_decode_ragged(h, _lib.ptr(enc_out.contiguous()), _lib.ptr(mel2ph), _lib.ptr(spk), _lib.ptr(speechsing),
                                                     _lib.ptr(f0), _lib.ptr(uv), rag[0], rag[1], B, Tt, T, _lib.ptr(pred), _lib.ptr(f0d),
                                                     _lib.ptr(bins), _lib.ptr(decoder_inp), _lib.ptr(mel_out), _lib.stream_ptr()),
                           'bsg_fs2_decode_ragged')
        ret = dict(decoder_inp=decoder_inp) if skip_decoder else dict(decoder_inp=decoder_inp, mel_out=mel_out)
        if self.use_pitch_embed:
            ret.update(pitch_pred=pred, f0_denorm=f0d, pitch_bin=bins)
        return ret

    def forward(self, txt_tokens, mel2ph=None, spk_embed=None, ref_mels=None, f0=None, uv=None, energy=None,
                skip_decoder=False, spk_embed_dur_id=None, spk_embed_f0_id=None, infer=False, rows=None, ragged=False, **kwargs):
        """``rows`` (slice, extension): generate only these batch rows — what a rank of a sharded run asks for.  The inputs
        stay the WHOLE batch's: the ESM attends over the batch axis, so every row's ``lang`` enters this rank's K / V; with ``mel2ph``
        given nothing else of the other rows is computed (``encode(rows=...)``).  With predicted durations the frame count T is the
        maximum over the whole batch (tts_modules.py:182), so the token-level front then runs on every row and is sliced afterwards.
        ``f0`` / ``uv`` [B,T] (use_pitch_embed): supplied pitch (log2 Hz) and unvoiced flags; never written.
        ``ragged=True`` (extension, ABI v20): every row is what this forward returns for that utterance ALONE — the B = 1 call on
        ``txt_tokens[b, :nt_b]``, ..., ``mel2ph[b, :n_b]`` with nt_b = (txt_tokens[b] > 0).sum() and n_b = (mel2ph[b] > 0).sum() of the given
        or predicted ``mel2ph`` — instead of depending on the batch around it (the ESM's softmax over the batch axis, LayerNorm's bias read
        by the k-tap convolutions in the padding).  Every float output is 0 beyond a row's end, ``mel2ph`` and ``dur_choice`` are 0,
        ``pitch_bin`` is 1; inputs are not read there, and no padding is computed.  ValueError unless the non-pad tokens (and the frames of a
        given ``mel2ph``) are a prefix of each row with at least one token; NotImplementedError with ``rows``.  The lengths cost one host
        read (with predicted durations the frame counts come with the read ``regulate`` makes anyway)."""
        if ragged and rows is not None:
            raise NotImplementedError('forward(ragged=True, rows=...): sharded ragged batches are not supported')
        return _lib.range_guarded(lambda: self._forward(txt_tokens, mel2ph, spk_embed, skip_decoder, rows, f0, uv, ragged=ragged, **kwargs),
                                  f'{type(self).__name__}.forward', device=self, owners=(self,))

    def _forward(self, txt_tokens, mel2ph, spk_embed, skip_decoder, rows, f0=None, uv=None, ragged=False, **kwargs):
        ret = {}
        local = rows is not None and mel2ph is not None      # the token front on this rank's rows only
        n_tok = n_frames = None
        if ragged:
            if mel2ph is None:
                n_tok, = prefix_lengths([txt_tokens > 0], ['txt_tokens'], [1])
            else:
                n_tok, n_frames = prefix_lengths([txt_tokens > 0, mel2ph.to(txt_tokens.device) > 0], ['txt_tokens', 'mel2ph'], [1, 0])
        enc = self.encode(txt_tokens, spk_embed, predict_dur=mel2ph is None, rows=rows if local else None, n_tok=n_tok, **kwargs)
        if mel2ph is None:
            if ragged:
                mel2ph, n_frames = self.regulate(enc, with_lengths=True)
            else:
                mel2ph = self.regulate(enc)
            ret['dur'] = enc['dur_xs'][:, :, None]
            ret['dur_choice'] = enc['dur']
        # (with mel2ph given the reference also runs the predictor for its training loss; inference does not use it)
        enc_out, spk = enc['enc_out'], enc['spk']
        speechsing = kwargs['speechsing'] if self.FRONT == _lib.FS2_FRONT_MIDI else None     # (the plain front has no style row)
        if rows is not None:
            if not local:
                enc_out = enc_out[rows]
            spk = None if spk is None else spk[rows]
            speechsing = None if speechsing is None else speechsing[rows]
            mel2ph = mel2ph[rows]
            f0 = None if f0 is None else f0[rows]
            uv = None if uv is None else uv[rows]
        ret['mel2ph'] = mel2ph
        ret.update(self.decode_all(enc_out, mel2ph, spk, speechsing, skip_decoder, f0=f0, uv=uv, n_tok=n_tok, n_frames=n_frames))
        return ret


class FastSpeech2MIDI(_FastSpeech2Base):
    FRONT = _lib.FS2_FRONT_MIDI

    def __init__(self, dictionary, out_dims=None):
        super().__init__()
        hp = hparams
        check_fs2_hparams(hp, plain=False)
        assert hp['use_spk_id'], 'BiSinger path: use_spk_id speaker table (SURVEY.md §8)'
        assert hp['ffn_act'] == 'gelu' and hp['ffn_padding'] == 'SAME' and hp['use_pos_embed'] and hp.get('rel_pos')
        self._init_base(dictionary, out_dims)
        H = self.hidden_size
        self._init_tail(out_dims)
        self.esm = ESM(d_model=H, nhead=8)
        self.encoder = FastspeechMIDIEncoder(self.esm, self.encoder_embed_tokens)
        self.midi_embed = Embedding(300, H, self.padding_idx)
        self.midi_dur_layer = Linear(1, H)
        self.is_slur_embed = Embedding(2, H)
        self.lang_embed = Embedding(2, H)
        self.style_embed = Embedding(3, H)

    def _token_table(self):
        return self.encoder.embed_positions.table(self.encoder.embed_positions.max_len)

    # ------------------------------------------------------------------ reference forward (fs2.py:94-197)
    @torch.no_grad()
    def encode(self, txt_tokens, spk_embed, predict_dur=False, rows=None, n_tok=None, **kwargs):
        """Token-level front: embeddings + ESM + FFT encoder (+ duration predictor)   (fs2.py:111-165).
        ``n_tok`` (B ints, not with ``rows``): a ragged batch (bsg_fs2midi_encode_ragged) — row b is the B = 1 call on its first n_tok[b]
        tokens: its own ESM (one key: a function of the token's lang id), zeros read beyond its end, nothing computed there.
        ESM attends over the batch axis (common_layers.py:853): the inputs are always the WHOLE batch's.  ``rows`` (a contiguous slice,
        extension): the outputs for these batch rows only — K / V of the ESM (projections of LN(lang_embed[lang]), :850-853, the only thing
        other rows contribute) are still formed for every row; Q, the ESM's FFN, the encoder and the duration predictor run on the rows
        asked for (bsg_fs2midi_encode_rows; SURVEY.md §8e: a rank of a sharded batch encodes its own utterances, not everybody's)."""
        lib = _lib.load()
        h = self.handle()
        dev = txt_tokens.device
        i64 = lambda t: t.to(device=dev, dtype=torch.long).contiguous()
        txt = i64(txt_tokens)
        B, Tt = txt.shape
        if Tt > self._n_rel:
            raise _lib.BsgError(f'T_txt={Tt} exceeds the positional table ({self._n_rel})')
        if kwargs.get('midi_dur') is None or kwargs.get('is_slur') is None:
            raise _lib.BsgError('midi_dur and is_slur are required (every BiSinger entry point passes them)')
        pitch_midi, lang, is_slur = i64(kwargs['pitch_midi']), i64(kwargs['lang']), i64(kwargs['is_slur'])
        midi_dur = kwargs['midi_dur'].to(dev, torch.float32).contiguous()
        spk = i64(spk_embed)
        row0, nb = 0, B
        if rows is not None:
            row0, stop, stride = rows.indices(B)
            if stride != 1 or stop <= row0:
                raise _lib.BsgError('rows must be a contiguous non-empty slice')
            nb = stop - row0
        enc_out = torch.empty(nb, Tt, self.hidden_size, device=dev)
        dur_xs = torch.empty(nb, Tt, device=dev) if predict_dur else None
        dur = torch.empty(nb, Tt, dtype=torch.long, device=dev) if predict_dur else None
        if n_tok is not None and rows is not None:
            raise NotImplementedError('encode(n_tok=..., rows=...): sharded ragged batches are not supported')
        with torch.cuda.device(dev):
            if n_tok is not None:
                _lib.check(lib.bsg_fs2midi_encode_ragged(h, _lib.ptr(txt), _lib.ptr(pitch_midi), _lib.ptr(midi_dur), _lib.ptr(is_slur),
                                                         _lib.ptr(lang), _lib.ptr(spk), (c_int32 * B)(*n_tok), B, Tt, _lib.ptr(enc_out),
                                                         _lib.ptr(dur_xs), _lib.ptr(dur), _lib.stream_ptr()), 'bsg_fs2midi_encode_ragged')
            elif rows is None:
                _lib.check(lib.bsg_fs2midi_encode(h, _lib.ptr(txt), _lib.ptr(pitch_midi), _lib.ptr(midi_dur), _lib.ptr(is_slur),
                                                  _lib.ptr(lang), _lib.ptr(spk), B, Tt, _lib.ptr(enc_out), _lib.ptr(dur_xs),
                                                  _lib.ptr(dur), _lib.stream_ptr()), 'bsg_fs2midi_encode')
            else:
                _lib.check(lib.bsg_fs2midi_encode_rows(h, _lib.ptr(txt), _lib.ptr(pitch_midi), _lib.ptr(midi_dur), _lib.ptr(is_slur),
                                                       _lib.ptr(lang), _lib.ptr(spk), B, Tt, row0, nb, _lib.ptr(enc_out),
                                                       _lib.ptr(dur_xs), _lib.ptr(dur), _lib.stream_ptr()), 'bsg_fs2midi_encode_rows')
        return dict(enc_out=enc_out, txt=txt, spk=spk, dur_xs=dur_xs, dur=dur)


class FastSpeech2(_FastSpeech2Base):
    """modules/fastspeech/fs2.py:24-240 with the 'fft' encoder and decoder, no rel_pos: what GaussianDiffusion builds when ``use_midi`` is
    absent or false (the DiffSinger / PopCS family).  Speaker forms: none, or ``use_spk_id``."""
    FRONT = _lib.FS2_FRONT_PLAIN

    def __init__(self, dictionary, out_dims=None):
        super().__init__()
        hp = hparams
        check_fs2_hparams(hp, plain=True)
        assert hp['ffn_act'] == 'gelu' and hp['ffn_padding'] == 'SAME' and hp['use_pos_embed']
        self._init_base(dictionary, out_dims)
        self.encoder = FastspeechEncoder(self.encoder_embed_tokens)
        self._init_tail(out_dims)

    def _token_table(self):
        return self.encoder.embed_positions.table(DEFAULT_MAX_TARGET_POSITIONS + 2)

    @torch.no_grad()
    def encode(self, txt_tokens, spk_embed, predict_dur=False, rows=None, n_tok=None, **kwargs):
        """Token-level front (fs2.py:100-129): one embedding launch, the FFT encoder (+ duration predictor).  Nothing couples the rows of a
        batch: ``rows`` (a contiguous slice) simply selects the rows that run.  ``n_tok`` (B ints, not with ``rows``): a ragged batch
        (bsg_fs2_encode_plain_ragged) — row b is the B = 1 call on its first n_tok[b] tokens."""
        lib = _lib.load()
        h = self.handle()
        dev = txt_tokens.device
        txt = txt_tokens.to(device=dev, dtype=torch.long).contiguous()
        B, Tt = txt.shape
        if Tt >= self._n_rel:
            raise _lib.BsgError(f'T_txt={Tt} exceeds the positional table ({self._n_rel})')
        spk = None
        if hasattr(self, 'spk_embed_proj'):
            if spk_embed is None:
                raise _lib.BsgError('use_spk_id: spk_embed (speaker ids [B]) is required')
            spk = spk_embed.to(device=dev, dtype=torch.long).contiguous()
        row0, nb = 0, B
        if rows is not None:
            row0, stop, stride = rows.indices(B)
            if stride != 1 or stop <= row0:
                raise _lib.BsgError('rows must be a contiguous non-empty slice')
            nb = stop - row0
        enc_out = torch.empty(nb, Tt, self.hidden_size, device=dev)
        dur_xs = torch.empty(nb, Tt, device=dev) if predict_dur else None
        dur = torch.empty(nb, Tt, dtype=torch.long, device=dev) if predict_dur else None
        if n_tok is not None and rows is not None:
            raise NotImplementedError('encode(n_tok=..., rows=...): sharded ragged batches are not supported')
        with torch.cuda.device(dev):
            if n_tok is not None:
                _lib.check(lib.bsg_fs2_encode_plain_ragged(h, _lib.ptr(txt), _lib.ptr(spk), (c_int32 * B)(*n_tok), B, Tt, _lib.ptr(enc_out),
                                                           _lib.ptr(dur_xs), _lib.ptr(dur), _lib.stream_ptr()), 'bsg_fs2_encode_plain_ragged')
            else:
                _lib.check(lib.bsg_fs2_encode_plain(h, _lib.ptr(txt), _lib.ptr(spk), B, Tt, row0, nb, _lib.ptr(enc_out), _lib.ptr(dur_xs),
                                                    _lib.ptr(dur), _lib.stream_ptr()), 'bsg_fs2_encode_plain')
        return dict(enc_out=enc_out, txt=txt, spk=spk, dur_xs=dur_xs, dur=dur)
