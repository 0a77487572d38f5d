"""The plain FastSpeech2 front and the frame-level pitch adaptor restated in float32 / float64 on top of oracle/fs2.py's helpers, plus the
formula inputs, weights and bounds that tests/test_fs2_pitch_cpu.py and tests/test_gpu_fs2_pitch.py share.

Follows (paths relative to the reference's train_bisinger):
  modules/fastspeech/fs2.py            FastSpeech2.forward :96-152, add_pitch :201-234 (pitch_type frame, pitch_ar false)
  modules/fastspeech/tts_modules.py    PitchPredictor :194-237 (no mask between the layers), FastspeechEncoder :312-349 (no rel_pos)
  modules/diffsinger_midi/fs2.py       FastSpeech2MIDI.forward :166-195 (the style row in the decoder input)
  utils/pitch_utils.py                 f0_to_coarse :22-31, denorm_f0 :63-76 (pitch_norm log)
"""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import fs2 as ofs2

F0_BIN = 256
MEL_MIN = 1127 * np.log(1 + 50.0 / 700)
MEL_MAX = 1127 * np.log(1 + 1100.0 / 700)

POPCS_HP = dict(use_midi=False, rel_pos=False, use_spk_id=False, use_pitch_embed=True, pitch_type='frame', pitch_ar=False, pitch_norm='log',
                use_uv=True, predictor_layers=2, predictor_kernel=5, dur_predictor_layers=2, dur_predictor_kernel=3, num_spk=1)

# One bound per output (x max(1, max |want|); f0_denorm relative to max(1, f0)): 4 x the largest deviation of the float32 restatement from
# the float64 one, measured on the CPU over every case of tests/test_gpu_fs2_pitch.py (frame_cases(), PLAIN, the MIDI end-to-end case).
# tests/test_fs2_pitch_cpu.py::test_bounds_cover_the_float32_restatement evaluates the cases up to 129 frames again and holds every
# float32 figure to bound / 4.  Largest float32 figures (where): pitch_pred 3.49e-7 (frame cases), f0_denorm 1.16e-6
# (frame cases, predicted f0), decoder_inp 6.09e-7, enc_out 6.89e-7 (both: MIDI end to end, 2 x 12 x 64), mel_out 8.56e-7
# (plain end to end, 2 x 100 x 203).
MEASURED_F32 = {'pitch_pred': 3.50e-7, 'f0_denorm': 1.17e-6, 'decoder_inp': 6.09e-7, 'enc_out': 6.90e-7, 'mel_out': 8.57e-7}
BOUND = {k: 4 * v for k, v in MEASURED_F32.items()}
TIE_DELTA = BOUND['pitch_pred'] * 125 + 1e-3      # distance of f0_mel + 0.5 from an integer below which either neighbouring bin is accepted


# ----------------------------------------------------------------------------------------------- arithmetic
def f0_to_mel_bins(f0_denorm):
    """-> (f0_mel after the affine map and the clamps (the value whose rounding is the bin), bin)   pitch_utils.py:22-31"""
    f0_mel = 1127 * (1 + f0_denorm / 700).log()
    pos = f0_mel > 0
    f0_mel = torch.where(pos, (f0_mel - MEL_MIN) * (F0_BIN - 2) / (MEL_MAX - MEL_MIN) + 1, f0_mel)
    f0_mel = torch.where(f0_mel <= 1, torch.ones_like(f0_mel), f0_mel)
    f0_mel = torch.where(f0_mel > F0_BIN - 1, torch.full_like(f0_mel, F0_BIN - 1), f0_mel)
    return f0_mel, (f0_mel + 0.5).long()


def bin_centre_f0(bins):
    """log2-Hz f0 (float32) whose f0_mel is exactly the integer `bins` (2 .. 254): as far from a rounding edge as a frame can be."""
    mel = (np.asarray(bins, np.float64) - 1) * (MEL_MAX - MEL_MIN) / (F0_BIN - 2) + MEL_MIN
    return np.log2(700 * (np.exp(mel / 1127) - 1)).astype(np.float32)


def pitch_predictor(sd, p, xs, n_layers, kernel, dtype):
    """PitchPredictor.forward: positions from the first channel, n x [pad, Conv1d, ReLU, LayerNorm(eps 1e-12)] WITHOUT masks, Linear(-> 2)."""
    g = lambda k: sd[p + k].to(dtype)
    pos = ofs2.make_positions(xs[..., 0], 0)
    table = ofs2.sinusoidal_table(max(4096, int(pos.max()) + 1), xs.shape[-1], 0).to(dtype)
    xs = xs + g('pos_embed_alpha') * table.index_select(0, pos.view(-1)).view(*pos.shape, -1)
    xs = xs.transpose(1, -1)
    for i in range(n_layers):
        xs = F.pad(xs, ((kernel - 1) // 2, (kernel - 1) // 2))
        xs = F.relu(F.conv1d(xs, g(f'conv.{i}.1.weight'), g(f'conv.{i}.1.bias')))
        xs = F.layer_norm(xs.transpose(1, -1), (xs.shape[1],), g(f'conv.{i}.3.weight'), g(f'conv.{i}.3.bias'), 1e-12).transpose(1, -1)
    return F.linear(xs.transpose(1, -1), g('linear.weight'), g('linear.bias'))


def frame_part(sd, prefix, enc, mel2ph, spk_id, style_id, hp, dtype, f0=None, uv=None):
    """fs2.py:131-146 (midi :168-189) from the encoder output on: -> dict(pitch_pred, f0_denorm, f0_mel, pitch_bin, decoder_inp)."""
    g = lambda k: sd[prefix + k].to(dtype)
    H = enc.shape[-1]
    enc = enc.to(dtype)
    gathered = torch.gather(F.pad(enc, [0, 0, 1, 0]), 1, mel2ph[..., None].repeat([1, 1, H]))
    keep = (mel2ph > 0).to(dtype)[:, :, None]
    spk = F.embedding(spk_id, g('spk_embed_proj.weight'))[:, None, :] if spk_id is not None else 0
    ret = {}
    dec = gathered
    if hp.get('use_pitch_embed'):
        pitch_inp = (gathered + spk) * keep
        ret['pitch_pred'] = pred = pitch_predictor(sd, prefix + 'pitch_predictor.', pitch_inp, hp['predictor_layers'], hp['predictor_kernel'], dtype)
        given_f0 = f0
        f0 = pred[:, :, 0] if f0 is None else f0.to(dtype)
        if hp.get('use_uv', True) and uv is None:
            uv = pred[:, :, 1] > 0
        f0d = 2 ** f0
        if uv is not None and hp.get('use_uv', True):
            f0d = torch.where(uv > 0, torch.zeros_like(f0d), f0d)
        ret['f0_denorm'] = f0d = torch.where(mel2ph == 0, torch.zeros_like(f0d), f0d)
        ret['f0_mel'], ret['pitch_bin'] = f0_to_mel_bins(f0d)
        if given_f0 is None:      # fs2.py:230 f0[pitch_padding] = 0 writes through the view f0 = pitch_pred[:, :, 0]
            ret['pitch_pred'] = torch.cat([torch.where(mel2ph == 0, torch.zeros_like(f0), pred[:, :, 0])[..., None], pred[:, :, 1:]], -1)
        dec = dec + F.embedding(ret['pitch_bin'], g('pitch_embed.weight'))
    dec = dec + spk
    if style_id is not None:
        dec = dec + F.embedding(style_id, g('style_embed.weight'))[:, None, :]
    ret['decoder_inp'] = dec * keep
    return ret


def plain_encoder(sd, prefix, txt, hp, dtype):
    """FastspeechEncoder.forward :329-349 without rel_pos."""
    H = hp['hidden_size']
    x = math.sqrt(H) * F.embedding(txt, sd[prefix + 'encoder.embed_tokens.weight'].to(dtype))
    pos = ofs2.make_positions(txt, 0)
    x = x + ofs2.sinusoidal_table(max(2000, int(pos.max()) + 1), H, 0).to(dtype).index_select(0, pos.view(-1)).view(*pos.shape, -1)
    return ofs2.fft_blocks(sd, prefix + 'encoder.', x, txt.eq(0), hp['enc_layers'], hp['num_heads'], hp['enc_ffn_kernel_size'], False, dtype)


def forward(sd, inp, hp, prefix='fs2.', dtype=torch.float32, f0=None, uv=None, skip_decoder=False):
    """FastSpeech2.forward (hp['use_midi'] false) or FastSpeech2MIDI.forward (true), infer=True, with the adaptor when hp['use_pitch_embed'].
    ``inp``: synth.synth_inputs' dict as tensors (mel2ph optional)."""
    hp = {**ofs2.DEFAULT_HP, **hp}
    g = lambda k: sd[prefix + k].to(dtype)
    txt = inp['txt_tokens']
    ret = {}
    if hp.get('use_midi'):
        r = ofs2.fs2_forward(sd, inp, prefix, hp, skip_decoder=True, dtype=dtype)
        enc, mel2ph = r['enc_out'], r['mel2ph']
        ret.update({k: r[k] for k in ('dur', 'dur_choice') if k in r})
        spk_id, style_id = inp['spk_embed'], inp['speechsing']
    else:
        enc = plain_encoder(sd, prefix, txt, hp, dtype)
        spk_id, style_id = (inp['spk_embed'] if hp.get('use_spk_id') else None), None
        mel2ph = inp.get('mel2ph')
        if mel2ph is None:
            spk = F.embedding(spk_id, g('spk_embed_proj.weight'))[:, None, :] if spk_id is not None else 0
            dur_inp = (enc + spk) * (txt > 0).to(dtype)[:, :, None]
            dur, xs = ofs2.duration_predictor(sd, prefix + 'dur_predictor.', dur_inp, txt == 0, hp['dur_predictor_layers'],
                                              hp['dur_predictor_kernel'], dtype)
            ret['dur'], ret['dur_choice'] = xs, dur
            mel2ph = ofs2.length_regulator(dur, txt == 0)
    ret['mel2ph'], ret['enc_out'] = mel2ph, enc
    ret.update(frame_part(sd, prefix, enc, mel2ph, spk_id, style_id, hp, dtype, f0, uv))
    if skip_decoder:
        return ret
    y = ofs2.fft_blocks(sd, prefix + 'decoder.', ret['decoder_inp'], None, hp['dec_layers'], hp['num_heads'], hp['dec_ffn_kernel_size'], True, dtype)
    ret['mel_out'] = F.linear(y, g('mel_out.weight'), g('mel_out.bias')) * (mel2ph > 0).to(dtype)[:, :, None]
    return ret


# ----------------------------------------------------------------------------------------------- formula weights and inputs
def make_pitch_visible(sd, prefix='fs2.'):
    """Raw formula weights put 2**pred near 1 Hz: every frame in bin 1.  The Linear's f0 row gets the bias of a sung pitch (log2 220 Hz) and
    half the weight scale (about +-1 octave at 2 sigma), so that predicted f0 spreads over the bins; the uv row stays (about half voiced).
    In place on a dict of tensors or arrays; returns it."""
    w, b = sd[prefix + 'pitch_predictor.linear.weight'], sd[prefix + 'pitch_predictor.linear.bias']
    w[0] = w[0] * 0.5
    b[0] = math.log2(220.0)
    # likewise the 2-layer duration predictor's raw output rounds to 0 frames per token: a bias of ln 4 gives durations around 3
    sd[prefix + 'dur_predictor.linear.bias'][0] = math.log(4.0)
    return sd


def frame_inputs(B, Tt, T, lens=None, seed=3, H=256):
    """Formula inputs of the frame-level part alone: enc_out [B,Tt,H] ~ N(0,1), mel2ph (row b cut to lens[b] frames), speaker and style
    ids, supplied f0 at bin centres (bins 2 .. 254) and uv (a fifth unvoiced)."""
    rs = np.random.RandomState(seed * 1000 + B * 100 + T)
    d = dict(enc_out=rs.standard_normal((B, Tt, H)).astype(np.float32),
             spk_embed=rs.randint(0, 2, size=(B,)).astype(np.int64), speechsing=np.ones((B,), np.int64),
             f0=bin_centre_f0(rs.randint(2, 255, size=(B, T))), uv=(rs.uniform(size=(B, T)) < 0.2).astype(np.float32))
    mel2ph = np.zeros((B, T), np.int64)
    for b in range(B):
        n = T if lens is None else lens[b]
        mel2ph[b, :n] = np.arange(n) * Tt // n + 1
    d['mel2ph'] = mel2ph
    return d


def near_ties(ref64, delta=None, uv_tol=None):
    """Boolean [B,T]: frames of the float64 restatement whose bin (or predicted uv state) a deviation within the bounds may flip."""
    delta = TIE_DELTA if delta is None else delta
    uv_tol = BOUND['pitch_pred'] * max(1.0, float(ref64['pitch_pred'].abs().max())) if uv_tol is None else uv_tol
    x = ref64['f0_mel'].double() + 0.5
    tie = (x - torch.round(x)).abs() < delta
    return tie, ref64['pitch_pred'][..., 1].abs() < uv_tol


def spec_of(module, prefix='fs2.'):
    return OrderedDict((prefix + k, tuple(v.shape)) for k, v in module.state_dict().items())


# ----------------------------------------------------------------------------------------------- shared cases
class PhoneEncoder:
    """65 phonemes, pad id 0: the dictionary the formula inputs of synth.synth_inputs index."""

    def __len__(self):
        return 65

    def pad(self):
        return 0


def build(front, depth=2, use_uv=True, spk=None, seed=0, pitch=True):
    """A drop-in (CPU, formula weights of `seed`, pitch made visible) and the hyper-parameters the restatement reads.  front: 'midi' (the
    BiSinger chain with use_pitch_embed) or 'plain' (the PopCS chain; `spk`: use_spk_id, default off)."""
    from bisinger_amd.fs2 import FastSpeech2, FastSpeech2MIDI
    from bisinger_amd.hparams import hparams
    from tests.util import load_formula_weights, use_config
    use_config()
    if front == 'plain':
        hparams.update(POPCS_HP)
        hparams['use_spk_id'] = bool(spk)
    hparams.update(use_pitch_embed=pitch, use_uv=use_uv, predictor_layers=depth, predictor_kernel=5)
    hp = dict(hidden_size=256, enc_layers=hparams['enc_layers'], dec_layers=hparams['dec_layers'], num_heads=hparams['num_heads'],
              enc_ffn_kernel_size=hparams['enc_ffn_kernel_size'], dec_ffn_kernel_size=hparams['dec_ffn_kernel_size'],
              dur_predictor_layers=hparams['dur_predictor_layers'], dur_predictor_kernel=hparams['dur_predictor_kernel'],
              use_midi=front == 'midi', use_spk_id=bool(hparams['use_spk_id']), use_pitch_embed=pitch, use_uv=use_uv,
              predictor_layers=depth, predictor_kernel=5)
    m = (FastSpeech2MIDI if front == 'midi' else FastSpeech2)(PhoneEncoder(), 80)
    load_formula_weights(m, seed, prefix='fs2.')
    if pitch:
        with torch.no_grad():
            make_pitch_visible({'fs2.' + k: v for k, v in m.state_dict().items()})
    use_config()      # the module keeps what it read; the global table goes back to the shipped configuration
    return m, hp


EDGE_T = (1, 2, 3, 5, 31, 32, 33, 127, 128, 129)
MODES = ('pred', 'f0', 'f0uv')


def frame_cases():
    """(front, depth, use_uv, mode, B, T, lens) of the predictor + tail edge cases: every T of EDGE_T at B = 1 and at B = 3 with rows of 33, 1
    and T frames in one batch, both depths, use_uv on and off and the three supply modes cycled over them, plus 2 x 1000."""
    out = []
    i = 0
    for T in EDGE_T:
        for B in (1, 3):
            lens = None if B == 1 else (33, 1, T)
            # (B alternates with i: depth and use_uv cycle on i // 2 and i // 4, so that both depths meet both batch shapes)
            out.append((('midi', 'plain')[(i // 3) % 2], (2, 5)[(i // 2) % 2], bool((i // 4 + 1) % 2), MODES[i % 3], B, T if B == 1 else max(33, T), lens))
            i += 1
    out.append(('plain', 2, True, 'pred', 2, 1000, (1000, 731)))
    out.append(('midi', 5, True, 'f0uv', 2, 1000, (1000, 731)))
    return out


def frame_reference(sd, hp, inp, mode, dtype):
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    f0 = t['f0'] if mode in ('f0', 'f0uv') else None
    uv = t['uv'] if mode == 'f0uv' else None
    return frame_part(sd, 'fs2.', t['enc_out'], t['mel2ph'], t['spk_embed'] if hp['use_spk_id'] else None,
                      t['speechsing'] if hp['use_midi'] else None, hp, dtype, f0, uv)


# ----------------------------------------------------------------------------------------------- the host that made the goldens
def golden_host_inv_freq():
    """oracle.freq.inv_freq with the float32 vectors of the host that made the goldens (tests/golden/inv_freq.npz; oracle/freq.py: another
    CPU's float32 exp differs by an ulp here and there, and a position table multiplies that by the row index — up to 4999 in the MIDI
    front's reversed table, 1e-5 on decoder_inp).  For monkeypatch.setattr(oracle.freq, 'inv_freq', ...), as tests/test_oracle_golden.py does."""
    import os
    from oracle import freq
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'inv_freq.npz'))
    host = freq.inv_freq

    def inv_freq(exponent):
        for k in ('sinusoidal', 'rel_pos'):
            if np.array_equal(exponent.numpy(), g[k + '.exponent']):
                return torch.from_numpy(g[k + '.value'].copy())
        return host(exponent)
    return inv_freq


def use_golden_host_tables(m):
    """The drop-in's position tables (built on the host with float32 torch ops, as the reference builds its own) from the oracle's table
    functions — call under the patch of golden_host_inv_freq(): the device then indexes the tables the reference indexed when the goldens
    were made.  Instance attributes on the holders; the handle is created anew."""
    H = m.hidden_size
    for holder in [m.decoder.embed_positions, m.encoder.embed_positions] + ([m.pitch_predictor.embed_positions] if m.use_pitch_embed else []):
        if type(holder).__name__ == 'RelPositionalEncoding':
            holder.table = lambda length: ofs2.rel_pos_table(length, H)
        else:
            holder.table = lambda num: ofs2.sinusoidal_table(num, H, 0)
    m.release()
    return m
