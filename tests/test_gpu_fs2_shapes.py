"""GPU parity of every FastSpeech2-MIDI launch form at its shape edges, against the float64 evaluation of the CPU oracle.

plan_fft() (csrc/fs2.hip) picks per call among nine attention forms (flash_attn_planes_kernel<2> with its keys on 1, 2 or 4 workgroups,
flash_attn_split_kernel<2> / <4>, flash_attn_kernel<2> / <4>, the score tensor + masked_softmax_kernel), two producers of Q / K / V^T (the
GEMM's own epilogue, qkv_split_kernel) and, inside launch_gemm_h2w, 32-, 64- or 128-row tiles with 4-, 8- or 16-step rings; the ESM has two
attention kernels.  tests/test_gpu_fs2.py and tests/test_gpu_edges.py reach part of that map, against the fp32 oracle at 1e-4 .. 3e-4.  Here

  * WHICH form ran is read from bsg_fs2midi_last_path / bsg_fftden_last_path (tokens written at the branch that launched), never restated
    from the thresholds: test_default_path_covers_every_launch_form fails and names the form if a retuned threshold moves a shape off it;
  * the shapes sit where the tilings end: rows shorter than one 32-key block, T % 32 in {0, 1, 31}, a last key split that owns one key,
    T % 4 != 0 (the scalar V^T epilogue), GEMM tiles that straddle several utterances, more than 64 utterances (the ESM's other kernel);
  * rows are cut to free lengths (_cut: the rule of synth.synth_inputs(ragged=True) with the token counts given), so that whole key blocks,
    whole key splits and whole query tiles lie in a row's padding: 3 x 1000 with rows of 1000, 225 and 50 frames;
  * the reference is oracle.fs2.fs2_forward(dtype=float64) (oracle.candidate_decoder.fft_denoiser_forward for the FFT denoiser); the fp32
    oracle's own deviation from it is printed per shape as the yardstick, with the ratio HIP / fp32 oracle;
  * compared are enc_out (of encode()), decoder_inp and mel_out: max-abs over everything, over the first 64 and the last 64 valid frames of
    every row, and per row; the padded frames must equal the reference (zero) exactly; no range event and no retry may happen;
  * test_stale_workspace_never_reaches_a_result runs short calls after a long one on one handle, once with every activation workspace
    filled with NaN bytes in between (bsg_fs2midi_debug_poison_workspace), and asks for bit-identity with a fresh handle: the planes
    attention reads K rows and V^T columns past T by design, which is harmless only while they are masked or zero;
  * the fallback forms run in one child process per switch set (the switches are read once per process) against the same references, and
    each set is checked by last_path to have changed the tokens it is meant to change; flash_attn_split_kernel<4> and flash_attn_kernel<4>,
    which a range-guard demotion lands on at 64 x 1000, are reached at 64 x 20 x 500.

Weights: the formula weights of seed 0 as in tests/test_gpu_fs2.py (seed 17 for the FFT denoiser, tests/test_gpu_f4.py).

Bar.  The project's bars are 1e-4 x max(1, max |want|) for enc_out and decoder_inp and 2e-4 for mel_out (tests/test_gpu_fs2.py, against the
fp32 oracle).  Measured on an MI355X against float64, every form of this file sits within 2 x of the fp32 oracle's own deviation at the
same shape (default path: at most 1.46 x, enc_out at 1 x 50 x 511; fallback forms: at most 1.97 x, mel_out of the fp32 pipe at 1 x 1 x 1,
1.78e-6 against 9.0e-7) — no case comes near the 10 x that would ask for an explanation.  The bar of this file is 4 x the largest
default-path figure per output (the margin is for other boxes and for the summation orders of the tile heights and key splits):
  enc_out 9.1e-6 (2.27e-6 at 64 x 12 x 33), decoder_inp 9.0e-6 (2.26e-6 at 64 x 12 x 33), mel_out 1.07e-5 (2.68e-6 at 16 x 100 x 1000),
each x max(1, max |want|) (max |want| is 3.1 .. 4.5 at every shape), for the whole batch, the edge windows and every row alike; the
fallback forms meet the same bar (their largest: 3.60e-6, mel_out of the fp32 pipe at 64 x 20 x 500).  FFT denoiser: 1.08e-5 (2.69e-6
at 2 x 1000; the project's bar is 2e-4).

Measured (max-abs against float64, whole batch: HIP|fp32 oracle; the edge-window and per-row figures are never above the whole-batch one and
are printed by the tests; B x T_txt x T; tiles = rows per tile of the stack's pre-split GEMMs):
  default path                       enc_out           decoder_inp        mel_out            ESM    enc attn   enc tiles dec attn   dec tiles
  1x1x1                             7.87e-07|6.89e-07  7.90e-07|6.85e-07  1.04e-06|9.00e-07  wave   split/nw2  32       split/nw2  32
  2x3x5                             9.12e-07|9.51e-07  1.09e-06|9.50e-07  1.50e-06|1.47e-06  wave   split/nw2  32       split/nw2  32
  1x4x10                            1.10e-06|9.83e-07  1.12e-06|1.02e-06  1.38e-06|1.47e-06  wave   split/nw2  32       split/nw2  32
  3x5x31                            1.28e-06|9.91e-07  1.32e-06|9.91e-07  1.69e-06|1.70e-06  wave   split/nw2  32       planes/ks1 32
  1x4x32                            1.10e-06|9.83e-07  1.12e-06|1.02e-06  1.58e-06|1.49e-06  wave   split/nw2  32       planes/ks1 32
  1x4x33                            1.10e-06|9.83e-07  1.12e-06|1.02e-06  1.47e-06|1.59e-06  wave   split/nw2  32       planes/ks1 32
  1x25x255                          1.01e-06|1.41e-06  1.06e-06|1.45e-06  2.13e-06|1.82e-06  wave   split/nw2  32       planes/ks2 32
  1x25x256                          1.01e-06|1.41e-06  1.06e-06|1.45e-06  1.74e-06|1.64e-06  wave   split/nw2  32       planes/ks2 32
  1x25x257                          1.01e-06|1.41e-06  1.06e-06|1.45e-06  1.70e-06|1.67e-06  wave   split/nw2  32       planes/ks2 32
  1x50x511                          1.78e-06|1.21e-06  1.77e-06|1.36e-06  1.74e-06|1.71e-06  wave   planes/ks1 32       planes/ks4 32
  2x100x1000                        1.41e-06|1.55e-06  1.41e-06|1.56e-06  1.76e-06|2.15e-06  wave   planes/ks1 32       planes/ks4 32,64
  2x100x1001                        1.41e-06|1.55e-06  1.41e-06|1.56e-06  2.04e-06|1.82e-06  wave   planes/ks1 32       planes/ks4 32,64
  2x100x993                         1.41e-06|1.55e-06  1.41e-06|1.56e-06  2.01e-06|1.92e-06  wave   planes/ks1 32       planes/ks4 32,64
  1x481x1000                        1.26e-06|1.40e-06  1.19e-06|1.42e-06  1.80e-06|1.76e-06  wave   planes/ks4 32       planes/ks4 32
  3x40x1000 lens [40, 9, 2]         1.45e-06|1.23e-06  1.44e-06|1.27e-06  2.09e-06|1.88e-06  wave   planes/ks1 32       planes/ks4 32,64
  4x30x301 lens [30, 30, 4, 17]     1.54e-06|1.84e-06  1.60e-06|1.93e-06  2.00e-06|1.82e-06  wave   planes/ks1 32       planes/ks2 32
  5x30x413                          1.73e-06|1.40e-06  1.70e-06|1.46e-06  1.89e-06|1.78e-06  wave   planes/ks1 32       planes/ks2 32,64
  64x12x33                          2.27e-06|1.71e-06  2.26e-06|1.73e-06  2.16e-06|2.07e-06  wave   planes/ks1 32,128   planes/ks1 32,128
  16x100x1000                       1.67e-06|1.58e-06  1.67e-06|1.64e-06  2.68e-06|2.16e-06  wave   planes/ks1 32,64    planes/ks1 64,128
  8x100x1001                        1.87e-06|1.62e-06  1.89e-06|1.53e-06  2.02e-06|2.22e-06  wave   planes/ks1 32       planes/ks2 32,64,128
  1x250x2500                        1.31e-06|1.58e-06  1.19e-06|1.68e-06  2.49e-06|2.27e-06  wave   planes/ks2 32       planes/ks4 32,64
  2x250x2499 lens [250, 31]         1.52e-06|1.53e-06  1.52e-06|1.68e-06  2.11e-06|1.92e-06  wave   planes/ks2 32       planes/ks2 32,64
  65x6x24                           1.94e-06|1.83e-06  1.95e-06|1.85e-06  2.40e-06|2.34e-06  thread split/nw2  32,128   planes/ks1 32,128
  8x40x120 rows 2:5                 1.84e-06|1.81e-06  1.85e-06|1.85e-06  1.74e-06|1.80e-06  wave   planes/ks1 32       planes/ks1 32
  64x20x200 rows 8:16               1.91e-06|1.64e-06  1.90e-06|1.71e-06  1.95e-06|1.97e-06  wave   planes/ks1 32       planes/ks1 32,64

  (every case: qkv:fused wherever the attention is planes, qkv:h2w under split/nw2; the ESM's GEMMs on h2w/32/deep, on gemm_split at
  65 utterances.  Both stacks reach every form: nothing had to be exempted.  The issue's 2 x 100 x 1001 has T % 32 == 9, so 2 x 100 x 993
  was added for the one-key last block on four splits, and 1 x 481 x 1000 for the encoder on four splits.)

  fallback forms (largest of the set over its shapes, enc_out / decoder_inp / mel_out; the attention it ran):
  split_attn   2.26e-6 / 2.31e-6 / 2.48e-6   split/nw2, split/nw4 at 64 x 20 x 500 (decoder), esm:thread
  fp32_pipe    2.71e-6 / 2.72e-6 / 3.60e-6   flash/nw2, flash/nw4 at 64 x 20 x 500 (decoder), gemm_fast, esm:thread
  softmax      1.45e-6 / 1.44e-6 / 2.37e-6   score tensor + masked_softmax_kernel, gemm_split (this switch leaves the pre-split path)
  qkv_split    1.45e-6 / 1.44e-6 / 2.01e-6   planes/ks1 fed by qkv_split_kernel
  ks8          1.45e-6 / 1.44e-6 / 2.32e-6   planes/ks8 at 257 (splits 5 .. 7 start beyond T) and at 1000 frames, ks2 at 33
  gemm_split   1.30e-6 / 1.44e-6 / 2.12e-6   split/nw2 on fp32 Q K V, gemm_split, esm:thread
  ring4        1.45e-6 / 1.44e-6 / 2.09e-6   64-row tiles and the 4-step ring everywhere, attention as the default

  FFT denoiser   1 x 1: 1.46e-6 | 9.96e-7 (split/nw2);  2 x 33: 2.13e-6 | 2.10e-6 (planes/ks1);  2 x 301: 2.28e-6 | 1.91e-6 (planes/ks2);
                 2 x 1000: 2.69e-6 | 2.12e-6 (planes/ks4)

Stale workspace: bit-identical to a fresh handle at all four shapes and for the denoiser, after finite stale data and after NaN bytes
over every activation workspace: what the planes attention reads past T is masked (K rows) or was zeroed by its producer (V^T columns).

No form deviated: nothing in the kernels or the host logic was changed for this file.
"""
import json
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from bisinger_amd import _lib, synth
from oracle import candidate_decoder as ocd, fs2 as ofs2
from tests.util import ROOT, cpu_sd, load_formula_weights, load_golden, use_config

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

F64, F32 = torch.float64, torch.float32
OUTS = ('enc_out', 'decoder_inp', 'mel_out')
# x max(1, max |want|).  The project's bars (tests/test_gpu_fs2.py) are 1e-4 for decoder_inp and enc_out, 2e-4 for mel_out
BAR = {'enc_out': 9.1e-6, 'decoder_inp': 9.0e-6, 'mel_out': 1.07e-5}      # 4 x the largest default-path deviation measured (module docstring)
DEN_BAR = 1.08e-5   # 4 x the FFT denoiser's largest (2.69e-6 at 2 x 1000); tests/test_gpu_f4.py: 2e-4
EDGE = 64           # frames at each end of a row's valid part


def C(B, Tt, T, lens=None, rows=None):
    """A case: B utterances of Tt tokens and T frames; `lens`: token count per row (row 0 full); `rows`: the rank front's batch rows."""
    return (B, Tt, T, tuple(lens) if lens else None, (rows.start, rows.stop) if rows else None)


TINY = [C(1, 1, 1), C(2, 3, 5), C(1, 4, 10)]                                       # B T < 32 or Tp > 3 T: no planes form
KS1 = [C(3, 5, 31), C(1, 4, 32), C(1, 4, 33)]                                      # one partial block; one block; a second block with ONE key
KS2 = [C(1, 25, 255), C(1, 25, 256), C(1, 25, 257)]                                # 8 / 8 / 9 blocks on two splits
KS4 = [C(1, 50, 511), C(2, 100, 1000), C(2, 100, 1001), C(2, 100, 993), C(1, 481, 1000)]   # 993: the last split ends in a one-key block; 481: the ENCODER on four splits, T_txt % 32 == 1
PADDED = [C(3, 40, 1000, [40, 9, 2]), C(4, 30, 301, [30, 30, 4, 17])]              # splits and query tiles in padding only; T % 4 != 0
ODD = [C(5, 30, 413), C(64, 12, 33)]                                               # odd everything; GEMM tiles over 3 - 4 utterances
BENCH = [C(16, 100, 1000), C(8, 100, 1001)]                                        # the bench shape and its T % 4 != 0 neighbour
LONG = [C(1, 250, 2500), C(2, 250, 2499, [250, 31])]                               # 79 key blocks
MANY = [C(65, 6, 24)]                                                              # more than 64 utterances: esm_attention_kernel<32>
RANK = [C(8, 40, 120, rows=slice(2, 5)), C(64, 20, 200, rows=slice(8, 16))]        # lrows != rows in the ESM
SHAPES = TINY + KS1 + KS2 + KS4 + PADDED + ODD + BENCH + LONG + MANY + RANK
SHORT_LIST = [C(1, 1, 1), C(1, 4, 33), C(1, 25, 257), C(3, 40, 1000, [40, 9, 2])]  # what every fallback form runs
NW4 = C(64, 20, 500)                                                               # cdiv(T, 128) B heads = 512: the four-wave forms
STALE_FIRST = C(2, 100, 1000)
STALE_THEN = [C(3, 5, 31), C(1, 4, 33), C(1, 25, 257), C(4, 30, 301, [30, 30, 4, 17])]

_REF = {}       # case -> inputs, float64 / fp32 references
_CASES = {}     # case -> figures of the default path


def _name(case):
    B, Tt, T, lens, rows = case
    return f'{B}x{Tt}x{T}' + (f' lens {list(lens)}' if lens else '') + (f' rows {rows[0]}:{rows[1]}' if rows else '')


def _cut(inp, lens):
    """Row b cut to lens[b] tokens: the rule of synth.synth_inputs(ragged=True), with the lengths free."""
    B, Tt = inp['txt_tokens'].shape
    T = inp['mel2ph'].shape[1]
    assert len(lens) == B and lens[0] == Tt and all(1 <= n <= Tt for n in lens)
    for b, n_tok in enumerate(lens):
        for k in ('txt_tokens', 'pitch_midi', 'midi_dur', 'is_slur', 'lang'):
            inp[k][b, n_tok:] = 0
        inp['mel2ph'][b] = np.minimum(np.arange(T) * Tt // T + 1, n_tok)
        inp['mel2ph'][b, T * n_tok // Tt:] = 0
        assert (inp['mel2ph'][b] > 0).any(), 'no row is empty'
    return inp


def _inputs(case):
    B, Tt, T, lens, rows = case
    inp = synth.synth_inputs(B, Tt, T, seed=5)
    return _cut(inp, lens) if lens else inp


def _row_groups(B, T, frames=8000):
    """Rows per oracle call: the float64 oracle holds [rows x heads, T, T] doubles per attention."""
    n = max(1, frames // T)
    return [slice(b, min(B, b + n)) for b in range(0, B, n)]


def _oracle(sd, inp, case, dtype):
    B, Tt, T, lens, rows = case
    ti = {k: torch.from_numpy(v) for k, v in inp.items()}
    if rows:
        r = ofs2.fs2_forward(sd, ti, dtype=dtype, rows=slice(*rows))
        return {k: r[k].double().numpy() for k in OUTS}
    groups = _row_groups(B, T)
    if len(groups) == 1:
        r = ofs2.fs2_forward(sd, ti, dtype=dtype)
        return {k: r[k].double().numpy() for k in OUTS}
    # the token-level front sees the whole batch in every call (the ESM couples rows); the frame-level part runs on the group's rows
    parts = [ofs2.fs2_forward(sd, ti, dtype=dtype, rows=g) for g in groups]
    return {k: np.concatenate([p[k].double().numpy() for p in parts]) for k in OUTS}


def _valid(inp, case):
    """Valid length of every output row: tokens for enc_out, frames for the two frame-level outputs."""
    rows = slice(*case[4]) if case[4] else slice(None)
    ntok = (inp['txt_tokens'][rows] > 0).sum(1)
    nfrm = (inp['mel2ph'][rows] > 0).sum(1)
    return {'enc_out': ntok, 'decoder_inp': nfrm, 'mel_out': nfrm}


def _figures(got, want, n_valid):
    """(whole, edge, per row): max-abs over everything, over the first EDGE and the last EDGE valid frames of every row, and per row."""
    d = np.abs(np.asarray(got, np.float64) - want)
    per_row = [float(d[b].max()) for b in range(d.shape[0])]
    edge = 0.0
    for b, n in enumerate(n_valid):
        n = int(n)
        edge = max(edge, float(d[b, :EDGE].max()), float(d[b, max(0, n - EDGE):max(n, 1)].max()))
    return float(d.max()), edge, per_row


def _ref(sd, case):
    if case not in _REF:
        inp = _inputs(case)
        want, w32 = _oracle(sd, inp, case, F64), _oracle(sd, inp, case, F32)
        nv = _valid(inp, case)
        _REF[case] = dict(inp=inp, want=want, valid=nv, wmax={k: float(np.abs(want[k]).max()) for k in OUTS},
                          f32={k: _figures(w32[k], want[k], nv[k]) for k in OUTS})
    return _REF[case]


class _Enc:
    def __len__(self):
        return 65

    def pad(self):
        return 0


def _make_fs2():
    use_config()
    from bisinger_amd.fs2 import FastSpeech2MIDI
    m = FastSpeech2MIDI(_Enc(), 80)
    load_formula_weights(m, 0, prefix='fs2.')
    return m.cuda()


@pytest.fixture(scope='module')
def fs2():
    m = _make_fs2()
    return m, cpu_sd(m, 'fs2.')


def _run(m, inp, rows=None):
    """encode() for enc_out, then the whole forward; ({output: numpy}, last_path of the forward).  No range event, no retry: last_path then
    names the pass that produced the output."""
    d = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    kw = {k: d[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')}
    rows = slice(*rows) if rows else None
    before = _lib.range_retries
    enc = m.encode(d['txt_tokens'], d['spk_embed'], rows=rows, **kw)
    r = m(d['txt_tokens'], d['mel2ph'], d['spk_embed'], None, None, None, None, infer=True, rows=rows, **kw)
    path = m.last_path()
    assert _lib.range_retries == before and m.gemm_range_peek() == 0, 'a range event fired: last_path would name the repeat'
    return {'enc_out': enc['enc_out'].cpu().numpy(), 'decoder_inp': r['decoder_inp'].cpu().numpy(), 'mel_out': r['mel_out'].cpu().numpy()}, path


def _record(tag, case, got, path, ref):
    rec = dict(path=path, tokens=path.split(), shape={k: got[k].shape for k in OUTS}, finite=all(bool(np.isfinite(got[k]).all()) for k in OUTS),
               fig={}, pad_ok={})
    for k in OUTS:
        if got[k].shape != ref['want'][k].shape:
            continue
        rec['fig'][k] = _figures(got[k], ref['want'][k], ref['valid'][k])
        rec['pad_ok'][k] = all(np.array_equal(got[k][b, int(n):], ref['want'][k][b, int(n):]) and not got[k][b, int(n):].any()
                               for b, n in enumerate(ref['valid'][k]))
    print(f'\nfs2 {tag} {_name(case)}: {path}')
    for k in OUTS:
        if k in rec['fig']:
            (w, e, pr), (w32, e32, pr32) = rec['fig'][k], ref['f32'][k]
            print(f'    {k:11s} hip {w:.2e} edge {e:.2e} worst row {max(pr):.2e} | fp32 oracle {w32:.2e} edge {e32:.2e} worst row {max(pr32):.2e} | '
                  f'hip / fp32 {w / max(w32, 1e-30):.2f} | max|want| {ref["wmax"][k]:.2f}' + (f' | rows {" ".join(f"{v:.1e}" for v in pr)}' if len(pr) <= 8 else ''))
    return rec


def _default_case(fs2, case):
    if case not in _CASES:
        m, sd = fs2
        ref = _ref(sd, case)
        got, path = _run(m, ref['inp'], case[4])
        _CASES[case] = _record('default', case, got, path, ref)
    return _CASES[case], _REF[case]


def _assert_parity(tag, rec, ref):
    assert rec['finite'], tag
    for k in OUTS:
        assert rec['shape'][k] == ref['want'][k].shape, (tag, k, rec['shape'][k])
        assert rec['pad_ok'][k], (tag, k, 'padded frames differ from the reference (zero)')
        bar = BAR[k] * max(1.0, ref['wmax'][k])
        whole, edge, per_row = rec['fig'][k]
        assert whole <= bar, (tag, k, whole, bar, rec['path'])
        assert edge <= bar, (tag, k, 'edge', edge, bar, rec['path'])
        assert max(per_row) <= bar, (tag, k, 'rows', per_row, bar, rec['path'])


@pytest.mark.parametrize('case', SHAPES, ids=_name)
def test_default_path_vs_fp64(case, fs2):
    rec, ref = _default_case(fs2, case)
    B, Tt, T, lens, rows = case
    nb = rows[1] - rows[0] if rows else B
    assert rec['shape'] == {'enc_out': (nb, Tt, 256), 'decoder_inp': (nb, T, 256), 'mel_out': (nb, T, 80)}
    _assert_parity(f'default {_name(case)}', rec, ref)
    sites = {t.split(':')[0] for t in rec['tokens']}
    assert {'esm', 'enc.qkv', 'enc.attn', 'enc.gemm', 'dec.qkv', 'dec.attn', 'dec.gemm'} <= sites, rec['path']
    for st in ('enc.', 'dec.'):      # one attention form and one QKV producer per stack: its layers are equal
        assert len([t for t in rec['tokens'] if t.startswith(st + 'attn:')]) == 1 and len([t for t in rec['tokens'] if t.startswith(st + 'qkv:')]) == 1


# Forms a stack cannot reach on the default path, with the reason (everything else is required of BOTH stacks)
UNREACHABLE = {}


def required_forms():
    req = [('esm_attention_wave_kernel', 'esm:wave'), ('esm_attention_kernel<32>', 'esm:thread')]
    for st in ('enc.', 'dec.'):
        req += [(f'{st} planes attention, keys on {n} workgroup(s)', f'{st}attn:planes/ks{n}') for n in (1, 2, 4)]
        req += [(f'{st} flash_attn_split_kernel<2>', f'{st}attn:split/nw2'), (f'{st} QKV planes from the GEMM epilogue', f'{st}qkv:fused')]
        req += [(f'{st} pre-split GEMM, {n}-row tiles', f'{st}gemm:h2w/{n}/') for n in (32, 64, 128)]
    return [(name, tok) for name, tok in req if tok not in UNREACHABLE]


def _has(tokens, tok):
    return any(t.startswith(tok) if tok.endswith('/') else t == tok for t in tokens)


def _min_frames(case):
    B, Tt, T, lens, rows = case
    return min(T * n // Tt for n in lens) if lens else T


def _ks(tokens, st='dec.'):
    for t in tokens:
        if t.startswith(st + 'attn:planes/ks'):
            return int(t.rsplit('ks', 1)[1])
    return 0


def test_default_path_covers_every_launch_form(fs2):
    """The union of last_path tokens over SHAPES holds every form of the default path for both FFT stacks, and the edges the shapes were
    chosen for were met ON the form they were chosen for.  Cases the parametrised test has run are taken from its record."""
    cases = OrderedDict((c, _default_case(fs2, c)[0]) for c in SHAPES)
    union = sorted({t for r in cases.values() for t in r['tokens']})
    missing = [name for name, tok in required_forms() if not _has(union, tok)]
    edges = OrderedDict([
        ('T % 32 == 1 on two key splits', [c for c, r in cases.items() if c[2] % 32 == 1 and _ks(r['tokens']) == 2]),
        ('T % 32 == 1 on four key splits', [c for c, r in cases.items() if c[2] % 32 == 1 and _ks(r['tokens']) == 4]),
        # split z takes the key blocks [z nbz, (z + 1) nbz), nbz = ceil(ceil(T / 32) / ks): a row that ends before nbz blocks leaves splits 1 .. of masked keys only
        ('a row that ends before the second key split starts', [c for c, r in cases.items() if _ks(r['tokens']) >= 2 and
                                                                _min_frames(c) <= -(-(-(-c[2] // 32)) // _ks(r['tokens'])) * 32]),
        ('T % 4 != 0 with the QKV planes from the GEMM epilogue', [c for c, r in cases.items() if c[2] % 4 and 'dec.qkv:fused' in r['tokens']]),
        ('the rank front (rows != batch) on the wave ESM', [c for c, r in cases.items() if c[4] and 'esm:wave' in r['tokens']]),
    ])
    missing += [name for name, hit in edges.items() if not hit]
    print('\nunion of launch tokens:', ' '.join(union))
    for name, tok in required_forms():
        print(f'  {name} [{tok}]:', [_name(c) for c, r in cases.items() if _has(r['tokens'], tok)])
    for name, hit in edges.items():
        print(f'  {name}:', [_name(c) for c in hit])
    assert not missing, f'launch forms / edges no shape reached: {missing}'


# ------------------------------------------------------------------------------------------------------------------
# stale workspace
# ------------------------------------------------------------------------------------------------------------------
def test_stale_workspace_never_reaches_a_result(fs2):
    """Short calls after a long one on one handle: the planes attention then reads K rows and V^T columns past T that the long call (or
    poison_workspace: NaN bytes) left behind.  Each result must be bit-identical to the same shape on a fresh handle."""
    m, sd = fs2
    other = _make_fs2()
    fresh = {}
    for case in STALE_THEN:
        other.release()      # a new handle: workspaces sized by this call, never written before
        fresh[case] = _run(other, _ref(sd, case)['inp'])
    for poison in (True, False):
        other.release()
        got, path = _run(other, _ref(sd, STALE_FIRST)['inp'])
        assert all(np.isfinite(got[k]).all() for k in OUTS)
        if poison:
            other.poison_workspace()
        for case in STALE_THEN:
            got, path = _run(other, _REF[case]['inp'])
            for k in OUTS:
                assert np.isfinite(got[k]).all(), (poison, _name(case), k, path)
                assert np.array_equal(got[k], fresh[case][0][k]), (poison, _name(case), k, float(np.abs(got[k].astype(np.float64) - fresh[case][0][k]).max()), path)
            assert path == fresh[case][1]
            rec = _record(f'stale (poison {poison})', case, got, path, _REF[case])
            _assert_parity(f'stale {_name(case)}', rec, _REF[case])
    other.release()


# ------------------------------------------------------------------------------------------------------------------
# the fallback forms, one child process per switch set
# ------------------------------------------------------------------------------------------------------------------
CHILD = r'''
import sys, json, torch, numpy as np
sys.path.insert(0, %r)
from tests import test_gpu_fs2_shapes as S
from bisinger_amd import _lib
torch.set_grad_enabled(False)
m = S._make_fs2()
out = {}
for f in sys.argv[2:]:
    z = np.load(f + '.inp.npz')
    inp = {k: z[k] for k in z.files if k != 'rows'}
    got, path = S._run(m, inp, tuple(int(v) for v in z['rows']) if 'rows' in z.files else None)
    np.savez(f + '.' + sys.argv[1] + '.npz', **got)
    out[f] = {'path': path, 'retries': _lib.range_retries, 'events': m.gemm_range_peek()}
print(json.dumps(out))
''' % ROOT


def _attn(tok):
    return {t.split('attn:')[1] for t in tok if '.attn:' in t}


def _gemm(tok):
    return {t.split('gemm:')[1] for t in tok if '.gemm:' in t}


def _check_split_attn(case, tok):
    assert _attn(tok) <= {'split/nw2', 'split/nw4'} and 'esm:thread' in tok, tok
    if case == NW4:
        assert 'dec.attn:split/nw4' in tok, tok


def _check_fp32(case, tok):
    assert _attn(tok) <= {'flash/nw2', 'flash/nw4'} and 'esm:thread' in tok, tok
    assert all(g.startswith(('gemm_fast', 'gemm_f32')) for g in _gemm(tok)) and any(g.startswith('gemm_fast') for g in _gemm(tok)), tok
    assert {t.split('qkv:')[1] for t in tok if '.qkv:' in t} == {'gemm'}, tok
    if case == NW4:
        assert 'dec.attn:flash/nw4' in tok, tok


def _check_softmax(case, tok):
    assert _attn(tok) == {'softmax'}, tok


def _check_qkv_split(case, tok):
    assert not _attn(tok) & {'planes/ks2', 'planes/ks4'} and not any(t.endswith('qkv:fused') for t in tok), tok
    for st in ('enc.', 'dec.'):
        assert (st + 'attn:planes/ks1' in tok) == (st + 'qkv:split_kernel' in tok), tok
    if case[2] >= 32:
        assert 'dec.qkv:split_kernel' in tok, tok


def _check_ks8(case, tok):
    if case[2] >= 257:      # at least 8 key blocks: eight splits; at 257 frames the splits 5 .. 7 start beyond T
        assert 'dec.attn:planes/ks8' in tok, tok


def _check_gemm_split(case, tok):
    assert all(g.startswith('gemm_split') for g in _gemm(tok)) and _gemm(tok), tok


def _check_ring4(case, tok):
    g = _gemm(tok)
    assert g and all(x.startswith('h2w/') and x.endswith('/ring4') and not x.startswith('h2w/32') for x in g), tok


FORMS = OrderedDict([
    ('split_attn', ({'BSG_FLASH_PLANES': '0', 'BSG_ESM_H2W': '0'}, _check_split_attn, True)),
    ('fp32_pipe', ({'BSG_GEMM_SPLIT': '0', 'BSG_H2': '0'}, _check_fp32, True)),
    ('softmax', ({'BSG_NO_FLASH_ATTN': '1'}, _check_softmax, False)),
    ('qkv_split', ({'BSG_QKV_FUSED': '0', 'BSG_FLASH_KS': '1'}, _check_qkv_split, False)),
    ('ks8', ({'BSG_FLASH_KS': '8'}, _check_ks8, False)),
    ('gemm_split', ({'BSG_GEMM_H2W': '0'}, _check_gemm_split, False)),
    ('ring4', ({'BSG_H2W_TINY': '0', 'BSG_H2W_RING': '4', 'BSG_H2W_DEEP': '0', 'BSG_H2W_DIRECT': '0'}, _check_ring4, False)),
])


def test_fallback_forms_vs_fp64(tmp_path, fs2):
    """What a range-guard demotion, a weight that cannot be split or a switch lands on, each against float64 at the short list (the two
    sets that own a four-wave attention also at 64 x 20 x 500), with last_path showing that the switch took the launches it is meant to."""
    m, sd = fs2
    files = OrderedDict()
    for case in SHORT_LIST + [NW4]:
        f = str(tmp_path / _name(case).replace(' ', '_').replace('[', '').replace(']', '').replace(',', '-').replace(':', '-'))
        extra = {'rows': np.asarray(case[4])} if case[4] else {}
        np.savez(f + '.inp.npz', **_ref(sd, case)['inp'], **extra)
        files[case] = f
    seen = set()
    gold = load_golden('fs2_paths.json')['forms']
    for name, (env, check, with_nw4) in FORMS.items():
        cases = SHORT_LIST + ([NW4] if with_nw4 else [])
        res = subprocess.run([sys.executable, '-c', CHILD, name] + [files[c] for c in cases], env=dict(os.environ, **env), capture_output=True,
                             text=True, timeout=600)
        assert res.returncode == 0, (name, res.stderr[-2000:])
        info = json.loads(res.stdout.strip().splitlines()[-1])
        for case in cases:
            r = info[files[case]]
            z = np.load(f'{files[case]}.{name}.npz')
            assert r['retries'] == 0 and r['events'] == 0, (name, _name(case), r)
            assert r['path'] == gold[name][_name(case)], (name, _name(case), r['path'], gold[name][_name(case)])
            rec = _record(name, case, {k: z[k] for k in OUTS}, r['path'], _REF[case])
            check(case, rec['tokens'])
            seen |= set(rec['tokens'])
            _assert_parity(f'{name} {_name(case)}', rec, _REF[case])
    for tok in ('dec.attn:split/nw4', 'dec.attn:flash/nw4', 'dec.attn:softmax', 'dec.qkv:split_kernel', 'dec.attn:planes/ks8', 'esm:thread'):
        assert tok in seen, tok


# ------------------------------------------------------------------------------------------------------------------
# the FFT candidate denoiser (shares launch_fft)
# ------------------------------------------------------------------------------------------------------------------
DEN_SHAPES = [(1, 1), (2, 33), (2, 301), (2, 1000)]
_DEN = {}


@pytest.fixture(scope='module')
def den(sd_spec):
    from bisinger_amd.diffnet import DIFF_DECODERS
    from bisinger_amd.hparams import hparams
    use_config('diff_decoder_type=fft')
    net = DIFF_DECODERS[hparams['diff_decoder_type']](hparams)
    spec = OrderedDict((k, tuple(s)) for k, s in sd_spec['FFT'])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(spec, seed=17).items()}, strict=False)
    use_config()
    net = net.cuda()
    return net, cpu_sd(net)


def _den_inputs(B, T):
    rs = np.random.RandomState(300 * B + T)
    return (rs.standard_normal((B, 1, 80, T)).astype(np.float32), rs.randint(0, 100, size=(B,)).astype(np.int64),
            rs.standard_normal((B, 256, T)).astype(np.float32))


def _den_run(net, B, T):
    x, t, cond = (torch.from_numpy(a).cuda() for a in _den_inputs(B, T))
    before = _lib.range_retries
    eps = net(x, t, cond)
    path = net.last_path()
    assert _lib.range_retries == before and net.gemm_range_peek() == 0, 'a range event fired: last_path would name the repeat'
    return eps.cpu().numpy(), path


@pytest.mark.parametrize('B,T', DEN_SHAPES)
def test_fft_denoiser_vs_fp64(B, T, den):
    net, sd = den
    x, t, cond = (torch.from_numpy(a) for a in _den_inputs(B, T))
    want = ocd.fft_denoiser_forward(sd, x, t, cond, dtype=F64).numpy()
    w32 = ocd.fft_denoiser_forward(sd, x, t, cond, dtype=F32).double().numpy()
    got, path = _den_run(net, B, T)
    assert path == load_golden('fs2_paths.json')['den'][f'{B}x{T}'], (B, T, path)
    _DEN[(B, T)] = got
    assert got.shape == want.shape == (B, 1, 80, T) and np.isfinite(got).all()
    d = np.abs(got.astype(np.float64) - want)
    d32 = np.abs(w32 - want)
    edge = max(float(d[..., :EDGE].max()), float(d[..., -EDGE:].max()))
    per_row = [float(d[b].max()) for b in range(B)]
    wmax = float(np.abs(want).max())
    print(f'\nfft denoiser {B}x{T}: hip {d.max():.2e} edge {edge:.2e} rows {" ".join(f"{v:.1e}" for v in per_row)} | fp32 oracle {d32.max():.2e} | '
          f'hip / fp32 {d.max() / max(d32.max(), 1e-30):.2f} | max|want| {wmax:.2f} | {path}')
    bar = DEN_BAR * max(1.0, wmax)
    assert d.max() <= bar and edge <= bar and max(per_row) <= bar, (B, T, float(d.max()), bar, path)
    tok = path.split()
    assert tok and all(t.startswith('den.') for t in tok), path
    want_attn = {1: 'den.attn:split/nw2', 33: 'den.attn:planes/ks1', 301: 'den.attn:planes/ks2', 1000: 'den.attn:planes/ks4'}[T]
    assert want_attn in tok, (path, want_attn)


def test_fft_denoiser_stale_workspace(den):
    """(2, 301) after (2, 1000) on one handle, with and without NaN bytes in between: bit-identical to (2, 301) on a fresh handle."""
    net, sd = den
    net.release()
    fresh, path0 = _den_run(net, 2, 301)
    for poison in (True, False):
        net.release()
        long_, _ = _den_run(net, 2, 1000)
        assert np.isfinite(long_).all()
        if poison:
            net.poison_workspace()
        got, path = _den_run(net, 2, 301)
        assert np.isfinite(got).all() and path == path0, (poison, path)
        assert np.array_equal(got, fresh), (poison, float(np.abs(got.astype(np.float64) - fresh).max()), path)
