"""GPU parity of the predicted-duration path at its shape edges: the length regulator exactly against an integer reference, the duration
predictor of both fronts against the float64 evaluation of the CPU oracle, the whole forward with predicted durations, and a batch with an
empty row.  Cases, references, bounds and the tie rule: tests/dur_cases.py (held on the CPU by tests/test_dur_cases_cpu.py).

  1. The regulator alone (bsg_length_regulator, called directly).  T_txt in {1, 2, 255, 256, 257, 8192} x B in {1, 3, 65} x T in {1, 255, 256,
     257, 5000} x five contents (about half the durations 0; leading and trailing runs of zeros; the whole mass in the first, the middle,
     the last token), with T equal to, below and above the largest row sum and with a token mask (non-zero durations on padding and on a
     masked token inside the row) or NULL; an all-zero row between others, a duration above 2^31, the golden hand case.  array_equal with
     numpy cumsum + searchsorted; the output is pre-filled with -1 and 1024 guard words behind B T must keep it.  T_txt = 8193, T = 0,
     B = 0 and a null pointer are refused with the cause in bsg_last_error and nothing written.
  2. The predictor of both fronts (FastSpeech2MIDI.encode on bsg_fs2midi_encode / _encode_rows, FastSpeech2.encode on bsg_fs2_encode_plain)
     against float64 at 1 x 1 .. 1 x 3 (rows no longer than the taps), 3 x 31, 2 x 32, 2 x 33, 1 x 127 .. 1 x 129, 4 x 257 cut to [257, 256, 1,
     130] tokens, 2 x 481 cut to [481, 33], 16 x 100, 65 x 6 and the rank rows 2:5 of 8 x 40 and 8:16 of 64 x 20, with the formula weights
     and with dur_predictor.linear.bias + 1.8.  dur_xs: one bound per (front, weight set), 4 x the largest err_fp32 of the set (the float32
     oracle against the float64 one, computed on the CPU before the set's first kernel), x max(1, max |want|); padded tokens exactly 0.  dur:
     exact on every decided token, either neighbour on an undecided one (the tie rule of tests/dur_cases.py), at most 1 % undecided.  The
     short list runs again under the fp32-pipe and gemm_split switch sets (one child process each), and after a 16 x 100 call on a handle
     whose workspaces were filled with NaN bytes (bit-identical to a fresh handle).
  3. model(txt, None, ..., infer=True) on both fronts at 3 x 31, 2 x 100, 65 x 6 and rows 2:5 of 8 x 40 with the raised bias (T = 560, 1362,
     235, 622 on the MIDI front): mel2ph is exactly the integer reference of the call's own dur_choice with T the largest row sum;
     decoder_inp and mel_out within BAR of tests/test_gpu_fs2_shapes.py of the float64 oracle FED that mel2ph; frames beyond a row's length
     exactly 0.  1 x 1 with the formula weights raises BsgError and never enters the decoder.
  4. A batch whose middle row has every duration 0 (crafted in the encode's result), through regulate() and decode_all(): that row of
     decoder_inp and mel_out exactly 0 and finite, NO range event, the other rows within BAR of the float64 oracle evaluated on them —
     on the default path (planes attention on 4 and on 2 key splits) and under fp32_pipe, gemm_split, split_attn and softmax.

Measured on an MI355X (bounds from that host's CPU; kernel = largest |dur_xs - float64| / max(1, max |want|) over the set's cases, in
brackets the case and its absolute figure; the float32 oracle's own absolute figures are 4.7e-7 .. 4.4e-6):
  front  weights  bound      kernel                        undecided   fp32_pipe           gemm_split
  midi   seed0    1.68e-5    3.30e-6 (1 x 3, 3.73e-6)      0 of 15     4.03e-6 (1 x 3)     1.60e-6 (4 x 257)
  midi   raised   1.67e-5    1.32e-6 (1 x 128, 6.30e-6)    1 of 13     1.54e-6 (1 x 3)     8.51e-7 (2 x 33)
  plain  seed0    1.57e-5    2.47e-6 (2 x 32, 4.31e-6)     0 of 15     3.28e-6 (4 x 257)   2.61e-6 (4 x 257)
  plain  raised   1.37e-5    1.30e-6 (16 x 100, 6.34e-6)   0 of 14     1.58e-6 (2 x 33)    9.34e-7 (2 x 33)
  (undecided: tokens over the set's cases; the one is a token of 1 x 127, 3.8e-5 from the rounding boundary at exp(xs) = 6.5, and the kernel
  took the float64 integer there as everywhere else: dur differed from the float64 oracle's on no token of any case or form.  Stale
  workspace: bit-identical at both shapes on both fronts.)
  whole forward, |got - float64| (bar 3.4e-5 .. 4.2e-5): decoder_inp at most 1.95e-6, mel_out at most 2.60e-6 (both at 65 x 6)
  empty row: rows 0 and 2 at most 1.84e-6 / 2.81e-6 (fp32_pipe, plain), row 1 exactly 0, 0 range events on every form

What the file found.  With an empty row in the batch every attention kernel inverted a row sum of 0: O = 0 and l = 0 gave 0 x inf.  The
final select by mel2ph kept the NaN out of mel_out, but the split-fp16 forms count a non-finite operand as a range event (7699 of them at
3 x 31 on the default path), so a forward with one empty utterance was repeated on the fp32 matrix pipe and, after a few such calls, the
handle stayed there.  flash_attn_kernel, flash_attn_split_kernel, flash_attn_planes_kernel and masked_softmax_kernel now give a row
without keys 0 (csrc/fs2.hip: `l > 0 ? 1 / l : 0`); rows with keys compute what they computed.  bsg_length_regulator's one refusal message
was split so that it names the argument it refuses.  Nothing else deviated.
"""
import json
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from bisinger_amd import _lib
from tests import dur_cases as dc
from tests.test_gpu_fs2_shapes import BAR, FORMS, _gemm
from tests.util import ROOT

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

MIDI_KW = ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')
_MODELS = {}
_FIG = OrderedDict()      # (front, wset, case name) -> (largest |dur_xs - float64| / max(1, max |want|), undecided tokens)


def model(front, wset):
    if (front, wset) not in _MODELS:
        _MODELS[(front, wset)] = dc.build(front, wset)[0].cuda()
    return _MODELS[(front, wset)]


def dev(inp):
    return {k: torch.from_numpy(v).cuda() for k, v in inp.items()}


def call_kw(front, d):
    return {k: d[k] for k in MIDI_KW} if front == 'midi' else {}


def run_encode(m, front, case):
    """encode(predict_dur=True) of the rows of `case` -> dict(xs, dur, enc_out: numpy; path).  No range event, no retry."""
    d = dev(dc.inputs(case))
    before = _lib.range_retries
    enc = m.encode(d['txt_tokens'], d['spk_embed'] if front == 'midi' else None, predict_dur=True,
                   rows=slice(*case[4]) if case[4] else None, **call_kw(front, d))
    out = dict(xs=enc['dur_xs'].cpu().numpy(), dur=enc['dur'].cpu().numpy(), enc_out=enc['enc_out'].cpu().numpy(), path=m.last_path())
    assert _lib.range_retries == before and m.gemm_range_peek() == 0, 'a range event fired'
    return out


def check_predict(front, wset, case, got, tag):
    ref = dc.reference(front, wset, case)
    what = (tag, front, wset, dc.name(case))
    err = dc.check_xs(got['xs'], ref, dc.allowed(front, wset, case), what)
    loose = dc.check_dur(got['dur'], ref, dc.bound(front, wset), what)
    rel = err / max(1.0, ref['wmax'])
    print(f'\n{tag} {front} {wset} {dc.name(case)}: dur_xs {err:.2e} (fp32 oracle {ref["err32"]:.2e}, allowed {dc.allowed(front, wset, case):.2e}; '
          f'/ max(1, max |want|) {rel:.2e} of {dc.bound(front, wset):.2e}); undecided {loose} of {int(ref["valid"].sum())}; '
          f'dur != float64 on {int((got["dur"] != ref["dur"]).sum())}')
    return rel, loose


# ------------------------------------------------------------------------------------------------------------------
# 1. the regulator alone, exactly
# ------------------------------------------------------------------------------------------------------------------
def regulate(dur, txt, T, B=None, Tt=None, null_dur=False, null_out=False):
    """bsg_length_regulator on an output buffer pre-filled with -1 with GUARD words behind B T -> (rc, the whole buffer)."""
    b, tt = dur.shape
    B, Tt = b if B is None else B, tt if Tt is None else Tt
    out = torch.full((max(b, B, 1) * max(T, 1) + dc.GUARD,), -1, dtype=torch.long, device='cuda')
    d = torch.from_numpy(np.ascontiguousarray(dur)).cuda()
    t = None if txt is None else torch.from_numpy(np.ascontiguousarray(txt)).cuda()
    rc = _lib.load().bsg_length_regulator(_lib.ptr(None if null_dur else d), _lib.ptr(t), _lib.ptr(None if null_out else out), B, Tt, T,
                                          _lib.stream_ptr())
    return rc, out.cpu().numpy()


def check_regulator(name, dur, txt, T):
    B = dur.shape[0]
    rc, buf = regulate(dur, txt, T)
    assert rc == 0, (name, _lib.load().bsg_last_error())
    want = dc.regulate_ref(dur, txt, T)
    assert np.array_equal(buf[:B * T].reshape(B, T), want), (name, np.argwhere(buf[:B * T].reshape(B, T) != want)[:5].tolist())
    assert (buf[B * T:] == -1).all(), (name, 'words behind B T were written')


@pytest.mark.parametrize('Tt', dc.REG_TT)
def test_regulator_exact(Tt):
    """Every B of {1, 3, 65} x every T of {1, 255, 256, 257, 5000} x every content kind at this T_txt (75 launches), array_equal with the integer
    reference; the guard words behind B T keep their -1."""
    n = 0
    for name, dur, txt, T in dc.reg_cases(Tt):
        check_regulator(name, dur, txt, T)
        n += 1
    assert n == len(dc.REG_B) * len(dc.REG_T) * len(dc.REG_KINDS)


def test_regulator_special_cases():
    for name, dur, txt, T in dc.reg_special():
        check_regulator(name, dur, txt, T)


def test_regulator_refusals():
    """What bsg_length_regulator refuses: bsg_last_error names the cause, nothing is written."""
    lib = _lib.load()
    dur = np.ones((2, 8193), np.int64)
    for kw, cause in ((dict(T=7), 'T_txt=8193'), (dict(T=0, Tt=4), 'T=0'), (dict(T=7, B=0, Tt=4), 'B=0'), (dict(T=7, Tt=4, null_dur=True), 'null dur'),
                      (dict(T=7, Tt=4, null_out=True), 'null mel2ph')):
        rc, buf = regulate(dur, None, **kw)
        msg = lib.bsg_last_error().decode()
        assert rc != 0 and 'length_regulator' in msg and cause in msg, (kw, rc, msg)
        assert (buf == -1).all(), (kw, 'the output was written')
    rc, buf = regulate(dur[:, :8192], None, 7)      # the limit itself is accepted
    assert rc == 0 and buf[:14].tolist() == [1, 2, 3, 4, 5, 6, 7] * 2 and (buf[14:] == -1).all()


# ------------------------------------------------------------------------------------------------------------------
# 2. the predictor against float64
# ------------------------------------------------------------------------------------------------------------------
PREDICT = [(f, w, c) for f in dc.FRONTS for w in dc.WSETS for c in dc.cases(f, w)]


@pytest.mark.parametrize('front,wset,case', PREDICT, ids=lambda v: dc.name(v).replace(' ', '') if isinstance(v, tuple) else v)
def test_predictor_vs_fp64(front, wset, case):
    dc.bound(front, wset)        # on the CPU, before any kernel of the set runs
    got = run_encode(model(front, wset), front, case)
    B, Tt, T, lens, rows = case
    nb = rows[1] - rows[0] if rows else B
    assert got['xs'].shape == got['dur'].shape == (nb, Tt)
    tok = got['path'].split()
    assert ('esm:wave' in tok or 'esm:thread' in tok) == (front == 'midi') and ('tok:front' in tok) == (front == 'plain'), got['path']
    _FIG[(front, wset, dc.name(case))] = check_predict(front, wset, case, got, 'default')


def test_predictor_figures():
    """The largest figure per (front, weight set) beside its bound (module docstring); cases the parametrised test has not run are run here."""
    for front, wset, case in PREDICT:
        if (front, wset, dc.name(case)) not in _FIG:
            _FIG[(front, wset, dc.name(case))] = check_predict(front, wset, case, run_encode(model(front, wset), front, case), 'default')
    for front in dc.FRONTS:
        for wset in dc.WSETS:
            fig = {k[2]: v for k, v in _FIG.items() if k[:2] == (front, wset)}
            worst = max(fig, key=lambda k: fig[k][0])
            print(f'\n{front} {wset}: bound {dc.bound(front, wset):.3e} x max(1, max |want|); kernel {fig[worst][0]:.3e} ({worst}); undecided '
                  f'{sum(v[1] for v in fig.values())} over {len(fig)} cases')
            assert fig[worst][0] <= dc.bound(front, wset)


@pytest.mark.parametrize('front', dc.FRONTS)
def test_stale_workspace_never_reaches_a_duration(front):
    """1 x 3 and 2 x 33 after 16 x 100 on one handle, with NaN bytes over every activation workspace in between
    (bsg_fs2midi_debug_poison_workspace): bit-identical to the same call on a fresh handle."""
    m = dc.build(front, 'seed0')[0].cuda()
    fresh = {}
    for case in dc.STALE_THEN:
        m.release()
        fresh[case] = run_encode(m, front, case)
    m.release()
    long_ = run_encode(m, front, dc.STALE_FIRST)
    assert np.isfinite(long_['xs']).all()
    m.poison_workspace()
    for case in dc.STALE_THEN:
        got = run_encode(m, front, case)
        for k in ('xs', 'dur', 'enc_out'):
            assert np.array_equal(got[k], fresh[case][k]), (front, dc.name(case), k)
        assert got['path'] == fresh[case]['path']
        check_predict(front, 'seed0', case, got, 'stale')
    m.release()


# ------------------------------------------------------------------------------------------------------------------
# 3. the whole forward with predicted durations
# ------------------------------------------------------------------------------------------------------------------
def check_frames(got, want, n_frames, tag):
    """decoder_inp / mel_out within BAR of the float64 oracle fed the same mel2ph; frames beyond a row's own length exactly 0."""
    for k in ('decoder_inp', 'mel_out'):
        g = np.asarray(got[k])
        assert g.shape == want[k].shape and np.isfinite(g).all(), (tag, k, g.shape, want[k].shape)
        err = float(np.abs(g.astype(np.float64) - want[k]).max())
        bar = BAR[k] * max(1.0, float(np.abs(want[k]).max()))
        print(f'    {tag} {k}: {err:.2e} (bar {bar:.2e}, max |want| {np.abs(want[k]).max():.2f})')
        assert err <= bar, (tag, k, err, bar)
        for b, n in enumerate(n_frames):
            assert not g[b, int(n):].any(), (tag, k, 'row', b, 'has a non-zero frame beyond its length', int(n))


@pytest.mark.parametrize('front', dc.FRONTS)
@pytest.mark.parametrize('case', dc.FORWARD, ids=lambda c: dc.name(c).replace(' ', ''))
def test_forward_with_predicted_durations(front, case):
    m = model(front, 'raised')
    inp = dc.inputs(case)
    d = dev(inp)
    rows = dc.rows_of(case)
    before = _lib.range_retries
    ret = m(d['txt_tokens'], None, d['spk_embed'] if front == 'midi' else None, infer=True, rows=slice(*case[4]) if case[4] else None,
            **call_kw(front, d))
    assert _lib.range_retries == before and m.gemm_range_peek() == 0, 'a range event fired'
    dur = ret['dur_choice'].cpu().numpy()          # the whole batch's: T is the maximum over every row
    txt = inp['txt_tokens']
    assert dur.shape == txt.shape and dur.dtype == np.int64
    T = dc.batch_T(dur, txt)
    want_m2p = dc.regulate_ref(dur, txt, T)
    got_m2p = ret['mel2ph'].cpu().numpy()
    assert got_m2p.shape == want_m2p[rows].shape and np.array_equal(got_m2p, want_m2p[rows]), 'mel2ph is not the regulator of the call\'s own durations'
    ref = dc.reference(front, 'raised', case)
    dc.check_xs(ret['dur'][rows, :, 0].cpu().numpy(), ref, dc.allowed(front, 'raised', case), (front, dc.name(case)))
    dc.check_dur(dur[rows], ref, dc.bound(front, 'raised'), (front, dc.name(case)))
    n_frames = (want_m2p[rows] > 0).sum(1)
    print(f'\nforward {front} {dc.name(case)}: T {T}, frames per row {n_frames.min()} .. {n_frames.max()}')
    assert n_frames.max() == T or case[4]
    want = dc.forward_fed(front, 'raised', case, want_m2p)
    check_frames({k: ret[k].cpu().numpy() for k in ('decoder_inp', 'mel_out')}, want, n_frames, f'{front} {dc.name(case)}')


@pytest.mark.parametrize('front', dc.FRONTS)
def test_empty_utterance_raises_and_decodes_nothing(front):
    """1 x 1 with the formula weights: the only duration rounds to 0; regulate() raises and the decoder is never entered."""
    m = model(front, 'seed0')
    d = dev(dc.inputs(dc.EMPTY))
    with pytest.raises(_lib.BsgError, match='empty utterance'):
        m(d['txt_tokens'], None, d['spk_embed'] if front == 'midi' else None, infer=True, **call_kw(front, d))
    tok = m.last_path().split()
    assert tok and not [t for t in tok if t.startswith('dec.')], tok


# ------------------------------------------------------------------------------------------------------------------
# 4. an empty row among others
# ------------------------------------------------------------------------------------------------------------------
EMPTY_ROW = dc.P(3, 31)
_EMPTY_REF = {}


def run_empty_row(m, front):
    """3 x 31 (raised bias) with the durations of row 1 set to 0 in the encode's result: regulate(), then decode_all() -> numpy dict."""
    d = dev(dc.inputs(EMPTY_ROW))
    enc = m.encode(d['txt_tokens'], d['spk_embed'] if front == 'midi' else None, predict_dur=True, **call_kw(front, d))
    enc['dur'] = enc['dur'].clone()
    enc['dur'][1] = 0
    mel2ph = m.regulate(enc)
    m.gemm_range_take()
    r = m.decode_all(enc['enc_out'], mel2ph, enc['spk'], d['speechsing'] if front == 'midi' else None)
    return dict(dur=enc['dur'].cpu().numpy(), mel2ph=mel2ph.cpu().numpy(), decoder_inp=r['decoder_inp'].cpu().numpy(), mel_out=r['mel_out'].cpu().numpy(),
                events=np.asarray(m.gemm_range_take()), path=np.asarray(m.last_path()))


def check_empty_row(front, got, tag):
    """Row 1 exactly 0 and finite, no range event (0 x inf in the attention's normalisation would raise one and send the call to the fp32
    pipe); rows 0 and 2 within BAR of the float64 oracle evaluated on THEM (the oracle's own value for a row without keys is no yardstick)."""
    txt = dc.inputs(EMPTY_ROW)['txt_tokens']
    want_m2p = dc.regulate_ref(got['dur'], txt, dc.batch_T(got['dur'], txt))
    assert np.array_equal(got['mel2ph'], want_m2p) and not want_m2p[1].any() and want_m2p[0].any() and want_m2p[2].any()
    for k in ('decoder_inp', 'mel_out'):
        assert np.isfinite(got[k]).all(), (tag, k, 'a non-finite value left the call')
        assert not got[k][1].any(), (tag, k, 'the empty row is not exactly 0')
    assert int(got['events']) == 0, (tag, 'range events', int(got['events']), str(got['path']))
    key = (front, got['mel2ph'].tobytes())
    if key not in _EMPTY_REF:
        _EMPTY_REF[key] = {b: dc.forward_fed(front, 'raised', dc.P(3, 31, rows=slice(b, b + 1)), want_m2p) for b in (0, 2)}
    for b in (0, 2):
        check_frames({k: got[k][b:b + 1] for k in ('decoder_inp', 'mel_out')}, _EMPTY_REF[key][b], (want_m2p[b:b + 1] > 0).sum(1), f'{tag} row {b}')


@pytest.mark.parametrize('front', dc.FRONTS)
def test_empty_row_among_others(front):
    got = run_empty_row(model(front, 'raised'), front)
    print(f'\nempty row {front}: T {got["mel2ph"].shape[1]}; {got["path"]}')
    check_empty_row(front, got, f'default {front}')


# ------------------------------------------------------------------------------------------------------------------
# the fallback forms, one child process per switch set
# ------------------------------------------------------------------------------------------------------------------
CHILD = r'''
import sys, json, torch, numpy as np
sys.path.insert(0, %r)
from tests import test_gpu_dur_shapes as S
from tests import dur_cases as dc
torch.set_grad_enabled(False)
out, fronts, with_predict = sys.argv[1], sys.argv[2].split(','), sys.argv[3] == '1'
paths = {}
for front in fronts:
    if with_predict:
        for wset, i in S.FALLBACK_JOBS:
            got = S.run_encode(S.model(front, wset), front, dc.FALLBACK_LIST[i])
            paths[f'{front}.{wset}.{i}'] = got.pop('path')
            np.savez(f'{out}.{front}.{wset}.{i}.npz', **got)
    np.savez(f'{out}.{front}.empty.npz', **S.run_empty_row(S.model(front, 'raised'), front))
print(json.dumps(paths))
''' % ROOT

FALLBACK_JOBS = [('seed0', 0), ('seed0', 1), ('seed0', 2), ('raised', 0), ('raised', 1)]      # (weight set, index into dc.FALLBACK_LIST)


def _is_fp32(tok):
    g = _gemm(tok)
    return bool(g) and all(x.startswith(('gemm_fast', 'gemm_f32')) for x in g)


def _is_gemm_split(tok):
    g = _gemm(tok)
    return bool(g) and all(x.startswith('gemm_split') for x in g)


# (switch set of tests/test_gpu_fs2_shapes.FORMS, fronts, the predictor's short list too?, what the launch record must show)
DUR_FORMS = OrderedDict([
    ('fp32_pipe', (('midi', 'plain'), True, _is_fp32)),
    ('gemm_split', (('midi', 'plain'), True, _is_gemm_split)),
    # the empty row alone, on the attention forms the two sets above do not reach: flash_attn_split_kernel and the score tensor
    ('split_attn', (('midi',), False, lambda tok: any(t.startswith('dec.attn:split/') for t in tok))),
    ('softmax', (('midi',), False, lambda tok: 'dec.attn:softmax' in tok)),
])


@pytest.mark.parametrize('form', list(DUR_FORMS))
def test_fallback_forms(form, tmp_path):
    """The predictor's short list (1 x 3, 2 x 33, 4 x 257 cut; the first two also with the raised bias) and the empty-row batch under the
    fp32-pipe and gemm_split switch sets, the empty-row batch also under split_attn and softmax: the same checks as on the default path."""
    fronts, with_predict, shows = DUR_FORMS[form]
    for front in fronts:          # the bounds, on the CPU, before the child's kernels run
        for wset in dc.WSETS:
            dc.bound(front, wset)
    out = str(tmp_path / form)
    res = subprocess.run([sys.executable, '-c', CHILD, out, ','.join(fronts), '1' if with_predict else '0'], env=dict(os.environ, **FORMS[form][0]),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (form, res.stderr[-2000:])
    paths = json.loads(res.stdout.strip().splitlines()[-1])
    for front in fronts:
        if with_predict:
            for wset, i in FALLBACK_JOBS:
                z = np.load(f'{out}.{front}.{wset}.{i}.npz')
                assert shows(paths[f'{front}.{wset}.{i}'].split()), (form, paths[f'{front}.{wset}.{i}'])
                check_predict(front, wset, dc.FALLBACK_LIST[i], {k: z[k] for k in z.files}, form)
        z = np.load(f'{out}.{front}.empty.npz')
        got = {k: z[k] for k in z.files}
        assert shows(str(got['path']).split()), (form, str(got['path']))
        check_empty_row(front, got, f'{form} {front}')
