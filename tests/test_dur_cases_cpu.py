"""CPU: what tests/test_gpu_dur_shapes.py rests on, checked before any kernel runs (tests/dur_cases.py).

  * regulate_ref (numpy cumsum + searchsorted) is oracle.fs2.length_regulator: on the hand case of tests/golden/fs2.npz and on every content
    kind of dur_cases.reg_case at small shapes with T equal to the largest row sum (the only T the oracle has), with and without a token mask;
  * the regulator's cases hold what they are there for: every (kind, fit, mask form) at every T_txt, truncated rows, zero tails, an all-zero
    row, non-zero durations on masked tokens that change the result if they are not ignored;
  * dur_cases.predict is oracle.fs2.fs2_forward's (tests/fs2_pitch_ref.forward's for the plain front) predictor, bit for bit in both types;
  * the chosen inputs: under the tie rule at the set's own bound no case has more than 1 % of its valid tokens undecided, the cases the
    inputs were measured at (dur_cases.NO_TIES, MIDI front) have none, and both fronts together have at most two over all cases; the float32
    oracle's integer durations equal the float64 ones on every decided token (here: on every token); the raised weight set keeps the batch
    T within 2500 at the shapes it runs and exceeds it at the ones it skips; 1 x 1 predicts an empty utterance with the formula weights,
    4 x 257 is cut to [257, 256, 1, 130] valid tokens, 65 x 6 has a row of a single frame; the rank cases' rows differ in `lang`.

Measured here (err_fp32 = float32 oracle against float64, absolute; the bound is 4 x its largest; T of the batch):
  midi   seed0   err_fp32 4.7e-7 .. 4.4e-6  bound 1.75e-5  zero durations 33 .. 58 % (100 % at 1 x 1)  largest duration 40   T 0 .. 549
  midi   raised  err_fp32 4.9e-7 .. 4.5e-6  bound 1.79e-5  zero durations 0 .. 7 %                     largest duration 249  T 3 .. 2094
  plain  seed0   err_fp32 1.3e-9 .. 4.3e-6  bound 1.71e-5  zero durations up to 68 % (1 x 1, 1 x 2: all)                     T 0 .. 383
  plain  raised                             bound 1.73e-5                                                                    T 3 .. 2213
  (test_chosen_inputs prints every case; float32 sums depend on the host, the bounds move by some percent with it)
"""
import numpy as np
import pytest
import torch

from oracle import fs2 as ofs2
from tests import dur_cases as dc
from tests import fs2_pitch_ref as R

torch.set_grad_enabled(False)


def test_regulate_ref_is_the_oracles_length_regulator(gold):
    g = gold('fs2')
    name, dur, txt, T = dc.reg_special()[-1]
    assert name == 'hand case' and np.array_equal(dc.regulate_ref(dur, txt, T), g['lr.mel2ph'])
    assert dc.regulate_ref([[2, 2, 3]], None, 7).tolist() == [[1, 1, 2, 2, 3, 3, 3]]       # the reference's docstring example
    n = 0
    for B in (1, 3):
        for Tt in (1, 2, 255, 256, 257):
            for T in (1, 255, 257):
                for k, kind in enumerate(dc.REG_KINDS):
                    for masked in (False, True):
                        dur, txt, T_ = dc.reg_case(B, Tt, T, kind, 'equal', masked, seed=100 * Tt + 10 * B + k)
                        want = ofs2.length_regulator(torch.from_numpy(dur), None if txt is None else torch.from_numpy(txt == 0)).numpy()
                        assert want.shape == (B, T), 'T is the largest row sum'
                        assert np.array_equal(dc.regulate_ref(dur, txt, T), want), (B, Tt, T, kind, masked)
                        n += 1
    assert n == 300
    for name, dur, txt, T in dc.reg_special():          # where T happens to be the largest row sum the oracle applies as well
        d = dur if txt is None else dur * (txt != 0)
        if 0 < d.sum(1).max() == T:
            want = ofs2.length_regulator(torch.from_numpy(dur), None if txt is None else torch.from_numpy(txt == 0)).numpy()
            assert np.array_equal(dc.regulate_ref(dur, txt, T), want), name


@pytest.mark.parametrize('Tt', dc.REG_TT)
def test_regulator_cases_hold_their_edges(Tt):
    seen, shapes = set(), set()
    ignored_matters = zero_row = 0
    for name, dur, txt, T in dc.reg_cases(Tt):
        B = dur.shape[0]
        assert dur.shape == (B, Tt) and dur.dtype == np.int64 and (txt is None or txt.shape == (B, Tt))
        kind, fit, form = name.split()[1:]
        seen.add((kind, fit, form))
        shapes.add((B, T))
        want = dc.regulate_ref(dur, txt, T)
        top = (dur if txt is None else dur * (txt != 0)).sum(1).max()
        assert (fit == 'equal') == (top == T) and (fit == 'trunc') == (top > T) and (fit == 'tail') == (top < T), (name, top)
        if fit != 'tail':
            assert (want[0] > 0).all()
        if fit == 'tail':
            assert (want[:, -1] == 0).all()
        if kind in ('first', 'middle', 'last') and top:
            assert len(set(want[0][want[0] > 0].tolist())) == 1      # one token owns every frame of the row
        if kind == 'half' and Tt >= 255 and top >= Tt:
            z = (dur[0] == 0).mean()
            assert 0.3 < z < 0.7, (name, z)
        if txt is not None and Tt > 1 and B > 1:
            assert (dur[txt == 0] > 0).all()
            ignored_matters += int(not np.array_equal(want, dc.regulate_ref(dur, None, T)))
        zero_row += int(B > 1 and not want[1].any() and want[0].any() and want[2].any())
    assert seen == {(k, f, m) for k in dc.REG_KINDS for f in dc.REG_FITS for m in ('txt', 'NULL')}, 'a combination is missing'
    assert shapes == {(B, T) for B in dc.REG_B for T in dc.REG_T}
    assert Tt == 1 or ignored_matters >= 5, 'a scan that ignored txt would give the same result'
    assert zero_row >= 3, 'no all-zero row between non-empty rows'


def test_regulator_special_cases():
    sp = {name: (dur, txt, T) for name, dur, txt, T in dc.reg_special()}
    dur, txt, T = sp['2^31 in one token']
    want = dc.regulate_ref(dur, txt, T)
    assert want[0, :10].tolist() == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5] and (want[0, 10:] == 6).all() and dur[0, 5] > 2 ** 31
    dur, txt, T = sp['2^33 on a masked token']
    want = dc.regulate_ref(dur, txt, T)
    assert want[1, 6:8].tolist() == [5, 5] and want[1, -1] == 130 and not np.array_equal(want, dc.regulate_ref(dur, None, T))
    for k in ('empty middle row', 'middle row masked away'):
        dur, txt, T = sp[k]
        want = dc.regulate_ref(dur, txt, T)
        assert not want[1].any() and (want[0] > 0).all() and want[2, 191] == 254 and not want[2, 192:].any(), k
    assert not dc.regulate_ref(*sp['all rows empty']).any()


@pytest.mark.parametrize('front', dc.FRONTS)
def test_predict_is_the_oracles_predictor(front):
    """dur_cases.predict shares one encoder evaluation among the weight sets; its result is the oracle's own forward's, bit for bit."""
    for wset, case in (('seed0', dc.P(3, 31)), ('raised', dc.P(2, 33)), ('seed0', dc.P(8, 40, rows=slice(2, 5)))):
        hp, sd = dc.weights(front, wset)
        ti = dc.tensors(dc.inputs(case), drop=('mel2ph',))
        for dtype in (dc.F64, dc.F32):
            if front == 'midi':
                r = ofs2.fs2_forward(sd, ti, hp=hp, skip_decoder=True, dtype=dtype)
            else:
                r = R.forward(sd, ti, hp, dtype=dtype, skip_decoder=True)
            dur, xs = dc.predict(front, wset, case, dtype)
            rows = dc.rows_of(case)
            assert np.array_equal(xs, r['dur'][rows, :, 0].double().numpy()), (front, wset, dc.name(case), dtype)
            assert np.array_equal(dur, r['dur_choice'][rows].numpy())
            if dtype == dc.F64 and not case[4]:
                assert np.array_equal(dc.regulate_ref(dur, ti['txt_tokens'].numpy(), r['mel2ph'].shape[1]), r['mel2ph'].numpy())
                assert dc.batch_T(dur, ti['txt_tokens'].numpy()) == r['mel2ph'].shape[1]


@pytest.mark.parametrize('front', dc.FRONTS)
def test_chosen_inputs(front):
    n_loose = 0
    for wset in dc.WSETS:
        bd = dc.bound(front, wset)
        print(f'\n{front} {wset}: bound {bd:.3e} x max(1, max |want|)')
        assert 0 < bd < 4e-5, 'float32 rounding through four encoder layers and five predictor layers, nothing else'
        for case in dc.cases(front, wset) + [c for c in dc.NO_TIES if c not in dc.PRED]:
            ref = dc.reference(front, wset, case)
            tol = dc.allowed(front, wset, case)
            loose = dc.undecided(ref['xs'], ref['valid'], bd)
            T = dc.batch_T(ref['dur'], ref['txt'])
            nv = int(ref['valid'].sum())
            print(f'  {dc.name(case):32s} err_fp32 {ref["err32"]:.2e}  max |want| {ref["wmax"]:.2f}  allowed {tol:.2e}  valid {nv:5d}  zero '
                  f'{100.0 * float((ref["dur"][ref["valid"]] == 0).mean()):3.0f} %  max dur {int(ref["dur"].max()):3d}  T {T:5d}  undecided {int(loose.sum())}')
            assert int(loose.sum()) <= dc.UNDECIDED_CAP * nv
            if front == 'midi' and case in dc.NO_TIES:
                assert int(loose.sum()) == 0, 'no undecided token where the cases were measured: the tie rule excuses nothing there'
            n_loose += int(loose.sum())
            dc.check_dur(ref['dur32'], ref, bd, (front, wset, dc.name(case), 'the float32 oracle'))
            dc.check_xs(ref['xs32'].astype(np.float32), ref, tol, (front, wset, dc.name(case), 'the float32 oracle'))
            assert not ref['xs'][~ref['valid']].any() and not ref['dur'][~ref['valid']].any()
            if wset == 'raised' and not case[4]:
                assert 0 < T <= dc.MAX_RAISED_T, (dc.name(case), T)
            if wset == 'raised' and nv >= 30:
                assert int(ref['dur'].max()) >= 20, 'the raised bias stretches the durations'
            if wset == 'seed0' and nv >= 30:
                z = float((ref['dur'][ref['valid']] == 0).mean())      # (the plain front's raw predictions sit lower: up to 0.7)
                assert 0.3 <= z <= (0.6 if front == 'midi' else 0.8), 'about half the durations are 0'
    assert n_loose <= 2, 'undecided tokens over every case of the front (tests/dur_cases.py names them)'
    # the shapes the raised set skips are the ones whose batch T passes the limit: xs moves by the bias alone, to float64 accuracy
    for case in dc.RAISED_SKIP[front]:
        ref = dc.reference(front, 'seed0', case)
        xs = np.where(ref['valid'], ref['xs'] + dc.RAISE, 0.0)
        dur = np.maximum(np.rint(np.exp(xs) - 1.0), 0).astype(np.int64) * ref['valid']
        print(f'  raised at {dc.name(case)}: T {dc.batch_T(dur, ref["txt"])} (skipped)')
        assert dc.batch_T(dur, ref['txt']) > dc.MAX_RAISED_T
    # the empty utterance and the row of a single valid token
    ref = dc.reference(front, 'seed0', dc.EMPTY)
    assert ref['valid'].all() and not ref['dur'].any()
    ref = dc.reference(front, 'seed0', dc.CUT[0])
    assert ref['valid'].sum(1).tolist() == [257, 256, 1, 130]
    if front == 'midi':
        ref = dc.reference(front, 'seed0', dc.P(65, 6))
        assert 1 in (ref['dur'] * ref['valid']).sum(1).tolist(), 'a row of one frame'


def test_rank_rows_differ_in_lang():
    for case in dc.RANK:
        lang = dc.inputs(case)['lang']
        assert len({tuple(r) for r in lang.tolist()}) == lang.shape[0], 'the ESM sees every row: a wrong row must show'
