"""Cases, references and bounds of the predicted-duration path: what tests/test_dur_cases_cpu.py (CPU) and tests/test_gpu_dur_shapes.py (GPU)
share.  The chain under test (csrc/fs2.hip: dur_predict, bsg_length_regulator, the three encode entry points):

  add_spk_kernel -> 5 x (3-tap convolution as a tapped GEMM with bias + ReLU -> LayerNorm(eps 1e-12) with the keep mask) -> Linear(256 -> 1)
  with the keep mask -> dur_from_log_kernel -> host sync (regulate) -> length_regulator_kernel

The regulator alone.  regulate_ref is the integer reference (numpy cumsum + searchsorted, int64; pinned to oracle.fs2.length_regulator by the
CPU test).  reg_cases(Tt) yields, for one T_txt of REG_TT, every B of REG_B x every T of REG_T x every content of REG_KINDS; how T relates to the
largest row sum (equal / truncating / zero tail) and whether a token mask is passed (a ragged one with non-zero durations on its padding and on
one masked token INSIDE the row, or NULL) cycle over the cases so that every kind meets every relation and both mask forms at every T_txt.
reg_special() holds what no cycle produces: a duration above 2^31, an all-zero row between two others, a batch of all-zero rows.

The predictor.  PRED (B x T_txt, optional token counts per row) and RANK (rows of a larger batch) are the shapes; inputs are
synth.synth_inputs(B, T_txt, 4 T_txt, seed=5, ragged=B > 2) (cut rows: the rule of tests/test_gpu_fs2_shapes._cut).  Two fronts: 'midi'
(FastSpeech2MIDI, speaker table: add_spk_kernel adds a row) and 'plain' (FastSpeech2 without speaker: add_spk_kernel only masks; built here
with the same 5-layer predictor).  Two weight sets: 'seed0' (the formula weights, about half the durations 0) and 'raised'
(dur_predictor.linear.bias + 1.8 in float32: durations up to about 50 frames), the latter only where the batch T stays <= 2500 (RAISED_SKIP, per front).
The float64 and the float32 evaluation of the CPU oracle share one encoder evaluation per (front, case, dtype); the predictor itself is
oracle.fs2.duration_predictor on (enc + spk) * keep, the two lines oracle.fs2.fs2_forward has in front of it (the CPU test holds the result to
fs2_forward's own, bit for bit).

Bound of dur_xs: one number per (front, weight set), 4 x the largest err_fp32 over that set's cases (err_fp32 = max-abs of the float32 oracle
against the float64 one), x max(1, max |want|) of the case: bound().

Tie rule of dur: with v = exp(xs64) - 1, a valid token is DECIDED when |v - floor(v) - 1/2| > bound exp(xs64) + 4 ulp32(exp(xs64)), or when
both neighbouring integers clamp to the same duration (v < 0: round(v) is 0 or -1, and clamp(min=0) makes both 0).  `bound` is the set's
number itself, WITHOUT the factor max(1, max |want|) of the dur_xs tolerance: an error of it in xs moves exp(xs) by bound x exp(xs), the
float32 exp and the subtraction add a few ulp.  (That is the reading under which the formula inputs behave as measured when the cases were
chosen — no undecided token at 3 x 31, 2 x 33, 2 x 100, 16 x 100, 65 x 6, 4 x 257 and 2 x 481 on the MIDI front with either weight set — and
it is the stricter one: with the factor, about 5, one token of the 84 of 3 x 31 would be excused, more than the cap.)  A decided token
must carry the float64 integer; an undecided one may carry either neighbour; at most UNDECIDED_CAP of a case's valid tokens may be
undecided.  Over all cases of both fronts two tokens are: one of 1 x 127 (MIDI, raised; 3.8e-5 from the boundary at exp(xs) = 6.5) and
one of 16 x 100 (plain, seed0; 4.3e-5 at 2.5, within a few percent of the margin: it may count as decided on another host).
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

from bisinger_amd import synth
from oracle import fs2 as ofs2
from tests import fs2_pitch_ref as R
from tests.test_gpu_fs2_shapes import C, _cut, _row_groups

F64, F32 = torch.float64, torch.float32
FRONTS = ('midi', 'plain')
WSETS = ('seed0', 'raised')
RAISE = 1.8
MAX_RAISED_T = 2500
UNDECIDED_CAP = 0.01

# ------------------------------------------------------------------------------------------------------------------
# the regulator alone
# ------------------------------------------------------------------------------------------------------------------
REG_TT = (1, 2, 255, 256, 257, 8192)      # 8192: the accepted limit, 64 KiB of dynamic LDS
REG_B = (1, 3, 65)
REG_T = (1, 255, 256, 257, 5000)          # 256 threads stride over T
REG_KINDS = ('half', 'runs', 'first', 'middle', 'last')
REG_FITS = ('equal', 'trunc', 'tail')
GUARD = 1024                              # int64 words behind B T that no launch may touch


def regulate_ref(dur, txt, T):
    """mel2ph [B,T] int64: frame j of row b belongs to the first token i with cumsum(dur)[i] > j (1-based), 0 beyond the row's sum; durations
    of tokens whose txt is 0 are ignored (txt None: nothing is)."""
    dur = np.asarray(dur, np.int64)
    if txt is not None:
        dur = np.where(np.asarray(txt) != 0, dur, 0)
    B, Tt = dur.shape
    cum = np.cumsum(dur, axis=1, dtype=np.int64)
    out = np.zeros((B, T), np.int64)
    frames = np.arange(T, dtype=np.int64)
    for b in range(B):
        i = np.searchsorted(cum[b], frames, side='right')
        out[b] = np.where(i < Tt, i + 1, 0)
    return out


def _spread(rs, n, total):
    """`total` frames over n tokens, every token at least 1 when total >= n."""
    if n == 0 or total == 0:
        return np.zeros(n, np.int64)
    if total < n:
        d = np.zeros(n, np.int64)
        d[rs.choice(n, size=total, replace=False)] = 1
        return d
    return 1 + rs.multinomial(total - n, np.full(n, 1.0 / n)).astype(np.int64)


def _row(rs, n, total, kind):
    """Durations of n valid tokens that sum to `total`."""
    d = np.zeros(n, np.int64)
    if n == 0:
        return d
    if kind == 'half':          # about half the tokens 0, scattered
        sel = np.flatnonzero(rs.uniform(size=n) < 0.5)
        sel = sel if len(sel) else np.array([rs.randint(n)])
        d[sel] = _spread(rs, len(sel), total)
    elif kind == 'runs':        # a leading and a trailing run of zeros
        a, b = n // 3, max(n // 3 + 1, n - n // 3)
        d[a:b] = _spread(rs, b - a, total)
    else:                       # the whole mass in one token
        d[{'first': 0, 'middle': n // 2, 'last': n - 1}[kind]] = total
    assert d.sum() == total, (kind, n, total, int(d.sum()))
    return d


def reg_case(B, Tt, T, kind, fit, masked, seed):
    """(dur [B,Tt], txt [B,Tt] or None, T).  Row 0 carries the largest row sum: T ('equal'), T + 1 + T // 3 ('trunc': the rows are cut) or
    T - 1 - T // 4 ('tail': every row ends in zeros); the other rows' sums are drawn up to it, row 1 of a batch of 65 is all zero."""
    rs = np.random.RandomState(seed)
    top = {'equal': T, 'trunc': T + 1 + T // 3, 'tail': max(0, T - 1 - T // 4)}[fit]
    dur = np.zeros((B, Tt), np.int64)
    txt = None
    if masked:
        txt = rs.randint(3, 65, size=(B, Tt)).astype(np.int64)
    for b in range(B):
        # valid tokens: row 0 all; under a mask every other row ends in at least one padded token (T_txt = 1: the odd rows are masked away)
        n = Tt if (b == 0 or not masked) else max(1 - b % 2, Tt - 1 - (b * 3) % max(1, Tt // 2))
        total = top if b == 0 else (0 if (B == 65 and b == 1) or n == 0 else int(rs.randint(0, top + 1)))
        inside = masked and n >= 4       # one masked token INSIDE the valid part: its duration is ignored too
        hole = n // 2 - 1 if inside else -1      # (never the token 'middle' puts its mass on)
        cols = np.array([j for j in range(n) if j != hole], np.int64)
        dur[b, cols] = _row(rs, len(cols), total, kind)
        if masked:
            txt[b, n:] = 0
            dur[b, n:] = rs.randint(1, 9, size=Tt - n)      # non-zero durations on padding
            if inside:
                txt[b, hole] = 0
                dur[b, hole] = 5
    return dur, txt, T


def reg_cases(Tt):
    """Every (B, T) of REG_B x REG_T with every content kind; fit and mask form cycle (5 kinds, 3 fits, 2 mask forms over 75 cases: each
    (kind, fit, mask) combination three times, on different (B, T))."""
    i = 0
    for B, T in itertools.product(REG_B, REG_T):
        for k, kind in enumerate(REG_KINDS):
            fit = REG_FITS[(i + k) % 3]
            masked = bool(((i + k) // 3) % 2)
            yield (f'{B}x{Tt}x{T} {kind} {fit} {"txt" if masked else "NULL"}',) + reg_case(B, Tt, T, kind, fit, masked, seed=7919 * Tt + 31 * i + k)
        i += 1


def reg_special():
    """(name, dur, txt, T) of the cases no cycle produces."""
    out = []
    # one duration above 2^31 (the running sum is 64-bit): token 5 swallows every frame behind the first five tokens' 10
    dur = np.full((1, 257), 3, np.int64)
    dur[0, :5] = 2
    dur[0, 5] = (1 << 31) + 7
    out.append(('2^31 in one token', dur, None, 5000))
    # ... and on a masked token, where it must be ignored (the sum would otherwise pass every frame)
    dur = np.full((3, 256), 2, np.int64)
    txt = np.full((3, 256), 9, np.int64)
    dur[1, 3] = (1 << 33) + 1
    txt[1, 3] = 0
    out.append(('2^33 on a masked token', dur, txt, 257))
    # an all-zero row between two others: its mel2ph is all 0
    dur = np.zeros((3, 257), np.int64)
    dur[0, ::2] = 2
    dur[2, 1::4] = 3      # 64 tokens: 192 frames, then a zero tail
    out.append(('empty middle row', dur, None, 258))
    txt = np.full((3, 257), 4, np.int64)
    dur2 = dur.copy()
    dur2[1] = 7
    txt[1] = 0      # the row is empty BECAUSE every token of it is masked
    out.append(('middle row masked away', dur2, txt, 258))
    out.append(('all rows empty', np.zeros((3, 2), np.int64), None, 255))
    # the hand case of tests/golden/fs2.npz (lr.mel2ph)
    out.append(('hand case', np.array([[2, 2, 3, 0], [1, 0, 4, 2]], np.int64), np.array([[5, 6, 7, 0], [5, 6, 7, 8]], np.int64), 7))
    return out


# ------------------------------------------------------------------------------------------------------------------
# the predictor
# ------------------------------------------------------------------------------------------------------------------
def P(B, Tt, lens=None, rows=None):
    return C(B, Tt, 4 * Tt, lens, rows)


TAPS = [P(1, 1), P(1, 2), P(1, 3)]                                   # rows no longer than the 3 taps
BLOCK = [P(3, 31), P(2, 32), P(2, 33), P(1, 127), P(1, 128), P(1, 129)]
CUT = [P(4, 257, [257, 256, 1, 130]), P(2, 481, [481, 33])]          # padding next to the last valid token; a row of ONE valid token
MANY = [P(16, 100), P(65, 6)]                                        # the bench shape; more than 64 utterances
RANK = [P(8, 40, rows=slice(2, 5)), P(64, 20, rows=slice(8, 16))]    # bsg_fs2midi_encode_rows (the plain front: rows that simply run)
PRED = TAPS + BLOCK + CUT + MANY + RANK
RAISED_SKIP = {'midi': tuple(CUT), 'plain': (CUT[1],)}               # batch T above MAX_RAISED_T with the raised bias (MIDI: 2976 and 5295; plain: 4067)
FALLBACK_LIST = [P(1, 3), P(2, 33), P(4, 257, [257, 256, 1, 130])]
STALE_FIRST = P(16, 100)
STALE_THEN = [P(1, 3), P(2, 33)]
FORWARD = [P(3, 31), P(2, 100), P(65, 6), P(8, 40, rows=slice(2, 5))]   # the whole forward with predicted durations, raised bias
NO_TIES = [P(3, 31), P(2, 33), P(2, 100), P(16, 100), P(65, 6)] + CUT   # MIDI front: no undecided token (module docstring)
EMPTY = P(1, 1)                                                      # seed0: every duration rounds to 0


def name(case):
    B, Tt, T, lens, rows = case
    return f'{B}x{Tt}' + (f' lens {list(lens)}' if lens else '') + (f' rows {rows[0]}:{rows[1]}' if rows else '')


def cases(front, wset):
    return [c for c in PRED if not (wset == 'raised' and c in RAISED_SKIP[front])]


def inputs(case):
    B, Tt, T, lens, rows = case
    if lens:
        return _cut(synth.synth_inputs(B, Tt, T, seed=5), lens)
    return synth.synth_inputs(B, Tt, T, seed=5, ragged=B > 2)


def rows_of(case):
    return slice(*case[4]) if case[4] else slice(None)


def build(front, wset='seed0'):
    """A fresh drop-in on the CPU (formula weights of seed 0; 'raised': dur_predictor.linear.bias + 1.8, added in float32) and the
    hyper-parameters the restatement of tests/fs2_pitch_ref.py reads.  'plain': the PopCS chain of that file without pitch adaptor and
    speaker, with the 5-layer duration predictor of the chain under test."""
    from bisinger_amd.fs2 import FastSpeech2, FastSpeech2MIDI
    from bisinger_amd.hparams import hparams
    from tests.util import cpu_sd, load_formula_weights, use_config
    use_config()
    if front == 'plain':
        hparams.update(R.POPCS_HP)
        hparams.update(use_pitch_embed=False, dur_predictor_layers=5, dur_predictor_kernel=3)
    hp = dict(hidden_size=256, enc_layers=hparams['enc_layers'], dec_layers=hparams['dec_layers'], num_heads=hparams['num_heads'],
              enc_ffn_kernel_size=hparams['enc_ffn_kernel_size'], dec_ffn_kernel_size=hparams['dec_ffn_kernel_size'],
              dur_predictor_layers=hparams['dur_predictor_layers'], dur_predictor_kernel=hparams['dur_predictor_kernel'],
              use_midi=front == 'midi', use_spk_id=bool(hparams['use_spk_id']), use_pitch_embed=False)
    assert hp['dur_predictor_layers'] == 5 and hp['dur_predictor_kernel'] == 3
    m = (FastSpeech2MIDI if front == 'midi' else FastSpeech2)(R.PhoneEncoder(), 80)
    load_formula_weights(m, 0, prefix='fs2.')
    if wset == 'raised':
        with torch.no_grad():
            m.dur_predictor.linear.bias += RAISE
    use_config()      # the module keeps what it read; the global table goes back to the shipped configuration
    return m, hp, cpu_sd(m, 'fs2.')


_SD = {}       # (front, wset) -> (hp, sd)
_ENC = {}      # (front, case, dtype) -> (dur_inp [nb,Tt,H], txt [nb,Tt])
_REF = {}      # (front, wset, case) -> reference record


def weights(front, wset):
    if (front, wset) not in _SD:
        _SD[(front, wset)] = build(front, wset)[1:]
    return _SD[(front, wset)]


def tensors(inp, drop=()):
    return {k: torch.from_numpy(v) for k, v in inp.items() if k not in drop}


def dur_input(front, case, dtype):
    """(enc + spk) * keep of the WHOLE batch of `case` and its tokens: the predictor's input (fs2_forward's dur_inp; the encoder does not
    depend on the weight set).  A rank case is evaluated as the reference evaluates it, on every row, and sliced afterwards."""
    key = (front, case[:4], dtype)
    if key not in _ENC:
        hp, sd = weights(front, 'seed0')
        ti = tensors(inputs(case))
        txt = ti['txt_tokens']
        if front == 'midi':
            enc = ofs2.fs2_forward(sd, ti, hp=hp, skip_decoder=True, dtype=dtype)['enc_out']
            enc = enc + F.embedding(ti['spk_embed'], sd['fs2.spk_embed_proj.weight'].to(dtype))[:, None, :]
        else:
            enc = R.plain_encoder(sd, 'fs2.', txt, {**ofs2.DEFAULT_HP, **hp}, dtype)
        _ENC[key] = (enc * (txt > 0).to(dtype)[:, :, None], txt)
    return _ENC[key]


def predict(front, wset, case, dtype):
    """-> (dur int64 [nb,Tt], xs float64 [nb,Tt]) of the rows of `case`, as numpy."""
    hp, sd = weights(front, wset)
    x, txt = dur_input(front, case, dtype)
    dur, xs = ofs2.duration_predictor(sd, 'fs2.dur_predictor.', x, txt == 0, hp['dur_predictor_layers'], hp['dur_predictor_kernel'], dtype)
    rows = rows_of(case)
    return dur[rows].numpy(), xs[rows, :, 0].double().numpy()


def reference(front, wset, case):
    """The float64 reference of a case with the float32 oracle's deviation from it: dict(txt, valid, xs, dur, xs32, dur32, err32, wmax)."""
    key = (front, wset, case)
    if key not in _REF:
        dur, xs = predict(front, wset, case, F64)
        dur32, xs32 = predict(front, wset, case, F32)
        txt = dur_input(front, case, F64)[1][rows_of(case)].numpy()
        _REF[key] = dict(txt=txt, valid=txt > 0, xs=xs, dur=dur, xs32=xs32, dur32=dur32, err32=float(np.abs(xs32 - xs).max()),
                         wmax=float(np.abs(xs).max()))
    return _REF[key]


def bound(front, wset):
    """4 x the largest err_fp32 over the set's cases (x max(1, max |want|) of the case where it is applied).  On the CPU, before any kernel of
    the set runs."""
    return 4.0 * max(reference(front, wset, c)['err32'] for c in cases(front, wset))


def allowed(front, wset, case):
    return bound(front, wset) * max(1.0, reference(front, wset, case)['wmax'])


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def neighbours(xs64):
    """(lo, hi): the two durations round(exp(xs) - 1) can fall on, after the clamp at 0."""
    fl = np.floor(np.exp(xs64) - 1.0)
    return np.maximum(fl, 0).astype(np.int64), np.maximum(fl + 1, 0).astype(np.int64)


def undecided(xs64, valid, tol):
    """Boolean [nb,Tt]: valid tokens whose integer duration an error of `tol` (bound(front, wset)) in xs may flip (module docstring)."""
    e = np.exp(xs64)
    v = e - 1.0
    near = np.abs(v - np.floor(v) - 0.5) <= tol * e + 4 * ulp32(e)
    lo, hi = neighbours(xs64)
    return near & (lo != hi) & valid


def check_dur(got_dur, ref, tol, what):
    """The tie rule on integer durations; -> the number of undecided tokens."""
    loose = undecided(ref['xs'], ref['valid'], tol)
    n_valid = int(ref['valid'].sum())
    assert int(loose.sum()) <= UNDECIDED_CAP * n_valid, (what, 'undecided tokens', int(loose.sum()), 'of', n_valid)
    got_dur = np.asarray(got_dur)
    assert got_dur.dtype == np.int64 and got_dur.shape == ref['dur'].shape, (what, got_dur.dtype, got_dur.shape)
    bad = np.argwhere((got_dur != ref['dur']) & ~loose)
    assert bad.size == 0, (what, 'dur differs on decided tokens', bad[:5].tolist(), got_dur[tuple(bad[0])], ref['dur'][tuple(bad[0])])
    lo, hi = neighbours(ref['xs'])
    assert bool(((got_dur == lo) | (got_dur == hi))[loose].all()), (what, 'an undecided token took a duration that is no neighbour')
    assert not got_dur[~ref['valid']].any(), (what, 'a padded token has a duration')
    return int(loose.sum())


def check_xs(got_xs, ref, tol, what):
    """dur_xs within tol of float64, exactly 0 on padded tokens; -> the largest deviation."""
    got_xs = np.asarray(got_xs)
    assert got_xs.dtype == np.float32 and got_xs.shape == ref['xs'].shape and np.isfinite(got_xs).all(), (what, got_xs.dtype, got_xs.shape)
    err = float(np.abs(got_xs.astype(np.float64) - ref['xs']).max())
    assert err <= tol, (what, 'dur_xs', err, tol)
    assert not got_xs[~ref['valid']].any(), (what, 'dur_xs of a padded token is not exactly 0')
    return err


def batch_T(dur, txt):
    """The frame count regulate() derives from a batch's durations."""
    return int((np.asarray(dur) * (np.asarray(txt) != 0)).sum(-1).max())


# ------------------------------------------------------------------------------------------------------------------
# the whole forward, fed a mel2ph
# ------------------------------------------------------------------------------------------------------------------
def forward_fed(front, wset, case, mel2ph_batch, dtype=F64):
    """decoder_inp and mel_out of the rows of `case` (numpy float64) from the CPU oracle FED mel2ph_batch [B,T] (the whole batch's), in row
    groups: an undecided duration cannot enter the frame-level comparison."""
    hp, sd = weights(front, wset)
    inp = dict(inputs(case), mel2ph=np.asarray(mel2ph_batch, np.int64))
    B, T = inp['mel2ph'].shape
    rows = rows_of(case)
    r0, r1, _ = rows.indices(B)
    parts = []
    for g in _row_groups(r1 - r0, T):
        sub = slice(r0 + g.start, r0 + g.stop)
        if front == 'midi':
            r = ofs2.fs2_forward(sd, tensors(inp), hp=hp, dtype=dtype, rows=sub)
        else:       # nothing couples the rows of the plain front
            r = R.forward(sd, {k: v[sub] for k, v in tensors(inp).items()}, hp, dtype=dtype)
        parts.append({k: r[k].double().numpy() for k in ('decoder_inp', 'mel_out')})
    return {k: np.concatenate([p[k] for p in parts]) for k in ('decoder_inp', 'mel_out')}
