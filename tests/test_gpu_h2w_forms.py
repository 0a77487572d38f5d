"""GPU: the pre-split GEMM (csrc/gemm_h2w.hip launch_gemm_h2w) on each of its 25 kernel instantiations — 13 for the [token][feature]
output, 6 for the [feature][frame] output, 6 ragged — and on each of its five epilogue paths (the direct store with the channel-quad
copies Cq / Ch, the rolled epilogue through LDS, the plane output, the V^T store of the QKV mode, the polyphase store), against the
float64 evaluation of tests/h2w_cases.py, through bsg_gemm_h2w_ex (force_form picks the tile height and ring where the dispatch would
pick by workgroup count and environment; `form` names what ran).

Sentinels.  Every fp32 output (C, Cq) is a set of windows in an int32 buffer filled with a NaN payload, every 16-bit output (Ch, out, vt)
in a buffer of one 16-bit NaN pattern: after the call every element outside the windows still holds the pattern, bit for bit.  bias, R and
rowscale sit between NaN guards, the weights are windows inside NaN, and the activation planes, which the entry builds itself, are fp16
NaN outside the logical rows x K windows (rows < lens[z] with lengths): a tap, a padding column or a ragged row that the kernel fails to
mask reads NaN and raises a range event.  Every case asserts that no range event was counted, runs twice and repeats bit for bit.

Bars, for every case: the suite's ceiling for unit-normal operands, 2e-6 * 4 * sqrt(K * taps) + 1e-5 (held to a numpy emulation of the
kernel's arithmetic in tests/test_h2w_cases_cpu.py), and 2 x the deviation of h2w_ref(float32) from h2w_ref(float64) + 2e-5 x the
result's scale.  Outputs stored as hi / lo fp16 planes of 16 v (out, vt) are compared as (hi + lo) / 16 under the same bars plus
2^-21 |want| (two 11-bit halves).  Where two outputs of one call hold the same value the check is exact: Cq == C bit for bit, Ch is the
round-to-nearest-even bf16 of C, out is hi = fp16(16 c), lo = fp16(16 c - hi) of the stored C (a lo half that is zero may carry either
sign: is_zero below).  Ch without C is compared with the bf16 roundings of (float64 - bar, float64 + bar): one bf16 ulp apart where the
float64 value lies within the bar of a rounding boundary, equal elsewhere; the share of elements that differ from the float64 value's own
rounding stays under 1 %.

Ragged (lens).  Rows below lens[z] equal the float64 reference of the item alone and, bit for bit, the non-ragged call of the same form on
the activation zeroed from lens[z] on; rows from lens[z] to the end of the straddling tile are exactly 0 in every output; tiles wholly
beyond it are untouched.  In the QKV mode this leaves the V^T padding keys T .. Tp - 1 of an item UNWRITTEN whenever its last tile lies
wholly beyond lens[z] (asserted below as "untouched").  That is what the attention expects: flash_attn_planes_kernel (csrc/fs2.hip)
scores the 32-key blocks that start below lens[b] only, masks the keys at or beyond lens[b] inside the last of them (kmask), and that
block ends at or before the end of the straddling GEMM tile (tile heights are multiples of 32), whose rows the product stores as zeros —
or at Tp, when the tile holds row T - 1 and zeroes the padding.  No key it multiplies is left to stale workspace, so nothing was changed
in the producers; tests/test_gpu_fs2_ragged.py runs the ragged front on a poisoned workspace already.

Every test prints, per instantiation and output kind, the largest hip deviation, the largest deviation of the float32 reference and the
largest deviation / bar of a single case.  Measured on an MI355X (all 25 instantiations named by `form`; hip / float32 reference / ratio):

  shape sweep, [token][feature]   plain: 32/deep, 32/ring16  4.2e-5 / 3.1e-5 / 0.22;  32/ring8, 64/ring8  4.0e-5 / 3.7e-5 / 0.24;
                                         32/ring4, 64/ring4, 128/ring4  3.8e-5 / 2.6e-5 / 0.25
                                  conv:  32/ring16, 32/ring8, 64/ring8  2.6e-4 / 5.6e-5 / 0.48;  32/ring4, 64/ring4, 128/ring4  1.4e-4 / 4.5e-5 / 0.36
  shape sweep, [feature][frame]   plain: 64/ring8  3.5e-5 / 3.6e-5 / 0.21;  64/ring4, 128/ring4  3.2e-5 / 2.7e-5 / 0.21
                                  conv:  64/ring8  2.9e-4 / 5.1e-5 / 0.54;  64/ring4, 128/ring4  1.4e-4 / 4.3e-5 / 0.38
  shape sweep, ragged             plain: 32/deep, 64/ring8, 128/ring4  4.9e-5 / 3.5e-5 / 0.25;  conv: 32/ring16, 64/ring8, 128/ring4  2.7e-4 / 5.0e-5 / 0.52
  epilogue sweep                  tok  3.6e-5 / 2.9e-5 / 0.21;  feat  3.9e-5 / 3.5e-5 / 0.24, the same under BSG_H2W_DIRECT=0
  quad outputs (64/ring8, 64/ring4, 128/ring4 alike)   C + Cq  4.4e-5 / 3.5e-5 / 0.32;  C + Ch  3.0e-5 / 2.9e-5 / 0.22;  Cq + Ch + C  3.2e-5 / 3.3e-5 / 0.23;
                                  Ch alone: every value inside the rounding range, near-tie share 0.022 % at most (cap 1 %)
  plane output (all 7 forms)      C  3.0e-5 / 2.6e-5 / 0.20;  out  2.7e-5 / 2.6e-5 / 0.17
  QKV mode (all 7 forms alike)    out  2.6e-5 / 2.9e-5 / 0.17;  vt  2.7e-5 / 2.9e-5 / 0.17
  polyphase (64/ring8, 64/ring4, 128/ring4 alike)      C  1.1e-4 / 5.1e-5 / 0.42
  ragged seams                    plain: C  3.2e-5 / 2.8e-5 / 0.23;  out  2.9e-5 / 2.8e-5 / 0.18;  vt  2.9e-5 / 2.8e-5 / 0.18
                                  conv:  C  2.7e-4 / 5.8e-5 / 0.68;  out  1.6e-4 / 4.5e-5 / 0.37
  dispatch (14 cases)             1.0e-5 .. 2.1e-5 / 1.2e-5 .. 3.5e-5 / 0.11 .. 0.20

The largest ratio is 0.68 (the k = 9 convolution at the ragged seams, 128-row tiles); no sentinel was written and no range event counted.
Where 16 c is -0 the kernel stores the lo half as -0 and numpy's split gives +0 (see is_zero).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bisinger_amd import _lib
from tests import h2w_cases as hc

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SENT32 = 0x7fc5a5a5              # fp32 outputs: a NaN with a payload no arithmetic produces
SENT16 = 0x7fc5                  # 16-bit outputs: NaN as fp16 and as bf16
T_DT = {32: torch.int32, 16: torch.int16}
SENT = {32: SENT32, 16: SENT16}


def launch(c, p, force):
    """One call of bsg_gemm_h2w_ex on fresh sentinel-filled output buffers -> (rc, form, {output: raw bits as numpy})."""
    dev = {k: torch.from_numpy(v).cuda() for k, v in p.host.items()}
    ptr = lambda k: (dev[k].data_ptr() + 4 * p.off[k]) if k in dev else None
    bufs = {k: torch.full((o['n'],), SENT[o['bits']], dtype=T_DT[o['bits']], device='cuda') for k, o in p.outs.items()}
    optr = lambda k: (bufs[k].data_ptr() + (p.outs[k]['bits'] // 8) * p.outs[k]['off']) if k in bufs else None
    d = _lib.H2wDesc(act=ptr('act'), w=ptr('w'), C=optr('C'), Cq=optr('Cq'), Ch=optr('Ch'), out=optr('out'), bias=ptr('bias'), R=ptr('R'),
                     rowscale=ptr('rowscale'), vt=optr('vt'), lens=ptr('lens'), **p.scal)
    form = ctypes.c_char_p()
    rc = _lib.load().bsg_gemm_h2w_ex(ctypes.byref(d), force, ctypes.byref(form), _lib.stream_ptr())
    torch.cuda.synchronize()
    raw = {k: b.cpu().numpy().view(np.uint32 if p.outs[k]['bits'] == 32 else np.uint16) for k, b in bufs.items()}
    return rc, (form.value.decode() if form.value else None), raw


def run(c, ops, force):
    """Lay the operands out, call the entry twice (the runs must agree bit for bit) -> (packed layout, raw buffers, name of the form)."""
    p = hc.pack(c, ops)
    rc, form, raw = launch(c, p, force)
    _lib.check(rc, f'bsg_gemm_h2w_ex {c.name}')
    rc2, form2, raw2 = launch(c, p, force)
    assert rc2 == 0 and form2 == form and all((raw[k] == raw2[k]).all() for k in raw), f'{c.name} on {form}: two runs differ'
    return p, raw, form


_REFS = {}


def reference(c, keep=True):
    """(operands, float64 reference, deviation of the float32 reference from it, scale): computed once per case, shared by the forms."""
    if c in _REFS:
        return _REFS[c]
    ops = hc.operands(c)
    r64 = hc.h2w_ref(c, ops, torch.float64)
    r32 = hc.h2w_ref(c, ops, torch.float32)
    r64.setflags(write=False)
    ref = (ops, r64, float(np.abs(r32 - r64).max()), max(1.0, float(np.abs(r64).max())))
    if keep:
        _REFS[c] = ref
    return ref


@pytest.fixture(autouse=True)
def _clean_range_word():
    _lib.gemm_range_take()
    yield


def is_zero(bits):
    """A 16-bit value that is zero, whatever its sign.  The lo half of a split is x - hi: where that is exactly zero the kernel's subtraction
    leaves -0 for some inputs (x = hi = -0, seen on the MI355X) where numpy's leaves +0; as an operand of the next product the two are the
    same number."""
    return (bits & 0x7fff) == 0


def same_lo(got, want):
    """lo halves agree bit for bit, or both are zero."""
    return (got == want) | (is_zero(got) & is_zero(want))


def written_rows(c, force):
    """[n_act, rows] bool: the rows of each activation item that the launch stores (everything without lens; with lens the tiles that start
    below lens[z], cut at rows)."""
    wr = np.ones((c.n_act, c.rows), bool)
    if c.lens is not None:
        t = hc.TILE[force]
        for za, n in enumerate(c.lens):
            wr[za, min(c.rows, -(-n // t) * t):] = False
    return wr


def untouched(c, p, raw, wr):
    """Every element outside the written windows still holds its sentinel."""
    for k, o in p.outs.items():
        inside = np.zeros(o['n'], bool)
        planes = (0, o['plane']) if 'plane' in o else (0,)
        if k == 'vt':
            B = o['idx'].shape[0]
            T = c.qkv_T
            wb = wr.reshape(B, T) if c.lens is None else wr                           # [B, T] keys written
            ix = np.broadcast_to(wb[:, None, :], o['idx'].shape)
            sel = [o['idx'][ix]] + [o['pad'][b].ravel() for b in range(B) if wb[b, T - 1]]   # the padding is zeroed by whoever stores key T - 1
            sel = np.concatenate(sel)
        elif c.up:
            sel = o['idx'].ravel()
        else:
            sel = o['idx'][np.broadcast_to(wr[np.arange(c.batch) % c.n_act][:, :, None], o['idx'].shape)]
        for pl in planes:
            inside[sel + pl] = True
        bad = raw[k][~inside] != SENT[o['bits']]
        assert not bad.any(), f'{c.name}: {int(bad.sum())} elements outside the written windows of {k} were written'


def check(c, force, stats=None, keep=True, expect_form=None):
    """One case on one form: sentinels, finiteness, the two bars per output kind, the exact relations between outputs, the range word."""
    ops, r64, dev32, scale = reference(c, keep)
    p, raw, form = run(c, ops, force)
    if force:
        assert form == hc.FORMS[force], (c.name, form)
    if expect_form:
        assert form == expect_form, (c.name, form, expect_form)
    tile_form = force or {v: k for k, v in hc.FORMS.items()}[form]
    wr = written_rows(c, tile_form)
    untouched(c, p, raw, wr)
    ceil = hc.ceiling(c)
    bar = min(ceil, 2 * dev32 + 2e-5 * scale)
    zi = np.arange(c.batch) % c.n_act
    live = np.ones((c.batch, c.rows), bool) if c.lens is None else (np.arange(c.rows)[None, :] < np.asarray(c.lens)[zi][:, None])
    dead = wr[zi] & ~live                                                            # stored rows at or beyond lens[z]: exactly zero
    res = {}

    def compare(kind, got, want, slack=0.0, rowmask=None):
        m = np.broadcast_to((live if rowmask is None else rowmask)[..., None], got.shape) if not c.up else np.ones(got.shape, bool)
        g, w = got[m], want[m]
        if g.size == 0:
            return
        assert np.isfinite(g).all(), f'{c.name} on {form}: {int((~np.isfinite(g)).sum())} non-finite values in {kind}'
        err = np.abs(g - w)
        dev = float(err.max())
        res[kind] = (dev, dev32, float((err / (bar + slack * np.abs(w))).max()))
        assert (err <= ceil + slack * np.abs(w)).all(), (c.name, form, kind, dev, ceil)
        assert (err <= 2 * dev32 + 2e-5 * scale + slack * np.abs(w)).all(), (c.name, form, kind, dev, dev32, scale)

    cval = None
    if c.C:
        cbits = raw['C'][p.outs['C']['idx']]
        cval = cbits.view(np.float32)
        compare('C', cval.astype(np.float64), hc.up_want(c, r64) if c.up else r64)
        if c.lens is not None:
            assert (cbits[dead] == 0).all(), f'{c.name} on {form}: rows beyond lens inside a straddling tile are not zero in C'
    if c.Cq:
        assert (raw['Cq'][p.outs['Cq']['idx']] == cbits).all(), f'{c.name} on {form}: Cq differs from C'
    if c.Ch:
        hbits = raw['Ch'][p.outs['Ch']['idx']]
        if c.C:
            assert (hbits == hc.bf16_rne(cval)).all(), f'{c.name} on {form}: Ch is not the bf16 rounding of C'
        else:
            lo, hi = hc.ch_range(r64, bar)
            got = hc.bf16_value(hbits)
            assert ((lo <= got) & (got <= hi)).all(), f'{c.name} on {form}: {int(((got < lo) | (got > hi)).sum())} Ch values outside the rounding of float64 +- bar'
            share = float((got != hc.bf16_value(hc.bf16_rne(r64.astype(np.float32)))).mean())
            res['Ch'] = (float(np.abs(got - r64).max()), dev32, share)
            assert share < hc.CH_TIE_CAP, (c.name, form, share)
    if c.out:
        o = p.outs['out']
        hi, lo = raw['out'][o['idx']], raw['out'][o['idx'] + o['plane']]
        Wo = o['idx'].shape[2]
        if c.C:
            whi, wlo = hc.split_bits(cval)
            assert (hi[live] == whi[live]).all() and same_lo(lo[live], wlo[live]).all(), f'{c.name} on {form}: out is not the hi / lo split of the stored C'
        compare('out', hc.planes_value(hi, lo), r64[:, :, :Wo], slack=2.0 ** -21)
        if c.lens is not None:
            assert (hi[dead] == 0).all() and is_zero(lo[dead]).all(), f'{c.name} on {form}: rows beyond lens inside a straddling tile are not zero in out'
    if c.qkv_T:
        o = p.outs['vt']
        B, H, T = o['idx'].shape
        hi, lo = raw['vt'][o['idx']], raw['vt'][o['idx'] + o['plane']]                  # [B, H, T]
        want = r64[:, :, 2 * H:].reshape(B, T, H).transpose(0, 2, 1)
        lv, dd = live.reshape(B, T), dead.reshape(B, T)
        got = hc.planes_value(hi, lo).transpose(0, 2, 1)                                 # [B, T, H]: rows first, as compare() masks them
        compare('vt', got, want.transpose(0, 2, 1), slack=2.0 ** -21, rowmask=lv)
        dmask = np.broadcast_to(dd[:, None, :], hi.shape)
        assert (hi[dmask] == 0).all() and is_zero(lo[dmask]).all(), f'{c.name} on {form}: keys beyond lens inside a straddling tile are not zero in vt'
        wb = wr.reshape(B, T)
        for b in range(B):
            if wb[b, T - 1]:
                assert (raw['vt'][o['pad'][b]] == 0).all() and (raw['vt'][o['pad'][b] + o['plane']] == 0).all(), \
                    f'{c.name} on {form}: the padding keys T .. Tp - 1 of item {b} are not exactly zero'
    assert _lib.gemm_range_take() == 0, f'{c.name} on {form}: in-range operands raised a range event (or a NaN outside a window was read)'
    if stats is not None:
        stats.append((c.name, res))
    return form, raw, p


def _report(what, inst, stats):
    kinds = sorted({k for _, r in stats for k in r})
    parts = []
    for k in kinds:
        rs = [(n, r[k]) for n, r in stats if k in r]
        worst = max(rs, key=lambda x: x[1][2])
        if k == 'Ch':   # Ch alone: the deviation is bf16's own rounding; what counts is the share of values on the other side of a near tie
            parts.append(f'Ch alone: inside the rounding range, near-tie share {worst[1][2]:.4%} ({worst[0]})')
            continue
        parts.append(f'{k}: hip {max(r[0] for _, r in rs):.2e}, fp32 yardstick {max(r[1] for _, r in rs):.2e}, ratio {worst[1][2]:.3f} ({worst[0]})')
    print(f'h2w forms, {what}, {inst}: {len(stats)} cases; ' + '; '.join(parts))


@pytest.mark.parametrize('inst', hc.INSTANCES, ids=hc.inst_id)
def test_shape_sweep(inst):
    """a. Every instantiation at its shape edges: rows around every tile height, taps wider than the item, K with 1, 2 and >= 3 slices per
    ring, Wn of 1 .. 3 (and 8) column tiles, workgroup counts that are and are not multiples of 8, two weight sets — everything on, in
    windowed layouts."""
    stats = []
    for c in hc.sweep_cases(inst):
        check(c, inst[2], stats)
    _report('shape sweep', hc.inst_id(inst), stats)


@pytest.mark.parametrize('a', [1, 0], ids=['tok', 'feat'])
def test_epilogue_sweep(a):
    """b. Each epilogue option alone, then all together, ldc % 4 != 0 and a C off the 16-byte grid (the scalar stores), the dense layouts;
    dispatched as every caller.  With act_is_a = 0 the plain cases take the direct store, the others the LDS image."""
    stats = []
    for c in hc.epilogue_cases(a):
        check(c, 0, stats)
    _report('epilogue sweep', 'tok' if a else 'feat', stats)


def lds_image_child():
    """Runs in a child under BSG_H2W_DIRECT=0 (a process reads the switch once): the plain [feature][frame] cases through the LDS image."""
    assert os.environ.get('BSG_H2W_DIRECT') == '0'
    _lib.gemm_range_take()
    stats = []
    for c in hc.lds_image_cases():
        check(c, 0, stats)
    _report('epilogue sweep under BSG_H2W_DIRECT=0', 'feat', stats)


def test_plain_feature_frame_output_through_the_lds_image():
    """b. The plain act_is_a = 0 cases once more in ONE child process under BSG_H2W_DIRECT=0."""
    p = subprocess.run([sys.executable, '-c', 'from tests import test_gpu_h2w_forms as t; t.lds_image_child()'], cwd=ROOT,
                       env=dict(os.environ, BSG_H2W_DIRECT='0'), capture_output=True, text=True, timeout=600)
    print((p.stdout or '').strip()[-600:])
    assert p.returncode == 0, (p.stdout or '')[-1500:] + (p.stderr or '')[-3000:]


@pytest.mark.parametrize('force', [5, 6, 7], ids=lambda f: hc.FORMS[f])
@pytest.mark.parametrize('combo', list(hc.QUAD_COMBOS))
def test_quad_outputs_of_the_direct_store(combo, force):
    """c. The conditioner hoist's pattern: two weight sets over three activations, Wn = 512, K = 256, C with Cq / Ch, Ch alone."""
    stats = []
    for c in hc.quad_cases(combo):
        check(c, force, stats)
    _report(f'quad outputs {combo}', hc.FORMS[force], stats)


@pytest.mark.parametrize('force', list(hc.FORMS), ids=lambda f: hc.FORMS[f])
def test_plane_output_is_the_split_of_c(force):
    """d. `out` together with C: the planes are exactly the hi / lo split of the stored C."""
    stats = []
    for c in hc.plane_cases():
        if hc.form_ok(c, force):
            check(c, force, stats)
    assert stats
    _report('plane output', hc.FORMS[force], stats)


@pytest.mark.parametrize('force', list(hc.FORMS), ids=lambda f: hc.FORMS[f])
def test_qkv_mode(force):
    """d. The QKV projection's own epilogue: Q | K planes and V^T planes in MFMA-fragment order against float64, keys T .. Tp - 1 exactly zero,
    T % 4 != 0 with utterance boundaries inside a group of four keys, nothing written outside vt's [B H][Tp] extent or out's windows."""
    stats = []
    for c in hc.qkv_cases():
        assert hc.form_ok(c, force)
        check(c, force, stats)
    _report('QKV mode', hc.FORMS[force], stats)


@pytest.mark.parametrize('force', [5, 6, 7], ids=lambda f: hc.FORMS[f])
def test_polyphase_output(force):
    """e. up_u = 8: every position of [0, up_lout) written (the sentinel is gone: the values are finite and within the bars), nothing beyond."""
    stats = []
    for c in hc.up_cases():
        check(c, force, stats)
    _report('polyphase output', hc.FORMS[force], stats)


@pytest.mark.parametrize('conv,force', hc.RAGGED_FORMS, ids=lambda v: str(v))
def test_ragged(conv, force):
    """f. lens at the seams of the tile height on the six ragged instantiations: see the module docstring."""
    stats = []
    cases = hc.ragged_cases(conv, force) + ([hc.ragged_qkv_case(force)] if not conv else [])
    for c in cases:
        _, raw, p = check(c, force, stats)
        # bit for bit the non-ragged call of the same form on the activation zeroed from lens[z] on, on the rows below lens[z]
        c2, o2 = hc.zeroed(c, reference(c)[0])
        p2, raw2, form2 = run(c2, o2, force)
        assert form2 == hc.FORMS[force]
        live = np.arange(c.rows)[None, :] < np.asarray(c.lens)[:, None]
        for k, o in p.outs.items():
            if k == 'vt':
                m = np.broadcast_to(live[:, None, :], o['idx'].shape)
            else:
                m = np.broadcast_to(live[:, :, None], o['idx'].shape)
            for pl in ((0, o['plane']) if 'plane' in o else (0,)):
                ix2 = p2.outs[k]['idx'].reshape(o['idx'].shape)        # (QKV: the twin's one item of B * T rows, utterance by utterance)
                assert (raw[k][o['idx'][m] + pl] == raw2[k][ix2[m] + p2.outs[k].get('plane', 0) * (pl != 0)]).all(), \
                    f'{c.name}: {k} differs from the zero-padded call'
        assert _lib.gemm_range_take() == 0
    _report('ragged', f"{hc.FORMS[force]}/{'conv' if conv else 'plain'}", stats)


@pytest.mark.skipif(any(k.startswith('BSG_H2W_') for k in os.environ), reason='a BSG_H2W_* switch is set: the dispatch under test is the default one')
@pytest.mark.parametrize('i', range(len(hc.dispatch_cases())), ids=lambda i: f'{hc.dispatch_cases()[i][0].name}->{hc.dispatch_cases()[i][1]}')
def test_dispatch_thresholds(i):
    """g. force_form = 0 at the default switches: the form on both sides of the tiny (256 workgroups of 64 rows) and small (512 of 128 rows)
    thresholds, deep for K = 256 and ring8 for K = 128, for both output layouts (act_is_a = 0 never goes tiny)."""
    c, want = hc.dispatch_cases()[i]
    stats = []
    check(c, 0, stats, keep=False, expect_form=want)
    _report('dispatch', want, stats)


REFUSALS = [(hc.Case(40, 128, 256, act_is_a=0, bias=True), (1, 2, 3, 4), '32-row'),
            (hc.Case(40, 128, 256, taps=3, bias=True), (1,), 'plain product'),
            (hc.Case(40, 128, 128, bias=True), (1,), 'plain product'),
            (hc.Case(40, 128, 64, bias=True), (2, 3, 5), 'does not divide'),
            (hc.Case(40, 128, 64, taps=3, bias=True), (2, 3, 5), 'does not divide'),
            (hc.Case(40, 128, 256, batch=2, lens=(40, 7), bias=True), (2, 3, 4, 6), 'ragged'),
            (hc.Case(40, 128, 256, taps=3, batch=2, lens=(40, 7), bias=True), (3, 4, 6), 'ragged')]


@pytest.mark.parametrize('i', range(len(REFUSALS)))
def test_forced_form_the_kernel_is_not_built_for_is_refused(i):
    """h. -22 with its message, nothing launched: every output buffer still holds its sentinel and `form` stays unset."""
    c, forces, word = REFUSALS[i]
    p = hc.pack(c, hc.operands(c))
    for force in forces:
        assert not hc.form_ok(c, force)
        rc, form, raw = launch(c, p, force)
        msg = _lib.load().bsg_last_error().decode()
        assert rc == -22 and form is None and 'force_form' in msg and word in msg, (force, rc, form, msg)
        assert all((raw[k] == SENT[p.outs[k]['bits']]).all() for k in raw)
