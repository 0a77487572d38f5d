"""CPU: what tests/test_gpu_h2w_forms.py rests on, without a GPU — the float64 reference of tests/h2w_cases.py against torch's conv1d, gelu
and conv_transpose1d, the decoders of the quad / plane / V^T / polyphase outputs, the layouts (every window disjoint from every other), the
case lists (every instantiation, every value the sweep promises), the Ch near-tie share of the float32 reference, and a numpy emulation of
the kernel's arithmetic (fp16 hi / lo splits of 16 x, three products, a float32 accumulator advanced in 16-deep steps) against the ceiling
the GPU file asserts: the bar is held to the arithmetic before any kernel runs.  This file pins the reference, not the kernel."""
from dataclasses import replace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import h2w_cases as hc

torch.set_grad_enabled(False)
T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()


@pytest.mark.parametrize('taps', [3, 5, 9, 17])
def test_reference_is_conv1d_same_padding(taps):
    c = hc.Case(37, 128, 64, taps=taps, batch=2, bias=True)
    ops = hc.operands(c)
    got = hc.h2w_ref(c, ops)
    w = T64(ops['w'][0]).permute(1, 2, 0)                                    # [Wn, K, taps]
    want = F.conv1d(T64(ops['act']).transpose(1, 2), w, T64(ops['bias'][0]), padding=taps // 2).transpose(1, 2).numpy()
    assert np.abs(got - want).max() < 1e-11


def test_reference_maps_z_to_activation_and_weight_set_and_orders_the_epilogue():
    c = hc.Case(9, 128, 64, taps=3, batch=6, zdiv=3).with_all()
    ops = hc.operands(c)
    got = hc.h2w_ref(c, ops)
    for z in range(6):
        zw, za = z // 3, z % 3
        w = T64(ops['w'][zw]).permute(1, 2, 0)
        v = F.conv1d(T64(ops['act'][za:za + 1]).transpose(1, 2), w, T64(ops['bias'][zw]), padding=1)[0].T
        v = torch.cat([v[:, :64] * float(np.float32(hc.ALPHA)), v[:, 64:]], 1)
        v = (F.gelu(v) + T64(ops['R'][z])) * T64(ops['rowscale'][za])[:, None]
        assert np.abs(got[z] - v.numpy()).max() < 1e-11, z
    assert (ops['rowscale'] == 0).any() and np.abs(ops['rowscale']).max() <= 1


def test_gelu_is_torchs():
    v = torch.linspace(-6, 6, 1001, dtype=torch.float64)
    assert (hc.gelu(v) - F.gelu(v)).abs().max() < 1e-15


def test_ragged_reference_is_the_item_alone():
    c = hc.ragged_cases(True, 5)[1]
    ops = hc.operands(c)
    got = hc.h2w_ref(c, ops)
    for z, n in enumerate(c.lens):
        assert (got[z, n:] == 0).all()
        if n == 0:
            continue
        alone = replace(c, rows=n, batch=1, lens=None)
        o1 = {k: v[z:z + 1, :n] if k in ('act', 'R', 'rowscale') else v for k, v in ops.items()}
        assert np.abs(hc.h2w_ref(alone, o1)[0] - got[z, :n]).max() < 1e-11, z
    # the non-ragged twin on the activation zeroed from lens[z] on agrees on the rows below lens[z]
    c2, o2 = hc.zeroed(c, ops)
    twin = hc.h2w_ref(c2, o2)
    for z, n in enumerate(c.lens):
        assert n == 0 or np.abs(twin[z, :n] - got[z, :n]).max() < 1e-11


@pytest.mark.parametrize('Lin,p,cut', [(1, 0, 0), (3, 4, 0), (33, 4, 3), (32, 0, 3)])
def test_polyphase_reference_is_conv_transpose1d(Lin, p, cut):
    """conv_transpose1d(k = 16, stride = 8, padding = 4) as ONE 2-tap product: W(tap, 8 co + r, ci) = w[ci][co][r + 8 (1 - tap)], tap_shift0 = -1,
    rows = Lin + 1, output position 8 q + r - up_p with up_p = 4 (the padding); up_p = 0 is the unpadded transposed convolution."""
    Ci, Co = 64, 16
    rs = np.random.RandomState(Lin)
    wt, x, b = rs.standard_normal((Ci, Co, 16)), rs.standard_normal((2, Ci, Lin)), rs.standard_normal(Co)
    full = F.conv_transpose1d(T64(x), T64(wt), T64(b), stride=8, padding=0).numpy()                   # [2, Co, 8 Lin + 8]
    lout = 8 * Lin - cut
    c = hc.Case(Lin + 1, 8 * Co, Ci, taps=2, shift0=-1, act_is_a=0, batch=2, bias=True, up=True, up_p=p, up_lout=lout)
    act = np.zeros((2, Lin + 1, Ci), np.float32)
    ops = {'act': np.concatenate([x.transpose(0, 2, 1), np.zeros((2, 1, Ci))], 1), 'w': hc.up_weights(wt)[None], 'bias': b[None]}
    got = hc.up_want(c, hc.h2w_ref(c, ops))
    assert got.shape == (2, Co, lout) and act.shape == ops['act'].shape
    assert np.abs(got - full[:, :, p:p + lout]).max() < 1e-11
    if p == 4 and cut == 0:
        same = F.conv_transpose1d(T64(x), T64(wt), T64(b), stride=8, padding=4).numpy()
        assert np.abs(got - same).max() < 1e-11
    # every position of [0, up_lout) comes from exactly one (q, r)
    q, r = hc.up_gather(c)
    assert ((8 * q + r - p) == np.arange(lout)).all() and q.max() <= Lin and r.max() < 8


def test_decoders_round_trip():
    t = np.arange(64)
    s = hc.stored(t)
    assert sorted(s) == list(t) and list(s[:16]) == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15] and (s[16:32] == s[:16] + 16).all()
    ix, ixp = hc.vt_index(3, 128, 33, 64)
    both = np.concatenate([ix.ravel(), ixp.ravel()])
    assert sorted(both) == list(range(3 * 128 * 64)) and ix[1, 2, 5] == (1 * 128 + 2) * 64 + 9
    q = hc.quad_index(5, 8)
    assert sorted(q.ravel()) == list(range(40)) and q[3, 6] == (1 * 5 + 3) * 4 + 2
    x = np.random.RandomState(0).standard_normal(4096).astype(np.float32) * np.float32(30)
    hi, lo = hc.split_bits(x)
    assert np.abs(hc.planes_value(hi, lo) - x).max() <= 2.0 ** -21 * np.abs(x).max()                  # two 11-bit halves
    b = hc.bf16_rne(x)
    assert (b == torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)).all()
    assert (hc.bf16_rne(np.array([1.00390625, 1.01171875], np.float32)) == [0x3f80, 0x3f82]).all()     # ties go to the even neighbour
    lo, hi = hc.ch_range(np.array([1.00390625, 1.0039, 1.002, 1.0], np.float64), 1e-5)
    assert list(lo) == [1.0, 1.0, 1.0, 1.0] and list(hi) == [1.0078125, 1.0078125, 1.0, 1.0]


def test_case_lists_cover_what_they_promise():
    assert len(hc.INSTANCES) == 25 and len(set(hc.INSTANCES)) == 25
    assert sum(1 for a, _, _, r in hc.INSTANCES if a and not r) == 13 and sum(1 for a, _, _, r in hc.INSTANCES if not a) == 6
    for inst in hc.INSTANCES:
        a, conv, force, rag = inst
        cs = hc.sweep_cases(inst)
        assert 10 <= len(cs) <= 17
        rows = {c.rows for c in cs}
        assert rows >= set(hc.ROWS) and (a or rows >= {62, 126})
        assert {c.Wn for c in cs} >= {128, 256, 384} and {c.batch for c in cs} >= {1, 2, 3}
        nwg = {(-(-c.rows // hc.TILE[force]) * (c.Wn // 128) * c.batch) % 8 == 0 for c in cs}
        assert nwg == {True, False}, hc.inst_id(inst)
        if conv:
            assert {c.taps for c in cs} >= {2, 3, 5, 9, 17} and any(c.Wn == 1024 for c in cs)
            assert all(c.taps == 17 for c in cs if c.rows <= 2)
            assert all(c.tap_shift0 == -1 for c in cs if c.taps == 2)
            odd = [c for c in cs if c.taps != 2]
            assert all((2 * c.taps) % hc.RING[force] and hc.RING[force] % (2 * c.taps) for c in odd)
            if not rag:
                assert {c.K for c in cs} >= ({64, 128, 256} if hc.RING[force] == 4 else {128, 256} if hc.RING[force] == 8 else {256})
        elif not rag:
            assert {c.K for c in cs} >= set(hc.PLAIN_K[force])
        else:
            assert {c.K for c in cs} == {256, 512}
        if rag:
            assert all(c.lens is not None and len(c.lens) == c.batch and max(c.lens) <= c.rows for c in cs)
        else:
            assert any(c.batch == 6 and c.zdiv == 3 for c in cs)
        assert all(c.bias and c.alpha == hc.ALPHA and c.alpha_ncols == c.Wn // 2 and c.act == hc.ACT_GELU and c.R and c.rowscale and not c.tight
                   for c in cs)
        assert all(hc.form_ok(c, force) for c in cs)
    # slice counts 1, 2 and >= 3 of the plain forms
    for force, ks in hc.PLAIN_K.items():
        bk = 256 if force == 1 else 64
        want = {1: {1, 2}, 2: {3}, 3: {2, 3}, 5: {2, 3}}.get(force, {1, 3})      # deep: one slice = nothing staged ahead; ring4: K = 64 = nothing prefetched
        assert {min(k // bk, 3) for k in ks} == want and all((k // 16) % hc.RING[force] == 0 for k in ks), force
    assert {c.qkv_T for c in hc.qkv_cases()} == set(hc.QKV_T) and {c.H for c in hc.qkv_cases()} == {128, 256}
    assert any(c.qkv_Tp == (c.qkv_T + 31) // 32 * 32 + 32 for c in hc.qkv_cases())
    ups = hc.up_cases()
    assert {c.rows - 1 for c in ups} == set(hc.UP_LIN) and {c.up_p for c in ups} == {0, 4} and {c.Wn for c in ups} == {128, 384}
    assert {c.K for c in ups} == {128, 512} and {c.batch for c in ups} == {1, 3} and {c.ldc_odd for c in ups} == {True, False}
    assert {c.up_lout - 8 * (c.rows - 1) for c in ups} == {0, -3}
    for conv, force in hc.RAGGED_FORMS:
        t = hc.TILE[force]
        for c in hc.ragged_cases(conv, force):
            assert set(c.lens) == {0, 1, t - 1, t, t + 1, c.rows - 1, c.rows} and hc.form_ok(c, force)
    # the dispatch table: the workgroup counts on both sides of each threshold
    count = lambda c, t: -(-c.rows // t) * (c.Wn // 128) * c.batch
    d = [c for c, _ in hc.dispatch_cases() if c.act_is_a]
    assert [count(d[0], 64), count(d[1], 64), count(d[2], 128), count(d[3], 128)] == [254, 256, 504, 512]
    assert max(c.rows * c.Wn * c.K * c.batch * c.taps for c in hc.all_cases()) <= 1024 * 128 * 64 * 64


def test_layouts_keep_every_window_apart():
    """C / Cq / Ch / out / vt, R and the activation planes: every logical element has a place of its own inside its buffer, the alignments the
    kernel's 16- and 8-byte stores need hold, and the descriptor's strides are the ones the index arrays were built from."""
    for c in hc.all_cases():
        ops = {'act': np.zeros((c.n_act, c.rows, c.K), np.float32), 'w': np.zeros((c.n_w, c.taps, c.Wn, c.K), np.float32)}
        if c.bias:
            ops['bias'] = np.zeros((c.n_w, c.Wn // 8 if c.up else c.Wn), np.float32)
        if c.R:
            ops['R'] = np.zeros((c.batch, c.rows, c.Wn), np.float32)
        if c.rowscale:
            ops['rowscale'] = np.zeros((c.n_act, c.rows), np.float32)
        p = hc.pack(c, ops)
        s = p.scal
        for name, o in p.outs.items():
            ix = o['idx'].ravel() if 'pad' not in o else np.concatenate([o['idx'].ravel(), o['pad'].ravel()])
            assert np.unique(ix).size == ix.size, (c.name, name)
            hi = o.get('plane', 0)
            assert ix.min() >= o['off'] and ix.max() + hi < o['n'] - 8, (c.name, name)
            if hi:
                assert ix.max() < o['off'] + hi and hi % 4 == 0, (c.name, name)
        assert np.unique(p.plane_idx).size == p.plane_idx.size and p.plane_idx.max() < p.plane_n
        assert s['lda'] % 8 == 0 and s['lda'] >= c.K and (c.n_act == 1 or (s['sAct'] % 8 == 0 and s['sAct'] >= c.rows * s['lda']))
        assert s['lda_src'] % 4 == 0 and s['sAct_src'] % 4 == 0 and p.off['act'] % 4 == 0
        if p.r_idx is not None:
            assert np.unique(p.r_idx).size == p.r_idx.size
        assert np.isnan(p.host['w']).sum() == p.host['w'].size - c.n_w * c.taps * c.Wn * c.K
        if not c.tight:
            assert s['lda'] > c.K
            if c.C and not c.up:
                assert s['ldc'] > (c.Wn if c.act_is_a else c.rows)
        if c.C:
            assert (s['ldc'] % 4 != 0) == (c.ldc_odd or (c.tight and (c.Wn if c.act_is_a else c.rows) % 4 != 0)), c.name
            assert p.outs['C']['off'] % 4 == c.c_off and (c.ldc_odd or c.tight or s['sC'] % 4 == 0)
        if c.Cq or c.Ch:
            assert s['sC'] % 4 == 0 and s['sC'] >= c.Wn * c.rows
        if c.out:
            assert s['ldo'] % 4 == 0 and s['sO'] % 4 == 0 and s['out_plane'] % 4 == 0 and (not c.qkv_T or s['ldo'] == 2 * c.H)
        if c.qkv_T:
            assert s['qkv_Tp'] % 32 == 0 and s['qkv_Tp'] >= s['qkv_T'] and s['vt_plane'] % 4 == 0 and c.rows % c.qkv_T == 0


def test_ch_seeds_keep_the_float32_reference_under_the_near_tie_cap():
    """c of the GPU file: `Ch` alone is compared with the bf16 rounding of the float64 reference, one ulp allowed where that value lies within the
    fp32 bar of a rounding boundary, and the share of elements that take it stays under 1 %.  The float32 reference itself must stay under
    that cap for the seeds in use, and differ from the float64 rounding nowhere else and by no more than one ulp."""
    for c in hc.quad_cases('Ch'):
        ops = hc.operands(c)
        r64, r32 = hc.h2w_ref(c, ops), hc.h2w_ref(c, ops, torch.float32)
        bar = min(hc.ceiling(c), 2 * float(np.abs(r32 - r64).max()) + 2e-5 * max(1.0, float(np.abs(r64).max())))
        lo, hi = hc.ch_range(r64, bar)
        got, own = (hc.bf16_value(hc.bf16_rne(r.astype(np.float32))) for r in (r32, r64))
        assert ((lo <= got) & (got <= hi)).all(), c.name
        print(f'{c.name}: float32 reference, {int((got != own).sum())} of {got.size} bf16 values on the other side of a near tie '
              f'({(lo != hi).mean():.2%} of the values lie within the bar of one)')
        assert (got != own).mean() < hc.CH_TIE_CAP, (c.name, (got != own).mean())


def test_emulated_arithmetic_is_within_the_ceiling():
    """Every distinct (shape, taps, options) of the GPU file through the numpy emulation of the kernel's products: the deviation from float64
    stays under the ceiling the GPU file asserts, so a kernel that misses it is wrong, not the bar.  Prints emulation / ceiling."""
    seen, worst, n = {}, (0.0, None), 0
    for c in hc.all_cases():
        # outputs, layouts, the output's orientation and forced forms do not change the arithmetic: one emulation per logical problem, the dispatch table's large batches cut to 3
        key = replace(c, tight=False, ldc_odd=False, c_off=0, C=True, Cq=False, Ch=False, out=False, wlayout='nk', tag='', act_is_a=1,
                      batch=min(c.batch, 3) if not (c.zdiv or c.lens) else c.batch)
        if key in seen or c.qkv_T or c.up:
            continue
        seen[key] = True
        ops = hc.operands(key)
        dev = float(np.abs(hc.h2w_emulate(key, ops) - hc.h2w_ref(key, ops)).max())
        ceil = hc.ceiling(key)
        n += 1
        if dev / ceil > worst[0]:
            worst = (dev / ceil, key.name)
        assert dev <= ceil, (key.name, dev, ceil)
    for c in hc.qkv_cases()[:4] + hc.up_cases()[:4]:
        ops = hc.operands(c)
        dev = float(np.abs(hc.h2w_emulate(c, ops) - hc.h2w_ref(c, ops)).max())
        assert dev <= hc.ceiling(c), (c.name, dev)
        worst = max(worst, (dev / hc.ceiling(c), c.name))
        n += 1
    print(f'h2w emulation: {n} problems, largest emulation / ceiling {worst[0]:.3f} ({worst[1]})')
    assert worst[0] > 0.01          # the emulation does round: a bar it sits far below would hold nothing
