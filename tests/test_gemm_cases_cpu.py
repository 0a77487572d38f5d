"""CPU: the reference of the generic GEMM sweep (tests/gemm_cases.py gemm_ref) is not self-invented.  Its tap sum is torch's conv1d
with SAME zero padding per batch item, its GELU and Mish are torch's, and the case lists hold what tests/test_gpu_gemm_forms.py
says they hold."""
from dataclasses import replace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_cases as gc

F64 = torch.float64


def _tap_cases():
    seen, out = set(), []
    for tb in (1, 0):
        for c in gc.sweep_cases(5, tb) + gc.consumer_cases():
            if c.taps > 1 and c.name not in seen:
                seen.add(c.name)
                out.append(c)
    return out


@pytest.mark.parametrize('c', _tap_cases(), ids=lambda c: c.name)
def test_tap_sum_is_conv1d_same_padding(c):
    """Epilogue off: gemm_ref == conv1d(A^T, W, padding = taps // 2) of every batch item alone, W[n, k, tap] = B_tap[n, k]."""
    plain = gc.Case(c.M, c.N, c.K, trans_b=c.trans_b, taps=c.taps, batch=c.batch, batch2=c.batch2, b_batched=c.b_batched)
    ops = gc.operands(plain)
    got = gc.gemm_ref(plain, ops, F64)
    for z in range(plain.nz):
        B = torch.from_numpy(ops['B'][z if plain.b_batched else 0]).double()            # [taps, N, K] or [taps, K, N]
        w = B.permute(1, 2, 0) if plain.trans_b else B.permute(2, 1, 0)                  # [N, K, taps]
        x = torch.from_numpy(ops['A'][z]).double().T[None]                               # [1, K, M]
        want = F.conv1d(x, w.contiguous(), padding=plain.taps // 2)[0].T.numpy()         # [M, N]
        assert np.abs(got[z] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (plain.name, z)


def test_activations_are_torchs():
    v = torch.cat([torch.linspace(-30, 30, 2001, dtype=F64), torch.tensor([-1e-9, 0.0, 1e-9, 25.0, 700.0, -700.0], dtype=F64)])
    assert (gc.gelu(v) - F.gelu(v)).abs().max() <= 1e-14
    assert (gc.mish(v) - F.mish(v)).abs().max() <= 1e-13
    assert torch.isfinite(gc.mish(v)).all()


def test_epilogue_order():
    """One element by hand: ((a.b + bias_n + bias_m) * alpha -> ReLU) * scale + shift + R, times rowscale; alpha only below alpha_ncols."""
    c = gc.Case(4, 6, 8, trans_b=1, batch=2).with_all()
    c = replace(c, alpha_ncols=3)
    ops = gc.operands(c)
    got = gc.gemm_ref(c, ops, F64)
    d = {k: v.astype(np.float64) for k, v in ops.items()}
    for z, i, j in [(0, 1, 0), (1, 1, 2), (1, 2, 3), (0, 3, 5), (1, 0, 1)]:
        v = d['A'][z, i] @ d['B'][z, 0, j] + d['bias_n'][z, j] + d['bias_m'][i]
        if j < 3:
            v *= float(np.float32(gc.ALPHA))
        v = max(v, 0.0) * d['post_scale_n'][j] + d['post_shift_n'][j] + d['R'][z, i, j]
        assert abs(got[z, i, j] - v * d['rowscale'][z, i]) <= 1e-12
    assert (ops['post_scale_n'] < 0).any() and (ops['rowscale'] == 0).any()


def test_inner_batch_shares_the_outer_operands():
    c = gc.Case(5, 4, 8, batch=3, batch2=2).with_all()
    ops = gc.operands(c)
    assert ops['A'].shape[0] == 6 and ops['R'].shape[0] == 3 and ops['rowscale'].shape[0] == 3 and ops['bias_n'].shape[0] == 3
    assert gc.gemm_ref(c, ops).shape == (6, 5, 4)


def test_sweep_holds_the_listed_values():
    aligned_k, extra_k = {4, 12, 16, 20, 36, 80, 256}, {1, 3, 33, 81}
    for form in gc.FORMS:
        for tb in (1, 0):
            cs = gc.sweep_cases(form, tb)
            assert {c.M for c in cs} >= {1, 2, 63, 64, 65, 127, 128, 129, 193}
            ns = {1, 2, 31, 33, 127, 128, 129} if tb else {4, 124, 128, 132} | ({1, 2, 33, 129} if form == 5 else set())
            assert {c.N for c in cs} >= ns
            assert {c.K for c in cs} >= aligned_k | (extra_k if form == 5 else set())
            assert {c.taps for c in cs} >= {1, 3, 5, 9} and {c.batch for c in cs} >= {1, 3}
            assert any(c.taps == 9 and c.M == 1 for c in cs) and any(c.taps == 9 and c.M == 2 for c in cs)
            assert sum(c.batch2 == 2 for c in cs) == 1
            if form != 5:
                assert all(c.K % 4 == 0 and (tb or c.N % 4 == 0) and c.pad % 4 == 0 for c in cs)
    for tb in (1, 0):
        cs = gc.epilogue_cases(tb)
        assert {c.act for c in cs} == {0, 1, 2, 3} and {c.alpha_ncols for c in cs if c.alpha != 1} >= {0, 40, cs[0].N + 5}


def _emulate(c, host, offs, d):
    """bsg_gemm_desc semantics (include/bisinger_hip.h) on the flat host buffers, in float64 numpy, reading only what a correct kernel may
    read: the layouts of tests/gemm_cases.py pack() and its descriptor must reproduce gemm_ref without touching a NaN."""
    b2 = max(d['batch2'], 1)
    M, N, K = d['M'], d['N'], d['K']
    out = np.zeros((d['batch'], M, N))
    g = lambda k: host[k].astype(np.float64)
    A, B = g('A'), g('B')
    j, k = np.arange(N), np.arange(K)
    for z in range(d['batch']):
        zo, zi = divmod(z, b2)
        a0 = offs['A'] + zo * d['sA'] + zi * d['sA2']
        b0 = offs['B'] + zo * d['sB'] + zi * d['sB2']
        acc = np.zeros((M, N))
        for tap in range(d['taps']):
            bt = b0 + tap * d['sTapB']
            Bt = B[bt + j[:, None] * d['ldb'] + k[None, :]] if d['trans_b'] else B[bt + k[None, :] * d['ldb'] + j[:, None]]      # [N, K]
            for i in range(M):
                r = i + d['tap_shift0'] + tap
                if 0 <= r < M:
                    acc[i] += Bt @ A[a0 + r * d['lda'] + k]
        v = acc
        if 'bias_n' in host:
            v = v + g('bias_n')[offs['bias_n'] + zo * d['sBiasN'] + j][None, :]
        if 'bias_m' in host:
            v = v + g('bias_m')[offs['bias_m'] + np.arange(M)][:, None]
        n = N if d['alpha_ncols'] == 0 else min(N, d['alpha_ncols'])
        v[:, :n] *= float(np.float32(d['alpha']))
        tv = torch.from_numpy(v)
        v = [tv, torch.relu(tv), F.gelu(tv), F.mish(tv)][d['act']].numpy()
        if 'post_scale_n' in host:
            v = v * g('post_scale_n')[offs['post_scale_n'] + j] + g('post_shift_n')[offs['post_shift_n'] + j]
        if 'R' in host:
            v = v + g('R')[offs['R'] + zo * d['sR'] + np.arange(M)[:, None] * d['ldr'] + j[None, :]]
        if 'rowscale' in host:
            v = v * g('rowscale')[offs['rowscale'] + zo * d['sRS'] + np.arange(M)][:, None]
        out[z] = v
    return out


def _layout_cases():
    cs = [(c, {}) for tb in (1, 0) for c in gc.sweep_cases(5, tb)] + [(c, {}) for c in gc.consumer_cases()]
    cs += [(c, {}) for tb in (1, 0) for c in gc.epilogue_cases(tb)[-6:]] + list(gc.UNALIGNED.values())
    return cs


@pytest.mark.parametrize('c,over', _layout_cases(), ids=lambda v: v.name if isinstance(v, gc.Case) else ','.join(v))
def test_packed_layout_and_descriptor_reproduce_the_reference(c, over):
    ops = gc.operands(c)
    L, host, offs, n_c, c_pre, inside, idx = gc.pack(c, ops, **over)
    d = gc.desc_scalars(c, L)
    got = _emulate(c, host, offs, d)
    want = gc.gemm_ref(c, ops, F64)
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= 1e-11 * max(1.0, np.abs(want).max())
    # C: the windows are disjoint, inside the buffer, and where the descriptor's strides put them
    assert inside.sum() == c.nz * c.M * c.N and idx.max() < n_c - 8 and idx.min() == c_pre
    b2 = max(c.batch2, 1)
    for z in (0, c.nz - 1):
        assert idx[z, c.M - 1, c.N - 1] == c_pre + (z // b2) * d['sC'] + (z % b2) * d['sC2'] + (c.M - 1) * d['ldc'] + c.N - 1
    # every padding element of A and B is NaN, and the windows start where the alignment rule wants them
    assert np.isnan(host['A']).sum() == host['A'].size - ops['A'].size and np.isnan(host['B']).sum() == host['B'].size - ops['B'].size
    if not over and c.pad % 4 == 0:
        assert offs['A'] % 4 == 0 and offs['B'] % 4 == 0
        assert all(d[k] % 4 == 0 for k in ('lda', 'ldb', 'sA', 'sA2', 'sB', 'sB2', 'sTapB'))
