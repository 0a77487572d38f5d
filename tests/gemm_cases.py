"""Cases, operands and the reference of the generic GEMM sweep (csrc/gemm.hip launch_gemm through bsg_gemm_ex), shared by
tests/test_gpu_gemm_forms.py (every kernel instantiation against float64) and tests/test_gemm_cases_cpu.py (the reference itself
against torch's conv1d / gelu / mish).  No GPU is needed to import this module.

A case is a `Case`: the logical problem (shape, taps, batch, which epilogue options are on) plus how its operands sit in memory
(`tight`: the consumers' dense layouts; otherwise every operand is a window inside a larger buffer, tests/test_gpu_gemm_forms.py).
`operands(case)` draws the logical arrays from a seed derived from the case; `gemm_ref(ops, dtype)` evaluates them.

Magnitudes: A, B, the biases and R are unit normal; alpha, post_scale_n and rowscale have magnitude <= 1, so the epilogue never
amplifies the contraction's rounding error and the ceiling for unit-normal operands, 2e-6 * 4 * sqrt(K * taps) + 1e-5
(tests/test_gpu_diffnet.py), applies to every case."""
import zlib
from dataclasses import dataclass, replace

import numpy as np
import torch

FORMS = {1: 'gemm_split/64', 2: 'gemm_split/128', 3: 'gemm_fast/64', 4: 'gemm_fast/128', 5: 'gemm_f32'}
ACT_NONE, ACT_RELU, ACT_GELU, ACT_MISH = 0, 1, 2, 3
ALPHA = 0.37


@dataclass(frozen=True)
class Case:
    M: int
    N: int
    K: int
    trans_b: int = 1
    taps: int = 1
    batch: int = 1               # number of outer batch items (zo)
    batch2: int = 0              # inner batch count (zi); 0 = none.  The launch's batch is batch * max(batch2, 1)
    b_batched: bool = True       # B has one matrix set per batch item (False: shared weights, sB = sB2 = 0)
    bias_m: bool = False
    bias_n: bool = False
    bias_n_batched: bool = False   # sBiasN != 0
    alpha: float = 1.0
    alpha_ncols: int = 0
    act: int = ACT_NONE
    post: bool = False
    R: bool = False
    rowscale: bool = False
    tight: bool = False          # dense layouts (lda = K, ldc = N, sA = M * lda, sRS = M ...): what the consumers pass
    pad: int = 4                 # padding columns / gap unit of the windowed layouts (a multiple of 4 keeps the problem aligned)
    tag: str = ''

    @property
    def nz(self):
        return self.batch * max(self.batch2, 1)

    @property
    def name(self):
        s = f'{self.tag}{self.M}x{self.N}x{self.K}' + ('t' if self.trans_b else 'n') + f'/taps{self.taps}/b{self.batch}'
        return s + (f'x{self.batch2}' if self.batch2 > 1 else '')

    def with_all(self, act=ACT_RELU):
        """The fixed "everything on" epilogue of the shape sweep."""
        return replace(self, bias_m=True, bias_n=True, bias_n_batched=True, alpha=ALPHA, alpha_ncols=max(1, self.N // 2), act=act,
                       post=True, R=True, rowscale=True)


def operands(c):
    """The logical arrays of a case (float32 numpy), from a seed derived from the whole case:
      A [nz, M, K]; B [nz or 1, taps, N, K] (trans_b) or [nz or 1, taps, K, N]; bias_m [M]; bias_n [batch or 1, N]; post_scale_n, post_shift_n [N];
      R [batch, M, N]; rowscale [batch, M] (about a third exact zeros, the first and the last row among them when M > 2).
    bias_n, R and rowscale move with the OUTER batch index only, as in the kernels."""
    rs = np.random.RandomState(zlib.crc32(repr(c).encode()) & 0x7fffffff)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    o = {'A': f(c.nz, c.M, c.K)}
    nb = c.nz if c.b_batched else 1
    o['B'] = f(nb, c.taps, c.N, c.K) if c.trans_b else f(nb, c.taps, c.K, c.N)
    if c.bias_m:
        o['bias_m'] = f(c.M)
    if c.bias_n:
        o['bias_n'] = f(c.batch if c.bias_n_batched else 1, c.N)
    if c.post:
        o['post_scale_n'] = (rs.uniform(0.5, 1.0, c.N) * rs.choice([-1.0, 1.0], c.N)).astype(np.float32)
        o['post_shift_n'] = f(c.N)
    if c.R:
        o['R'] = f(c.batch, c.M, c.N)
    if c.rowscale:
        r = rs.uniform(0.5, 1.0, (c.batch, c.M)).astype(np.float32)
        r[rs.uniform(size=r.shape) < 0.3] = 0
        if c.M > 2:
            r[:, 0] = 0
            r[:, -1] = 0
            r[:, 1] = 0.75
        o['rowscale'] = r
    return o


def gelu(v):
    return v * 0.5 * (1.0 + torch.erf(v * 0.70710678118654752440))


def mish(v):
    return v * torch.tanh(torch.log1p(torch.exp(-v.abs())) + torch.clamp(v, min=0))      # softplus without overflow


def gemm_ref(c, ops, dtype=torch.float64):
    """The operation of launch_gemm on the logical arrays, evaluated in `dtype` -> [nz, M, N] float64 numpy:
      1. sum over taps of A rows shifted by tap_shift0 + tap = tap - taps // 2 times B_tap; rows outside [0, M) of the batch item are zero
      2. + bias_n, + bias_m      3. * alpha on columns < alpha_ncols (0: every column)      4. the activation
      5. * post_scale_n + post_shift_n      6. + R      7. * rowscale"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    A, B = t(ops['A']), t(ops['B'])
    nz, M, N = c.nz, c.M, c.N
    b2 = max(c.batch2, 1)
    out = torch.zeros(nz, M, N, dtype=dtype)
    for z in range(nz):
        zo = z // b2
        Bz = B[z if c.b_batched else 0]
        acc = torch.zeros(M, N, dtype=dtype)
        for tap in range(c.taps):
            shift = tap - c.taps // 2
            lo, hi = max(0, -shift), min(M, M - shift)          # output rows i with 0 <= i + shift < M
            if lo >= hi:
                continue
            a = A[z, lo + shift:hi + shift]
            acc[lo:hi] += a @ (Bz[tap].T if c.trans_b else Bz[tap])
        v = acc
        if c.bias_n:
            v = v + t(ops['bias_n'])[zo if c.bias_n_batched else 0][None, :]
        if c.bias_m:
            v = v + t(ops['bias_m'])[:, None]
        if c.alpha != 1.0:
            al = torch.tensor(np.float32(c.alpha).item(), dtype=dtype)
            n = N if c.alpha_ncols == 0 else min(N, c.alpha_ncols)
            v = torch.cat([v[:, :n] * al, v[:, n:]], 1)
        if c.act == ACT_RELU:
            v = torch.clamp(v, min=0)
        elif c.act == ACT_GELU:
            v = gelu(v)
        elif c.act == ACT_MISH:
            v = mish(v)
        if c.post:
            v = v * t(ops['post_scale_n'])[None, :] + t(ops['post_shift_n'])[None, :]
        if c.R:
            v = v + t(ops['R'])[zo]
        if c.rowscale:
            v = v * t(ops['rowscale'])[zo][:, None]
        out[z] = v
    return out.double().numpy()


def ceiling(c):
    """The suite's ceiling for unit-normal operands (tests/test_gpu_diffnet.py test_gemm_f32 / test_gemm_presplit)."""
    return 2e-6 * 4 * (c.K * c.taps) ** 0.5 + 1e-5


# ---- the shape sweep: (M, N, K, taps, batch, batch2) ---------------------------------------------------------------------------------
# No cross product: every value of the issue's table appears once or more in each list, and each list runs on every instantiation
# it is written for.  M = 1 and 2 carry 9 taps (M < taps / 2: most taps read nothing but rows outside the item).
_SWEEP_T = [(1, 1, 4, 9, 1, 0), (2, 2, 12, 9, 3, 0), (63, 31, 16, 3, 1, 0), (64, 33, 20, 5, 3, 0), (65, 127, 36, 1, 1, 0),
            (127, 128, 80, 5, 3, 0), (128, 129, 256, 3, 1, 0), (129, 129, 16, 1, 3, 0), (193, 33, 12, 5, 1, 0), (65, 33, 20, 3, 3, 2)]
_SWEEP_N = [(1, 4, 4, 9, 1, 0), (2, 124, 12, 9, 3, 0), (63, 128, 16, 3, 1, 0), (64, 132, 20, 5, 3, 0), (65, 4, 36, 1, 1, 0),
            (127, 124, 80, 5, 3, 0), (128, 128, 256, 3, 1, 0), (129, 132, 16, 1, 3, 0), (193, 124, 12, 5, 1, 0), (65, 132, 20, 3, 3, 2)]
# gemm_f32 only: K and (trans_b = 0) N that are no multiple of 4, in windows with odd padding (lda, ldb, the strides: all unaligned)
_EXTRA_T = [(5, 3, 1, 3, 1, 0), (66, 34, 3, 5, 3, 0), (130, 130, 33, 1, 1, 0), (7, 129, 81, 9, 3, 0)]
_EXTRA_N = [(5, 1, 1, 3, 1, 0), (66, 2, 3, 5, 3, 0), (130, 33, 33, 1, 1, 0), (7, 129, 81, 9, 3, 0)]


def _mk(rows, trans_b, **kw):
    return [Case(M, N, K, trans_b=trans_b, taps=taps, batch=b, batch2=b2, **kw).with_all() for M, N, K, taps, b, b2 in rows]


def sweep_cases(form, trans_b):
    """The shape sweep of one instantiation, "everything on"."""
    cases = _mk(_SWEEP_T if trans_b else _SWEEP_N, trans_b)
    if form == 5:
        cases += _mk(_EXTRA_T if trans_b else _EXTRA_N, trans_b, pad=3, tag='odd:')
    return cases


def consumer_cases(trans_b=1):
    """The consumers' exact argument patterns (dense layouts, shared weights):
      pe_conv_gemm (csrc/pe_nsf.hip): M = T, N = 256, K = 80 / 256, 5 taps, batch = B, ReLU, post-affine, rowscale with sRS = T holding zeros;
      the N = 2, ldc = 2 Linear of the pitch predictor (pe_linear: bias_n, M = B * T rows);
      the batched bias_n with sBiasN = N and a batched residual (FS2's decoder input, csrc/fs2.hip)."""
    out = []
    for T in (5, 129):
        for K in (80, 256):
            out.append(Case(T, 256, K, taps=5, batch=3, b_batched=False, bias_n=True, act=ACT_RELU, post=True, rowscale=True, tight=True,
                            tag='pe_conv:'))
    out.append(Case(3 * 129, 2, 256, b_batched=False, bias_n=True, tight=True, tag='pe_lin2:'))
    out.append(Case(5, 2, 256, b_batched=False, bias_n=True, tight=True, tag='pe_lin2:'))
    out.append(Case(77, 256, 256, batch=3, b_batched=False, bias_n=True, bias_n_batched=True, R=True, tight=True, tag='fs2_dec:'))
    return out


def epilogue_cases(trans_b):
    """Two fixed shapes (whole tiles; partial tiles in M, N and K with taps and a batch), each option alone, then all together."""
    out = []
    for base in (Case(128, 128, 32, trans_b=trans_b, tag='epi:'), Case(77, 45 if trans_b else 44, 20, trans_b=trans_b, taps=3, batch=2, tag='epi:')):
        N = base.N
        out.append(base)
        out.append(replace(base, bias_m=True))
        out.append(replace(base, bias_n=True))
        out.append(replace(base, bias_n=True, bias_n_batched=True))
        out += [replace(base, alpha=ALPHA, alpha_ncols=n) for n in (0, 40, N + 5)]
        out += [replace(base, act=a) for a in (ACT_RELU, ACT_GELU, ACT_MISH)]
        out.append(replace(base, post=True))
        out.append(replace(base, R=True))
        out.append(replace(base, rowscale=True))
        out += [replace(base.with_all(a), alpha_ncols=40) for a in (ACT_NONE, ACT_RELU, ACT_GELU, ACT_MISH)]
        # ldc != N (and every other padding) is on in all of the above: the windowed layout.  Off: the dense one
        out += [replace(base, tight=True), replace(base.with_all(), alpha_ncols=40, tight=True)]
    return out


# ---- memory layouts ---------------------------------------------------------------------------------------------------------------------
GUARD = 8                        # NaN elements on each side of the small operands


def layout(c, **over):
    """Element counts of the windowed (or dense) layout of a case.  `over`: the auto-dispatch test breaks one alignment at a time."""
    pad = 0 if c.tight else c.pad
    b2 = max(c.batch2, 1)
    halo = c.taps // 2 + 1
    L = dict(halo=halo, a_off=0, b_off=0)
    L['lda'] = c.K + pad
    L['ldb'] = (c.K if c.trans_b else c.N) + pad
    L['ldc'] = c.N + (0 if c.tight else 5)
    L['ldr'] = c.N + (0 if c.tight else 7)
    L['sTapB'] = (c.N if c.trans_b else c.K) * L['ldb'] + 2 * pad
    L['sBiasN'] = (c.N + (0 if c.tight else 3)) if c.bias_n_batched else 0
    L['sRS'] = c.M + (0 if c.tight else 3)
    L['sA_gap'] = L['sB_gap'] = pad
    L.update(over)
    # item strides: with an inner batch, zi moves by s?2 and zo by b2 * s?2 plus a gap of its own, so all six strides differ
    a_item = (c.M + (0 if c.tight else L['halo'])) * L['lda'] + L['sA_gap']
    b_item = c.taps * L['sTapB'] + L['sB_gap']
    c_item = c.M * L['ldc'] + (0 if c.tight else 11)
    if b2 > 1:
        L.update(sA2=a_item, sB2=b_item, sC2=c_item, sA=b2 * a_item + 8, sB=b2 * b_item + 12, sC=b2 * c_item + 9)
    else:
        L.update(sA2=0, sB2=0, sC2=0, sA=a_item, sB=b_item, sC=c_item)
    if not c.b_batched:
        L.update(sB=0, sB2=0)
    L['sR'] = c.M * L['ldr'] + (0 if c.tight else 13)
    return L


def _nan(n):
    return np.full(n, np.nan, np.float32)


def _small(rows, stride):
    """[n, w] logical rows at `stride` elements apart inside NaN -> (buffer, offset of the first row)."""
    n, w = rows.shape
    buf = _nan(GUARD + max(n - 1, 0) * stride + w + GUARD)
    for i in range(n):
        buf[GUARD + i * stride:GUARD + i * stride + w] = rows[i]
    return buf, GUARD


def pack(c, ops, **over):
    """Lay the operands of a case out -> (L, host buffers, element offset of each window, C buffer length, offset of C's first window,
    mask of the elements of C inside a window, index [nz, M, N] of every result in the C buffer)."""
    L = layout(c, **over)
    b2 = max(c.batch2, 1)
    zoff = lambda z, s, s2: (z // b2) * s + (z % b2) * s2
    host, offs = {}, {}
    # A: `halo` NaN rows before the first item (a multiple of 4 elements, so the window stays 16-byte aligned) and after the last
    a_pre = (L['halo'] * L['lda'] + 3) // 4 * 4 + 4 + L['a_off']
    a = _nan(a_pre + zoff(c.nz - 1, L['sA'], L['sA2']) + (c.M + L['halo']) * L['lda'] + 8)
    for z in range(c.nz):
        o = a_pre + zoff(z, L['sA'], L['sA2'])
        for i in range(c.M):
            a[o + i * L['lda']:o + i * L['lda'] + c.K] = ops['A'][z, i]
    host['A'], offs['A'] = a, a_pre
    rows_b, w_b = (c.N, c.K) if c.trans_b else (c.K, c.N)
    b_pre = 8 + L['b_off']
    nb = c.nz if c.b_batched else 1
    b = _nan(b_pre + zoff(nb - 1, L['sB'], L['sB2']) + c.taps * L['sTapB'] + rows_b * L['ldb'] + 8)
    for z in range(nb):
        for t in range(c.taps):
            o = b_pre + zoff(z, L['sB'], L['sB2']) + t * L['sTapB']
            for r in range(rows_b):
                b[o + r * L['ldb']:o + r * L['ldb'] + w_b] = ops['B'][z, t, r]
    host['B'], offs['B'] = b, b_pre
    if c.bias_m:
        host['bias_m'], offs['bias_m'] = _small(ops['bias_m'][None], 0)
    if c.bias_n:
        host['bias_n'], offs['bias_n'] = _small(ops['bias_n'], L['sBiasN'])
    if c.post:
        host['post_scale_n'], offs['post_scale_n'] = _small(ops['post_scale_n'][None], 0)
        host['post_shift_n'], offs['post_shift_n'] = _small(ops['post_shift_n'][None], 0)
    if c.R:
        r = _nan(GUARD + (c.batch - 1) * L['sR'] + c.M * L['ldr'] + GUARD)
        for z in range(c.batch):
            for i in range(c.M):
                o = GUARD + z * L['sR'] + i * L['ldr']
                r[o:o + c.N] = ops['R'][z, i]
        host['R'], offs['R'] = r, GUARD
    if c.rowscale:
        host['rowscale'], offs['rowscale'] = _small(ops['rowscale'], L['sRS'])
    c_pre = 16
    n_c = c_pre + zoff(c.nz - 1, L['sC'], L['sC2']) + c.M * L['ldc'] + 16
    inside = np.zeros(n_c, bool)
    idx = np.zeros((c.nz, c.M, c.N), np.int64)
    for z in range(c.nz):
        for i in range(c.M):
            o = c_pre + zoff(z, L['sC'], L['sC2']) + i * L['ldc']
            assert not inside[o:o + c.N].any()
            inside[o:o + c.N] = True
            idx[z, i] = np.arange(o, o + c.N)
    return L, host, offs, n_c, c_pre, inside, idx


def desc_scalars(c, L):
    """Every bsg_gemm_desc field that is no pointer, for a case in layout L."""
    return dict(M=c.M, N=c.N, K=c.K, lda=L['lda'], ldb=L['ldb'], ldc=L['ldc'], sA=L['sA'], sB=L['sB'], sC=L['sC'], batch2=c.batch2,
                sA2=L['sA2'], sB2=L['sB2'], sC2=L['sC2'], trans_b=c.trans_b, taps=c.taps, tap_shift0=-(c.taps // 2), sTapB=L['sTapB'],
                sBiasN=L['sBiasN'], alpha=c.alpha, alpha_ncols=c.alpha_ncols, act=c.act, ldr=L['ldr'] if c.R else 0,
                sR=L['sR'] if c.R else 0, sRS=L['sRS'], batch=c.nz)


# ---- auto dispatch: one broken alignment at a time -> gemm_f32 ---------------------------------------------------------------------------
AUTO = Case(70, 36, 20, taps=3, batch=2).with_all()
UNALIGNED = {
    'K%4': (replace(AUTO, K=18, pad=2), dict(sA_gap=4, sB_gap=4)),  # lda = ldb = 20, strides multiples of 4: only K breaks the rule
    'lda%4': (AUTO, dict(lda=23)),
    'ldb%4': (AUTO, dict(ldb=21)),
    'sA%4': (AUTO, dict(sA_gap=6)),
    'sTapB%4': (AUTO, dict(sTapB=36 * 24 + 5, sB_gap=5)),          # sB = 3 * 869 + 5 stays a multiple of 4
    'A+4B': (AUTO, dict(a_off=1)),
    'B+4B': (AUTO, dict(b_off=1)),
    'N%4,trans_b=0': (replace(AUTO, N=38, trans_b=0), dict(ldb=40)),
}
