"""Cases, operands, layouts, decoders and the float64 reference of the pre-split GEMM sweep (csrc/gemm_h2w.hip launch_gemm_h2w through
bsg_gemm_h2w_ex), shared by tests/test_gpu_h2w_forms.py (every kernel instantiation against float64) and tests/test_h2w_cases_cpu.py (the
reference itself against torch's conv1d / gelu / conv_transpose1d, the decoders, the layouts, and a numpy emulation of the kernel's
arithmetic against the ceiling).  No GPU is needed to import this module.

A `Case` is the logical problem (shape, taps, batch / zdiv, epilogue options, which outputs, which mode) plus how its operands sit in
memory (`tight`: the consumers' dense layouts; otherwise every operand is a window inside a larger buffer).  `operands(case)` draws the
logical arrays from a seed derived from the case, `h2w_ref(case, ops, dtype)` evaluates them, `pack(case, ops)` lays them out.

The operation, per batch index z (activation item za = z % zdiv, weight set zw = z // zdiv):
  v(i, n) = sum_tap sum_k act[za][i + tap_shift0 + tap][k] w[zw][tap][n][k]     rows outside [0, rows) — with lens: [0, lens[za]) — are zero
  v += bias[zw][n];  v *= alpha on weight rows n < alpha_ncols (0: all);  ReLU / GELU (erf);  v += R[z](i, n);  v *= rowscale[za][i]
and, with lens, rows i >= lens[za] of the result are zero.

Magnitudes as in tests/gemm_cases.py: unit-normal operands, |alpha| and rowscale <= 1 with exact zeros in rowscale, so the epilogue never
amplifies the contraction's rounding error and gemm_cases.ceiling (2e-6 * 4 * sqrt(K * taps) + 1e-5) applies to every case."""
import zlib
from dataclasses import dataclass, replace

import numpy as np
import torch

from tests import gemm_cases as gc

FORMS = {1: 'h2w/32/deep', 2: 'h2w/32/ring16', 3: 'h2w/32/ring8', 4: 'h2w/32/ring4', 5: 'h2w/64/ring8', 6: 'h2w/64/ring4', 7: 'h2w/128/ring4'}
RING = {1: 16, 2: 16, 3: 8, 4: 4, 5: 8, 6: 4, 7: 4}
TILE = {1: 32, 2: 32, 3: 32, 4: 32, 5: 64, 6: 64, 7: 128}
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
ALPHA = 0.37
ceiling = gc.ceiling            # reads .K and .taps of a case


@dataclass(frozen=True)
class Case:
    rows: int
    Wn: int
    K: int
    taps: int = 1
    shift0: int = None           # tap_shift0; None: -(taps // 2), SAME padding
    act_is_a: int = 1
    batch: int = 1               # number of batch indices z
    zdiv: int = 0                # activation items (0: = batch, one weight set); batch // zdiv weight sets
    bias: bool = False
    alpha: float = 1.0
    alpha_ncols: int = 0
    act: int = ACT_NONE
    R: bool = False
    rowscale: bool = False
    C: bool = True
    Cq: bool = False
    Ch: bool = False
    out: bool = False
    qkv_T: int = 0               # QKV mode: rows = B * T (batch 1) or rows = T (ragged), Wn = 3 H, out and vt, no C
    qkv_Tp: int = 0
    up: bool = False             # polyphase output (up_u = 8): Wn = 8 Co, taps 2, shift0 -1, bias per co
    up_p: int = 0
    up_lout: int = 0
    lens: tuple = None           # ragged: one row count per activation item
    wlayout: str = 'nk'          # fp32 weight source: 'nk' [tap][Wn][K] rows padded; 'kn' [tap][K][Wn] (transposed); 'conv' [Wn][K][taps] (Conv1d)
    tight: bool = False
    ldc_odd: bool = False        # ldc % 4 != 0
    c_off: int = 0               # 1: C starts 4 bytes past a 16-byte boundary
    seed: int = 0
    tag: str = ''

    @property
    def n_act(self):
        return self.zdiv or self.batch

    @property
    def n_w(self):
        return self.batch // self.n_act

    @property
    def tap_shift0(self):
        return -(self.taps // 2) if self.shift0 is None else self.shift0

    @property
    def H(self):
        return self.Wn // 3

    @property
    def name(self):
        s = f'{self.tag}{self.rows}x{self.Wn}x{self.K}/taps{self.taps}/b{self.batch}' + (f'/zdiv{self.zdiv}' if self.zdiv else '')
        return s + (f'/lens{list(self.lens)}' if self.lens else '') + ('' if self.act_is_a else '/T')

    def with_all(self):
        """The fixed "everything on" epilogue of the shape sweep."""
        return replace(self, bias=True, alpha=ALPHA, alpha_ncols=self.Wn // 2, act=ACT_GELU, R=True, rowscale=True)


def steps(c):
    return c.K // 16 * c.taps


def form_ok(c, force):
    """What bsg_gemm_h2w_ex accepts as a forced form for a case (the refusals of include/bisinger_hip.h)."""
    if force <= 4 and not c.act_is_a:
        return False
    if force == 1 and not (c.taps == 1 and c.K % 256 == 0):
        return False
    if steps(c) % RING[force]:
        return False
    if c.lens is not None:
        return c.K % 256 == 0 and (force in (5, 7) or force == (1 if c.taps == 1 else 2))
    return True


def operands(c):
    """The logical arrays of a case (float32 numpy): act [n_act, rows, K]; w [n_w, taps, Wn, K]; bias [n_w, Wn] (polyphase: [1, Wn / 8]);
    R [batch, rows, Wn] at the logical (i, n); rowscale [n_act, rows] with about a third exact zeros."""
    rs = np.random.RandomState(zlib.crc32(repr(c).encode()) & 0x7fffffff)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    o = {'act': f(c.n_act, c.rows, c.K), 'w': f(c.n_w, c.taps, c.Wn, c.K)}
    if c.bias:
        o['bias'] = f(c.n_w, c.Wn // 8 if c.up else c.Wn)
    if c.R:
        o['R'] = f(c.batch, c.rows, c.Wn)
    if c.rowscale:
        r = rs.uniform(0.5, 1.0, (c.n_act, c.rows)).astype(np.float32)
        r[rs.uniform(size=r.shape) < 0.3] = 0
        if c.rows > 2:
            r[:, 0] = 0
            r[:, -1] = 0
            r[:, 1] = 0.75
        o['rowscale'] = r
    return o


def gelu(v):
    return v * 0.5 * (1.0 + torch.erf(v * 0.70710678118654752440))


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def epilogue(c, ops, z, v, dtype):
    """bias, alpha, activation, R, rowscale on the accumulated [rows, Wn] of batch index z, in the kernel's order."""
    zw, za = z // c.n_act, z % c.n_act
    if c.bias:
        b = _t(ops['bias'], dtype)[zw]
        v = v + (b.repeat_interleave(8) if c.up else b)[None, :]
    if c.alpha != 1.0:
        al = torch.tensor(np.float32(c.alpha).item(), dtype=dtype)
        n = c.Wn if c.alpha_ncols == 0 else min(c.Wn, c.alpha_ncols)
        v = torch.cat([v[:, :n] * al, v[:, n:]], 1)
    if c.act == ACT_RELU:
        v = torch.clamp(v, min=0)
    elif c.act == ACT_GELU:
        v = gelu(v)
    if c.R:
        v = v + _t(ops['R'], dtype)[z]
    if c.rowscale:
        v = v * _t(ops['rowscale'], dtype)[za][:, None]
    if c.lens is not None:
        v = v.clone()
        v[c.lens[za]:] = 0
    return v


def _tap_rows(c, tap, M):
    """Output rows [lo, hi) whose tap reads a row inside [0, M), and the shift."""
    shift = c.tap_shift0 + tap
    return max(0, -shift), min(M, M - shift), shift


def h2w_ref(c, ops, dtype=torch.float64):
    """The operation on the logical arrays, evaluated in `dtype` -> [batch, rows, Wn] float64 numpy (always (i, n), whatever act_is_a)."""
    A, W = _t(ops['act'], dtype), _t(ops['w'], dtype)
    out = torch.zeros(c.batch, c.rows, c.Wn, dtype=dtype)
    for z in range(c.batch):
        zw, za = z // c.n_act, z % c.n_act
        M = c.rows if c.lens is None else c.lens[za]
        acc = torch.zeros(c.rows, c.Wn, dtype=dtype)
        for tap in range(c.taps):
            lo, hi, shift = _tap_rows(c, tap, M)
            if lo < hi:
                acc[lo:hi] += A[za, lo + shift:hi + shift] @ W[zw, tap].T
        out[z] = epilogue(c, ops, z, acc, dtype)
    return out.double().numpy()


def split16(x):
    """hi, lo fp16 halves (as float64) of 16 x, the kernel's operand split."""
    x16 = x.astype(np.float32) * np.float32(16)
    hi = x16.astype(np.float16)
    lo = (x16 - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def h2w_emulate(c, ops):
    """The kernel's arithmetic in numpy -> [batch, rows, Wn] float64: operands x 16 split into fp16 hi + lo, the three products hi·hi, hi·lo,
    lo·hi (lo·lo dropped), each 16-deep step added to a float32 accumulator in the kernel's (slice, tap, kk) order, x 2^-8, then the
    epilogue in float32."""
    ah, al = split16(ops['act'])
    wh, wl = split16(ops['w'])
    bk = 32 if c.taps > 1 else 64
    out = np.zeros((c.batch, c.rows, c.Wn))
    for z in range(c.batch):
        zw, za = z // c.n_act, z % c.n_act
        M = c.rows if c.lens is None else c.lens[za]
        acc = np.zeros((c.rows, c.Wn), np.float32)
        for s0 in range(0, c.K, bk):
            for tap in range(c.taps):
                lo, hi, shift = _tap_rows(c, tap, M)
                if lo >= hi:
                    continue
                for k0 in range(s0, s0 + bk, 16):
                    k = slice(k0, k0 + 16)
                    a_h, a_l = ah[za, lo + shift:hi + shift, k], al[za, lo + shift:hi + shift, k]
                    for x, y in ((a_h, wl[zw, tap, :, k]), (a_h, wh[zw, tap, :, k]), (a_l, wh[zw, tap, :, k])):
                        acc[lo:hi] = (acc[lo:hi].astype(np.float64) + x @ y.T).astype(np.float32)
        v = torch.from_numpy(acc * np.float32(1 / 256))
        out[z] = epilogue(c, ops, z, v, torch.float32).double().numpy()
    return out


# ---- decoders of the other outputs --------------------------------------------------------------------------------------------------------
def stored(t):
    """Position of key t inside a V^T row: the groups of 4 inside 16 keys in MFMA-fragment order 0-3, 8-11, 4-7, 12-15."""
    t = np.asarray(t)
    g4 = (t >> 2) & 3
    return (t & ~15) + ((((g4 & 1) << 1) | (g4 >> 1)) << 2) + (t & 3)


def quad_index(rows, Wn):
    """[rows, Wn] -> element offset of (i, n) in the channel-quad order [Wn / 4][rows][4] of Cq / Ch."""
    i, n = np.meshgrid(np.arange(rows), np.arange(Wn), indexing='ij')
    return ((n >> 2) * rows + i) * 4 + (n & 3)


def vt_index(B, H, T, Tp):
    """([B, H, T] offsets of the keys, [B, H, Tp - T] offsets of the padding) in the V^T plane [B * H][Tp]."""
    b, d, t = np.meshgrid(np.arange(B), np.arange(H), np.arange(Tp), indexing='ij')
    ix = (b * H + d) * Tp + stored(t)
    return ix[:, :, :T], ix[:, :, T:]


def up_gather(c):
    """Polyphase: for every output position pos in [0, up_lout) the activation row q and the phase r with 8 q + r - up_p == pos."""
    pos = np.arange(c.up_lout) + c.up_p
    return pos // 8, pos % 8


def up_want(c, ref):
    """[batch, rows, Wn] reference -> [batch, Co, up_lout], C[co][8 q + r - up_p] = ref[q][8 co + r]."""
    q, r = up_gather(c)
    Co = c.Wn // 8
    return np.stack([ref[:, q, 8 * co + r] for co in range(Co)], 1)


def bf16_rne(x):
    """float32 -> bf16 bits, round to nearest even."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff).astype(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def split_bits(cval):
    """The stored fp32 C -> (hi, lo) fp16 bit patterns of the plane output: hi = fp16(16 c), lo = fp16(16 c - hi)."""
    x = np.ascontiguousarray(cval, np.float32) * np.float32(16)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def planes_value(hi_bits, lo_bits):
    return (hi_bits.view(np.float16).astype(np.float64) + lo_bits.view(np.float16).astype(np.float64)) / 16


# ---- memory layouts ---------------------------------------------------------------------------------------------------------------------
GUARD = 8


def _c4(n):
    return (n + 3) // 4 * 4


def _nan(n):
    return np.full(n, np.nan, np.float32)


@dataclass
class Packed:
    host: dict          # name -> float32 / int32 numpy buffer of an input
    off: dict           # name -> element offset of its first window
    outs: dict          # name -> dict(n = elements, off = element offset the pointer gets, idx = ..., bits = 32 / 16)
    scal: dict          # every bsg_h2w_desc field that is no pointer
    plane_idx: np.ndarray   # [n_act, rows, K] offsets of the activation windows inside ONE plane of the buffer the entry builds
    plane_n: int


def pack(c, ops):
    """Lay a case out.  Inputs are windows inside NaN; outputs are described by index arrays into sentinel-filled buffers:
      C   [batch, rows, Wn] (polyphase: [batch, Co, up_lout]);  Cq, Ch [batch, rows, Wn];  out [batch, rows, Wo] (hi; lo out_plane behind), Wo = Wn or 2 H;
      vt  [B, H, T] with vt_pad [B, H, Tp - T] (hi; lo vt_plane behind)."""
    pad = 0 if c.tight else 1
    rows, K, Wn, taps = c.rows, c.K, c.Wn, c.taps
    host, off, outs, s = {}, {}, {}, {}
    # activation (fp32 source) and the planes the entry builds
    lda_src = K + 4 * pad
    sAct_src = rows * lda_src + 8 * pad
    a = _nan(GUARD + (c.n_act - 1) * sAct_src + rows * lda_src + GUARD)
    for za in range(c.n_act):
        for i in range(rows):
            o = GUARD + za * sAct_src + i * lda_src
            a[o:o + K] = ops['act'][za, i]
    host['act'], off['act'] = a, GUARD
    lda = K + 8 * pad
    sAct = rows * lda + 16 * pad
    za_, i_, k_ = np.meshgrid(np.arange(c.n_act), np.arange(rows), np.arange(K), indexing='ij')
    plane_idx = za_ * sAct + i_ * lda + k_
    plane_n = ((c.n_act - 1) * sAct + rows * lda + 7) // 8 * 8
    # weights
    if c.wlayout == 'nk':
        ldw = K + 4 * pad
        ts, rs_, ks = Wn * ldw + 4 * pad, ldw, 1
    elif c.wlayout == 'kn':
        ldw = Wn + 3 * pad
        ts, rs_, ks = K * ldw + 5 * pad, 1, ldw
    else:
        ts, rs_, ks = 1, K * taps, taps
    t_, n_, k2_ = np.meshgrid(np.arange(taps), np.arange(Wn), np.arange(K), indexing='ij')
    widx = t_ * ts + n_ * rs_ + k2_ * ks
    wext = int(widx.max()) + 1
    sW = wext + 7 * pad
    w = _nan(GUARD + (c.n_w - 1) * sW + wext + GUARD)
    for zw in range(c.n_w):
        w[GUARD + zw * sW + widx] = ops['w'][zw]
    host['w'], off['w'] = w, GUARD
    # small operands between NaN guards
    sBias = sRS = sR = ldr = 0
    if c.bias:
        nb = ops['bias'].shape[1]
        sBias = (nb + 3 * pad) if c.n_w > 1 else 0
        b = _nan(GUARD + (c.n_w - 1) * sBias + nb + GUARD)
        for zw in range(c.n_w):
            b[GUARD + zw * sBias:GUARD + zw * sBias + nb] = ops['bias'][zw]
        host['bias'], off['bias'] = b, GUARD
    if c.rowscale:
        sRS = rows + 3 * pad
        r = _nan(GUARD + (c.n_act - 1) * sRS + rows + GUARD)
        for za in range(c.n_act):
            r[GUARD + za * sRS:GUARD + za * sRS + rows] = ops['rowscale'][za]
        host['rowscale'], off['rowscale'] = r, GUARD
    z_, i3, n3 = np.meshgrid(np.arange(c.batch), np.arange(rows), np.arange(Wn), indexing='ij')
    r_idx = None
    if c.R:
        ldr = (Wn if c.act_is_a else rows) + 7 * pad
        sR = (rows if c.act_is_a else Wn) * ldr + 13 * pad
        r_idx = GUARD + z_ * sR + (i3 * ldr + n3 if c.act_is_a else n3 * ldr + i3)
        r = _nan(int(r_idx.max()) + 1 + GUARD)
        r[r_idx] = ops['R']
        host['R'], off['R'] = r, GUARD
    if c.lens is not None:
        host['lens'], off['lens'] = np.asarray(c.lens, np.int32), 0
    # outputs
    ldc = sC = 0
    inner, outer = (Wn, rows) if c.act_is_a else (rows, Wn)      # C is [outer][ldc]
    if c.up:
        inner, outer = c.up_lout, Wn // 8
    ldc = inner + (0 if c.tight else 5 if c.ldc_odd else 4 * ((inner + 3) // 4) - inner + 4)
    sC = outer * ldc if c.tight else outer * ldc + 11 if c.ldc_odd else _c4(outer * ldc) + 12
    if c.Cq or c.Ch:
        sC = max(sC, Wn * rows + 12 * pad)
    c_pre = 16 + c.c_off
    if c.C:
        if c.up:
            zz, co, pos = np.meshgrid(np.arange(c.batch), np.arange(Wn // 8), np.arange(c.up_lout), indexing='ij')
            idx = c_pre + zz * sC + co * ldc + pos
        else:
            idx = c_pre + z_ * sC + (i3 * ldc + n3 if c.act_is_a else n3 * ldc + i3)
        outs['C'] = dict(n=int(idx.max()) + 1 + 16, off=c_pre, idx=idx, bits=32)
    for name, on, bits in (('Cq', c.Cq, 32), ('Ch', c.Ch, 16)):
        if on:
            idx = 16 + z_ * sC + quad_index(rows, Wn)[None]
            outs[name] = dict(n=int(idx.max()) + 1 + 16, off=16, idx=idx, bits=bits)
    ldo = sO = out_plane = 0
    if c.out:
        Wo = 2 * c.H if c.qkv_T else Wn
        ldo = Wo if (c.tight or c.qkv_T) else Wo + 4
        sO = rows * ldo + 8 * pad
        idx = 16 + z_[:, :, :Wo] * sO + i3[:, :, :Wo] * ldo + n3[:, :, :Wo]
        out_plane = _c4(int(idx.max()) + 1) + 8
        outs['out'] = dict(n=16 + 2 * out_plane + 16, off=16, idx=idx, bits=16, plane=out_plane)
    vt_plane = 0
    if c.qkv_T:
        B = c.batch if c.lens is not None else rows // c.qkv_T
        ix, ixp = vt_index(B, c.H, c.qkv_T, c.qkv_Tp)
        vt_plane = B * c.H * c.qkv_Tp + 12
        outs['vt'] = dict(n=16 + 2 * vt_plane + 16, off=16, idx=16 + ix, pad=16 + ixp, bits=16, plane=vt_plane)
    s.update(lda_src=lda_src, sAct_src=sAct_src, lda=lda, sAct=sAct, ts=ts, rs=rs_, ks=ks, sW=sW, rows=rows, K=K, Wn=Wn, taps=taps,
             tap_shift0=c.tap_shift0, act_is_a=c.act_is_a, batch=c.batch, zdiv=c.zdiv, ldc=ldc, sC=sC, out_plane=out_plane, ldo=ldo, sO=sO,
             sBias=sBias, alpha=c.alpha, alpha_ncols=c.alpha_ncols, act_fn=c.act, ldr=ldr, sR=sR, sRS=sRS, up_u=8 if c.up else 0, up_p=c.up_p,
             up_lout=c.up_lout, qkv_T=c.qkv_T, qkv_Tp=c.qkv_Tp, qkv_H=c.H if c.qkv_T else 0, vt_plane=vt_plane)
    p = Packed(host, off, outs, s, plane_idx, plane_n)
    p.r_idx = r_idx
    return p


# ---- a. the shape sweep: every instantiation at its shape edges -----------------------------------------------------------------------------
ROWS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]
ROWS_T = ROWS + [62, 126]                 # act_is_a = 0: a partial quad of the store along the frames next to a 64- / 128-row tile end
PLAIN_K = {1: [256, 512], 2: [256, 512], 3: [128, 384], 4: [64, 192, 320], 5: [128, 384], 6: [64, 192, 320], 7: [64, 192, 320]}
CONV_TAPS = [17, 17, 3, 5, 9, 2, 3, 5, 9, 17, 3, 5, 9, 3]
INSTANCES = ([(1, conv, f, False) for conv in (False, True) for f in range(1, 8) if not (conv and f == 1)] +
             [(0, conv, f, False) for conv in (False, True) for f in (5, 6, 7)] +
             [(1, False, 1, True), (1, True, 2, True), (1, False, 5, True), (1, True, 5, True), (1, False, 7, True), (1, True, 7, True)])


def inst_id(v):
    a, conv, f, rag = v
    return f"{FORMS[f]}/{'conv' if conv else 'plain'}/{'tok' if a else 'feat'}" + ('/ragged' if rag else '')


def _conv_k(force, taps, j, ragged):
    """K of a conv case: 64 / 128 / 256 in turn where the ring divides K / 16 * taps (a slice's 2 x taps steps then neither divide nor are a
    multiple of the ring for taps 3, 5, 9, 17); ragged: K % 256 == 0."""
    if ragged:
        return 256
    ks = [k for k in (64, 128, 256) if (k // 16 * taps) % RING[force] == 0]
    return ks[j % len(ks)]


def _sweep_lens(rows, batch, j):
    """Ragged shape sweep: the last item full, the others cut (one just below rows, one in the middle, one empty every third case)."""
    pat = [rows, max(rows - 1, 0), rows // 2 if j % 3 else 0]
    return tuple(pat[(batch - 1 - b) % 3] for b in range(batch))


def sweep_cases(inst):
    a, conv, force, ragged = inst
    out = []
    rows_list = ROWS if a else ROWS_T
    for j, rows in enumerate(rows_list):
        taps = CONV_TAPS[j] if conv else 1
        K = _conv_k(force, taps, j, ragged) if conv else ([256, 512][j % 2] if ragged else PLAIN_K[force][j % len(PLAIN_K[force])])
        Wn = [128, 256, 384][j % 3]
        batch = [1, 2, 3][(j // 2) % 3]
        c = Case(rows, Wn, K, taps=taps, shift0=-1 if taps == 2 else None, act_is_a=a, batch=batch, wlayout=('conv' if j % 2 else 'nk') if conv else ('kn' if j % 4 == 3 else 'nk'))
        if ragged:
            c = replace(c, lens=_sweep_lens(rows, batch, j))
        out.append(c.with_all())
    # 2 x 2 x 2 whole tiles: a workgroup count that is a multiple of 8 (the XCD remap without a remainder) on every tile height
    t = TILE[force]
    taps = 3 if conv else 1
    c = Case(2 * t, 256, _conv_k(force, taps, 2, ragged) if conv else (256 if ragged else PLAIN_K[force][-1]), taps=taps, act_is_a=a, batch=2)
    out.append((replace(c, lens=(2 * t, 2 * t - 1)) if ragged else c).with_all())
    if conv:   # the weight-stationary XCD remap: (Wn / 128) % 8 == 0 with taps > 1
        c = Case(33, 1024, _conv_k(force, 3, 1, ragged), taps=3, act_is_a=a, batch=2)
        out.append((replace(c, lens=(33, 17)) if ragged else c).with_all())
    if not ragged:   # two weight sets over three activation items: bias by set, R by z, rowscale by activation item
        taps = 5 if conv else 1
        K = _conv_k(force, taps, 1, False) if conv else PLAIN_K[force][0]
        out.append(Case(65, 128, K, taps=taps, act_is_a=a, batch=6, zdiv=3).with_all())
    assert all(form_ok(c, force) for c in out), [c.name for c in out if not form_ok(c, force)]
    return out


# ---- b. epilogues, one option at a time -----------------------------------------------------------------------------------------------------
def epilogue_cases(a):
    out = []
    for base in (Case(128, 128, 128, act_is_a=a, tag='epi:'), Case(77, 128, 128, taps=3, batch=2, act_is_a=a, tag='epi:')):
        out.append(base)
        out.append(replace(base, bias=True))
        out += [replace(base, bias=True, alpha=ALPHA, alpha_ncols=n) for n in (0, 40, base.Wn + 5)]
        out += [replace(base, act=ACT_RELU), replace(base, act=ACT_GELU), replace(base, R=True), replace(base, rowscale=True)]
        out.append(replace(base.with_all(), alpha_ncols=40))
        out += [replace(base, bias=True, ldc_odd=True), replace(base, bias=True, c_off=1), replace(base.with_all(), ldc_odd=True),
                replace(base.with_all(), c_off=1)]
        out += [replace(base, tight=True), replace(base.with_all(), alpha_ncols=40, tight=True)]
    return out


def lds_image_cases():
    """The plain act_is_a = 0 cases of b (nothing but bias / alpha: the direct store), for the child under BSG_H2W_DIRECT=0."""
    return [c for c in epilogue_cases(0) if c.act == ACT_NONE and not c.R and not c.rowscale]


# ---- c. quad outputs of the direct store (the conditioner hoist's pattern) ----------------------------------------------------------------
QUAD_COMBOS = {'C+Cq': dict(Cq=True), 'C+Ch': dict(Ch=True), 'Ch': dict(Ch=True, C=False), 'Cq+Ch+C': dict(Cq=True, Ch=True)}
CH_TIE_CAP = 0.01


def quad_cases(combo):
    return [Case(rows, 512, 256, act_is_a=0, batch=6, zdiv=3, bias=True, alpha=ALPHA, alpha_ncols=256, tag=f'quad:{combo}:', **QUAD_COMBOS[combo])
            for rows in (1, 63, 64, 65, 130)]


def ch_range(want64, bar):
    """bf16 values (as float64) of want - bar and want + bar, rounded to nearest even: a result inside the fp32 bar rounds to a bf16 value
    between the two.  Where the float64 value lies further than `bar` from a rounding boundary both equal its own rounding; within `bar`
    of one they are one bf16 ulp apart (and more than one only where a bf16 ulp is smaller than the bar: |value| < 128 bar)."""
    lo = bf16_value(bf16_rne((want64 - bar).astype(np.float32)))
    hi = bf16_value(bf16_rne((want64 + bar).astype(np.float32)))
    return lo, hi


# ---- d. plane output and the QKV mode -------------------------------------------------------------------------------------------------------
def plane_cases():
    return [replace(Case(77, 256, 128, taps=3, batch=2, out=True, tag='planes:').with_all(), act=ACT_RELU),
            Case(129, 128, 256, batch=3, out=True, bias=True, tag='planes:'), Case(64, 128, 64, out=True, tight=True, tag='planes:')]


QKV_T = [1, 3, 4, 31, 32, 33, 64, 65]


def qkv_cases():
    out = []
    for j, T in enumerate(QKV_T):
        for B in (1, 3):
            H = 128 if (j + B) % 2 else 256
            Tp = (T + 31) // 32 * 32 + (32 if (T == 33 and B == 3) else 0)
            out.append(Case(B * T, 3 * H, 256, C=False, out=True, qkv_T=T, qkv_Tp=Tp, bias=True, alpha=ALPHA, alpha_ncols=H, tag=f'qkv:B{B}:T{T}:'))
    return out


# ---- e. polyphase output ---------------------------------------------------------------------------------------------------------------------
UP_LIN = [1, 3, 31, 32, 33, 129]


def up_cases():
    out = []
    for j, Lin in enumerate(UP_LIN):
        for v in range(2):
            Co, K = 16 if (j + v) % 2 else 48, 128 if j % 2 else 512
            p = 4 * ((j + v) % 2)
            lout = 8 * Lin - (3 if v else 0)
            out.append(Case(Lin + 1, 8 * Co, K, taps=2, shift0=-1, act_is_a=0, batch=3 if (j % 3 == v) else 1, bias=v == 0 or j % 2 == 0, up=True, up_p=p,
                            up_lout=lout, ldc_odd=bool((j + v) % 3 == 0), wlayout='nk', tag=f'up:Lin{Lin}:'))
    return out


def up_weights(wt):
    """conv_transpose1d weight [Ci][Co][16] (kernel 16, stride 8) -> W[tap][8 co + r][ci] = wt[ci][co][r + 8 (1 - tap)] of the 2-tap product."""
    Ci, Co, k = wt.shape
    assert k == 16
    W = np.zeros((2, 8 * Co, Ci), wt.dtype)
    for tap in range(2):
        for r in range(8):
            W[tap, r::8, :] = wt[:, :, r + 8 * (1 - tap)].T
    return W


# ---- f. ragged -----------------------------------------------------------------------------------------------------------------------------
RAGGED_FORMS = [(False, 1), (True, 2), (False, 5), (True, 5), (False, 7), (True, 7)]


def ragged_cases(conv, force):
    """lens at the seams of the tile height: 0, 1, tile - 1, tile, tile + 1, rows - 1, rows — one batch item each."""
    t = TILE[force]
    rows = 2 * t + 3
    lens = (0, 1, t - 1, t, t + 1, rows - 1, rows)
    base = Case(rows, 128, 256, taps=9 if conv else 1, batch=len(lens), lens=lens, tag='rag:')
    return [replace(base, bias=True), replace(base.with_all(), out=True)]


def ragged_qkv_case(force):
    t = TILE[force]
    T = 2 * t + 4
    lens = (T, t + 1, 1, 0, T - 1, t)
    return Case(T, 384, 256, batch=len(lens), lens=lens, C=False, out=True, qkv_T=T, qkv_Tp=(T + 31) // 32 * 32, bias=True, alpha=ALPHA, alpha_ncols=128,
                tag='rag:qkv:')


def zeroed(c, ops):
    """The non-ragged twin of a ragged case: the activation zeroed from lens[z] on (rowscale and R stay; the epilogue's own zeroing is the
    ragged kernel's, so only rows < lens[z] are compared)."""
    o = dict(ops)
    a = ops['act'].copy()
    for za, n in enumerate(c.lens):
        a[za, n:] = 0
    o['act'] = a
    if c.qkv_T:   # without lengths the QKV mode takes ONE batch item of B * T rows: the utterances stacked
        o['act'] = a.reshape(1, c.batch * c.rows, c.K)
        return replace(c, lens=None, rows=c.batch * c.rows, batch=1), o
    return replace(c, lens=None), o


# ---- g. the dispatch: both sides of each threshold ---------------------------------------------------------------------------------------------
def dispatch_cases():
    """(case, expected form) at the default switches: tiny = fewer than 256 workgroups of 64-row tiles (act_is_a only), small = fewer than
    512 of 128-row tiles."""
    out = []
    for a in (1, 0):
        out += [(replace(c, tight=True), f) for c, f in [(Case(65, 128, 64, batch=127, act_is_a=a, bias=True, tag='disp:'), 'h2w/32/ring4' if a else 'h2w/64/ring4'),
                (Case(65, 128, 64, batch=128, act_is_a=a, bias=True, tag='disp:'), 'h2w/64/ring4'),
                (Case(1024, 128, 64, batch=63, act_is_a=a, bias=True, tag='disp:'), 'h2w/64/ring4'),
                (Case(1024, 128, 64, batch=64, act_is_a=a, bias=True, tag='disp:'), 'h2w/128/ring4'),
                (Case(40, 128, 256, act_is_a=a, bias=True, tag='disp:'), 'h2w/32/deep' if a else 'h2w/64/ring8'),
                (Case(40, 128, 128, batch=2, act_is_a=a, bias=True, tag='disp:'), 'h2w/32/ring8' if a else 'h2w/64/ring8'),
                (Case(300, 128, 128, batch=64, act_is_a=a, bias=True, tag='disp:'), 'h2w/64/ring8')]      # 320 of 64 rows, 192 of 128: neither tiny nor large
                ]
    return out


def all_cases():
    """Every case of the GPU file (for the CPU checks of layouts and arithmetic)."""
    out = []
    for inst in INSTANCES:
        out += sweep_cases(inst)
    out += epilogue_cases(1) + epilogue_cases(0)
    for combo in QUAD_COMBOS:
        out += quad_cases(combo)
    out += plane_cases() + qkv_cases() + up_cases()
    for conv, force in RAGGED_FORMS:
        out += ragged_cases(conv, force)
    out += [ragged_qkv_case(f) for f in (1, 5, 7)]
    out += [c for c, _ in dispatch_cases()]
    return list(dict.fromkeys(out))
