// DiffNet (WaveNet noise predictor) on gfx950 — the >97 %-of-FLOPs hot loop of BiSinger's mel generation.
//
// Reference semantics: /root/reference/train_bisinger/usr/diff/net.py
//   ResidualBlock.forward :66-78, DiffNet.forward :107-130, SinusoidalPosEmb :32-44.
//
// One launch of residual_layer_kernel computes a whole ResidualBlock for a tile of N_TILE frames of one
// utterance, with every intermediate ([2C,T] pre-activation, gated z, [2C,T] output projection) kept on
// chip:
//
//   stage  xs = x[:, t0-8 : t0+N_TILE+8] + diffusion_projection(step)   (zero outside [0,T): the conv's
//          zero padding pads x + d, net.py:69-71)                                       -> LDS  [C][N_TILE+16]
//   GEMM1  y = W_dil[2C x 3C] * im2col(xs)  (3 dilated taps = 3 shifted reads of the same LDS image),
//          accumulators initialised with the step-invariant conditioner term (hoisted to prepare()),
//          v_mfma_f32_32x32x2_f32, A fragments streamed from L2 in pre-packed fragment order (one
//          global_load_dwordx4 per lane = 4 k-steps), B fragments = conflict-free ds_read_b32 rows.
//   gate   z = sigmoid(y[:C]) * tanh(y[C:])  in registers (a wave owns gate rows c and filter rows C+c)
//          -> LDS [C][N_TILE] (aliases xs)
//   GEMM2  o = W_out[2C x C] * z ; residual half: x_out = (x + o)/sqrt(2) ; skip half: skip += o
//
// 8 waves per workgroup, each a 32-row slice of the gate/filter (GEMM1) and residual/skip (GEMM2) rows.  Algorithmic work:
// 2*(2C*3C + 2C*C) = 1,048,576 FLOP per frame per layer (C = 256); algorithmic HBM bytes per frame per
// layer = 6*C*4 = 6 KB (x in, x out, conditioner term 2C, skip read+write)  -> AI = 171 FLOP/B: bound by
// the fp32 MFMA roof (157.3 TFLOP/s), not HBM.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "bsg_common.h"
#include "bsg_ws.h"
#include "diffnet_res.h"
#include "diffnet_tail.h"
#include "diffnet_forms.h"

namespace bsg {

namespace {


// ------------------------------------------------------------------------------------------------
// weight packing: out[((mt*(K/8) + q)*64 + lane)*4 + j] = W(m = 32*mt + (lane&31), k = 8*q + 2*j + (lane>>5))
// with W(m,k) at src[m*sm + (k % Kc)*sc + (k / Kc)*st]  (dilated conv: k = tap*C + ci, src [2C][C][3]).
// ------------------------------------------------------------------------------------------------
__global__ void pack_a_frag_kernel(const float* __restrict__ src, float* __restrict__ out, int M, int K, int Kc,
                                   long long sm, long long sc, long long st) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)M * K;
  if (i >= total) return;
  const int j = (int)(i & 3);
  const int lane = (int)((i >> 2) & 63);
  const long long rest = i >> 8;
  const int Kq = K / 8;
  const int q = (int)(rest % Kq);
  const int mt = (int)(rest / Kq);
  const int m = 32 * mt + (lane & 31);
  const int k = 8 * q + 2 * j + (lane >> 5);
  out[i] = src[(long long)m * sm + (long long)(k % Kc) * sc + (long long)(k / Kc) * st];
}

// Winograd F(2,3) weights of the k=3 dilated conv, in 16x16x4 A-fragment order:
//   U0 = w0, U1 = (w0+w1+w2)/2, U2 = (w0-w1+w2)/2, U3 = w2;   out[comp][mt16][q][lane][jj] = U_comp(m, k),
//   m = 16*mt16 + (lane&15), k = 16*q + 4*jj + (lane>>4)       (src [2C][C][3])
__global__ void pack_wino_kernel(const float* __restrict__ w, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * 2 * C * C) return;
  const int jj = i & 3, lane = (i >> 2) & 63, rest = i >> 8;
  const int q = rest & 15, mt = (rest >> 4) & 31, comp = rest >> 9;
  const int m = 16 * mt + (lane & 15), k = 16 * q + 4 * jj + (lane >> 4);
  const float* p = w + ((long long)m * C + k) * 3;
  const float w0 = p[0], w1 = p[1], w2 = p[2];
  float u;
  if (comp == 0) u = w0;
  else if (comp == 1) u = (w0 + w1 + w2) * 0.5f;
  else if (comp == 2) u = (w0 - w1 + w2) * 0.5f;
  else u = w2;
  out[i] = u;
}

__global__ void vec_add_kernel(const float* a, const float* b, float* o, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = a[i] + b[i];
}

// ------------------------------------------------------------------------------------------------
// fused residual block
// ------------------------------------------------------------------------------------------------

#define BSG_STAMP(i)                                                                                   \
  do {                                                                                                 \
    if (STAMP) {                                                                                       \
      __builtin_amdgcn_sched_barrier(0);                                                               \
      const unsigned long long _t = __builtin_amdgcn_s_memtime();                                      \
      __builtin_amdgcn_s_waitcnt(0xC07F);                                                              \
      if (lane == 0) a.stamps[((long long)tile_id * 8 + wave) * 10 + (i)] = _t;                      \
      __builtin_amdgcn_sched_barrier(0);                                                               \
    }                                                                                                  \
  } while (0)

#define BSG_MFMA8(ACC0, ACC1, A0_, A1_, B_)                                                  \
  ACC0 = __builtin_amdgcn_mfma_f32_32x32x2f32(A0_[0], B_[0], ACC0, 0, 0, 0);                  \
  ACC1 = __builtin_amdgcn_mfma_f32_32x32x2f32(A1_[0], B_[0], ACC1, 0, 0, 0);                  \
  ACC0 = __builtin_amdgcn_mfma_f32_32x32x2f32(A0_[1], B_[1], ACC0, 0, 0, 0);                  \
  ACC1 = __builtin_amdgcn_mfma_f32_32x32x2f32(A1_[1], B_[1], ACC1, 0, 0, 0);                  \
  ACC0 = __builtin_amdgcn_mfma_f32_32x32x2f32(A0_[2], B_[2], ACC0, 0, 0, 0);                  \
  ACC1 = __builtin_amdgcn_mfma_f32_32x32x2f32(A1_[2], B_[2], ACC1, 0, 0, 0);                  \
  ACC0 = __builtin_amdgcn_mfma_f32_32x32x2f32(A0_[3], B_[3], ACC0, 0, 0, 0);                  \
  ACC1 = __builtin_amdgcn_mfma_f32_32x32x2f32(A1_[3], B_[3], ACC1, 0, 0, 0);

// Software-pipelined MFMA stream over two row tiles that share the B fragment.  Group q = 4 k-steps = 8 MFMAs.
// A fragments live in a ring of NS register sets: set s holds group q+s and is refilled with group q+s+NS right
// after its MFMAs have issued, i.e. NS-1 groups (>= 512 cycles each) before it is needed again; the B fragment of
// the next group is read from LDS while the current group multiplies.  sched_barrier pins this order: left alone,
// hipcc sinks the refills next to their consumers and every trip waits a full L2 latency.
template <int NS, typename LDB>
__device__ __forceinline__ void mfma_pipe(f32x16& acc0, f32x16& acc1, f32x4 (&A0)[NS], f32x4 (&A1)[NS], rsrc_t rs, int vfrag,
                                          int sa0, int sa1, int q_begin, int q_end, int q_last, LDB ldb) {
  f32x4 Bf[2];
  Bf[0] = ldb(q_begin);
#pragma unroll 1
  for (int q = q_begin; q < q_end; q += NS) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int qn = q + s + 1 <= q_last ? q + s + 1 : q_last;
      Bf[(s + 1) & 1] = ldb(qn);
      __builtin_amdgcn_sched_barrier(0);
      BSG_MFMA8(acc0, acc1, A0[s], A1[s], Bf[s & 1])
      __builtin_amdgcn_sched_barrier(0);
      const int qr = q + s + NS <= q_last ? q + s + NS : q_last;
      A0[s] = ldf4(rs, vfrag, sa0 + qr * 1024);
      A1[s] = ldf4(rs, vfrag, sa1 + qr * 1024);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// GEMM1 of the residual block as Winograd F(2,3) over the dilated taps, for one wave: 4 row tiles of 16 (sw[] = their byte
// offsets in the packed Winograd weights) x 16 output pairs, K = 4 components x 256 channels.
//   y0 += M0 + M1 + M2   (output frame t of the pair),   y1 += M1 - M2 - M3   (frame t + d),   M_comp = U_comp * V_comp
//   V0 = x[t-d] - x[t+d],  V1 = x[t] + x[t+d],  V2 = x[t+d] - x[t],  V3 = x[t] - x[t+2d]     (x = the staged, zero-padded xs)
// The B fragment of group (comp, q) — channels 16 q + 4 jj + lq — is formed in registers: V = x[xo + oa] + sgn * x[xo + ob], one FMA
// with sgn = +-1 (the exact sum / difference).  Loop structure: components outside, the 16 channel groups inside, so that inside
// the loop the LDS addresses are two running offsets plus immediates and a group costs NO address arithmetic (the first form
// of this loop recomputed component, offsets and sign per group: ~15 scalar / vector instructions between two MFMA blocks, which
// a lone workgroup on a CU — 2 waves per SIMD — could not hide: GEMM1 phase 58 -> 43 us per layer in the stack launch).  The
// last group of a component prefetches the first of the next one (peeled tail).  One block = 16 MFMAs (v_mfma_f32_16x16x4_f32);
// the next group's LDS reads are issued before them (their latency passes under the MFMAs), its transform and the weight loads
// of the group NR ahead behind them; sched_barrier pins that order.  On entry AW[0..NR) hold the weights of groups 0..NR-1.
// ------------------------------------------------------------------------------------------------
template <int NTI, int NR>   // NTI row tiles of 16 per wave (sw[] = their byte offsets), NR = depth of the weight ring (groups in flight)
__device__ __forceinline__ void wino_gemm1(f32x4 (&y0)[NTI], f32x4 (&y1)[NTI], f32x4 (&AW)[NR][NTI], const float* xs, const int xo, const int dil,
                                           const rsrc_t rs_aw, const int vfrag, const int (&sw)[NTI]) {
  constexpr int LDX = 32 + 2 * HALO;
  static_assert(NR == 2 || NR == 4, "ring depth");
  f32x4 M[NTI];
#pragma unroll
  for (int i = 0; i < NTI; ++i) M[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto offs = [&](int comp, int& oa, int& ob, float& sgn) {
    oa = xo + ((comp == 2) - (comp == 0)) * dil;
    ob = xo + ((comp < 2) + 2 * (comp == 3)) * dil;
    sgn = comp == 1 ? 1.0f : -1.0f;
  };
  // byte offset of group g's weights inside a row tile of the packed matrix [comp][32 tiles][16 q][64 lanes][4] (clamped: a repeat at the end)
  auto wso = [](int g) {
    g = g < 63 ? g : 63;
    return ((g >> 4) * 512 + (g & 15)) * 1024;
  };
  auto block = [&](f32x4 (&A)[NTI], const f32x4& Bcur, f32x4& Bnext, int ia, int ib, float sgn, int so) {
    f32x4 ra, rb;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) { ra[jj] = xs[ia + 4 * jj * LDX]; rb[jj] = xs[ib + 4 * jj * LDX]; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int i = 0; i < NTI; ++i) M[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[i][jj], Bcur[jj], M[i], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) Bnext[jj] = __builtin_fmaf(sgn, rb[jj], ra[jj]);
#pragma unroll
    for (int i = 0; i < NTI; ++i) A[i] = ldf4(rs_aw, vfrag, sw[i] + so);
    __builtin_amdgcn_sched_barrier(0);
  };
  f32x4 Bw[2];
  int na, nb;
  float nsgn;
  offs(0, na, nb, nsgn);
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) Bw[0][jj] = __builtin_fmaf(nsgn, xs[nb + 4 * jj * LDX], xs[na + 4 * jj * LDX]);
#pragma unroll 1
  for (int comp = 0; comp < 4; ++comp) {
    int ia = na + 16 * LDX, ib = nb + 16 * LDX;   // group q + 1 of this component
    const float sgn = nsgn;
    offs(comp < 3 ? comp + 1 : 3, na, nb, nsgn);
    int g = comp * 16 + NR;                       // group whose weights the first block requests
#pragma unroll 1
    for (int q = 0; q < 16 - NR; q += NR) {
#pragma unroll
      for (int s = 0; s < NR; ++s) block(AW[s], Bw[s & 1], Bw[(s + 1) & 1], ia + 16 * s * LDX, ib + 16 * s * LDX, sgn, wso(g + s));
      ia += 16 * NR * LDX; ib += 16 * NR * LDX; g += NR;
    }
#pragma unroll
    for (int s = 0; s < NR - 1; ++s) block(AW[s], Bw[s & 1], Bw[(s + 1) & 1], ia + 16 * s * LDX, ib + 16 * s * LDX, sgn, wso(g + s));
    block(AW[NR - 1], Bw[(NR - 1) & 1], Bw[NR & 1], na, nb, nsgn, wso(g + NR - 1));   // (comp, 15) reads (comp + 1, 0)
    // the component is complete (FMAs with 0 / +-1: exact, branch-free)
    const float c0 = comp < 3 ? 1.0f : 0.0f, c1 = comp == 1 ? 1.0f : comp >= 2 ? -1.0f : 0.0f;
#pragma unroll
    for (int i = 0; i < NTI; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        y0[i][r] = __builtin_fmaf(c0, M[i][r], y0[i][r]);
        y1[i][r] = __builtin_fmaf(c1, M[i][r], y1[i][r]);
        M[i][r] = 0.f;
      }
  }
}

// One workgroup = 8 waves = one 32-frame tile of one utterance; wave w owns gate rows [32w,32w+32) and filter
// rows [256+32w, ...) in GEMM1 and residual rows [32w, ...) + skip rows [256+32w, ...) in GEMM2.
// Both GEMM loops are software-pipelined by hand: A fragments (global, L2) are requested a full 8-MFMA group
// before use and B fragments (LDS) one group before use; sched_barrier pins that order (left alone, hipcc
// sinks the prefetch loads next to their consumers, which exposes the L2 latency on every trip).
template <bool STAMP, int NS, bool WINO>   // NS: depth of the A-fragment ring of GEMM2 (and of GEMM1 when !WINO); WINO: GEMM1 as
                                         // Winograd F(2,3) over the dilated taps (2/3 of the MFMA work)
__device__ __forceinline__ void residual_tile(const ResArgs& a, const int tile_id) {
  constexpr int NT = 32;               // frames per workgroup
  constexpr int LDX = NT + 2 * HALO;   // xs row stride (48 floats = 12 x 16 B)
  constexpr int LDZ = NT;              // zs row stride

  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;
  float* zs = lds;  // aliases xs after the barrier that ends GEMM1

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lh = lane >> 5;
  const int b = tile_id / a.tiles_per_row;
  const int t0 = (tile_id - b * a.tiles_per_row) * NT;
  const int T = a.T;
  const int tb = a.t_dev ? (int)a.t_dev[b] : a.t_uniform;
  const int col = t0 + l31;            // this lane's frame in every accumulator tile
  const bool col_ok = col < T;
  const int colc = col_ok ? col : T - 1;   // clamped: loads stay unconditional, results are masked

  const unsigned plane = (unsigned)C * T * 4;
  const rsrc_t rs_x = mk_rsrc(a.x_in + (long long)b * C * T, plane);
  const rsrc_t rs_xo = mk_rsrc(a.x_out + (long long)b * C * T, plane);
  const rsrc_t rs_sk = mk_rsrc(a.skip + (long long)b * C * T, plane);
  const rsrc_t rs_ct = mk_rsrc(a.condterm + (long long)b * 2 * C * T, 2 * plane);
  const rsrc_t rs_a1 = mk_rsrc(a.apack1, 2 * C * 3 * C * 4);
  const rsrc_t rs_a2 = mk_rsrc(a.apack2, 2 * C * C * 4);
  const rsrc_t rs_bo = mk_rsrc(a.bias_out, 2 * C * 4);
  const rsrc_t rs_dp = mk_rsrc(a.dproj + ((long long)tb * a.L + a.layer) * C, C * 4);
  const int vcol = (lh * 4 * T + colc) * 4;   // per-lane byte offset inside a [rows][T] plane (row half + frame)
  const int rowT = T * 4;                     // bytes per row
  const int vfrag = lane * 16;                // per-lane byte offset inside a packed 1-KB A fragment group

  BSG_STAMP(0);
  if (STAMP && lane == 0) a.stamps[((long long)tile_id * 8 + wave) * 10 + 8] = __builtin_amdgcn_s_memrealtime();
  // ---- (1) the first A fragments fly while the x tile is staged ------------------------------------
  f32x16 acc0, acc1;
  f32x4 Ag[NS], Af[NS];
  const int sa_g = wave * 96 * 1024, sa_f = (8 + wave) * 96 * 1024;   // gate / filter tile of the packed dilated conv
  // Winograd: 4 row tiles of 16 (gate 32w..+15, gate +16, filter 256+32w.., filter +16), ring of 2 groups
  const rsrc_t rs_aw = mk_rsrc(a.apackw, 4 * 2 * C * C * 4);
  f32x4 AW[2][4];
  int sw[4];
  if constexpr (WINO) {
    sw[0] = (2 * wave) * 16 * 1024; sw[1] = (2 * wave + 1) * 16 * 1024;
    sw[2] = (16 + 2 * wave) * 16 * 1024; sw[3] = (16 + 2 * wave + 1) * 16 * 1024;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int i = 0; i < 4; ++i) AW[k][i] = ldf4(rs_aw, vfrag, sw[i] + k * 1024);
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      Ag[k] = ldf4(rs_a1, vfrag, sa_g + k * 1024);
      Af[k] = ldf4(rs_a1, vfrag, sa_f + k * 1024);
    }
  }

  // ---- (2) stage xs = x + d (zero padded) ------------------------------------------------------
  if ((T & 3) == 0) {
    // 256 rows x 12 float4; a float4 is entirely inside or entirely outside [0,T)
#pragma unroll 3
    for (int k = 0; k < 6; ++k) {
      const int idx = tid + 512 * k;
      const int c = idx / 12, j4 = idx - c * 12;
      const int t = t0 - HALO + 4 * j4;
      const bool ok = t >= 0 && t < T;
      f32x4 v = ldf4(rs_x, ok ? (c * T + t) * 4 : 0, 0);
      const float d = ldf(rs_dp, c * 4, 0);
      v += d;
      if (!ok) v = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(xs + c * LDX + 4 * j4) = v;
    }
  } else {
#pragma unroll 4
    for (int idx = tid; idx < C * LDX; idx += 512) {
      const int c = idx / LDX, j = idx - c * LDX;
      const int t = t0 - HALO + j;
      const bool ok = t >= 0 && t < T;
      const float v = ldf(rs_x, ok ? (c * T + t) * 4 : 0, 0) + ldf(rs_dp, c * 4, 0);
      xs[idx] = ok ? v : 0.f;
    }
  }
  // Winograd form (registers to spare below its 128-VGPR budget): the residual input x of this wave's rows — the initial
  // accumulator of GEMM2 — is requested together with the staging loads, while the tile's lines are in flight / L2-hot, instead
  // of after the gate (≈50 us later, when they have left L2 and cost 16 MB of fabric reads per launch a second time)
  if constexpr (WINO) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = ldf(rs_x, vcol, (32 * wave + acc_row0(r)) * rowT);
  }
  __syncthreads();
  BSG_STAMP(1);

  float z[16];
  int zoff[16];   // LDS element offsets of z[] (compile-time pattern + per-lane part; folded by the compiler)
  if constexpr (!WINO) {
    // ---- (3) GEMM1: y = W_dil * im2col(xs): 96 groups of 8 MFMAs ----------------------------------
    {
      const float* xrow = xs + lh * LDX + HALO + l31;
      const int dil = a.dil;
      auto ldb = [&](int q) {
        const int tap = q >> 5, cg = q & 31;
        const float* p = xrow + 8 * cg * LDX + (tap - 1) * dil;
        return f32x4{p[0], p[2 * LDX], p[4 * LDX], p[6 * LDX]};
      };
      BSG_STAMP(2);
      mfma_pipe<NS>(acc0, acc1, Ag, Af, rs_a1, vfrag, sa_g, sa_f, 0, 96, 95, ldb);
    }
    BSG_STAMP(3);
    // ---- (4) + hoisted conditioner term, gate: z = sigmoid(gate) * tanh(filter)   (net.py:71-74) --------
    // The 64 KB/workgroup conditioner tile is the largest HBM stream of the layer.  It is requested here, not at
    // kernel start: all workgroups of a launch start together, and 32 MB requested at t=0 by an idle chip costs
    // ~15k cycles with the MFMA pipe empty; by now the co-resident workgroups have drifted apart, so this
    // latency hides under their MFMA work.
    float cg[16], cf[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      cg[r] = ldf(rs_ct, vcol, (32 * wave + acc_row0(r)) * rowT);
      cf[r] = ldf(rs_ct, vcol, (C + 32 * wave + acc_row0(r)) * rowT);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      z[r] = fast_sigmoid(acc0[r] + cg[r]) * fast_tanh(acc1[r] + cf[r]);
      zoff[r] = (32 * wave + acc_row(r, lh)) * LDZ + l31;
    }
  } else {
    // ---- (3w) GEMM1 as Winograd F(2,3) along the dilated taps -------------------------------------
    // For the output pair (t, t+d):  y[t] = M0+M1+M2,  y[t+d] = M1-M2-M3,  M_j = sum_c U_j[.,c] * V_j[c], with
    //   V0 = x[t-d]-x[t+d], V1 = x[t]+x[t+d], V2 = x[t+d]-x[t], V3 = x[t]-x[t+2d]   (x = the staged, zero-padded tile)
    // 4 GEMMs of K = 256 over 16 pairs instead of one of K = 768 over 32 frames: 2/3 of the MFMA work.  16x16x4 MFMAs
    // (N = 16 pairs); lane = (pair p = lane&15, k-row lq = lane>>4); pair p of dilation d sits at tp = (p/d)*2d + p%d.
    const int p16 = lane & 15, lq = lane >> 4, dil = a.dil;
    const int ld = dil == 1 ? 0 : dil == 2 ? 1 : dil == 4 ? 2 : 3;
    const int tp = ((p16 >> ld) << (ld + 1)) + (p16 & (dil - 1));
    f32x4 y0[4], y1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) y0[i] = y1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    BSG_STAMP(2);
    wino_gemm1<4, 2>(y0, y1, AW, xs, lq * LDX + HALO + tp, dil, rs_aw, vfrag, sw);
    BSG_STAMP(3);
    // ---- (4w) + hoisted conditioner term, gate ----------------------------------------------------
    const int f0c = t0 + tp < T ? t0 + tp : T - 1, f1c = t0 + tp + dil < T ? t0 + tp + dil : T - 1;
    const int vc0 = (lq * 4 * T + f0c) * 4, vc1 = (lq * 4 * T + f1c) * 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int so_g = (32 * wave + 16 * i + r) * rowT, so_f = so_g + C * rowT;
        const float cg0 = ldf(rs_ct, vc0, so_g), cf0 = ldf(rs_ct, vc0, so_f);
        const float cg1 = ldf(rs_ct, vc1, so_g), cf1 = ldf(rs_ct, vc1, so_f);
        z[i * 8 + r] = fast_sigmoid(y0[i][r] + cg0) * fast_tanh(y0[2 + i][r] + cf0);
        z[i * 8 + 4 + r] = fast_sigmoid(y1[i][r] + cg1) * fast_tanh(y1[2 + i][r] + cf1);
        zoff[i * 8 + r] = (32 * wave + 16 * i + 4 * lq + r) * LDZ + tp;
        zoff[i * 8 + 4 + r] = (32 * wave + 16 * i + 4 * lq + r) * LDZ + tp + dil;
      }
  }
  BSG_STAMP(4);
  // loads GEMM2 needs first fly across the two barriers: its first A fragments and the residual input x,
  // which becomes the initial accumulator of the residual rows (x + b_out + W_out z, then / sqrt(2))
  const int sb_r = wave * 32 * 1024, sb_s = (8 + wave) * 32 * 1024;   // residual / skip tile of the packed output projection
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    Ag[k] = ldf4(rs_a2, vfrag, sb_r + k * 1024);
    Af[k] = ldf4(rs_a2, vfrag, sb_s + k * 1024);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    if constexpr (!WINO) acc0[r] = ldf(rs_x, vcol, (32 * wave + acc_row0(r)) * rowT);
    acc1[r] = ldf(rs_bo, lh * 16, (C + 32 * wave + acc_row0(r)) * 4);
  }
  __syncthreads();  // every wave is done reading xs
#pragma unroll
  for (int r = 0; r < 16; ++r) zs[zoff[r]] = z[r];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc0[r] += ldf(rs_bo, lh * 16, (32 * wave + acc_row0(r)) * 4);
  __syncthreads();
  BSG_STAMP(5);

  // ---- (5) GEMM2: o = W_out * z; residual rows and skip rows share the B fragment ---------------
  float prevs[16];
  {
    const float* zrow = zs + lh * LDZ + l31;
    auto ldb = [&](int q) {
      const float* p = zrow + 8 * q * LDZ;
      return f32x4{p[0], p[2 * LDZ], p[4 * LDZ], p[6 * LDZ]};
    };
    mfma_pipe<NS>(acc0, acc1, Ag, Af, rs_a2, vfrag, sb_r, sb_s, 0, 16, 31, ldb);
    // the running skip sum is added after the chain (keeps the small products out of a large accumulator)
#pragma unroll
    for (int r = 0; r < 16; ++r) prevs[r] = ldf(rs_sk, vcol, (32 * wave + acc_row0(r)) * rowT);
    mfma_pipe<NS>(acc0, acc1, Ag, Af, rs_a2, vfrag, sb_r, sb_s, 16, 32, 31, ldb);
  }
  BSG_STAMP(6);
  if (col_ok) {
    const int vst = (lh * 4 * T + col) * 4;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int so = (32 * wave + acc_row0(r)) * rowT;
      stf(acc0[r] / 1.41421356237309504880f, rs_xo, vst, so);                      // (x + residual) / sqrt(2), net.py:78
      stf(((a.first ? 0.f : prevs[r]) + acc1[r]) / a.skip_div, rs_sk, vst, so);    // running skip sum (/ sqrt(L) last, :126)
    }
  }
  BSG_STAMP(7);
  if (STAMP && lane == 0) a.stamps[((long long)tile_id * 8 + wave) * 10 + 9] = __builtin_amdgcn_s_memrealtime();
}
#undef BSG_MFMA8

template <bool STAMP, bool WINO>
__global__ __launch_bounds__(512, WINO ? 4 : 6) void residual_layer_kernel(ResArgs a) {
  // XCD-aware tile order: workgroup i runs on XCD i % 8; a contiguous run of tiles per XCD lets neighbouring tiles share
  // their halo lines in one L2 (the halo of a tile is its neighbours' core)
  const int n_tiles = a.B * a.tiles_per_row, per_xcd = (n_tiles + 7) >> 3;
  const int tile_id = ((int)blockIdx.x & 7) * per_xcd + ((int)blockIdx.x >> 3);
  if (tile_id >= n_tiles) return;
  residual_tile<STAMP, 2, WINO>(a, tile_id);
}

// ------------------------------------------------------------------------------------------------
// Small launches (B * ceil(T/32) <= the number of CUs): one tile per workgroup leaves most of the chip idle and the layer
// is bound by ONE CU's matrix rate (393 k MFMA cycles per tile over 4 SIMDs = 42 us).  Here a tile is computed by a PAIR
// of workgroups (2*tile, 2*tile + 1), each owning half of the channels:
//   part p: gate rows [128p, 128p+128) + filter rows [256+128p, ...)  ->  z channels [128p, 128p+128)   (Winograd GEMM1)
//   exchange: each part stores its z half to a global scratch tile write-through (sc1), every wave drains (vmcnt(0)),
//             barrier, one relaxed agent-scope flag store (value = launch epoch); one lane polls the partner's flag (bounded),
//             ONE agent-scope acquire, barrier, plain loads of the partner half   (same protocol as the stack launch)
//   part p: residual rows [128p, ...) + skip rows [256+128p, ...) of GEMM2 over all 256 z channels
// Wave w owns ONE 16-row tile (gate/filter, then residual/skip): 16x16x4 MFMAs throughout.  The host only takes this
// path when every workgroup of the launch is resident (2 * tiles <= 2 per CU), so the partner is always running.
// ------------------------------------------------------------------------------------------------
struct SplitArgs {
  ResArgs base;
  const float* apack2w;   // output projection packed for 16x16x4 MFMAs [32 row tiles][16 k-groups][64][4]
  float* zbuf;            // [tiles][C][32] scratch for the z exchange
  unsigned* flags;        // [tiles][parts][parts]: (producer, consumer)
  unsigned* status;       // += 1 for a poll that gave up
  unsigned epoch;         // launch counter (never 0): the value a flag takes in this launch
  int inject;             // fault injection (bsg_diffnet_debug_inject_giveup): consumers give up at once, without waiting
};

// dconv[((s*L + l)*4 + v)*2C + row] = sum_ci w[row][ci][tap] * dproj[s][l][ci] for tap = v < 3, all three taps for v = 3 (fp64 accumulation):
// the share of the step term d (constant over the frames) in dilated_conv_l(x + d), which the 16-row stack launch adds to the conditioner
// term instead of adding d to every frame of its conv image (net.py:67,72-74).  One workgroup per 4 weight rows: the layer's step terms
// [S][C] (padded rows: the threads of a row group read one column of it) and the 4 rows' weights in LDS, a thread per (row, step).
constexpr int DCONV_ROWS = 4, DCONV_SMAX = 128;
__global__ __launch_bounds__(DCONV_ROWS * DCONV_SMAX) void dconv_kernel(const float* __restrict__ w, const float* __restrict__ dproj, float* __restrict__ out,
                                                                           int S, int L, int l) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  float* ds = reinterpret_cast<float*>(lds_raw);            // [DCONV_SMAX][C + 1]: the steps blockIdx.y * DCONV_SMAX ..
  float* ws = ds + (size_t)DCONV_SMAX * (C + 1);            // [DCONV_ROWS][3 C]
  const int tid = threadIdx.x, row0 = blockIdx.x * DCONV_ROWS, s0 = blockIdx.y * DCONV_SMAX;
  const int ns = S - s0 < DCONV_SMAX ? S - s0 : DCONV_SMAX;
  for (int i = tid; i < ns * C; i += blockDim.x) ds[(i / C) * (C + 1) + i % C] = dproj[((long long)(s0 + i / C) * L + l) * C + i % C];
  for (int i = tid; i < DCONV_ROWS * 3 * C; i += blockDim.x) ws[i] = w[(long long)row0 * 3 * C + i];
  __syncthreads();
  const int r = tid / DCONV_SMAX, sl = tid % DCONV_SMAX, st = s0 + sl;
  if (sl >= ns) return;
  double acc[3] = {0.0, 0.0, 0.0};
  const float* wr = ws + r * 3 * C;
  const float* dr = ds + sl * (C + 1);
  for (int ci = 0; ci < C; ++ci) {
    const double d = (double)dr[ci];
    acc[0] += (double)wr[ci * 3] * d;
    acc[1] += (double)wr[ci * 3 + 1] * d;
    acc[2] += (double)wr[ci * 3 + 2] * d;
  }
  float* o = out + ((long long)st * L + l) * 4 * (2 * C) + row0 + r;
  o[0] = (float)acc[0];
  o[2 * C] = (float)acc[1];
  o[2 * 2 * C] = (float)acc[2];
  o[3 * 2 * C] = (float)(acc[0] + acc[1] + acc[2]);
}

// out[((mt*(K/16) + q)*64 + lane)*4 + jj] = W(m = 16*mt + (lane&15), k = 16*q + 4*jj + (lane>>4)),  W row-major [M][K]
__global__ void pack_a16_kernel(const float* __restrict__ w, float* __restrict__ out, int M, int K) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * K) return;
  const int jj = i & 3, lane = (i >> 2) & 63, rest = i >> 8;
  const int KQ = K / 16;
  const int q = rest % KQ, mt = rest / KQ;
  out[i] = w[(long long)(16 * mt + (lane & 15)) * K + 16 * q + 4 * jj + (lane >> 4)];
}

// WIDE = false: the pair form described above (2 workgroups x 8 waves per tile).  WIDE = true: ONE workgroup of 16 waves per
// tile — the same wave program, z exchanged through LDS only — for launches of 129..256 tiles (B = 5..8 at T=1000), where the
// regular launch has one 8-wave workgroup per CU: 4 waves per SIMD instead of 2 for the same matrix work.
// NPART = 4 (launches of <= 64 tiles, B <= 2): four workgroups of 4 waves per tile, each a quarter of the channels; every part
// publishes its z quarter to the three others through per-(producer, consumer) flags.
template <bool WIDE, int NPART>
__global__ __launch_bounds__(WIDE ? 1024 : 1024 / NPART, 4) void residual_split_kernel(SplitArgs s) {
  const ResArgs& a = s.base;
  constexpr int NT = 32, LDX = NT + 2 * HALO, LDZ = 48, NR = 4;   // NR: depth of the A-fragment rings (k-groups)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;
  float* zs = lds;   // [C][LDZ], aliases xs after the barrier that ends GEMM1

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p16 = lane & 15, lq = lane >> 4;
  constexpr int WAVES = WIDE ? 16 : 16 / NPART, NTHR = 64 * WAVES;
  const int tile_id = WIDE ? (int)blockIdx.x : (int)blockIdx.x / NPART;
  const int part = WIDE ? 0 : (int)blockIdx.x % NPART;
  const int b = tile_id / a.tiles_per_row;
  const int t0 = (tile_id - b * a.tiles_per_row) * NT;
  const int T = a.T;
  const int tb = a.t_dev ? (int)a.t_dev[b] : a.t_uniform;

  const unsigned plane = (unsigned)C * T * 4;
  const rsrc_t rs_x = mk_rsrc(a.x_in + (long long)b * C * T, plane);
  const rsrc_t rs_xo = mk_rsrc(a.x_out + (long long)b * C * T, plane);
  const rsrc_t rs_sk = mk_rsrc(a.skip + (long long)b * C * T, plane);
  const rsrc_t rs_ct = mk_rsrc(a.condterm + (long long)b * 2 * C * T, 2 * plane);
  const rsrc_t rs_aw = mk_rsrc(a.apackw, 4 * 2 * C * C * 4);
  const rsrc_t rs_a2 = mk_rsrc(s.apack2w, 2 * C * C * 4);
  const rsrc_t rs_bo = mk_rsrc(a.bias_out, 2 * C * 4);
  const rsrc_t rs_dp = mk_rsrc(a.dproj + ((long long)tb * a.L + a.layer) * C, C * 4);
  const rsrc_t rs_zb = mk_rsrc(s.zbuf + (long long)tile_id * C * NT, C * NT * 4);
  const int rowT = T * 4, vfrag = lane * 16;
  const int gt = WIDE ? wave : WAVES * part + wave;   // this wave's 16-row tile: gate 16gt.., filter C+16gt..; later residual 16gt.., skip C+16gt..

  // ---- (1) first A fragments fly while the x tile is staged ---------------------------------------
  const int sw[2] = {gt * 16 * 1024, (16 + gt) * 16 * 1024};
  f32x4 AW[NR][2];
#pragma unroll
  for (int k = 0; k < NR; ++k)
#pragma unroll
    for (int i = 0; i < 2; ++i) AW[k][i] = ldf4(rs_aw, vfrag, sw[i] + k * 1024);

  // ---- (2) stage xs = x + d (zero padded), as residual_tile ---------------------------------------
  if ((T & 3) == 0) {
#pragma unroll 3
    for (int k = 0; k < 3072 / NTHR; ++k) {
      const int idx = tid + NTHR * k;
      const int c = idx / 12, j4 = idx - c * 12;
      const int t = t0 - HALO + 4 * j4;
      const bool ok = t >= 0 && t < T;
      f32x4 v = ldf4(rs_x, ok ? (c * T + t) * 4 : 0, 0);
      const float d = ldf(rs_dp, c * 4, 0);
      v += d;
      if (!ok) v = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(xs + c * LDX + 4 * j4) = v;
    }
  } else {
#pragma unroll 4
    for (int idx = tid; idx < C * LDX; idx += NTHR) {
      const int c = idx / LDX, j = idx - c * LDX;
      const int t = t0 - HALO + j;
      const bool ok = t >= 0 && t < T;
      const float v = ldf(rs_x, ok ? (c * T + t) * 4 : 0, 0) + ldf(rs_dp, c * 4, 0);
      xs[idx] = ok ? v : 0.f;
    }
  }
  __syncthreads();

  // ---- (3) GEMM1, Winograd F(2,3) over the dilated taps (see residual_tile), one gate + one filter tile of 16 rows ----
  const int dil = a.dil;
  const int ld = dil == 1 ? 0 : dil == 2 ? 1 : dil == 4 ? 2 : 3;
  const int tp = ((p16 >> ld) << (ld + 1)) + (p16 & (dil - 1));
  f32x4 y0[2], y1[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) y0[i] = y1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  wino_gemm1<2, NR>(y0, y1, AW, xs, lq * LDX + HALO + tp, dil, rs_aw, vfrag, sw);
  // ---- (4) + conditioner term, gate --------------------------------------------------------------------
  float z0[4], z1[4];
  {
    const int f0c = t0 + tp < T ? t0 + tp : T - 1, f1c = t0 + tp + dil < T ? t0 + tp + dil : T - 1;
    const int vc0 = (lq * 4 * T + f0c) * 4, vc1 = (lq * 4 * T + f1c) * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int so_g = (16 * gt + r) * rowT, so_f = so_g + C * rowT;
      const float cg0 = ldf(rs_ct, vc0, so_g), cf0 = ldf(rs_ct, vc0, so_f);
      const float cg1 = ldf(rs_ct, vc1, so_g), cf1 = ldf(rs_ct, vc1, so_f);
      z0[r] = fast_sigmoid(y0[0][r] + cg0) * fast_tanh(y0[1][r] + cf0);
      z1[r] = fast_sigmoid(y1[0][r] + cg1) * fast_tanh(y1[1][r] + cf1);
    }
  }
  // loads GEMM2 needs first: its A fragments, the residual input (initial accumulator) and the biases
  const int sr = gt * 16 * 1024, ss = (16 + gt) * 16 * 1024;
  f32x4 AR[NR], AS[NR];
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    AR[k] = ldf4(rs_a2, vfrag, sr + k * 1024);
    AS[k] = ldf4(rs_a2, vfrag, ss + k * 1024);
  }
  int vcol[2];
  bool col_ok[2];
  f32x4 accR[2], accS[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int col = t0 + 16 * ct + p16;
    col_ok[ct] = col < T;
    vcol[ct] = (lq * 4 * T + (col_ok[ct] ? col : T - 1)) * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      accR[ct][r] = ldf(rs_x, vcol[ct], (16 * gt + r) * rowT) + ldf(rs_bo, lq * 16, (16 * gt + r) * 4);
      accS[ct][r] = ldf(rs_bo, lq * 16, (C + 16 * gt + r) * 4);
    }
  }
  __syncthreads();   // every wave is done reading xs
  // ---- (5) z: own half -> LDS and (write-through) -> the exchange tile; partner half <- exchange tile ------
  if constexpr (WIDE) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * gt + 4 * lq + r;
      zs[row * LDZ + tp] = z0[r];
      zs[row * LDZ + tp + dil] = z1[r];
    }
    __syncthreads();
  } else {
  {
    const int vz = ((4 * lq) * NT + tp) * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * gt + 4 * lq + r;
      zs[row * LDZ + tp] = z0[r];
      zs[row * LDZ + tp + dil] = z1[r];
      if (s.inject && part == 0) continue;   // injected fault: part 0 never publishes, its partners consume whatever the tile held
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, z0[r]), rs_zb, vz, (16 * gt + r) * NT * 4, 16);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, z1[r]), rs_zb, vz + dil * 4, (16 * gt + r) * NT * 4, 16);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    // flags[tile][producer][consumer]: a producer publishes to each of the other parts; a consumer clears what it has consumed,
    // so that a replay of this very launch (a captured graph holding a single layer launch replays the same epoch) cannot match
    // a stale value; the producer sets it again only in a later launch
    unsigned* f = s.flags + (long long)tile_id * (NPART * NPART);
#pragma unroll
    for (int o = 0; o < NPART; ++o)
      if (o != part) __hip_atomic_store(f + part * NPART + o, s.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int o = 0; o < NPART; ++o) {
      if (o == part) continue;
      unsigned spins = s.inject ? (1u << 22) : 0u;   // injected fault: the first failed poll gives up (or none is made at all)
      if (s.inject) atomicAdd(s.status, 1u);
      while (!s.inject && __hip_atomic_load(f + o * NPART + part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != s.epoch) {
        __builtin_amdgcn_s_sleep(2);
        // ~ seconds: never reached unless a partner is not resident; once any wait of this handle has given up (status != 0: the host
        // repeats the call without hand-offs anyway) the others stop within a thousand polls
        if (++spins > (1u << 22) || ((spins & 1023u) == 0u && __hip_atomic_load(s.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
          atomicAdd(s.status, 1u);
          break;
        }
      }
      __hip_atomic_store(f + o * NPART + part, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  {
    // the other parts' channels: (NPART-1) * C/NPART rows of 8 float4
    constexpr int CP = C / NPART, ITEMS = (NPART - 1) * CP * 8;
#pragma unroll
    for (int k = 0; k < ITEMS / NTHR; ++k) {
      const int idx = tid + NTHR * k;
      int c = idx >> 3;
      const int j4 = idx & 7;
      c += c >= part * CP ? CP : 0;   // skip the own block
      *reinterpret_cast<f32x4*>(zs + c * LDZ + 4 * j4) = ldf4(rs_zb, (c * NT + 4 * j4) * 4, 0);
    }
  }
  __syncthreads();
  }
  // ---- (6) GEMM2: residual tile + skip tile of 16 rows x 2 column tiles of 16 frames -------------------------
  {
    const float* zb = zs + lq * LDZ + p16;
    auto ldbz = [&](int q, int ct) {
      const float* p = zb + 16 * q * LDZ + 16 * ct;
      return f32x4{p[0], p[4 * LDZ], p[8 * LDZ], p[12 * LDZ]};
    };
    f32x4 Bz[2][2];
    Bz[0][0] = ldbz(0, 0);
    Bz[0][1] = ldbz(0, 1);
#pragma unroll 1
    for (int q = 0; q < 16; q += NR) {
#pragma unroll
      for (int s2 = 0; s2 < NR; ++s2) {
        const int qn = q + s2 + 1 < 16 ? q + s2 + 1 : 15;
        Bz[(s2 + 1) & 1][0] = ldbz(qn, 0);
        Bz[(s2 + 1) & 1][1] = ldbz(qn, 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          accR[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(AR[s2][jj], Bz[s2 & 1][0][jj], accR[0], 0, 0, 0);
          accS[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(AS[s2][jj], Bz[s2 & 1][0][jj], accS[0], 0, 0, 0);
          accR[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(AR[s2][jj], Bz[s2 & 1][1][jj], accR[1], 0, 0, 0);
          accS[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(AS[s2][jj], Bz[s2 & 1][1][jj], accS[1], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        const int qr = q + s2 + NR < 16 ? q + s2 + NR : 15;
        AR[s2] = ldf4(rs_a2, vfrag, sr + qr * 1024);
        AS[s2] = ldf4(rs_a2, vfrag, ss + qr * 1024);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  // ---- (7) epilogue --------------------------------------------------------------------------------
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    float prevs[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) prevs[r] = a.first ? 0.f : ldf(rs_sk, vcol[ct], (16 * gt + r) * rowT);
    if (col_ok[ct]) {
      const int vst = (lq * 4 * T + t0 + 16 * ct + p16) * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int so = (16 * gt + r) * rowT;
        stf(accR[ct][r] / 1.41421356237309504880f, rs_xo, vst, so);   // (x + residual) / sqrt(2), net.py:78
        stf((prevs[r] + accS[ct][r]) / a.skip_div, rs_sk, vst, so);   // running skip sum (/ sqrt(L) last, :126)
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Stack launches: all L residual layers of a group of rows in ONE launch with the residual stream on chip (diffnet_h2.hip: split-fp16
// form, the fp32 default; diffnet_f43.hip: Winograd F(4,3) on the fp32 matrix pipe; diffnet_bf16.hip: bf16-operand configuration; the
// host side — plan_stack / launch_stack — is below).  (The first form, a F(2,3) kernel with two 32-frame workgroups per CU, lived here
// in the first half of round 2; it was 3 % slower than two chains of per-layer launches, was superseded by the forms above and removed.)
// The hand-off protocol all of them share: per layer the only inter-workgroup traffic is the 8-frame edge of the new conv image that
// each of the two neighbour tiles needs as its halo (dilation <= 8): published write-through (sc1) into an exchange array that is
// double-buffered by layer parity; flag[tile] = launch epoch * 64 + number of layers published.  Producer: sc1 stores -> every storing
// wave s_waitcnt vmcnt(0) -> barrier -> one relaxed agent-scope flag store.  Consumer: one lane polls the two neighbour flags (relaxed,
// s_sleep, bounded: a give-up is counted in `status` and handled by the host in the same call) -> barrier -> sc1 buffer loads of the
// handed-off bytes to registers (cdna_hip_programming.md Guideline 16, MI355X_MICROARCH.md hand-off "valid forms": no agent-scope
// acquire, which would invalidate the CU's L1 — the weight stream's — every layer).  Double buffering is enough: a tile can only
// publish layer l+2 after its neighbours published l+1, which they do after reading its l.  Every workgroup of a launch must be
// resident (neighbours wait for each other): the host launches whole rows, at most one workgroup per CU, never inside a stream capture.
// ------------------------------------------------------------------------------------------------

// ------------------------------------------------------------------------------------------------
// sampler: one ancestral step, elementwise over [B][M][T]   (shallow_diffusion_tts.py:134-166)
// ------------------------------------------------------------------------------------------------
__global__ void ddpm_step_kernel(float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ noise,
                                 StepCoef k, long long n4, unsigned long long seed, unsigned stream,
                                 unsigned long long quad0) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
  const f32x4 ev = reinterpret_cast<const f32x4*>(eps)[i];
  f32x4 nv;
  if (noise) nv = reinterpret_cast<const f32x4*>(noise)[i];
  else if (k.sigma != 0.f) nv = philox_normal4(seed, stream, quad0 + (unsigned long long)i);
  else nv = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    // every product/sum rounded separately, like the reference's elementwise ATen ops (no FMA contraction)
    float x0 = __fsub_rn(__fmul_rn(k.recip, xv[e]), __fmul_rn(k.recipm1, ev[e]));   // :134-138
    x0 = fminf(fmaxf(x0, -1.0f), 1.0f);                                              // :154
    const float mean = __fadd_rn(__fmul_rn(k.pc1, x0), __fmul_rn(k.pc2, xv[e]));    // :141-144
    o[e] = __fadd_rn(mean, __fmul_rn(k.sigma, nv[e]));                               // :166
  }
  reinterpret_cast<f32x4*>(x)[i] = o;
}

// ------------------------------------------------------------------------------------------------
// step tail + next head, fused (DDPM loop only): for one 32-frame tile
//   h    = relu(W_skip * s + b)            s = skip sum / sqrt(L), written by the last residual layer   (net.py:126-128)
//   eps  = W_out * h + b                                                                               (net.py:129)
//   x   <- p_sample(x, eps, noise)         same arithmetic as ddpm_step_kernel                  (shallow_diffusion_tts.py:149-166)
//   xa   = relu(W_in * x + b)              the NEXT step's input projection                            (net.py:116-118)
// Replaces three GEMM launches + the sampler launch per step (~150 us -> ~20 us at B=16, T=1000): the three
// projections are too small (0.04-0.13 MFLOP/frame) to fill the chip as separate 128x128-tile GEMMs.
// ------------------------------------------------------------------------------------------------
#define BSG_MFMA4(ACC, A_, B_)                                                \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A_[0], B_[0], ACC, 0, 0, 0);      \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A_[1], B_[1], ACC, 0, 0, 0);      \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A_[2], B_[2], ACC, 0, 0, 0);      \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A_[3], B_[3], ACC, 0, 0, 0);

// acc += A[tile rows] * Bs, K = 8*NQ, A fragments from `rs` at byte offset `sbase`, B rows from LDS `bs` (stride 32)
template <int NQ>
__device__ __forceinline__ void tile_gemm(f32x16& acc, rsrc_t rs, int vfrag, int sbase, const float* brow) {
  auto ldb = [&](int q) {
    const float* p = brow + 8 * q * 32;
    return f32x4{p[0], p[2 * 32], p[4 * 32], p[6 * 32]};
  };
  f32x4 A0 = ldf4(rs, vfrag, sbase), A1 = ldf4(rs, vfrag, sbase + (NQ > 1 ? 1024 : 0));
  f32x4 B0 = ldb(0), B1;
#pragma unroll 1
  for (int q = 0; q < NQ; q += 2) {
    B1 = ldb(q + 1 < NQ ? q + 1 : NQ - 1);
    __builtin_amdgcn_sched_barrier(0);
    BSG_MFMA4(acc, A0, B0)
    __builtin_amdgcn_sched_barrier(0);
    const int q2 = q + 2 < NQ ? q + 2 : NQ - 1;
    A0 = ldf4(rs, vfrag, sbase + q2 * 1024);
    B0 = ldb(q2);
    __builtin_amdgcn_sched_barrier(0);
    if (q + 1 < NQ) { BSG_MFMA4(acc, A1, B1) }
    __builtin_amdgcn_sched_barrier(0);
    const int q3 = q + 3 < NQ ? q + 3 : NQ - 1;
    A1 = ldf4(rs, vfrag, sbase + q3 * 1024);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int MP, bool PLMS>   // MP = in_dims padded to a multiple of 8 (K of the head GEMM), in_dims <= 96; PLMS: multistep update form
__global__ __launch_bounds__(512, 4) void step_tail_kernel(TailArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* ss = lds;               // [C][32]  skip tile, then h tile
  float* xin = lds + C * 32;     // [96][32] updated x tile (rows >= M zero)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lh = lane >> 5;
  const int b = blockIdx.x / a.tiles_per_row;
  const int t0 = (blockIdx.x - b * a.tiles_per_row) * 32;
  const int T = a.T, M = a.M;
  const int col = t0 + l31;
  const bool col_ok = col < T;
  const int colc = col_ok ? col : T - 1;
  const rsrc_t rs_s = mk_rsrc(a.skip + (long long)b * C * T, (unsigned)C * T * 4);
  const rsrc_t rs_xa = mk_rsrc(a.xa_next + (long long)b * C * T, (unsigned)C * T * 4);
  const rsrc_t rs_x = mk_rsrc(a.x + (long long)b * M * T, (unsigned)M * T * 4);
  const rsrc_t rs_ws = mk_rsrc(a.ws_pack, C * C * 4);
  const rsrc_t rs_wo = mk_rsrc(a.wo_pack, 96 * C * 4);
  const rsrc_t rs_wi = mk_rsrc(a.wi_pack, C * MP * 4);
  const rsrc_t rs_bs = mk_rsrc(a.b_skip, C * 4);
  const rsrc_t rs_bf = mk_rsrc(a.b_fin, 96 * 4);
  const rsrc_t rs_bi = mk_rsrc(a.b_in, C * 4);
  const int vfrag = lane * 16, rowT = T * 4;
  const int vcol = (lh * 4 * T + colc) * 4;

  // ---- stage the skip tile ---------------------------------------------------------------------
  if (a.skip_h) {
    // channel-quad bf16: 64 quads x 32 frames, one 8-byte load per item
    const rsrc_t rs_sh = mk_rsrc(a.skip_h + (long long)b * C * T, (unsigned)C * T * 2);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int idx = tid + 512 * k;
      const int q = idx >> 5, f = idx & 31;
      const int t = t0 + f;
      using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
      u32x2 v = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_sh, t < T ? (q * T + t) * 8 : 0, 0, 0));
      if (t >= T) v = u32x2{0u, 0u};
      ss[(4 * q) * 32 + f] = bf16_lo(v[0]);
      ss[(4 * q + 1) * 32 + f] = bf16_hi(v[0]);
      ss[(4 * q + 2) * 32 + f] = bf16_lo(v[1]);
      ss[(4 * q + 3) * 32 + f] = bf16_hi(v[1]);
    }
  } else if ((T & 3) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int idx = tid + 512 * k;
      const int c = idx >> 3, j4 = idx & 7;
      const int t = t0 + 4 * j4;
      f32x4 v = ldf4(rs_s, t < T ? (c * T + t) * 4 : 0, 0);
      if (t >= T) v = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(ss + c * 32 + 4 * j4) = v;
    }
  } else {
    for (int idx = tid; idx < C * 32; idx += 512) {
      const int c = idx >> 5, t = t0 + (idx & 31);
      const float v = ldf(rs_s, t < T ? (c * T + t) * 4 : 0, 0);
      ss[idx] = t < T ? v : 0.f;
    }
  }
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = ldf(rs_bs, lh * 16, (32 * wave + acc_row0(r)) * 4);
  __syncthreads();
  // ---- h = relu(W_skip s + b) ------------------------------------------------------------------
  tile_gemm<32>(acc, rs_ws, vfrag, wave * 32 * 1024, ss + lh * 32 + l31);
  __syncthreads();   // every wave is done reading s
#pragma unroll
  for (int r = 0; r < 16; ++r) ss[(32 * wave + acc_row(r, lh)) * 32 + l31] = fmaxf(acc[r], 0.f);
  __syncthreads();
  // ---- eps = W_out h + b; sampler update on the 3 row tiles that cover the M mel bins -----------
  if (wave < 3) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = ldf(rs_bf, lh * 16, (32 * wave + acc_row0(r)) * 4);
    float xv[16], nv[16];
    const rsrc_t rs_n = mk_rsrc(a.noise ? a.noise + (long long)b * M * T : a.x, a.noise ? (unsigned)M * T * 4 : 0u);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      // the lane's row is m0 + 4*lh; rows >= M fall outside the descriptor's range and read as 0 (raw-buffer
      // range check), and are never stored
      const int m0 = 32 * wave + acc_row0(r);
      xv[r] = ldf(rs_x, vcol, m0 * rowT);
      nv[r] = a.noise ? ldf(rs_n, vcol, m0 * rowT) : 0.f;
    }
    float h1v[PLMS ? 16 : 1], h2v[PLMS ? 16 : 1], h3v[PLMS ? 16 : 1];
    if constexpr (PLMS) {
      const unsigned hb = (unsigned)M * T * 4;
      const rsrc_t rs_h1 = mk_rsrc(a.h1 + (long long)b * M * T, hb);
      const rsrc_t rs_h2 = mk_rsrc(a.plms_hist > 1 ? a.h2 + (long long)b * M * T : a.x, a.plms_hist > 1 ? hb : 0u);
      const rsrc_t rs_h3 = mk_rsrc(a.plms_hist > 2 ? a.h3 + (long long)b * M * T : a.x, a.plms_hist > 2 ? hb : 0u);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int so = (32 * wave + acc_row0(r)) * rowT;
        h1v[r] = ldf(rs_h1, vcol, so);
        h2v[r] = ldf(rs_h2, vcol, so);   // zero-size descriptors read as 0
        h3v[r] = ldf(rs_h3, vcol, so);
      }
    }
    tile_gemm<32>(acc, rs_wo, vfrag, wave * 32 * 1024, ss + lh * 32 + l31);
    const int vst = (lh * 4 * T + col) * 4;
    const rsrc_t rs_en = mk_rsrc(PLMS ? a.e_new + (long long)b * M * T : a.x, PLMS ? (unsigned)M * T * 4 : 0u);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = 32 * wave + acc_row(r, lh);
      float o = 0.f;
      if (m < M) {
        if constexpr (PLMS) {
          o = plms_update(xv[r], acc[r], h1v[r], h2v[r], h3v[r], a.plms_hist, a.pk, nullptr);
          if (col_ok) stf(acc[r], rs_en, vst, (32 * wave + acc_row0(r)) * rowT);
        } else {
          float nz = nv[r];
          if (!a.noise && a.k.sigma != 0.f)
            nz = philox_normal1(a.seed, a.stream, a.quad_row0 + ((unsigned long long)b * M + m) * T + colc);
          float x0 = __fsub_rn(__fmul_rn(a.k.recip, xv[r]), __fmul_rn(a.k.recipm1, acc[r]));
          x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
          const float mean = __fadd_rn(__fmul_rn(a.k.pc1, x0), __fmul_rn(a.k.pc2, xv[r]));
          o = __fadd_rn(mean, __fmul_rn(a.k.sigma, nz));
        }
        if (col_ok) stf(o, rs_x, vst, (32 * wave + acc_row0(r)) * rowT);
      }
      xin[m * 32 + l31] = o;
    }
  }
  if (!a.do_head) return;
  __syncthreads();
  // ---- next step's input projection: xa = relu(W_in x + b) --------------------------------------
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = ldf(rs_bi, lh * 16, (32 * wave + acc_row0(r)) * 4);
  tile_gemm<MP / 8>(acc, rs_wi, vfrag, wave * (MP / 8) * 1024, xin + lh * 32 + l31);
  if (col_ok) {
    const int vst = (lh * 4 * T + col) * 4;
#pragma unroll
    for (int r = 0; r < 16; ++r) stf(fmaxf(acc[r], 0.f), rs_xa, vst, (32 * wave + acc_row0(r)) * rowT);
  }
}
#undef BSG_MFMA4

__global__ void pad_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows_src, int rows_dst, int cols_src,
                                int cols_dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows_dst * cols_dst) return;
  const int r = i / cols_dst, c = i - r * cols_dst;
  dst[i] = (r < rows_src && c < cols_src) ? src[(long long)r * cols_src + c] : 0.f;
}

__global__ void philox_fill_kernel(float* __restrict__ x, long long n4, unsigned long long seed, unsigned stream,
                                   unsigned long long quad0) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  reinterpret_cast<f32x4*>(x)[i] = philox_normal4(seed, stream, quad0 + (unsigned long long)i);
}

// Row-keyed draws (bsg_philox_normal_rows): row b of x [rows][M][T] from its OWN stream (seed[b], stream) — element m n_b + c at
// x[b][m][c] for c < n_b = len[b], what philox_fill_kernel writes for the row alone at T = n_b — and 0 at n_b <= c < T.  The seeds and
// lengths of up to 32 rows travel in the launch's arguments (nothing is copied, a captured call replays them).
// blockIdx.y: the row.  Work item i of a row: i < M n_b / 4: quad i of the row's stream, every draw evaluated once; its four values go
// to (m, c) = (idx / n_b, idx % n_b), one 16-byte store where they stay in one mel row and the address allows it (rows of odd T start
// unaligned), single floats elsewhere.  The items behind: four elements each of the zero tail, M (T - n_b) in all.
constexpr int kPhiloxRowsPerLaunch = 32;
struct PhiloxRows {
  unsigned long long seed[kPhiloxRowsPerLaunch];
  int len[kPhiloxRowsPerLaunch];
};
__global__ __launch_bounds__(256) void philox_fill_rows_kernel(float* __restrict__ x, PhiloxRows rows, int M, int T, unsigned stream) {
  const int b = blockIdx.y, nb = rows.len[b];
  float* xb = x + (long long)b * M * T;
  const long long nq = (long long)M * nb / 4;   // (M n_b is a multiple of 4: the host refuses anything else)
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nq) {
    const f32x4 z = philox_normal4(rows.seed[b], stream, (unsigned long long)i);
    const long long idx = 4 * i;
    int m = (int)(idx / nb), c = (int)(idx - (long long)m * nb);
    float* p = xb + (long long)m * T + c;
    if (c + 3 < nb && (reinterpret_cast<unsigned long long>(p) & 15ull) == 0) {
      *reinterpret_cast<f32x4*>(p) = z;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xb[(long long)m * T + c] = z[e];
        if (++c == nb) { c = 0; ++m; }
      }
    }
    return;
  }
  const int pad = T - nb;
  const long long nz = (long long)M * pad;
  for (long long e = 4 * (i - nq), end = e + 4 < nz ? e + 4 : nz; e < end; ++e) {
    const int m = (int)(e / pad);
    xb[(long long)m * T + nb + (int)(e - (long long)m * pad)] = 0.f;
  }
}

// mel_out[b,t,m] = denorm(x[b,m,t]) * (mel2ph[b,t] > 0)     (shallow_diffusion_tts.py:268-272, :278-279)
// [M][64]-frame tile through LDS: reads coalesced along t, writes coalesced along m.
__global__ __launch_bounds__(256) void mel_finish_kernel(const float* __restrict__ x, const float* __restrict__ smin,
                                                         const float* __restrict__ smax, const long long* __restrict__ mel2ph,
                                                         float* __restrict__ out, int M, int T) {
  extern __shared__ float tile[];   // [M][65]
  const int b = blockIdx.y, t0 = blockIdx.x * 64, tid = threadIdx.x;
  for (int i = tid; i < M * 64; i += 256) {
    const int m = i >> 6, j = i & 63;
    const int t = t0 + j;
    tile[m * 65 + j] = t < T ? x[((long long)b * M + m) * T + t] : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < 64 * M; i += 256) {
    const int j = i / M, m = i - j * M;
    const int t = t0 + j;
    if (t >= T) continue;
    const float lo = smin[m], hi = smax[m];
    float v = __fadd_rn(__fmul_rn(__fadd_rn(tile[m * 65 + j], 1.0f) / 2.0f, __fsub_rn(hi, lo)), lo);
    if (mel2ph && mel2ph[(long long)b * T + t] <= 0) v = v * 0.f;
    out[((long long)b * T + t) * M + m] = v;
  }
}

// shallow-diffusion start x = q_sample(norm_spec(fs2_mel)^T, K_step-1)          (:249-252, :203-208, :275-276)
__global__ __launch_bounds__(256) void mel_start_kernel(const float* __restrict__ mel, const float* __restrict__ smin,
                                                        const float* __restrict__ smax, const float* __restrict__ noise,
                                                        float ca, float cb, float* __restrict__ x, int M, int T) {
  extern __shared__ float tile[];   // [64][M+1]
  const int b = blockIdx.y, t0 = blockIdx.x * 64, tid = threadIdx.x;
  for (int i = tid; i < 64 * M; i += 256) {
    const int j = i / M, m = i - j * M;
    const int t = t0 + j;
    float v = 0.f;
    if (t < T) {
      const float lo = smin[m], hi = smax[m];
      v = __fsub_rn(__fmul_rn(__fsub_rn(mel[((long long)b * T + t) * M + m], lo) / __fsub_rn(hi, lo), 2.0f), 1.0f);
    }
    tile[j * (M + 1) + m] = v;
  }
  __syncthreads();
  for (int i = tid; i < M * 64; i += 256) {
    const int m = i >> 6, j = i & 63;
    const int t = t0 + j;
    if (t >= T) continue;
    const long long o = ((long long)b * M + m) * T + t;
    x[o] = __fadd_rn(__fmul_rn(ca, tile[j * (M + 1) + m]), __fmul_rn(cb, noise[o]));
  }
}

// PLMS transfer x_pred = x + x_delta  (shallow_diffusion_tts.py:174-182); eps' = blend of eps history (:191-198)
__global__ void plms_step_kernel(const float* __restrict__ x, float* __restrict__ xo, const float* __restrict__ e0,
                                 const float* __restrict__ e1, const float* __restrict__ e2,
                                 const float* __restrict__ e3, PlmsCoef k, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int n_hist = e3 ? 3 : e2 ? 2 : e1 ? 1 : 0;
  xo[i] = plms_update(x[i], e0[i], e1 ? e1[i] : 0.f, e2 ? e2[i] : 0.f, e3 ? e3[i] : 0.f, n_hist, k, nullptr);
}

// ragged batches (bsg_diffnet_prepare_ragged): the same update on the frames t < len[b] of every row only — the padding of xo is left as
// it was.  grid (ceil(T / 256), M, B)
__global__ void plms_step_ragged_kernel(const float* __restrict__ x, float* __restrict__ xo, const float* __restrict__ e0,
                                        const float* __restrict__ e1, const float* __restrict__ e2, const float* __restrict__ e3, PlmsCoef k,
                                        const int* __restrict__ len, int M, int T) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.z;
  if (t >= len[b]) return;
  const long long i = ((long long)b * M + blockIdx.y) * T + t;
  const int n_hist = e3 ? 3 : e2 ? 2 : e1 ? 1 : 0;
  xo[i] = plms_update(x[i], e0[i], e1 ? e1[i] : 0.f, e2 ? e2[i] : 0.f, e3 ? e3[i] : 0.f, n_hist, k, nullptr);
}

// ragged batches: v [B][M][T] = 0 at the frames of each row's padding (t >= len[b]).  grid (ceil(T / 256), M, B)
__global__ void ragged_zero_pad_kernel(float* __restrict__ v, const int* __restrict__ len, int M, int T) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.z;
  if (t >= T || t < len[b]) return;
  v[((long long)b * M + blockIdx.y) * T + t] = 0.f;
}

}  // namespace

}  // namespace bsg

// ================================================================================================
// host side
// ================================================================================================
using namespace bsg;

struct bsg_diffnet {
  bsg_diffnet_cfg cfg;
  int M, L;
  Guard guard;   // this handle's range-event word and split-fp16 GEMM switch (input / conditioner projections)
  // packed / derived weights (library-owned)
  float* w_in = nullptr;    // [C][M]
  float* b_in = nullptr;    // [C]
  float* apack1 = nullptr;  // [L][2C*3C]
  float* apack2 = nullptr;  // [L][2C*C]
  float* apackw = nullptr;  // [L][4*2C*C]  Winograd form of the dilated conv
  float* apackw43 = nullptr;  // [L][6*2C*C]  Winograd F(4,3) form (diffnet_f43.hip)
  unsigned short* apack1h = nullptr;  // [L][2C*3C] bf16 fragments (bf16-operand form, diffnet_bf16.hip)
  unsigned short* apack2h = nullptr;  // [L][2C*C]
  unsigned short* apack1s = nullptr;  // [L][2 planes][2C*3C] hi / lo fp16 fragments (split-fp16 form of the fp32 stack launch, diffnet_h2.hip)
  unsigned short* apack2s = nullptr;  // [L][2 planes][2C*C]
  float* h2_scale = nullptr;          // [L][4] power-of-two scales of the split-fp16 form
  unsigned short* tail_s = nullptr;   // split-fp16 step tail (fused into the h2 stack launch): skip [2*C*C], output [2*96*C], input projection [2*C*96]
  float* tail_scale = nullptr;        // [3][2] scales of the three projections (+ 3 words of scratch)
  unsigned short* tail_h = nullptr;   // bf16 step tail (step_tail_bf16_kernel): skip projection [C*C], output projection [96*C], input projection [C*96]
  int compute = BSG_COMPUTE_F32;      // bsg_diffnet_set_compute
  unsigned short* condterm_h = nullptr;  // [L][B][2C/4][T][4] bf16 (bf16 mode only)
  unsigned short* skip_h = nullptr;      // [B][C/4][T][4] bf16
  size_t cap_bt_h = 0;
  unsigned short* wcond_pack = nullptr;  // [L][2 x 2C x H] the conditioner projections as pre-split fp16 fragments (gemm_h2w.hip)
  unsigned* pack_bad = nullptr;          // device word: packed conditioner weights beyond the fp16 range (then wcond_pack is not used)
  bool cond_h2w_ok = false;
  unsigned short* cond_planes = nullptr; // [2][B][T][H] fp16: hi / lo of 16 x cond, transposed (the activation operand of the pre-split GEMM)
  size_t cap_cond_planes = 0;            // B x T the planes are sized for
  float* w_cond = nullptr;  // [L][2C][H]
  float* b_cond = nullptr;  // [L][2C]  (b_cond + b_dil)
  float* b_out = nullptr;   // [L][2C]
  float* w_skip = nullptr;  // [C][C]
  float* b_skip = nullptr;
  float* w_fin = nullptr;   // [M][C]
  float* b_fin = nullptr;
  float* dproj = nullptr;   // [S][L][C]
  float* dconv = nullptr;   // [S][L][4][2C]: dilated_conv_l's taps applied to dproj[s][l] (tap 0, 1, 2, their sum): diffnet_h2q.hip
  // fused step tail/head (DDPM loop): packed skip / output / input projections
  float* ws_pack = nullptr;  // [C*C]
  float* wo_pack = nullptr;  // [96*C]
  float* wi_pack = nullptr;  // [C*MP]
  float* b_fin96 = nullptr;  // [96]
  int MP = 0;
  // What is bound: written by a prepare as ONE record — cleared at its start, committed at its successful end, so a prepare that fails
  // leaves nothing bound and check_bound() refuses the next compute call.  bsg_diffnet_prepare_ragged adds `ragged` behind its prepare;
  // ensure_cond_quads() / ensure_cond_rows() add the layout they derive.
  struct Bound {
    int B = 0, T = 0;                  // B = 0: nothing is bound
    int compute = BSG_COMPUTE_F32;     // bsg_diffnet_set_compute mode the condition was bound under
    bool tok = false;                  // the condition came per token: cond_tok / tok_dev hold the term's table and every frame's token id
    int K = 0;                         // ... with K token columns per item
    bool ragged = false;               // the condition came with row lengths (rg_dev)
    bool rows = false, quads = false, quads_h = false;   // condterm / condterm_q / condterm_h hold the bound condition's term
  } bound;
  // workspaces for the bound (B,T); every shape-sized buffer and its capacity word is listed in ws_table()
  size_t cap_bt = 0;
  float* condterm = nullptr;  // [L][B][2C][T]
  float* condterm_q = nullptr;   // the same in channel-quad order [L][B][2C/4][T][4]: what the 16-row stack launch and the part forms load (16 bytes per lane)
  size_t cap_cond_q = 0;         // frames it holds
  // the ROW layout (condterm) is what the fallback launches read (32-row stack launch, F(4,3), per-layer and channel-split kernels); the
  // default launches read the quads.  Round 6: prepare writes ONE layout (plan_bind) — the quads whenever the HANDLE can take the 16-row
  // launch (fp32 compute, BSG_COND_QUAD / BSG_H2_Q on, not demoted), whatever launch the bound shape takes; the bf16 quads under bf16
  // compute; the rows otherwise — and the rows are derived from the quads by ensure_cond_rows() the first time a launch that reads them
  // runs (655 MB less per pass at B = 16)
  size_t cap_cond_rows = 0;      // frames condterm holds (allocated on demand)
  // token binding (bsg_diffnet_prepare_tokens): the term per TOKEN, [L][B][2C/4][K][4], and every frame's token id.  The token form of the
  // 16-row stack launch gathers from it; every other launch reads the per-frame layouts above, which ensure_cond_quads() / ensure_cond_rows()
  // expand from the table the first time such a launch runs (bound.quads / bound.rows are false behind a token prepare that kept the table)
  float* cond_tok = nullptr;     // [L][B][2C/4][bound.K][4]
  size_t cap_cond_tok = 0;       // B x K it holds
  int* tok_dev = nullptr;        // [B][T] token id of every frame, clamped to [0, bound.K)
  size_t cap_tok = 0;            // frames it holds
  unsigned* tok_bad = nullptr;   // device word: ids the last conversion found outside [0, K)
  float* cond_exp = nullptr;     // [B][H][T]: the per-frame condition of a token prepare that cannot keep the table (bf16 compute, no pre-split GEMM)
  size_t cap_cond_exp = 0;
  float* xa = nullptr;        // [B][C][T]
  float* xb = nullptr;
  float* skip = nullptr;
  float* hid = nullptr;
  float* eps = nullptr;       // [B][M][T]
  float* eps_hist[4] = {nullptr, nullptr, nullptr, nullptr};  // PLMS history + x_pred scratch
  float* xpred = nullptr;
  // live timing of the dominant kernel: one event pair around the L residual-layer launches of a forward
  bool prof_on = false;
  std::vector<hipEvent_t> prof_ev;
  size_t prof_used = 0;
  size_t prof_launches = 0;   // layer-equivalents covered by the recorded pairs (L per evaluation)
  // on-chip stack launches: edge exchange [2][tiles][2][C][8], flags [tiles] + status word
  float* hx = nullptr;
  unsigned* flags = nullptr;
  size_t flags_cap = 0;                // tiles the exchange array and the flags are sized for
  unsigned* epoch_dev = nullptr;       // [2] launch epoch of the stack / part launches in device memory + workgroups done (diffnet_res.h StackArgs::epoch)
  unsigned long long* clk = nullptr;   // [4] s_memtime / s_memrealtime at the start and end of tile 0 of the last profiled stack launch
  bool h2_off = false;                 // bsg_diffnet_set_h2(h, 0): this handle multiplies on the fp32 matrix pipe only
  bool q_off = false;                  // bsg_diffnet_set_h2q(h, 0): the 32-row stack launch (|x + d| < 60000) instead of the 16-row one (|x| < 3750)
  unsigned short *apack1q = nullptr, *apack2q = nullptr;   // the split-fp16 weights once more as 16-row fragments (part forms)
  unsigned short* part_zx = nullptr;   // part forms: exchange slots of the z parts [tiles][P][2 planes][tile frames][C/P] fp16
  unsigned short* part_ix = nullptr;   //             ... of the image parts [2 parities][tiles][P][2 planes][tile frames][C/P]
  unsigned* part_flags = nullptr;      //             [2][tiles][P] image / z flags
  size_t part_cap = 0;                 // 32-frame tile equivalents the exchange buffers are sized for
  int num_cus = 0;
  const char* last_path = "none";      // form of the last residual-layer launch (bsg_diffnet_last_path)
  int last_chains = 0;                 // launch chains of the last sampler call: 2 = the half-batch chains of dual_fork (bsg_diffnet_last_launch)
  int last_groups = 0;                 // launch groups of the last stack launch (0: the last launch was no stack launch)
  // channel-split launch for small batches (residual_split_kernel)
  float* apack2w = nullptr;            // [L][2C*C] output projection packed for 16x16x4 MFMAs
  float* zbuf = nullptr;               // [tiles][C][32] z exchange scratch
  unsigned* split_flags = nullptr;     // [tiles][16] (producer, consumer) flags + status word
  size_t split_cap = 0;                // tiles the scratch is sized for
  unsigned split_epoch = 0;
  bool split_off = false;              // bsg_diffnet_set_split(h, 0): regular launches only (the self-heal path after a give-up)
  int inject_giveup = 0;               // bsg_diffnet_debug_inject_giveup: split launches left that give up without waiting
  int inject_nowait = 0;               // the same entry with a NEGATIVE count: part launches left that skip their waits silently (timing experiment)
  int inject_xcc = 0;                  // bsg_diffnet_debug_inject_xcc: part launches left in which odd parts report another XCD
  bool parts_off = false;              // bsg_diffnet_set_parts(h, 0): no part forms (several workgroups per tile on CUs of ONE XCD); the one-workgroup-per-tile launches stay
  FormMemo forms;                      // every launch form's LDS grant and residency on this handle's device (diffnet_forms.h)
  // two half-batches on two streams (dual_fork): the second stream and the events that fork and join it
  hipStream_t st2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // ragged binding (bsg_diffnet_prepare_ragged, bound.ragged): every row of the bound (B, T) decoded at its own frame count
  int* rg_dev = nullptr;               // [B rounded up to even] row lengths, then the tile tables {row, tile} of every launch group
  size_t rg_cap = 0;                   // ints rg_dev holds
  std::vector<int> rg_group_off;       // per launch group: offset of its table (in tiles) behind the lengths ...
  std::vector<int> rg_group_tiles;     // ... and its tile count
  std::vector<int32_t> rg_lens;        // the bound row lengths once more on the host: what bsg_ddpm_sample_rows draws each row's noise at
  // row-keyed draws (bsg_ddpm_sample_rows): the step's noise [B][M][T], filled in front of every step
  float* row_noise = nullptr;
  size_t row_noise_cap = 0;            // frames B x T it holds (grown by the first keyed call of a shape)
  DevOwned owned;                      // every allocation that lives as long as the handle (own_alloc): destroy frees them
};

// h->num_cus, asked of the device once
static int num_cus(bsg_diffnet* h) {
  if (h->num_cus) return BSG_OK;
  int dev = 0;
  BSG_HIP(hipGetDevice(&dev));
  BSG_HIP(hipDeviceGetAttribute(&h->num_cus, hipDeviceAttributeMultiprocessorCount, dev));
  return BSG_OK;
}

// Every shape-sized buffer of the handle (bsg_ws.h): destroy and grow() walk this one table.  WS_ZERO: flag words (flag values are launch
// epoch x 64 + layers published, so a zeroed word is older than every launch).  `lazy`: the refusal a compute call that would have to grow
// the group gets on a captured stream.
static const char* const kLazyRows = "diffnet: the row layout of the conditioner term is allocated by the first eager call of a fallback launch; run it once before capturing";
static const char* const kLazyQuads = "diffnet: the per-frame conditioner term of a token binding is allocated by the first eager call that reads it; run it once before capturing";
static const char* const kLazyRowNoise = "ddpm_sample_rows: the buffer of a step's row-keyed draws is allocated by the first eager call of this shape; run it once before capturing";
static const char* const kLazyPart = "part launch: the exchange buffers of this shape are allocated by its first eager call; run it once before capturing";
static std::vector<WsBuf> ws_table(bsg_diffnet* h) {   // (a vector: its size is the initialiser's)
  const size_t f = sizeof(float), u = sizeof(unsigned), s = sizeof(unsigned short), M = h->M, term = (size_t)h->L * 2 * C;
  const size_t part_tile = (size_t)2 * 32 * C * s;   // all parts of a 32-frame tile: 2 planes x 32 frames x C fp16 = 32 KB
  return {
      // cap_bt, frames B x T: activations, eps, and the PLMS history ring + x_pred scratch (5 x [B][M][T]: 2 % of the conditioner term) —
      // here, so that no sampler call allocates
      {&h->cap_bt, (void**)&h->xa, C * f},          {&h->cap_bt, (void**)&h->xb, C * f},
      {&h->cap_bt, (void**)&h->skip, C * f},        {&h->cap_bt, (void**)&h->hid, C * f},
      {&h->cap_bt, (void**)&h->eps, M * f},         {&h->cap_bt, (void**)&h->eps_hist[0], M * f},
      {&h->cap_bt, (void**)&h->eps_hist[1], M * f}, {&h->cap_bt, (void**)&h->eps_hist[2], M * f},
      {&h->cap_bt, (void**)&h->eps_hist[3], M * f}, {&h->cap_bt, (void**)&h->xpred, M * f},
      // flags_cap, tiles of one stack launch: flags + 4 status words, edge exchange
      {&h->flags_cap, (void**)&h->flags, u, 4 * u, WS_ZERO},     {&h->flags_cap, (void**)&h->hx, (size_t)2 * 2 * C * 8 * f},
      // split_cap, 32-frame tiles of the batch: channel-split scratch, 16 flags per tile + 4 status words
      {&h->split_cap, (void**)&h->zbuf, (size_t)C * 32 * f}, {&h->split_cap, (void**)&h->split_flags, 16 * u, 4 * u, WS_ZERO},
      // cap_bt_h, frames (bf16 compute only)
      {&h->cap_bt_h, (void**)&h->condterm_h, term * s}, {&h->cap_bt_h, (void**)&h->skip_h, C * s},
      // the binding's own: token ids (frames), GEMM operand planes (B x K or B x T columns), token table (B x K), expanded condition (frames)
      {&h->cap_tok, (void**)&h->tok_dev, sizeof(int)},
      {&h->cap_cond_planes, (void**)&h->cond_planes, (size_t)2 * C * s},
      {&h->cap_cond_tok, (void**)&h->cond_tok, term * f},
      {&h->cap_cond_exp, (void**)&h->cond_exp, C * f},
      // the conditioner term per frame, as quads and as rows
      {&h->cap_cond_q, (void**)&h->condterm_q, term * f, 0, 0, kLazyQuads},
      {&h->cap_cond_rows, (void**)&h->condterm, term * f, 0, 0, kLazyRows},
      // part_cap, 32-frame tile equivalents (slots scale with the tile width): z parts, image parts of 2 parities, [2][tiles][4] flags
      {&h->part_cap, (void**)&h->part_zx, part_tile, 0, 0, kLazyPart}, {&h->part_cap, (void**)&h->part_ix, 2 * part_tile, 0, 0, kLazyPart},
      {&h->part_cap, (void**)&h->part_flags, 2 * 4 * u, 0, WS_ZERO, kLazyPart},
      // rg_cap, ints: row lengths and tile tables of a ragged binding
      {&h->rg_cap, (void**)&h->rg_dev, sizeof(int)},
      // row_noise_cap, frames B x T: one step's row-keyed draws
      {&h->row_noise_cap, (void**)&h->row_noise, M * f, 0, 0, kLazyRowNoise},
  };
}

// (the capacity test comes first, so that a call that grows nothing builds no table)
static int grow(bsg_diffnet* h, size_t* cap, size_t need, hipStream_t st, GrowHow how = GROW_BOUND) {
  return need <= *cap ? BSG_OK : ws_grow(ws_table(h), "diffnet", cap, need, st, how);
}

extern "C" void bsg_diffnet_destroy(bsg_diffnet* h) {
  if (!h) return;
  guard_free(&h->guard);
  h->owned.free_all();
  ws_free(ws_table(h));
  for (hipEvent_t e : h->prof_ev) (void)hipEventDestroy(e);
  if (h->st2) (void)hipStreamDestroy(h->st2);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  delete h;
}

static int copy_dev(float* dst, const void* src, size_t n, hipStream_t st) {
  BSG_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st));
  return BSG_OK;
}

#define TRY(expr)              \
  do {                         \
    int _rc = (expr);          \
    if (_rc != BSG_OK) return _rc; \
  } while (0)

static int gemm_nt(const float* A, const float* W, float* Cc, const float* bias_n, int M, int N, int K, int lda, int ldc,
                   int act, hipStream_t st) {
  GemmArgs g{};
  g.A = A; g.B = W; g.C = Cc; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = K; g.ldc = ldc; g.trans_b = 1;
  g.taps = 1; g.bias_n = bias_n; g.alpha = 1.f; g.act = act; g.batch = 1;
  return launch_gemm(g, st);
}

// conv1x1 over [B][K][T] -> [B][M][T]
static int conv1x1(const float* W, const float* bias, const float* X, float* Y, int M, int K, int B, int T, int act,
                   hipStream_t st) {
  GemmArgs g{};
  g.A = W; g.B = X; g.C = Y; g.M = M; g.N = T; g.K = K; g.lda = K; g.ldb = T; g.ldc = T; g.trans_b = 0;
  g.sA = 0; g.sB = (long long)K * T; g.sC = (long long)M * T; g.taps = 1; g.bias_m = bias; g.alpha = 1.f; g.act = act;
  g.batch = B;
  return launch_gemm(g, st);
}

static int tmp_alloc(std::vector<float*>& tmp, float** p, size_t n) {
  BSG_HIP(hipMalloc((void**)p, n * sizeof(float)));
  tmp.push_back(*p);
  return BSG_OK;
}

// the weights of create, packed into every form the launches read.  `tmp` receives the temporaries: create_impl frees them on every path
static int create_pack(bsg_diffnet* h, const void* const* w, const float* step_table, hipStream_t st, std::vector<float*>& tmp) {
  const int M = h->M, L = h->L, S = h->cfg.max_steps;
  TRY(own_alloc(h->owned, &h->w_in, (size_t)C * M));
  TRY(own_alloc(h->owned, &h->b_in, C));
  TRY(own_alloc(h->owned, &h->apack1, (size_t)L * 2 * C * 3 * C));
  TRY(own_alloc(h->owned, &h->apack2, (size_t)L * 2 * C * C));
  TRY(own_alloc(h->owned, &h->apackw, (size_t)L * 4 * 2 * C * C));
  TRY(own_alloc(h->owned, &h->apackw43, (size_t)L * 6 * 2 * C * C));
  TRY(own_alloc(h->owned, &h->apack2w, (size_t)L * 2 * C * C));
  TRY(own_alloc(h->owned, &h->apack1h, (size_t)L * 2 * C * 3 * C));
  TRY(own_alloc(h->owned, &h->apack2h, (size_t)L * 2 * C * C));
  TRY(own_alloc(h->owned, &h->apack1s, (size_t)L * 2 * 2 * C * 3 * C));
  TRY(own_alloc(h->owned, &h->apack2s, (size_t)L * 2 * 2 * C * C));
  TRY(own_alloc(h->owned, &h->apack1q, (size_t)L * 2 * 2 * C * 3 * C));
  TRY(own_alloc(h->owned, &h->apack2q, (size_t)L * 2 * 2 * C * C));
  TRY(own_alloc(h->owned, &h->h2_scale, (size_t)(4 * L + 2 * L)));   // table + [2L] scratch of the max reduction
  TRY(own_alloc(h->owned, &h->w_cond, (size_t)L * 2 * C * C));
  TRY(own_alloc(h->owned, &h->wcond_pack, (size_t)L * 2 * 2 * C * C));
  TRY(own_alloc(h->owned, &h->pack_bad, 1));
  BSG_HIP(hipMemsetAsync(h->pack_bad, 0, sizeof(unsigned), st));
  TRY(own_alloc(h->owned, &h->b_cond, (size_t)L * 2 * C));
  TRY(own_alloc(h->owned, &h->b_out, (size_t)L * 2 * C));
  TRY(own_alloc(h->owned, &h->w_skip, (size_t)C * C));
  TRY(own_alloc(h->owned, &h->b_skip, C));
  TRY(own_alloc(h->owned, &h->w_fin, (size_t)M * C));
  TRY(own_alloc(h->owned, &h->b_fin, M));
  TRY(own_alloc(h->owned, &h->dproj, (size_t)S * L * C));
  TRY(own_alloc(h->owned, &h->dconv, (size_t)S * L * 4 * 2 * C));
  TRY(copy_dev(h->w_in, w[0], (size_t)C * M, st));
  TRY(copy_dev(h->b_in, w[1], C, st));
  // step-embedding MLP over the whole table: D = W2 * mish(W1 * e + b1) + b2        (net.py:92-96,120)
  float *hid = nullptr, *dtab = nullptr;
  TRY(tmp_alloc(tmp, &hid, (size_t)S * 4 * C));
  TRY(tmp_alloc(tmp, &dtab, (size_t)S * C));
  TRY(gemm_nt(step_table, (const float*)w[2], hid, (const float*)w[3], S, 4 * C, C, C, 4 * C, ACT_MISH, st));
  TRY(gemm_nt(hid, (const float*)w[4], dtab, (const float*)w[5], S, C, 4 * C, 4 * C, C, ACT_NONE, st));
  {   // split-fp16 form: per-layer power-of-two scales from max |w|, then the hi / lo fragments below
    std::vector<const float*> w1(L), w2(L);
    for (int l = 0; l < L; ++l) { w1[l] = (const float*)w[6 + 8 * l]; w2[l] = (const float*)w[6 + 8 * l + 6]; }
    TRY(h2_scales(w1.data(), w2.data(), L, reinterpret_cast<unsigned*>(h->h2_scale + 4 * L), h->h2_scale, st));
  }
  for (int l = 0; l < L; ++l) {
    const void* const* lw = w + 6 + 8 * l;
    // dilated conv [2C][C][3] -> fragment order with k = tap*C + ci
    {
      const long long total = (long long)2 * C * 3 * C;
      hipLaunchKernelGGL(pack_a_frag_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, (const float*)lw[0],
                         h->apack1 + (size_t)l * total, 2 * C, 3 * C, C, (long long)3 * C, 3LL, 1LL);
    }
    hipLaunchKernelGGL(pack_wino_kernel, dim3(cdiv(4LL * 2 * C * C, 256)), dim3(256), 0, st, (const float*)lw[0],
                       h->apackw + (size_t)l * 4 * 2 * C * C);
    {
      const long long total = (long long)2 * C * C;
      hipLaunchKernelGGL(pack_a_frag_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, (const float*)lw[6],
                         h->apack2 + (size_t)l * total, 2 * C, C, C, (long long)C, 1LL, 0LL);
    }
    TRY(pack_wino43((const float*)lw[0], h->apackw43 + (size_t)l * 6 * 2 * C * C, st));
    TRY(pack_a_frag_bf16((const float*)lw[0], h->apack1h + (size_t)l * 2 * C * 3 * C, 2 * C, 3 * C, C, (long long)3 * C, 3LL, 1LL, st));
    TRY(pack_a_frag_bf16((const float*)lw[6], h->apack2h + (size_t)l * 2 * C * C, 2 * C, C, C, (long long)C, 1LL, 0LL, st));
    TRY(pack_a_frag_h2((const float*)lw[0], h->apack1s + (size_t)l * 2 * 2 * C * 3 * C, 2 * C, 3 * C, C, (long long)3 * C, 3LL, 1LL, h->h2_scale + 4 * l, 0, st));
    TRY(pack_a_frag_h2((const float*)lw[6], h->apack2s + (size_t)l * 2 * 2 * C * C, 2 * C, C, C, (long long)C, 1LL, 0LL, h->h2_scale + 4 * l, 1, st));
    TRY(pack_a_frag_q((const float*)lw[0], h->apack1q + (size_t)l * 2 * 2 * C * 3 * C, 2 * C, 3 * C, C, (long long)3 * C, 3LL, 1LL, h->h2_scale + 4 * l, 0, st));
    TRY(pack_a_frag_q((const float*)lw[6], h->apack2q + (size_t)l * 2 * 2 * C * C, 2 * C, C, C, (long long)C, 1LL, 0LL, h->h2_scale + 4 * l, 1, st));
    hipLaunchKernelGGL(pack_a16_kernel, dim3(cdiv(2 * C * C, 256)), dim3(256), 0, st, (const float*)lw[6], h->apack2w + (size_t)l * 2 * C * C,
                       2 * C, C);
    hipLaunchKernelGGL(vec_add_kernel, dim3(cdiv(2 * C, 256)), dim3(256), 0, st, (const float*)lw[5], (const float*)lw[1],
                       h->b_cond + (size_t)l * 2 * C, 2 * C);
    if (hipGetLastError() != hipSuccess) { set_error("diffnet_create: pack kernels failed"); return BSG_EHIP; }
    TRY(copy_dev(h->w_cond + (size_t)l * 2 * C * C, lw[4], (size_t)2 * C * C, st));
    TRY(h2w_pack_into(h->wcond_pack + (size_t)l * 2 * 2 * C * C, (const float*)lw[4], 2 * C, C, 1, 0, C, 1, h->pack_bad, st));
    TRY(copy_dev(h->b_out + (size_t)l * 2 * C, lw[7], 2 * C, st));
    // diffusion_projection of the tabulated step embedding -> dproj[s][l][:]            (net.py:67)
    TRY(gemm_nt(dtab, (const float*)lw[2], h->dproj + (size_t)l * C, (const float*)lw[3], S, C, C, C, L * C, ACT_NONE, st));
    const size_t dl = ((size_t)DCONV_SMAX * (C + 1) + DCONV_ROWS * 3 * C) * sizeof(float);
    (void)hipFuncSetAttribute((const void*)dconv_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dl);
    hipLaunchKernelGGL(dconv_kernel, dim3(2 * C / DCONV_ROWS, cdiv(S, DCONV_SMAX)), dim3(DCONV_ROWS * DCONV_SMAX), dl, st, (const float*)lw[0], (const float*)h->dproj,
                       h->dconv, S, L, l);
    if (hipGetLastError() != hipSuccess) { set_error("diffnet_create: dconv kernel failed"); return BSG_EHIP; }
  }
  const void* const* tw = w + 6 + 8 * L;
  TRY(copy_dev(h->w_skip, tw[0], (size_t)C * C, st));
  TRY(copy_dev(h->b_skip, tw[1], C, st));
  TRY(copy_dev(h->w_fin, tw[2], (size_t)M * C, st));
  TRY(copy_dev(h->b_fin, tw[3], M, st));
  if (M > 96) return BSG_OK;
  const int MP = (M + 7) / 8 * 8;
  h->MP = MP;
  float *wo_pad = nullptr, *wi_pad = nullptr, *wi_pad96 = nullptr;
  TRY(own_alloc(h->owned, &h->ws_pack, (size_t)C * C));
  TRY(own_alloc(h->owned, &h->wo_pack, (size_t)96 * C));
  TRY(own_alloc(h->owned, &h->wi_pack, (size_t)C * MP));
  TRY(own_alloc(h->owned, &h->b_fin96, 96));
  TRY(tmp_alloc(tmp, &wo_pad, (size_t)96 * C));
  TRY(tmp_alloc(tmp, &wi_pad, (size_t)C * MP));
  hipLaunchKernelGGL(pack_a_frag_kernel, dim3(cdiv((long long)C * C, 256)), dim3(256), 0, st, (const float*)tw[0], h->ws_pack, C, C, C, (long long)C, 1LL, 0LL);
  hipLaunchKernelGGL(pad_rows_kernel, dim3(cdiv(96 * C, 256)), dim3(256), 0, st, (const float*)tw[2], wo_pad, M, 96, C, C);
  hipLaunchKernelGGL(pack_a_frag_kernel, dim3(cdiv((long long)96 * C, 256)), dim3(256), 0, st, (const float*)wo_pad, h->wo_pack, 96, C, C, (long long)C, 1LL, 0LL);
  hipLaunchKernelGGL(pad_rows_kernel, dim3(cdiv(C * MP, 256)), dim3(256), 0, st, (const float*)w[0], wi_pad, C, C, M, MP);
  hipLaunchKernelGGL(pack_a_frag_kernel, dim3(cdiv((long long)C * MP, 256)), dim3(256), 0, st, (const float*)wi_pad, h->wi_pack, C, MP, MP, (long long)MP, 1LL, 0LL);
  hipLaunchKernelGGL(pad_rows_kernel, dim3(1), dim3(256), 0, st, (const float*)tw[3], h->b_fin96, M, 96, 1, 1);
  if (hipGetLastError() != hipSuccess) { set_error("diffnet_create: tail pack kernels failed"); return BSG_EHIP; }
  // the same three projections as bf16 fragments (bf16-operand configuration); the input projection's K is padded to 96
  TRY(tmp_alloc(tmp, &wi_pad96, (size_t)C * 96));
  const size_t tail_n = (size_t)C * C + 96 * C + C * 96;
  if (own_alloc(h->owned, &h->tail_h, tail_n) != BSG_OK) { set_error("diffnet_create: out of device memory"); return BSG_EHIP; }
  hipLaunchKernelGGL(pad_rows_kernel, dim3(cdiv(C * 96, 256)), dim3(256), 0, st, (const float*)w[0], wi_pad96, C, C, M, 96);
  TRY(pack_a_frag_bf16((const float*)tw[0], h->tail_h, C, C, C, (long long)C, 1LL, 0LL, st));
  TRY(pack_a_frag_bf16(wo_pad, h->tail_h + C * C, 96, C, C, (long long)C, 1LL, 0LL, st));
  TRY(pack_a_frag_bf16(wi_pad96, h->tail_h + C * C + 96 * C, C, 96, 96, 96LL, 1LL, 0LL, st));
  // and as split-fp16 fragments (hi / lo planes) for the tail fused into the split-fp16 stack launch
  if (own_alloc(h->owned, &h->tail_s, 2 * tail_n) != BSG_OK || own_alloc(h->owned, &h->tail_scale, 9) != BSG_OK) {
    set_error("diffnet_create: out of device memory");
    return BSG_EHIP;
  }
  return h2_tail_pack((const float*)tw[0], wo_pad, wi_pad96, h->tail_s, h->tail_s + 2 * C * C, h->tail_s + 2 * C * C + 2 * 96 * C,
                      reinterpret_cast<unsigned*>(h->tail_scale + 6), h->tail_scale, st);
}

// create: pack, read the pre-split GEMM's range word back, and free the temporaries once the stream is idle — on every path
static int create_impl(bsg_diffnet* h, const void* const* w, const float* step_table, hipStream_t st) {
  std::vector<float*> tmp;
  const int rc = create_pack(h, w, step_table, st, tmp);
  unsigned pack_bad = 1;
  if (rc == BSG_OK && hipMemcpyAsync(&pack_bad, h->pack_bad, sizeof(unsigned), hipMemcpyDeviceToHost, st) != hipSuccess) pack_bad = 1;
  hipError_t e = hipStreamSynchronize(st);
  h->cond_h2w_ok = rc == BSG_OK && e == hipSuccess && pack_bad == 0;
  for (float* p : tmp) (void)hipFree(p);
  if (rc != BSG_OK) return rc;
  BSG_HIP(e);
  return BSG_OK;
}

extern "C" int bsg_diffnet_create(bsg_diffnet** out, const bsg_diffnet_cfg* cfg, const void* const* dev_weights,
                                  int32_t n_weights, const float* step_table, void* stream) {
  BSG_REQUIRE(out && cfg && dev_weights && step_table, "diffnet_create: null argument");
  BSG_REQUIRE(cfg->residual_channels == C && cfg->encoder_hidden == C,
              "diffnet_create: residual_channels=%d hidden=%d; kernels are built for 256/256", cfg->residual_channels,
              cfg->encoder_hidden);
  BSG_REQUIRE(cfg->in_dims > 0 && cfg->in_dims % 4 == 0 && cfg->in_dims <= 128, "diffnet_create: in_dims=%d unsupported", cfg->in_dims);
  BSG_REQUIRE(cfg->residual_layers > 0 && cfg->residual_layers <= 64, "diffnet_create: residual_layers=%d", cfg->residual_layers);
  BSG_REQUIRE(cfg->dilation_cycle_length >= 1 && cfg->dilation_cycle_length <= 4,
              "diffnet_create: dilation_cycle_length=%d (max dilation 8 supported)", cfg->dilation_cycle_length);
  BSG_REQUIRE(cfg->max_steps > 0, "diffnet_create: max_steps=%d", cfg->max_steps);
  BSG_REQUIRE(n_weights == 10 + 8 * cfg->residual_layers, "diffnet_create: expected %d weight tensors, got %d",
              10 + 8 * cfg->residual_layers, n_weights);
  for (int i = 0; i < n_weights; ++i) BSG_REQUIRE(dev_weights[i] != nullptr, "diffnet_create: weight %d is null", i);
  bsg_diffnet* h = new bsg_diffnet();
  h->cfg = *cfg;
  h->M = cfg->in_dims;
  h->L = cfg->residual_layers;
  int rc = guard_init(&h->guard, (hipStream_t)stream);
  if (rc == BSG_OK) rc = create_impl(h, dev_weights, step_table, (hipStream_t)stream);
  if (rc != BSG_OK) {
    bsg_diffnet_destroy(h);
    return rc;
  }
  *out = h;
  return BSG_OK;
}

// [z][R/4][T][4] -> [z][R][T]: lanes along T, one 16-byte load and four dword stores (256 B contiguous per row and wave)
__global__ __launch_bounds__(256) void quad_to_rows_kernel(const float* __restrict__ q, float* __restrict__ rows, int R, int T) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const long long z = blockIdx.z, qr = blockIdx.y;
  const f32x4 v = *reinterpret_cast<const f32x4*>(q + ((z * (R / 4) + qr) * T + t) * 4);
  float* o = rows + (z * R + 4 * qr) * T + t;
  o[0] = v[0]; o[(long long)T] = v[1]; o[2LL * T] = v[2]; o[3LL * T] = v[3];
}

// the rows of the bound condition's term, derived from its quads the first time a launch that reads rows runs behind a prepare that wrote
// only the quads (a fallback after a range event or a give-up, BSG_H2_Q=0 shapes, the per-layer hooks): 2 x 655 MB at B = 16, once
// [z][R/4][K][4] -> [z][R/4][T][4] through tok [B][T] (z = l B + b): a frame's quad is a COPY of its token's, so the expanded term equals what
// a per-frame prepare writes wherever the projection of a column does not depend on the column's place in the GEMM
__global__ __launch_bounds__(256) void tok_to_quads_kernel(const float* __restrict__ tab, const int* __restrict__ tok, float* __restrict__ q, int R4,
                                                           int K, int T, int B) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const long long z = blockIdx.z, qr = blockIdx.y;
  const int k = tok[(z % B) * T + t];
  *reinterpret_cast<f32x4*>(q + ((z * R4 + qr) * T + t) * 4) = *reinterpret_cast<const f32x4*>(tab + ((z * R4 + qr) * K + k) * 4);
}

// int64 token ids -> int32, clamped to [0, K) (as the front's gathers treat an id beyond the table); *bad counts the ids that were clamped
__global__ void tok_convert_kernel(const long long* __restrict__ src, int* __restrict__ dst, long long n, int K, unsigned* __restrict__ bad) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long long v = src[i];
  const bool out = v < 0 || v >= K;
  dst[i] = out ? 0 : (int)v;
  if (out) atomicAdd(bad, 1u);
}

// [B][K][H] token rows -> [B][H][T] frames through tok: the per-frame condition of a token prepare that takes the per-frame path
__global__ __launch_bounds__(256) void tok_expand_cond_kernel(const float* __restrict__ ct, const int* __restrict__ tok, float* __restrict__ cond,
                                                              int K, int T) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const long long b = blockIdx.z;
  const int c = blockIdx.y;
  cond[(b * C + c) * T + t] = ct[(b * K + tok[b * T + t]) * C + c];
}

// the quads of a token binding's term, expanded from the table the first time a launch that reads per-frame quads runs behind
// bsg_diffnet_prepare_tokens (part forms, 32-frame tiles, BSG_COND_TOK=0) — and the source of ensure_cond_rows() below
static int ensure_cond_quads(bsg_diffnet* h, hipStream_t st) {
  const bsg_diffnet::Bound& b = h->bound;
  if (b.quads || !b.tok) return BSG_OK;
  TRY(grow(h, &h->cap_cond_q, (size_t)b.B * b.T, st, GROW_LAZY));
  const long long zs = (long long)h->L * b.B;
  BSG_REQUIRE(zs <= 65535, "diffnet: L * B = %lld launch slices", zs);
  hipLaunchKernelGGL(tok_to_quads_kernel, dim3(cdiv(b.T, 256), 2 * C / 4, (unsigned)zs), dim3(256), 0, st, (const float*)h->cond_tok,
                     (const int*)h->tok_dev, h->condterm_q, 2 * C / 4, b.K, b.T, b.B);
  BSG_LAUNCH_CHECK();
  h->bound.quads = true;
  return BSG_OK;
}

// the rows (condterm, [L][B][2C][T]) on demand: only the fallback launches read them
static int ensure_cond_rows(bsg_diffnet* h, hipStream_t st) {
  const bsg_diffnet::Bound& b = h->bound;
  if (b.rows) return BSG_OK;
  TRY(ensure_cond_quads(h, st));
  if (!b.quads) {
    set_error("diffnet: the conditioner term of the bound condition exists in the bf16 layout only (bound under BSG_COMPUTE_BF16); call bsg_diffnet_prepare again");
    return BSG_ESTATE;
  }
  TRY(grow(h, &h->cap_cond_rows, (size_t)b.B * b.T, st, GROW_LAZY));
  const long long zs = (long long)h->L * b.B;
  BSG_REQUIRE(zs <= 65535, "diffnet: L * B = %lld launch slices", zs);
  hipLaunchKernelGGL(quad_to_rows_kernel, dim3(cdiv(b.T, 256), 2 * C / 4, (unsigned)zs), dim3(256), 0, st, (const float*)h->condterm_q, h->condterm, 2 * C, b.T);
  BSG_LAUNCH_CHECK();
  h->bound.rows = true;
  return BSG_OK;
}

// How a prepare binds a condition: the form of the hoisted conditioner projection, its columns, the layouts of the term it writes, and the
// workspaces all of that needs.  plan_bind() decides, ensure_bind_ws() grows, launch_bind() launches.
enum BindProj {
  PROJ_H2W,      // all L projections of all B items as ONE launch of the pre-split GEMM (gemm_h2w.hip)
  PROJ_ONE_GEMM, // B = 1: ONE conv1x1 of L x 2C rows
  PROJ_LAYERS,   // L conv1x1 launches
};
struct BindPlan {
  BindProj proj;
  bool tokens;    // a bsg_diffnet_prepare_tokens call: the frames' token ids are converted and checked
  bool table;     // ... that keeps the term per TOKEN (cond_tok, quads only): the projection runs over K columns per item
  bool expand;    // ... that cannot: its condition is expanded to frames first (cond_exp) and takes the per-frame path
  int cols;       // columns per item of the projection: K with `table`, else T
  // the layouts written.  ONE per pass: the rows only when neither the quads nor the bf16 quads are written (BSG_COND_ROWS=1: the rows as
  // well, round 5's way)
  bool rows, quads;
  bool quads_h_direct;    // bf16 compute: the GEMM's epilogue rounds the term to bf16 quads itself and writes NO fp32 copy (until round 5 the
                          // 2.6 GB of fp32 at B = 64 went to HBM and 20 conversion launches read them back; BSG_COND_BF16_DIRECT=0: that form)
  bool quads_h_convert;   // bf16 compute otherwise: L conversion launches from the rows
  // capacity each workspace group needs, in its own unit (ws_table); 0: not used by this binding
  size_t bt, flag_tiles, split_tiles, bt_h, tok, planes, cond_tok, cond_exp, quad_frames, row_frames;
};

// needs h->num_cus; otherwise pure: no HIP call, no write to the handle
static BindPlan plan_bind(const bsg_diffnet* h, int B, int K, int T, bool tokens) {
  const DnSwitches& sw = dn_switches();
  const bool bf16 = h->compute == BSG_COMPUTE_BF16;
  const bool h2w = sw.gemm_h2w && h->cond_h2w_ok && gemm_split_enabled() && h2w_supports(T, 2 * C, C, 1, C) && (long long)h->L * B <= 65535;
  // the 16-row stack launch (diffnet_h2q.hip) loads the term as channel quads: can this HANDLE take it (BSG_H2_Q=0 / BSG_COND_QUAD=0: not)?
  // The bound shape is not asked: its launch may read the rows, which ensure_cond_rows() then derives
  const bool q_launch = sw.cond_quad && sw.h2_q && !bf16 && h->apack1q && !h->h2_off && !h->split_off;
  BindPlan p{};
  p.tokens = tokens;
  // no table in these states (bf16 compute, the GEMMs on the fp32 matrix pipe, a handle demoted off the 16-row launch): the per-frame path
  p.table = tokens && h2w && h2w_supports(K, 2 * C, C, 1, C) && q_launch;
  p.expand = tokens && !p.table;
  p.cols = p.table ? K : T;
  p.proj = h2w ? PROJ_H2W : B == 1 ? PROJ_ONE_GEMM : PROJ_LAYERS;
  if (!p.table) {
    p.quads = h2w && q_launch;
    p.quads_h_direct = h2w && bf16 && sw.cond_bf16_direct;
    p.quads_h_convert = bf16 && !p.quads_h_direct;
    p.rows = sw.cond_rows || !(p.quads || p.quads_h_direct);
  }
  const size_t bt = (size_t)B * T, tiles = (size_t)B * cdiv(T, 32);
  p.bt = bt;
  // the stack launch handles at most 2 workgroups per CU at a time (larger batches run as groups of rows, one after the other)
  p.flag_tiles = std::min(tiles, 2 * (size_t)h->num_cus);
  p.split_tiles = tiles;
  p.bt_h = bf16 ? bt : 0;
  p.tok = tokens ? bt : 0;
  p.planes = h2w ? (size_t)B * p.cols : 0;
  p.cond_tok = p.table ? (size_t)B * K : 0;
  p.cond_exp = p.expand ? bt : 0;
  p.quad_frames = p.quads ? bt : 0;
  p.row_frames = p.rows ? bt : 0;
  return p;
}

static int ensure_bind_ws(bsg_diffnet* h, BindPlan& p, hipStream_t st) {
  TRY(grow(h, &h->cap_bt, p.bt, st));
  TRY(grow(h, &h->flags_cap, p.flag_tiles, st));
  // once per handle, with their initial values: the launch epoch {1, 0} — epochs start at 1: a zeroed flag word is older than every launch
  // (flag values = epoch * 64 + layers published) — the profiling clocks, the bad-id word of the token conversion
  if (!h->epoch_dev) {
    TRY(own_alloc(h->owned, &h->epoch_dev, 2));
    const unsigned init[2] = {1u, 0u};
    BSG_HIP(hipMemcpy(h->epoch_dev, init, sizeof(init), hipMemcpyHostToDevice));
  }
  if (!h->clk) {
    TRY(own_alloc(h->owned, &h->clk, 4));
    BSG_HIP(hipMemsetAsync(h->clk, 0, 4 * sizeof(unsigned long long), st));
  }
  if (p.tokens && !h->tok_bad) TRY(own_alloc(h->owned, &h->tok_bad, 1));
  const struct { size_t* cap; size_t need; } groups[] = {{&h->split_cap, p.split_tiles},     {&h->cap_bt_h, p.bt_h},         {&h->cap_tok, p.tok},
                                                          {&h->cap_cond_planes, p.planes}, {&h->cap_cond_tok, p.cond_tok}, {&h->cap_cond_exp, p.cond_exp}};
  for (const auto& g : groups) TRY(grow(h, g.cap, g.need, st));
  TRY(grow(h, &h->cap_cond_q, p.quad_frames, st, GROW_SOFT));
  if (h->cap_cond_q < p.quad_frames) {
    // THE amendment of the plan: out of memory for the quads, so this binding writes the rows and the launches read those (dword loads: a
    // few per cent slower), nothing fails
    p.quads = false;
    p.quad_frames = 0;
    p.rows = true;
    p.row_frames = p.bt;
  }
  return grow(h, &h->cap_cond_rows, p.row_frames, st, GROW_LAZY);
}

// the arguments of the pre-split GEMM over `p.cols` columns per item (K token columns or T frames): batch index z = l B + b writes
// term[l][b] = W_l cond_b + (b_cond + b_dil) in the plan's layouts — [2C][cols] rows, lanes along the columns; the same epilogue stores the
// quads; the weights were split at create
static H2wArgs cond_gemm_args(const bsg_diffnet* h, const BindPlan& p, int B) {
  const int cols = p.cols;
  H2wArgs g{};
  g.act = h->cond_planes; g.act_plane = (long long)B * cols * C; g.lda = C; g.sAct = (long long)cols * C; g.wpack = h->wcond_pack;
  g.sW = (long long)2 * 2 * C * C; g.zdiv = B; g.rows = cols; g.K = C; g.Wn = 2 * C; g.taps = 1; g.act_is_a = 0;
  g.C = p.rows ? h->condterm : nullptr; g.ldc = cols; g.sC = (long long)2 * C * cols;
  g.Cq = p.table ? h->cond_tok : p.quads ? h->condterm_q : nullptr;
  g.Ch = p.quads_h_direct ? h->condterm_h : nullptr;
  g.bias = h->b_cond; g.sBias = 2 * C; g.alpha = 1.f; g.act_fn = ACT_NONE; g.batch = h->L * B;
  return g;
}

static int launch_bind(bsg_diffnet* h, const BindPlan& p, const float* cond, const float* cond_tok, const int64_t* tok, int B, int K, int T,
                       hipStream_t st) {
  const size_t bt = (size_t)B * T;
  if (p.tokens) {
    // the frames' token ids, converted and clamped once (the launches index the table with them unchecked)
    BSG_HIP(hipMemsetAsync(h->tok_bad, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(tok_convert_kernel, dim3(cdiv((long long)bt, 256)), dim3(256), 0, st, (const long long*)tok, h->tok_dev, (long long)bt, K, h->tok_bad);
    BSG_LAUNCH_CHECK();
    if (!is_capturing(st)) {   // (a captured binding cannot wait: its ids are clamped, not reported)
      unsigned bad = 0;
      BSG_HIP(hipMemcpyAsync(&bad, h->tok_bad, sizeof(unsigned), hipMemcpyDeviceToHost, st));
      BSG_HIP(hipStreamSynchronize(st));
      BSG_REQUIRE(bad == 0, "diffnet_prepare_tokens: %u token ids outside [0, K=%d)", bad, K);
    }
  }
  if (p.expand) {
    BSG_REQUIRE(B <= 65535, "diffnet_prepare_tokens: B=%d", B);
    hipLaunchKernelGGL(tok_expand_cond_kernel, dim3(cdiv(T, 256), C, B), dim3(256), 0, st, cond_tok, (const int*)h->tok_dev, h->cond_exp, K, T);
    BSG_LAUNCH_CHECK();
    cond = h->cond_exp;
  }
  if (p.proj == PROJ_H2W) {
    // the activation as hi / lo fp16 planes [B][cols][H]: the condition is transposed and split once; the token rows are [B][K][H] already,
    // so a split in place of the transposing split, then the SAME launch and epilogue with K columns per item instead of T
    const size_t n = (size_t)B * p.cols;
    if (p.table) TRY(h2w_split_rows(cond_tok, h->cond_planes, h->cond_planes + n * C, (long long)n, C, C, st));
    else TRY(h2w_split_transposed(cond, h->cond_planes, h->cond_planes + n * C, B, C, T, st));
    TRY(launch_gemm_h2w(cond_gemm_args(h, p, B), st));
  } else if (p.proj == PROJ_ONE_GEMM) {
    // a single utterance: the L projections are ONE GEMM of L x 2C rows ([L][2C][C] weights and [L][1][2C][T] outputs are contiguous) — twenty
    // launches of 64 workgroups each left most of the chip idle (1.0 -> 0.15 ms of a 25-ms pass)
    TRY(conv1x1(h->w_cond, h->b_cond, cond, h->condterm, h->L * 2 * C, C, 1, T, ACT_NONE, st));
  }
  for (int l = 0; l < h->L; ++l) {
    if (p.proj == PROJ_LAYERS)
      TRY(conv1x1(h->w_cond + (size_t)l * 2 * C * C, h->b_cond + (size_t)l * 2 * C, cond,
                  h->condterm + (size_t)l * 2 * C * bt, 2 * C, C, B, T, ACT_NONE, st));
    if (p.quads_h_convert)
      TRY(f32_to_quad_bf16(h->condterm + (size_t)l * 2 * C * bt, h->condterm_h + (size_t)l * 2 * C * bt, B, 2 * C, T, st));
  }
  return BSG_OK;
}

// bsg_diffnet_prepare (cond: [B][H][T]) and bsg_diffnet_prepare_tokens (cond null; cond_tok [B][K][H], tok [B][T]): workspaces, flags and the
// hoisted conditioner projection.  Nothing is bound while it runs: a failure at any point (bad token ids among them) leaves it so
static int prepare_impl(bsg_diffnet* h, const float* cond, const float* cond_tok, const int64_t* tok, int32_t B, int32_t K, int32_t T,
                        hipStream_t st) {
  h->bound = bsg_diffnet::Bound{};
  TRY(num_cus(h));
  BindPlan p = plan_bind(h, B, K, T, cond_tok != nullptr);
  TRY(ensure_bind_ws(h, p, st));
  TRY(launch_bind(h, p, cond, cond_tok, tok, B, K, T, st));
  bsg_diffnet::Bound b;
  b.B = B; b.T = T; b.compute = h->compute;
  b.tok = p.table; b.K = p.table ? K : 0;
  b.rows = p.rows; b.quads = p.quads; b.quads_h = p.quads_h_direct || p.quads_h_convert;
  h->bound = b;
  return BSG_OK;
}

extern "C" int bsg_diffnet_prepare(bsg_diffnet* h, const float* cond, int32_t B, int32_t T, void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  BSG_REQUIRE(h && cond, "diffnet_prepare: null argument");
  BSG_REQUIRE(B > 0 && T > 0, "diffnet_prepare: B=%d T=%d", B, T);
  BSG_REQUIRE((long long)B * T < (1LL << 31) / (2 * C), "diffnet_prepare: B*T=%lld too large", (long long)B * T);
  return prepare_impl(h, cond, nullptr, nullptr, B, 0, T, (hipStream_t)stream);
}

extern "C" int bsg_diffnet_prepare_tokens(bsg_diffnet* h, const float* cond_tok, const int64_t* tok, int32_t B, int32_t K, int32_t T, void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  BSG_REQUIRE(h && cond_tok && tok, "diffnet_prepare_tokens: null argument");
  BSG_REQUIRE(B > 0 && T > 0 && K > 0, "diffnet_prepare_tokens: B=%d K=%d T=%d", B, K, T);
  BSG_REQUIRE((long long)B * T < (1LL << 31) / (2 * C), "diffnet_prepare_tokens: B*T=%lld too large", (long long)B * T);
  BSG_REQUIRE((long long)B * K < (1LL << 31) / (2 * C), "diffnet_prepare_tokens: B*K=%lld too large", (long long)B * K);
  return prepare_impl(h, nullptr, cond_tok, tok, B, K, T, (hipStream_t)stream);
}

// GEMM1 of the residual block: BSG_WINO unset = 2: Winograd F(2,3) kernels, and the F(4,3) stack launch (diffnet_f43.hip) for launches
// that fill the chip with 64-frame tiles (plan_stack; BSG_STACK43=2: for any shape); 1: F(2,3) only; 0: the direct K=768 form
static bool use_wino() { return dn_switches().wino != 0; }

// A pair of workgroups per tile pays (a z exchange through L2) only when single workgroups would leave CUs idle: measured on
// MI355X at T=1000, B = 1 / 2 / 4 (32 / 64 / 128 tiles): 63 -> 41, 64 -> 42, 65 -> 47 us per layer; B = 6 (192 tiles): 68 -> 70.
// So: at most one workgroup per CU after the split, which also keeps every workgroup of the launch resident (the partner
// of a polling workgroup is always running).  Between 129 and 256 tiles the 16-wave form (no inter-workgroup traffic) takes over.
// BSG_SPLIT=0 disables both.
// The pair form runs with at most one workgroup per CU by construction of its threshold, but the dispatcher may still place two
// of them on one CU while others stay empty; asking for more than half of the CU's 160 KB of LDS (only 48 KB are used) makes
// that impossible.
static constexpr size_t kSplitLds = 84 * 1024;

// The fp32 per-layer launches.  LAYER_PLAIN: residual_layer_kernel<stamps, wino>, arguments (ResArgs a), 32-frame tiles: 48 KB of LDS -> 3
// workgroups per CU.  (Wider tiles of 64 / 128 frames were built and measured in round 1: 0-50 % slower at every batch size, because fewer
// workgroups per CU hide less of the L2 latency of the weight stream.)  The channel-split kernels, arguments (SplitArgs s): F(2,3) forms
// without stamps; the pair / 4-way form at the padded LDS size (one workgroup per CU by construction) or, small_lds, at the plain size (two
// chains share a CU); all of them are granted the padded size.
const KernelForm* bsg::layer_form(LayerForm layer, bool small_lds, bool stamps, bool wino) {
  constexpr size_t lds = (size_t)C * (32 + 2 * HALO) * sizeof(float);
  static const KernelForm plain[] = {
      {FORM_LAYER_DIRECT, (const void*)residual_layer_kernel<false, false>, nullptr, 512, lds, lds, "layer", nullptr},
      {FORM_LAYER_DIRECT_STAMPS, (const void*)residual_layer_kernel<true, false>, nullptr, 512, lds, lds, "layer", nullptr},
      {FORM_LAYER_WINO, (const void*)residual_layer_kernel<false, true>, nullptr, 512, lds, lds, "layer", nullptr},
      {FORM_LAYER_WINO_STAMPS, (const void*)residual_layer_kernel<true, true>, nullptr, 512, lds, lds, "layer", nullptr},
  };
  static const KernelForm split[] = {
      {FORM_SPLIT2, (const void*)residual_split_kernel<false, 2>, nullptr, 512, kSplitLds, kSplitLds, "split2", nullptr},
      {FORM_SPLIT2_SMALL, (const void*)residual_split_kernel<false, 2>, nullptr, 512, lds, kSplitLds, "split2", nullptr},
      {FORM_SPLIT4, (const void*)residual_split_kernel<false, 4>, nullptr, 256, kSplitLds, kSplitLds, "split4", nullptr},
      {FORM_SPLIT4_SMALL, (const void*)residual_split_kernel<false, 4>, nullptr, 256, lds, kSplitLds, "split4", nullptr},
      {FORM_WIDE, (const void*)residual_split_kernel<true, 1>, nullptr, 1024, lds, kSplitLds, "wide", nullptr},
  };
  switch (layer) {
    case LAYER_PLAIN: return &plain[2 * wino + stamps];
    case LAYER_SPLIT2: return &split[small_lds];
    case LAYER_SPLIT4: return &split[2 + small_lds];
    case LAYER_WIDE: return &split[4];
    default: return bf16_layer_form(stamps);
  }
}

// step_tail_kernel<mp, plms>: skip projection, output projection, sampler update of x (DDPM, or PLMS) and the next evaluation's
// in-projection.  Arguments (TailArgs a); one workgroup per 32-frame tile.
const KernelForm* bsg::tail_f32_form(int mp, bool plms) {
  constexpr size_t lds = (size_t)(C * 32 + 96 * 32) * sizeof(float);
  static const KernelForm forms[] = {
      {FORM_TAIL_F32_80, (const void*)step_tail_kernel<80, false>, nullptr, 512, lds, lds, "step_tail", nullptr},
      {FORM_TAIL_F32_96, (const void*)step_tail_kernel<96, false>, nullptr, 512, lds, lds, "step_tail", nullptr},
      {FORM_TAIL_F32_80_PLMS, (const void*)step_tail_kernel<80, true>, nullptr, 512, lds, lds, "step_tail", nullptr},
      {FORM_TAIL_F32_96_PLMS, (const void*)step_tail_kernel<96, true>, nullptr, 512, lds, lds, "step_tail", nullptr},
  };
  return &forms[2 * plms + (mp != 80)];
}

// The launches of a call: which form runs the L residual layers, and how the batch splits into launch groups.  plan_stack() decides it
// from the shape, the handle's state and what the plan is for (PlanScope), and writes nothing on the handle (what it asks of the device
// is kept in h->forms, a memo), so a query (bsg_diffnet_uses_handoffs, ragged_launch_ok) and the launch it predicts agree; every compute
// entry plans once and hands the plan to the launches, which read nothing else about the call.
enum PlanScope {
  PLAN_WHOLE,        // the whole batch of a call
  PLAN_HALF_BIG,     // half of a batch of more tiles than CUs (dual_fork): per-layer launches of the one-workgroup-per-tile kernel
  PLAN_HALF_SMALL,   // half of a smaller batch (dual_fork): the channel-split kernels without the LDS padding, so that workgroups of the
                     // two chains can share a CU
  PLAN_RAGGED,       // the bound ragged batch: its ragged stack launch, or STACK_NONE where the handle's state has none
};

struct StackPlan {
  const KernelForm* form = nullptr;   // the stack launch (diffnet_forms.h: its family, tile width, parts and variant); null: one launch per layer
  int rows = 0;         // rows per launch group (a ragged call: one launch per group of the plan bound by bsg_diffnet_prepare_ragged, rows = B)
  LayerForm layer = LAYER_PLAIN;   // no stack launch: the form of the per-layer launches
  bool small_lds = false;          // ... and the pair / 4-way form at the un-padded LDS size (PLAN_HALF_SMALL)
  int row0 = 0;         // the launches work on rows [row0, row0 + B) of the bound batch (the second half-batch chain of dual_fork)
  StackForm family() const { return form ? form->family : STACK_NONE; }
  int nct() const { return form ? form->nct : 2; }   // column tiles of 32 frames per workgroup: tiles of 32 * nct frames (F(4,3), bf16: 64)
  bool ragged() const { return form && form->variant == FORM_RAGGED; }
  bool tok() const { return form && form->variant == FORM_TOKEN; }   // the launch gathers the conditioner term from the token table
};

// the channel-split form of a per-layer launch of B x T (LAYER_PLAIN: none); small_lds: at the un-padded LDS size
static LayerForm use_split(const bsg_diffnet* h, int B, int T, bool small_lds) {
  const int env = dn_switches().split;
  if (!env || h->split_off || !h->num_cus || !h->zbuf) return LAYER_PLAIN;
  const long long tiles = (long long)B * cdiv(T, 32);
  if ((size_t)tiles > h->split_cap) return LAYER_PLAIN;
  // residency is what makes a hand-off terminate: every workgroup of the launch (and, for two chains sharing CUs, of both
  // launches: dual_scope checks that sum) must fit the device at the LDS size actually launched
  auto fits = [&](LayerForm f) { return h->forms.resident(*layer_form(f, small_lds, false, true)) >= 1; };
  if (4 * tiles <= h->num_cus && env != 2 && fits(LAYER_SPLIT4)) return LAYER_SPLIT4;   // BSG_SPLIT=2: no 4-way split (A/B measurements)
  if (2 * tiles <= h->num_cus) return fits(LAYER_SPLIT2) ? LAYER_SPLIT2 : LAYER_PLAIN;
  if (tiles <= h->num_cus && env != 3) return fits(LAYER_WIDE) ? LAYER_WIDE : LAYER_PLAIN;   // BSG_SPLIT=3: pair form only (A/B measurements)
  return LAYER_PLAIN;
}

// The per-layer launch of B x T rows: what a plan without a stack form runs, and all that the entries of ONE layer plan
// (bsg_diffnet_residual_layer, bsg_diffnet_debug_stamps: they never take a stack launch).  The channel-split kernels are F(2,3) forms of
// the fp32 configuration and carry no stamps; the half of a big batch keeps the one-workgroup-per-tile kernel.
static void plan_layer(const bsg_diffnet* h, StackPlan& plan, int B, int T, PlanScope scope, bool stamps = false) {
  plan.small_lds = scope == PLAN_HALF_SMALL;
  if (h->compute == BSG_COMPUTE_BF16) plan.layer = LAYER_BF16;
  else plan.layer = !stamps && use_wino() && scope != PLAN_HALF_BIG ? use_split(h, B, T, plan.small_lds) : LAYER_PLAIN;
}

// one layer of rows [plan.row0, plan.row0 + B) in the form plan.layer
static int launch_layer(bsg_diffnet* h, const StackPlan& plan, int layer, const float* x_in, const long long* t_dev, int t_uniform, float* x_out,
                        float* skip, int B, int T, hipStream_t st, unsigned long long* stamps = nullptr) {
  ResArgs a{};
  a.x_in = x_in; a.x_out = x_out; a.skip = skip;
  a.condterm = h->condterm + ((size_t)layer * h->bound.B + plan.row0) * 2 * C * (size_t)T;   // [L][B bound][2C][T], this launch's rows
  a.dproj = h->dproj; a.t_dev = t_dev; a.t_uniform = t_uniform;
  a.apack1 = h->apack1 + (size_t)layer * 2 * C * 3 * C;
  a.apack2 = h->apack2 + (size_t)layer * 2 * C * C;
  a.apackw = h->apackw + (size_t)layer * 4 * 2 * C * C;
  a.apackw43 = h->apackw43 + (size_t)layer * 6 * 2 * C * C;
  a.apack1h = h->apack1h + (size_t)layer * 2 * C * 3 * C;
  a.apack2h = h->apack2h + (size_t)layer * 2 * C * C;
  a.bias_out = h->b_out + (size_t)layer * 2 * C;
  a.B = B; a.T = T; a.L = h->L; a.layer = layer;
  a.dil = 1 << (layer % h->cfg.dilation_cycle_length);
  a.first = layer == 0;
  a.skip_div = layer == h->L - 1 ? sqrtf((float)h->L) : 1.0f;
  a.stamps = stamps;
  const LayerForm form = plan.layer;
  const KernelForm& kf = *layer_form(form, plan.small_lds, stamps != nullptr, use_wino());
  dim3 grid;
  void* args[1] = {&a};
  SplitArgs s{};
  if (form == LAYER_SPLIT2 || form == LAYER_SPLIT4 || form == LAYER_WIDE) {
    // small launch: a pair of workgroups per tile, each half of the channels (residual_split_kernel)
    a.tiles_per_row = cdiv(T, 32);
    s.base = a;
    s.apack2w = h->apack2w + (size_t)layer * 2 * C * C;
    // exchange tiles and flags of this launch's rows (two half-batch chains may be in flight at once)
    const size_t tile0 = (size_t)plan.row0 * a.tiles_per_row;
    s.zbuf = h->zbuf + tile0 * C * 32;
    s.flags = h->split_flags + tile0 * 16;
    s.status = h->split_flags + 16 * h->split_cap;
    if (++h->split_epoch == 0) h->split_epoch = 1;
    s.epoch = h->split_epoch;
    if (h->inject_giveup > 0 && form != LAYER_WIDE) { s.inject = 1; --h->inject_giveup; }
    args[0] = &s;
    grid = dim3((form == LAYER_WIDE ? 1 : form == LAYER_SPLIT4 ? 4 : 2) * B * a.tiles_per_row);
  } else {
    a.tiles_per_row = cdiv(T, form == LAYER_BF16 ? 64 : 32);
    grid = dim3(8 * cdiv(B * a.tiles_per_row, 8));   // see the tile order in residual_layer_kernel / residual_layer_bf16_kernel
  }
  const bool ext = form == LAYER_BF16 && skip != h->skip + (size_t)plan.row0 * C * T;
  if (form == LAYER_BF16) {
    // the running skip sum lives in h->skip_h (bf16); a caller-supplied fp32 buffer (the unit-test hook) is converted
    // in and out around the launch
    a.condterm_h = h->condterm_h + ((size_t)layer * h->bound.B + plan.row0) * 2 * C * (size_t)T;
    a.skip_h = h->skip_h + (size_t)plan.row0 * C * T;
    if (ext && !a.first) TRY(f32_to_quad_bf16(skip, h->skip_h, B, C, T, st));
  }
  TRY(launch_form(h->forms, kf, false, grid, args, st));
  h->last_path = kf.name;
  h->last_groups = 0;
  return ext ? quad_bf16_to_f32(h->skip_h, skip, B, C, T, st) : BSG_OK;
}

// A tile row is ceil(T / (32 nct)) workgroups that wait for each other, and every workgroup of a launch must be resident: at most
// occ x CUs workgroups, whole rows only.  It pays when a launch has more workgroups than CUs (two per CU overlap each other's waits);
// smaller launches keep the channel-split kernels.  `ragged`: the ragged stack launch of the bound batch (bsg_diffnet_prepare_ragged), if
// the handle's state has one.  Leaves plan.form null where no stack launch runs.
static void stack_form(const bsg_diffnet* h, StackPlan& plan, int B, int T, hipStream_t st, bool ragged) {
  const DnSwitches& sw = dn_switches();
  const bool exchange = !h->split_off && h->num_cus && h->hx && h->epoch_dev;   // hand-off launches are on, and prepare has allocated their edge exchange
  auto fits = [&](const KernelForm* f) { return f && h->forms.resident(*f) >= 1; };
  if (h->compute == BSG_COMPUTE_BF16) {
    // bf16-operand configuration: the stack launch (the default; BSG_STACK_BF16=0 selects per-layer launches).  64-frame tiles, one
    // workgroup per CU (256 registers per wave), whole rows per launch group.  Measured on one box, ms per 100-step pass at T=1000,
    // stack / per-layer: B=1 43.2 / 56.4, B=16 58.2 / 87.8, B=32 109.7 / 133.3, B=64 213.8 / 237.3 (tools/bench_small.py with
    // BSG_DTYPE=bf16).  Per layer and tile ~21.5 us, of which the two GEMMs' MFMAs are ~7.  Whether it is taken
    // does not depend on B.
    if (!sw.stack_bf16 || !exchange || !fits(bf16_stack_form(false))) return;
    const int tpr = cdiv(T, 64);
    const long long slots = h->num_cus;
    if (ragged) {   // residual_stack_bf16_varlen_kernel: groups from the bound plan
      if (fits(bf16_stack_form(true))) { plan.form = bf16_stack_form(true); plan.rows = B; }
    } else if (tpr <= slots) {
      plan.form = bf16_stack_form(false);
      plan.rows = slots / tpr < B ? (int)(slots / tpr) : B;
    }
    return;
  }
  if (ragged) {
    // the ragged form of the 16-row launch on 64-frame tiles, groups from the bound plan.  Not on a handle that was demoted off the 16-row
    // launch (bsg_diffnet_set_h2q / set_h2 / set_split 0, or the process switches BSG_H2 / BSG_H2_Q = 0), and it reads the conditioner
    // term's channel quads only
    if (sw.h2 && sw.h2_q && !h->h2_off && !h->q_off && exchange && h->apack1q && h->apack2q && h->dconv && h->bound.quads) {
      const KernelForm* f = h2q_form(2, FORM_RAGGED, true, 0);
      if (fits(f)) { plan.form = f; plan.rows = B; }
    }
    return;
  }
  {
    // split-fp16 form (diffnet_h2.hip): fp32 operands as hi + lo fp16 terms on the 16-bit matrix pipe; 64-frame tiles, one workgroup per
    // CU, whole rows per launch group, every batch size.  BSG_H2=0 / bsg_diffnet_set_h2(h, 0): off (the kernels of the fp32 matrix pipe)
    // (round 4: the launch epoch of the flags lives in device memory, so these launches can be captured and replayed; only the part forms'
    // exchange buffers must exist already — their first eager call allocates them)
    const bool capturing = is_capturing(st);
    if (sw.h2 && !h->h2_off && h->compute == BSG_COMPUTE_F32 && exchange && h->apack1s) {
      // tile width: 32 frames (one column tile per workgroup) while those tiles fit ONE launch group, else 64 frames (two column tiles:
      // half the weight stream per frame).  ms per 100-step pass at T = 1000 on one box (tools/bench_small.py), 32-frame / 64-frame /
      // fp32-pipe kernels (BSG_H2=0):  B=1 55 / 70 / 60,  B=2 53 / 70 / 64,  B=4 52 / 70 / 84,  B=6 56 / 74 / 119,  B=8 69 / 76 / 132,
      // B=10 115 / 80 / 187,  B=12 113 / 87 / 198,  B=16 134 / 103 / 200 — so the launch is taken for every batch size (BSG_H2_NCT=1 / 2
      // forces a width)
      const int env_nct = sw.h2_nct;
      int nct = (long long)B * cdiv(T, 32) > h->num_cus ? 2 : 1;
      if (env_nct == 1 || env_nct == 2) nct = env_nct;
      {
        // part forms (residual_part_h2_kernel): several workgroups on as many CUs of an XCD share a tile, each a part of the channels and of
        // the weight stream; the whole batch in one launch.  Quads of 32-frame tiles while B * ceil(T / 32) <= CUs / 4 (one or two utterances
        // at T = 1000), quads of 64-frame tiles while B * ceil(T / 64) <= CUs / 4 (B <= 4), pairs of 64-frame tiles (8 waves each) while
        // B * ceil(T / 64) <= CUs / 2 (B <= 8).  ms per 100-step pass at T = 1000, one workgroup per tile / part form: B=1 54.5 / 24.1,
        // B=2 52.6 / 25.4, B=3 52.0 / 32.0, B=4 51.5 / 35.0, B=5 54.8 / 46.0, B=6 57.1 / 49.6, B=8 69.1 / 59.4.  BSG_H2_PART=0: none
        // (BSG_H2_QUAD=0 / BSG_H2_QUAD64=0 / BSG_H2_PAIR64=0: not that form)
        auto part = [&](int parts, int pn) {
          if (!fits(part_form(parts, pn))) return false;
          plan.form = part_form(parts, pn); plan.rows = B;
          return true;
        };
        const long long t32 = (long long)B * cdiv(T, 32), t64 = (long long)B * cdiv(T, 64);
        const bool part_bufs = !capturing || (size_t)(2 * t64) <= h->part_cap;   // (sized in 32-frame tile equivalents; 2 t64 >= t32)
        if (sw.h2_part && !h->parts_off && env_nct == 0 && h->apack1q && part_bufs) {
          if (sw.h2_quad && 4 * 8 * cdiv(t32, 8) <= h->num_cus && part(4, 1)) return;
          if (sw.h2_quad64 && 4 * 8 * cdiv(t64, 8) <= h->num_cus && part(4, 2)) return;
          if (sw.h2_pair64 && 2 * 8 * cdiv(t64, 8) <= h->num_cus && part(2, 2)) return;
        }
      }
      // 16-row matrix tiles (residual_stack_q_kernel, diffnet_h2q.hip; round 5): the same launch with every product a v_mfma_f32_16x16x32_f16 —
      // the same matrix cycles, but the chip holds a higher clock under that shape.  BSG_H2_Q=0: the 32-row form (residual_stack_h2_kernel)
      // (the form launched is the one BSG_H2Q_FAIR / BSG_H2Q_DIAG select; whether the 16-row launch fits is asked of its default form)
      const bool q = sw.h2_q && !h->q_off && h->apack1q && h->apack2q && fits(h2q_form(nct, FORM_PLAIN, true, 0));
      const int tpr = cdiv(T, 32 * nct);
      if ((q || fits(h2_form(nct))) && tpr <= h->num_cus) {
        plan.form = q ? h2q_form(nct, FORM_PLAIN, sw.h2q_fair != 0, sw.h2q_diag) : h2_form(nct);
        plan.rows = h->num_cus / tpr < B ? h->num_cus / tpr : B;
        // the token form: a token binding, the 16-row launch at 64-frame tiles (BSG_COND_TOK=0: the expanded per-frame term instead)
        if (q && nct == 2 && h->bound.tok && sw.cond_tok && fits(h2q_form(2, FORM_TOKEN, true, 0))) plan.form = h2q_form(2, FORM_TOKEN, true, 0);
        return;
      }
    }
  }
  if (sw.wino == 2) {
    // F(4,3) form (diffnet_f43.hip): 64-frame tiles, one workgroup per CU, whole rows per launch group; BSG_STACK43=0 keeps per-layer
    // launches.  A launch group takes the same time whatever part of the chip it fills, so the form is taken when the groups are
    // >= 90 % full (B = 15, 16, 29..32, .. at T = 1000): it is ~6 % faster than two chains of per-layer F(2,3) launches, not more.
    const int env43 = sw.stack43;
    if (env43 && h->compute == BSG_COMPUTE_F32 && exchange) {
      const int tpr43 = cdiv(T, 64);
      if (fits(f43_form()) && tpr43 <= h->num_cus) {
        const int rows43 = h->num_cus / tpr43 < B ? h->num_cus / tpr43 : B;
        const int groups = cdiv(B, rows43);
        if (env43 == 2 || (long long)B * tpr43 * 10 >= (long long)groups * h->num_cus * 9) {   // BSG_STACK43=2: any shape (tests)
          plan.form = f43_form();
          plan.rows = rows43;
        }
      }
    }
  }
}

static StackPlan plan_stack(const bsg_diffnet* h, int B, int T, hipStream_t st, PlanScope scope = PLAN_WHOLE) {
  StackPlan plan;
  if (scope != PLAN_HALF_BIG) stack_form(h, plan, B, T, st, scope == PLAN_RAGGED);
  if (!plan.form && scope != PLAN_RAGGED) plan_layer(h, plan, B, T, scope);
  return plan;
}

// The arguments of launch group g: rows [r0, r0 + nb) of this call's batch (r0 = g x plan.rows), or group g of the bound ragged plan —
// a workgroup then finds its row and tile in the group's table, and every pointer is the bound batch's row 0 (rows are not contiguous
// inside a group).
// Flag values of one stack launch: launch epoch x 64 + layers published (L < 64).  The launch epoch of the handle's flags lives in device
// memory (round 4: a captured launch can be replayed): every workgroup reads it at entry, the last one through its layers advances it and,
// before the 32-bit flag values could come round to a slot that was last written long ago (a large tile index after > 2^25 launches of
// smaller batches), zeroes the flags and starts the epochs again (diffnet_res.h).
static int stack_args(bsg_diffnet* h, const StackPlan& plan, int g, const long long* t_dev, int t_uniform, int B, int T, hipStream_t st,
                      unsigned long long* stamps, StackArgs& p) {
  const int tpr = cdiv(T, 32 * plan.nct());
  const int r0 = plan.ragged() ? 0 : g * plan.rows;
  const int nb = B - r0 < plan.rows ? B - r0 : plan.rows;
  const size_t row = (size_t)plan.row0 + r0;
  p = StackArgs{};
  p.x_in = h->xa + row * C * T;
  p.skip = h->skip + row * C * T;
  p.dproj = h->dproj; p.t_dev = t_dev ? t_dev + r0 : nullptr; p.t_uniform = t_uniform;
  p.bias_out = h->b_out;
  p.T = T; p.L = h->L; p.tiles_per_row = tpr;
  p.ct_stride = (long long)2 * C * h->bound.B * T;   // bound batch: per-layer stride of the conditioner term
  p.n_tiles = plan.ragged() ? h->rg_group_tiles[g] : nb * tpr; p.cycle = h->cfg.dilation_cycle_length;
  BSG_REQUIRE((size_t)p.n_tiles <= h->flags_cap && h->L < 64, "stack launch: %d tiles exceed the exchange array (%zu)", p.n_tiles, h->flags_cap);
  p.hx = h->hx; p.flags = h->flags; p.status = h->flags + h->flags_cap;
  BSG_REQUIRE(h->epoch_dev, "stack launch: no launch epoch (bsg_diffnet_prepare allocates it)");
  p.epoch = h->epoch_dev;
  p.fbase = 0;
  p.flag_words = (int)h->flags_cap;
  p.pflag_words = 0;   // part forms: set with p.pflags
  // the flags a wrapping launch zeroes: BOTH arrays of the handle, whichever form wraps (a part launch replaces these with its own below)
  p.wrap_pflags = h->part_flags;
  p.wrap_pflag_words = h->part_flags ? (int)(2 * h->part_cap * 4) : 0;
  if (dn_switches().debug_wrap_r04) { p.wrap_pflags = nullptr; p.wrap_pflag_words = 0; }
  const bool part = plan.family() == STACK_PART;
  if (h->inject_giveup > 0) { p.inject = 1; --h->inject_giveup; }
  else if (h->inject_xcc > 0 && part) { p.inject = 2; --h->inject_xcc; }
  else if (h->inject_nowait > 0 && part) { p.inject = 3; --h->inject_nowait; }
  p.stamps = stamps && g == 0 ? stamps : nullptr;
  p.clk = h->prof_on && g == 0 ? h->clk : nullptr;
  if (plan.ragged()) {
    p.vl_len = h->rg_dev;
    p.vl_tiles = reinterpret_cast<const int2*>(h->rg_dev + ((h->bound.B + 1) & ~1)) + h->rg_group_off[g];   // the tables follow the lengths
  }
  if (plan.family() == STACK_BF16) {
    p.skip_h = h->skip_h + row * C * T;
    p.condterm_h = h->condterm_h + row * 2 * C * T;
    p.apack1h = h->apack1h; p.apack2h = h->apack2h;
    return BSG_OK;
  }
  p.condterm = h->condterm + row * 2 * C * T;
  p.dconv = h->dconv; p.apackw = h->apackw; p.apack2 = h->apack2;
  if (stamps) p.stamp_mode = live_stamp_mode();
  if (plan.family() == STACK_F43) {
    p.apackw43 = h->apackw43;
    return BSG_OK;
  }
  p.apack1s = h->apack1s; p.apack2s = h->apack2s; p.h2_scale = h->h2_scale;
  p.apack1q = h->apack1q; p.apack2q = h->apack2q;
  p.condterm_q = plan.family() != STACK_H2 && h->bound.quads ? h->condterm_q + row * 2 * C * T : nullptr;
  if (plan.family() == STACK_H2Q) BSG_REQUIRE(p.apack1q && p.apack2q && p.dconv, "16-row stack launch: the 16-row weight fragments / the step-term table are missing");
  if (plan.tok()) {
    BSG_REQUIRE(h->bound.tok && h->cond_tok && h->tok_dev && h->bound.K > 0, "stack launch: no token binding");
    p.condterm_q = h->cond_tok + row * 2 * C * h->bound.K;
    p.ct_stride = (long long)2 * C * h->bound.B * h->bound.K;
    p.tok = h->tok_dev + row * T;
    p.tok_K = h->bound.K;
  }
  if (part) {
    // the exchange buffers for this launch's 32-frame tile equivalents, at least one per CU; a shape's first eager call allocates them
    TRY(grow(h, &h->part_cap, std::max((size_t)h->num_cus, (size_t)p.n_tiles * plan.nct()), st, GROW_LAZY));
    p.zx = h->part_zx; p.ix = h->part_ix; p.pflags = h->part_flags;
    BSG_REQUIRE(p.zx && p.ix && p.hx && p.pflags && p.apack1q && p.apack2q, "part launch: exchange buffers / 16-row weight fragments missing");
    p.pflag_words = (int)(2 * h->part_cap * 4);
    p.wrap_pflags = h->part_flags; p.wrap_pflag_words = p.pflag_words;   // (also under BSG_DEBUG_WRAP_R04: a part launch always zeroed its own)
  }
  return BSG_OK;
}

// `a` moved to the rows starting r rows further on: the tensors a launch group or a half-batch chain works on, and its Philox index
static TailArgs tail_rows(TailArgs a, size_t r) {
  const size_t mo = r * a.M * a.T;
  a.x += mo; a.xa_next += r * C * a.T; a.quad_row0 += mo;
  if (a.e_new) a.e_new += mo;
  for (const float** p : {&a.noise, &a.h1, &a.h2, &a.h3}) if (*p) *p += mo;
  return a;
}

// the planned stack launch of rows [plan.row0, plan.row0 + B): its launch groups one after the other on `st`; `tail`: the sampler
// step's tail in the same launch (split-fp16 forms)
static int launch_stack(bsg_diffnet* h, const StackPlan& plan, const long long* t_dev, int t_uniform, int B, int T, hipStream_t st,
                        unsigned long long* stamps = nullptr, const TailArgs* tail = nullptr) {
  BSG_REQUIRE(plan.form && plan.rows > 0, "stack launch: no launch form selected");
  const KernelForm& f = *plan.form;
  BSG_REQUIRE(!tail || f.fn_tail, "stack launch: a fused tail needs the split-fp16 form");
  BSG_REQUIRE(f.family != STACK_PART || plan.rows >= B, "part launch: whole batch");
  BSG_REQUIRE(!plan.ragged() || (h->bound.ragged && h->rg_dev && plan.row0 == 0 && (f.family == STACK_BF16 || h->bound.quads)),
              "ragged stack launch: no ragged plan / conditioner quads bound");
  const int groups = plan.ragged() ? (int)h->rg_group_tiles.size() : cdiv(B, plan.rows);
  for (int g = 0; g < groups; ++g) {
    StackArgs p;
    TRY(stack_args(h, plan, g, t_dev, t_uniform, B, T, st, stamps, p));
    // the step tail in the same launch: its tensors start at this launch group's first row
    TailArgs a = tail ? tail_rows(*tail, plan.ragged() ? 0 : (size_t)g * plan.rows) : TailArgs{};
    void* args[] = {&p, &a};   // (the forms without a tail instantiation take p alone)
    TRY(launch_form(h->forms, f, tail != nullptr, dim3(8 * (f.parts ? f.parts : 1) * cdiv(p.n_tiles, 8)), args, st));
  }
  h->last_path = tail ? f.name_tail : f.name;
  h->last_groups = groups;
  return BSG_OK;
}

static int check_bound(bsg_diffnet* h, int B, int T, const char* who) {
  if (!h) { set_error("%s: null handle", who); return BSG_EINVAL; }
  if (h->bound.B == 0 || h->bound.B != B || h->bound.T != T) {
    set_error("%s: (B=%d,T=%d) does not match the condition bound by bsg_diffnet_prepare (B=%d,T=%d)", who, B, T, h->bound.B, h->bound.T);
    return BSG_ESTATE;
  }
  if (h->compute != h->bound.compute) {
    // (either way: a BF16 prepare writes the bf16 quads only — since round 5 no fp32 copy — and an F32 prepare no bf16 quads)
    set_error("%s: the condition was bound under another bsg_diffnet_set_compute mode (%d) than the current one (%d); call bsg_diffnet_prepare again", who,
              h->bound.compute, h->compute);
    return BSG_ESTATE;
  }
  return BSG_OK;
}

// The step tail, what runs after the stack in a sampler step: skip and output projection, the DDPM or PLMS update of x, the next evaluation's input
// projection.  plan_tail() alone decides its form, from the handle's state and the stack plan of its rows ("Which tail runs").
enum TailForm {
  TAIL_UNFUSED,       // no fused tail (BSG_NO_FUSED_TAIL, or no packed tail weights): forward_impl + ddpm_step_kernel / plms_step_kernel
  TAIL_IN_STACK,      // inside the split-fp16 stack launch (residual_stack_h2_kernel / residual_stack_q_kernel with a TailArgs)
  TAIL_H2,            // step_tail_h2_kernel behind a part launch
  TAIL_F32,           // step_tail_kernel<MP, plms> on the fp32 matrix pipe
  TAIL_BF16,          // step_tail_bf16_kernel (bf16 configuration; BSG_TAIL_BF16=0: TAIL_F32)
  TAIL_BF16_RAGGED,   // step_tail_bf16_varlen_kernel: one launch over the tiles of every launch group of the bound ragged batch
};

struct TailPlan {
  TailForm form = TAIL_UNFUSED;
  int tile = 32;           // frames per tile that TailArgs::tiles_per_row counts: 64 in the stack launch, 32 for the launches of their own
  int mp = 0;              // TAIL_F32: in_dims padded to a multiple of 8, the instantiation of step_tail_kernel (80 or 96)
  bool first_h2 = false;   // a DDPM call's first input projection: in_proj_h2_kernel (the split-fp16 tails), else the generic GEMM
};

// A ragged plan takes the tail on the 16-bit matrix pipe whatever BSG_H2_TAIL says: its launch has no other fp32 tail.
static TailPlan plan_tail(const bsg_diffnet* h, const StackPlan& plan) {
  TailPlan tp;
  tp.mp = h->MP;
  if (!h->ws_pack || (tp.mp != 80 && tp.mp != 96) || live_no_fused_tail()) return tp;
  const bool h2 = h->tail_s && h->M <= 96 && (plan.ragged() || dn_switches().h2_tail);
  if (h2 && (plan.family() == STACK_H2 || plan.family() == STACK_H2Q)) { tp.form = TAIL_IN_STACK; tp.tile = 64; }
  else if (h2 && plan.family() == STACK_PART) tp.form = TAIL_H2;
  else if (h->compute == BSG_COMPUTE_BF16 && live_tail_bf16() && h->tail_h) tp.form = plan.ragged() ? TAIL_BF16_RAGGED : TAIL_BF16;
  else tp.form = TAIL_F32;
  tp.first_h2 = tp.form == TAIL_IN_STACK || tp.form == TAIL_H2;
  return tp;
}

// Can the handle's CURRENT state decode the bound ragged batch with the ragged launch?  When its ragged plan has a stack launch
// (stack_form: the conditions of the launch itself) and the tail that launch needs (plan_tail): in the fp32 configuration the one inside
// the launch, in the bf16 configuration the ragged bf16 step tail.  (The callers otherwise decode the rows one by one.)
static bool ragged_launch_ok(const bsg_diffnet* h) {
  if (!h->bound.ragged || h->bound.compute != h->compute) return false;
  const StackPlan plan = plan_stack(h, h->bound.B, h->bound.T, nullptr, PLAN_RAGGED);
  const TailForm tail = plan_tail(h, plan).form;
  return plan.family() != STACK_NONE && (tail == TAIL_IN_STACK || tail == TAIL_BF16_RAGGED);
}

// entry of a compute call on a ragged binding: refused under stream capture and where the handle has no ragged launch
static int ragged_enter(bsg_diffnet* h, hipStream_t st, const char* who) {
  if (!h->bound.ragged) return BSG_OK;
  if (is_capturing(st)) {
    set_error("%s: a ragged batch (bsg_diffnet_prepare_ragged) cannot be captured; run it eagerly", who);
    return BSG_ESTATE;
  }
  if (!ragged_launch_ok(h)) {
    set_error("%s: the bound ragged batch has no ragged launch in this handle's state (bsg_diffnet_ragged_native = 0): decode its rows one by one", who);
    return BSG_ESTATE;
  }
  return BSG_OK;
}

// Does the launch this shape takes read the ROW layout of the conditioner term?  (The 16-row stack launch and the part forms read the quads,
// the bf16 launches the bf16 quads; everything else — 32-row launch, F(4,3), per-layer and channel-split kernels — the rows.)
static bool cond_rows_needed(const bsg_diffnet* h, const StackPlan& plan) {
  if (h->bound.quads_h) return false;
  return !((plan.family() == STACK_H2Q || plan.family() == STACK_PART) && h->bound.quads);
}
// (behind a token binding: nothing for the token form, the expanded quads for the other launches that read quads, the rows for the rest)
static int cond_layout_for(bsg_diffnet* h, const StackPlan& plan, hipStream_t st) {
  if (plan.tok()) return BSG_OK;
  if (h->bound.tok && (plan.family() == STACK_H2Q || plan.family() == STACK_PART)) TRY(ensure_cond_quads(h, st));
  return cond_rows_needed(h, plan) ? ensure_cond_rows(h, st) : BSG_OK;
}

// The L residual layers of one evaluation of rows [plan.row0, plan.row0 + B): input h->xa (the in-projection of x), output the skip sum
// in h->skip(_h).  The planned stack launch — with the sampler step's tail inside it when `tail` is given — or one launch per layer.
static int run_layers(bsg_diffnet* h, const StackPlan& plan, const long long* t_dev, int t_uniform, int B, int T, hipStream_t st,
                      const TailArgs* tail = nullptr) {
  const bool prof = h->prof_on && h->prof_used + 2 <= h->prof_ev.size();
  if (prof) BSG_HIP(hipEventRecord(h->prof_ev[h->prof_used], st));
  if (plan.family() != STACK_NONE) {
    TRY(launch_stack(h, plan, t_dev, t_uniform, B, T, st, nullptr, tail));
  } else {
    const size_t off = (size_t)plan.row0 * C * T;
    float* cur = h->xa + off;
    float* nxt = h->xb + off;
    for (int l = 0; l < h->L; ++l) {
      TRY(launch_layer(h, plan, l, cur, t_dev, t_uniform, nxt, h->skip + off, B, T, st));
      float* tmp = cur; cur = nxt; nxt = tmp;
    }
  }
  if (prof) {
    BSG_HIP(hipEventRecord(h->prof_ev[h->prof_used + 1], st));
    h->prof_used += 2;
    h->prof_launches += h->L;   // layer-equivalents (a stack launch runs L layers in one kernel; a fused tail is ~1 % of its FLOPs)
  }
  return BSG_OK;
}

// eps = DiffNet(x, t); t either per-row on the device or uniform
static int forward_impl(bsg_diffnet* h, const StackPlan& plan, const float* x, const long long* t_dev, int t_uniform, float* eps, int B, int T,
                        hipStream_t st) {
  TRY(conv1x1(h->w_in, h->b_in, x, h->xa, C, h->M, B, T, ACT_RELU, st));  // net.py:116-118
  TRY(run_layers(h, plan, t_dev, t_uniform, B, T, st));
  if (h->compute == BSG_COMPUTE_BF16) TRY(quad_bf16_to_f32(h->skip_h, h->skip, B, C, T, st));
  if (plan.ragged()) {   // ragged: the stack launch stored no skip sum at a row's padding; the projections below read every frame of B x T
    hipLaunchKernelGGL(ragged_zero_pad_kernel, dim3(cdiv(T, 256), C, B), dim3(256), 0, st, h->skip, (const int*)h->rg_dev, C, T);
    BSG_LAUNCH_CHECK();
  }
  TRY(conv1x1(h->w_skip, h->b_skip, h->skip, h->hid, C, C, B, T, ACT_RELU, st));   // net.py:127-128
  TRY(conv1x1(h->w_fin, h->b_fin, h->hid, eps, h->M, C, B, T, ACT_NONE, st));      // net.py:129
  if (plan.ragged()) {   // ragged: the projections above ran on every frame of B x T; the padding's eps is 0
    hipLaunchKernelGGL(ragged_zero_pad_kernel, dim3(cdiv(T, 256), h->M, B), dim3(256), 0, st, eps, (const int*)h->rg_dev, h->M, T);
    BSG_LAUNCH_CHECK();
  }
  return BSG_OK;
}

extern "C" int bsg_diffnet_forward(bsg_diffnet* h, const float* x, const int64_t* t, float* eps, int32_t B, int32_t T,
                                   void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  TRY(check_bound(h, B, T, "diffnet_forward"));
  BSG_REQUIRE(x && t && eps, "diffnet_forward: null argument");
  TRY(ragged_enter(h, (hipStream_t)stream, "diffnet_forward"));
  const StackPlan plan = plan_stack(h, B, T, (hipStream_t)stream, h->bound.ragged ? PLAN_RAGGED : PLAN_WHOLE);
  TRY(cond_layout_for(h, plan, (hipStream_t)stream));
  return forward_impl(h, plan, x, (const long long*)t, 0, eps, B, T, (hipStream_t)stream);
}

extern "C" int bsg_diffnet_residual_layer(bsg_diffnet* h, int32_t layer, const float* x_in, const int64_t* t, float* x_out,
                                          float* skip, int32_t B, int32_t T, void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  TRY(check_bound(h, B, T, "diffnet_residual_layer"));
  BSG_REQUIRE(x_in && t && x_out && skip && x_in != x_out, "diffnet_residual_layer: null or aliased argument");
  BSG_REQUIRE(layer >= 0 && layer < h->L, "diffnet_residual_layer: layer %d out of range", layer);
  if (h->compute == BSG_COMPUTE_F32) TRY(ensure_cond_rows(h, (hipStream_t)stream));
  StackPlan plan;
  plan_layer(h, plan, B, T, PLAN_WHOLE);
  return launch_layer(h, plan, layer, x_in, (const long long*)t, 0, x_out, skip, B, T, (hipStream_t)stream);
}

// rows [plan.row0, plan.row0 + B) of a sampler call's batch on stream st: their stack plan, the tail behind it and the tail's arguments
struct SubBatch { int B; hipStream_t st; StackPlan plan; TailPlan tail; TailArgs args; };

// The chain of B rows from plan.row0 of x [.][M][T].  args: what the handle and the plans decide of its tail's arguments, filled once per call
// (a step adds the sampler's own fields); x and xa_next at the call's row 0 (tail_rows moves them with the sampler's tensors), the chain's skip sum
static SubBatch sub_batch(const bsg_diffnet* h, const StackPlan& plan, float* x, int B, int T, hipStream_t st) {
  SubBatch sub{B, st, plan, plan_tail(h, plan), TailArgs{}};
  const size_t off = (size_t)plan.row0 * C * T;
  TailArgs& a = sub.args;
  a.x = x; a.xa_next = h->xa;
  a.skip = h->skip + off; a.skip_h = h->compute == BSG_COMPUTE_BF16 ? h->skip_h + off : nullptr;
  a.b_skip = h->b_skip; a.b_fin = h->b_fin96; a.b_in = h->b_in; a.B = B; a.T = T; a.M = h->M; a.tiles_per_row = cdiv(T, sub.tail.tile);
  a.status = h->flags ? h->flags + h->flags_cap : nullptr;   // (step_tail_h2_kernel, in_proj_h2_kernel: word 1 += range events)
  if (sub.tail.first_h2) {   // the 16-bit matrix pipe: split-fp16 weights and their scales
    a.ws_s = h->tail_s; a.wo_s = h->tail_s + 2 * C * C; a.wi_s = h->tail_s + 2 * C * C + 2 * 96 * C; a.tail_scale = h->tail_scale;
  } else if (sub.tail.form == TAIL_F32) {
    a.ws_pack = h->ws_pack; a.wo_pack = h->wo_pack; a.wi_pack = h->wi_pack;
  } else if (sub.tail.form != TAIL_UNFUSED) {   // the projections on bf16 MFMAs
    a.ws_h = h->tail_h; a.wo_h = h->tail_h + C * C; a.wi_h = h->tail_h + C * C + 96 * C;
  }
  return sub;
}

// a launch of its own in front of or behind the stack: `a` (TailArgs) on `grid` workgroups, and whatever else the form takes behind it
static int launch_step(const bsg_diffnet* h, const KernelForm* f, TailArgs a, int grid, hipStream_t st, const void* arg1 = nullptr, const void* arg2 = nullptr) {
  void* args[] = {&a, &arg1, &arg2};
  return launch_form(h->forms, *f, false, dim3(grid), args, st);
}

// The input projection of a DDPM call's first evaluation, the chain's rows of x into h->xa (TailPlan::first_h2).
static int first_in_projection(bsg_diffnet* h, const SubBatch& sub) {
  TailArgs a = tail_rows(sub.args, sub.plan.row0);
  if (!sub.tail.first_h2) return conv1x1(h->w_in, h->b_in, a.x, a.xa_next, C, h->M, a.B, a.T, ACT_RELU, sub.st);
  a.tiles_per_row = cdiv(a.T, 32);   // one workgroup per 32-frame tile, also in front of the stack launch's 64-frame tails
  BSG_REQUIRE(a.x && a.xa_next && a.b_in && a.wi_s && a.tail_scale && a.M <= 96, "split-fp16 input projection: fragments missing or in_dims > 96");
  return launch_step(h, h2_step_form(true), a, a.B * a.tiles_per_row, sub.st);
}

// One sampler step of a chain from the in-projected x in h->xa: the residual stack, then the tail in the chain's form.  `step`: sub.args
// with the sampler's own fields set, at the call's row 0.
static int run_step(bsg_diffnet* h, const SubBatch& sub, int t_uniform, const TailArgs& step) {
  TailArgs a = tail_rows(step, sub.plan.row0);
  if (sub.tail.form == TAIL_IN_STACK) return run_layers(h, sub.plan, nullptr, t_uniform, a.B, a.T, sub.st, &a);   // one launch per step
  TRY(run_layers(h, sub.plan, nullptr, t_uniform, a.B, a.T, sub.st));
  switch (sub.tail.form) {
    case TAIL_H2:
      BSG_REQUIRE(a.ws_s && a.wo_s && a.wi_s && a.tail_scale && a.M <= 96, "split-fp16 step tail: fragments missing or in_dims > 96");
      return launch_step(h, h2_step_form(false), a, a.B * a.tiles_per_row, sub.st);
    case TAIL_BF16:
      a.tiles_per_row = cdiv(a.T, 64);
      return launch_step(h, bf16_tail_form(false, a.plms_hist != 0), a, a.B * a.tiles_per_row, sub.st);
    case TAIL_BF16_RAGGED: {   // one launch over the tiles of every launch group's table (they follow the row lengths in rg_dev)
      BSG_REQUIRE(sub.plan.row0 == 0 && h->rg_dev, "ragged bf16 step tail: no ragged plan bound");
      int n_tiles = 0;
      for (int t : h->rg_group_tiles) n_tiles += t;
      BSG_REQUIRE(n_tiles > 0, "ragged bf16 step tail: no tile table");
      return launch_step(h, bf16_tail_form(true, a.plms_hist != 0), a, n_tiles, sub.st, h->rg_dev + ((h->bound.B + 1) & ~1), h->rg_dev);
    }
    default:   // TAIL_F32 (TAIL_UNFUSED is each sampler's forward_impl path and never comes here)
      BSG_REQUIRE(!sub.plan.ragged(), "step tail: a ragged call needs the bf16 tail in the bf16 configuration");
      return launch_step(h, tail_f32_form(sub.tail.mp, a.plms_hist != 0), a, a.B * a.tiles_per_row, sub.st);
  }
}

// Two half-batches on two streams.  One launch per layer puts all workgroups of the chip in the same phase (they stage, hit
// the gate and drain together, and the younger of the two workgroups of a CU finishes alone); two independent launch chains
// drift apart and fill each other's gaps: measured 239.6 -> 226.5 ms per 100 steps at B=16, T=1000 (+5.8 %), +4.0 % at B=32,
// +9.9 % at B=12, +1.2 % at B=64, +4 % for the bf16 form at B=64; four chains are worse (a CU only holds two of these
// workgroups).  On one of the boxes measured the two chains brought no gain (and no loss).  BSG_DUAL=0 disables.
// Returns what each half is planned as (PlanScope), or PLAN_WHOLE: one chain.  `plan`: the whole batch's.
static PlanScope dual_scope(const bsg_diffnet* h, const StackPlan& plan, int B, int T) {
  const int dual_env = dn_switches().dual, split_env = dn_switches().split;
  const long long tiles = (long long)B * cdiv(T, 32);
  const bool big = tiles > h->num_cus;
  // 129..256 tiles (B = 5..8): two chains of channel-split launches (each workgroup half the matrix work, two per CU, one of each
  // chain) instead of one chain of 16-wave workgroups
  // (measured per 100 steps at T=1000: B=5 130.5 -> 105.9 ms, B=6 133.5 -> 120.4, B=8 135.9 -> 133.8; BSG_DUAL=2: big batches only)
  // 65..128 tiles (B = 3, 4): two chains of 4-way split launches: B=3 89.0 -> 83.8 ms, B=4 93.3 -> 90.6
  bool small = dual_env != 2 && !big && 4 * tiles > h->num_cus && h->compute == BSG_COMPUTE_F32 && split_env && !h->split_off;
  if (small) {
    // two chains of split launches share CUs (un-padded LDS): all workgroups of BOTH launches must be resident at once, or a
    // polling workgroup could wait for a partner that cannot start.  Per half: parts x tiles workgroups of 1024/parts threads.
    double cus = 0.0;   // CUs the workgroups of both launches occupy at the residency the runtime reports for each form
    for (int half = 0; half < 2; ++half) {
      const long long th = (long long)(half ? B - B / 2 : B / 2) * cdiv(T, 32);
      const int parts = 4 * th <= h->num_cus && split_env != 2 ? 4 : 2 * th <= h->num_cus ? 2 : 0;
      int occ = h->forms.resident(*layer_form(parts == 4 ? LAYER_SPLIT4 : LAYER_SPLIT2, true, false, true));
      const int cap = parts == 4 ? 3 : 2;   // 48 KB of LDS each -> 3 per CU; 8 waves of 128 VGPRs -> 2 per CU
      if (occ > cap) occ = cap;
      if (!parts || occ < 1) return PLAN_WHOLE;
      cus += (double)(parts * th) / occ;
    }
    small = cus <= (double)h->num_cus;
  }
  const bool dual = dual_env && B >= 2 && use_wino() && plan.family() == STACK_NONE && (big || small);
  return !dual ? PLAN_WHOLE : big ? PLAN_HALF_BIG : PLAN_HALF_SMALL;
}

// What both sampler entries keep of a call
struct SamplerFrame {
  StackPlan plan;     // the whole batch's stack plan
  TailPlan tail;      // ... and the tail behind it; TAIL_UNFUSED: the entry's forward_impl loop
  SubBatch subs[2];   // the chains of the fused steps; until dual_fork, [0] is the whole batch on the caller's stream
  int n_sub = 0;      // chains; 0: not forked yet
};

// the entries' shared checks in front of their own: the binding and the schedule
static int sampler_enter(bsg_diffnet* h, const bsg_schedule* s, int B, int T, const char* who, bool plms) {
  TRY(check_bound(h, B, T, who));
  h->last_chains = 1;   // this call's count from here on: the unfused loop and an early return never reach sampler_end
  return check_schedule(s, who, plms);
}

// ... and behind them: the whole batch's plans, the conditioner term in the layout its launch reads
static int sampler_begin(bsg_diffnet* h, SamplerFrame& f, float* x, int B, int T, hipStream_t st, const char* who) {
  TRY(ragged_enter(h, st, who));
  f.plan = plan_stack(h, B, T, st, h->bound.ragged ? PLAN_RAGGED : PLAN_WHOLE);
  TRY(cond_layout_for(h, f.plan, st));
  f.subs[0] = sub_batch(h, f.plan, x, B, T, st); f.tail = f.subs[0].tail;
  return BSG_OK;
}

// The chains of the fused steps: two half-batches on two streams where `may_split` and dual_scope say so and the fork succeeds, each
// half planned for what it is; else (always for a ragged batch: one chain of its launch groups) the whole batch stays the one chain.
static void dual_fork(bsg_diffnet* h, SamplerFrame& f, bool may_split) {
  const SubBatch w = f.subs[0];
  const int B0 = w.B / 2, T = w.args.T;
  const PlanScope half = may_split && !w.plan.ragged() ? dual_scope(h, w.plan, w.B, T) : PLAN_WHOLE;
  bool two = half != PLAN_WHOLE;   // the fork: the second stream and its events are created at the first one; a failed call leaves one chain
  if (two && !h->st2)
    two = hipStreamCreateWithFlags(&h->st2, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) == hipSuccess &&
          hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) == hipSuccess;
  f.n_sub = two && hipEventRecord(h->ev_fork, w.st) == hipSuccess && hipStreamWaitEvent(h->st2, h->ev_fork, 0) == hipSuccess ? 2 : 1;
  if (f.n_sub == 1) return;
  f.subs[0] = sub_batch(h, plan_stack(h, B0, T, w.st, half), w.args.x, B0, T, w.st);
  StackPlan second = plan_stack(h, w.B - B0, T, h->st2, half);
  second.row0 = B0;
  f.subs[1] = sub_batch(h, second, w.args.x, w.B - B0, T, h->st2);
}

// joins the second stream back into the caller's (also after an error, so that the caller's stream stays ordered after everything
// that was enqueued on the second one) and records the call's chain count
static int sampler_end(bsg_diffnet* h, const SamplerFrame& f, int rc) {
  h->last_chains = f.n_sub == 2 ? 2 : 1;
  if (f.n_sub == 2) {
    hipError_t e1 = hipEventRecord(h->ev_join, h->st2);
    hipError_t e2 = hipStreamWaitEvent(f.subs[0].st, h->ev_join, 0);
    if (rc == BSG_OK && (e1 != hipSuccess || e2 != hipSuccess)) { set_error("sampler: stream join failed"); rc = BSG_EHIP; }
  }
  return rc;
}

// Both DDPM entries.  row_seeds (host [B], bsg_ddpm_sample_rows: noise null, row0 0): every step's draws are written to h->row_noise by
// bsg_philox_normal_rows in front of the step's launches — a chain's rows on the chain's stream, so stream order covers the buffer's reuse by
// the next step — and the step reads them as supplied noise.  Without, nothing here differs from the unkeyed call.
static int ddpm_sample_impl(bsg_diffnet* h, const bsg_schedule* s, float* x, const float* noise, uint64_t seed, const uint64_t* row_seeds,
                            int32_t t_start, int32_t n_steps, int32_t B, int32_t T, int32_t row0, int32_t B_total, void* stream,
                            const char* who) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  TRY(sampler_enter(h, s, B, T, who, false));
  BSG_REQUIRE(x, "%s: null x", who);
  BSG_REQUIRE(t_start < s->num_timesteps && t_start < h->cfg.max_steps && n_steps >= 0 && t_start - n_steps + 1 >= 0,
              "%s: steps [%d..%d] outside the schedule (%d) / step table (%d)", who, t_start - n_steps + 1, t_start,
              s->num_timesteps, h->cfg.max_steps);
  BSG_REQUIRE(row0 >= 0 && row0 + B <= B_total, "%s: rows [%d,%d) outside the global batch %d", who, row0, row0 + B, B_total);
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)B * h->M * T;
  BSG_REQUIRE(n % 4 == 0, "%s: B*M*T must be a multiple of 4", who);
  SamplerFrame f;
  TRY(sampler_begin(h, f, x, B, T, st, who));
  // keyed: the row lengths are the binding's (T for a padded one); what the fill would refuse is refused here, before a step is enqueued
  const int32_t* lens = row_seeds && h->bound.ragged ? h->rg_lens.data() : nullptr;
  if (row_seeds) {
    for (int b = 0; b < B; ++b)
      BSG_REQUIRE((long long)h->M * (lens ? lens[b] : T) % 4 == 0, "%s: row %d draws M * n = %d * %d values, no multiple of 4", who, b, h->M, lens ? lens[b] : T);
    TRY(grow(h, &h->row_noise_cap, (size_t)B * T, st, GROW_LAZY));
  }
  auto fill = [&](int i, int r0, int rows, hipStream_t on) {   // the keyed draws of step i for rows [r0, r0 + rows), enqueued on `on`
    return bsg_philox_normal_rows(h->row_noise + (size_t)r0 * h->M * T, rows, h->M, T, lens ? lens + r0 : nullptr, row_seeds + r0, (uint32_t)(i + 1), on);
  };
  const unsigned long long elem0 = (unsigned long long)row0 * h->M * T;   // Philox: the flat element index of this shard's row 0
  auto coef = [&](int i) {
    return StepCoef{s->sqrt_recip_alphas_cumprod[i], s->sqrt_recipm1_alphas_cumprod[i], s->posterior_mean_coef1[i], s->posterior_mean_coef2[i], s->sigma[i]};
  };
  if (f.tail.form == TAIL_UNFUSED) {
    for (int k = 0; k < n_steps; ++k) {
      const int i = t_start - k;
      TRY(forward_impl(h, f.plan, x, nullptr, i, h->eps, B, T, st));
      if (row_seeds) TRY(fill(i, 0, B, st));
      hipLaunchKernelGGL(ddpm_step_kernel, dim3(cdiv(n / 4, 256)), dim3(256), 0, st, x, (const float*)h->eps,
                         row_seeds ? (const float*)h->row_noise : noise ? noise + (long long)k * n : nullptr, coef(i), n / 4, (unsigned long long)seed, (unsigned)(i + 1), elem0 / 4);
      BSG_LAUNCH_CHECK();
    }
    return BSG_OK;
  }
  // fused loop: [in-projection once] -> per step: 20 residual layers -> the step tail, which leaves the next step's in-projection
  dual_fork(h, f, n_steps > 0);
  int rc = BSG_OK;
  for (int u = 0; u < f.n_sub && rc == BSG_OK; ++u) rc = first_in_projection(h, f.subs[u]);
  for (int k = 0; k < n_steps && rc == BSG_OK; ++k) {
    const int i = t_start - k;
    for (int u = 0; u < f.n_sub && rc == BSG_OK; ++u) {
      TailArgs a = f.subs[u].args;
      a.noise = noise ? noise + (long long)k * n : nullptr; a.k = coef(i); a.do_head = k + 1 < n_steps;
      a.seed = seed; a.quad_row0 = elem0; a.stream = (unsigned)(i + 1);
      if (row_seeds) {
        a.noise = h->row_noise;   // (at the call's row 0, like x: run_step moves both to the chain's rows)
        rc = fill(i, f.subs[u].plan.row0, f.subs[u].B, f.subs[u].st);
      }
      if (rc == BSG_OK) rc = run_step(h, f.subs[u], i, a);
    }
  }
  return sampler_end(h, f, rc);
}

extern "C" int bsg_ddpm_sample(bsg_diffnet* h, const bsg_schedule* s, float* x, const float* noise, uint64_t seed,
                               int32_t t_start, int32_t n_steps, int32_t B, int32_t T, int32_t row0, int32_t B_total,
                               void* stream) {
  return ddpm_sample_impl(h, s, x, noise, seed, nullptr, t_start, n_steps, B, T, row0, B_total, stream, "ddpm_sample");
}

// ABI v22: bsg_ddpm_sample with every row's draws from the row's own stream (seeds_host[b], i + 1) at the row's bound length
extern "C" int bsg_ddpm_sample_rows(bsg_diffnet* h, const bsg_schedule* s, float* x, const uint64_t* seeds_host, int32_t t_start,
                                    int32_t n_steps, int32_t B, int32_t T, void* stream) {
  BSG_REQUIRE(seeds_host, "ddpm_sample_rows: null seeds_host");
  return ddpm_sample_impl(h, s, x, nullptr, 0, seeds_host, t_start, n_steps, B, T, 0, B, stream, "ddpm_sample_rows");
}

extern "C" int bsg_diffnet_set_compute(bsg_diffnet* h, int32_t mode) {
  BSG_REQUIRE(h, "diffnet_set_compute: null handle");
  BSG_REQUIRE(mode == BSG_COMPUTE_F32 || mode == BSG_COMPUTE_BF16, "diffnet_set_compute: unknown mode %d", mode);
  h->compute = mode;
  return BSG_OK;
}

extern "C" int bsg_diffnet_debug_stamps(bsg_diffnet* h, int32_t layer, const float* x_in, const int64_t* t, float* x_out,
                                       float* skip, int32_t B, int32_t T, uint64_t* stamps, void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  TRY(check_bound(h, B, T, "diffnet_debug_stamps"));
  BSG_REQUIRE(x_in && t && x_out && skip && stamps && x_in != x_out, "diffnet_debug_stamps: null or aliased argument");
  BSG_REQUIRE(layer >= 0 && layer < h->L, "diffnet_debug_stamps: layer %d out of range", layer);
  if (h->compute == BSG_COMPUTE_F32) TRY(ensure_cond_rows(h, (hipStream_t)stream));
  StackPlan plan;
  plan_layer(h, plan, B, T, PLAN_WHOLE, true);   // stamps: the un-split kernel
  return launch_layer(h, plan, layer, x_in, (const long long*)t, 0, x_out, skip, B, T, (hipStream_t)stream, (unsigned long long*)stamps);
}

extern "C" int bsg_diffnet_status(bsg_diffnet* h, int32_t* handoff_timeouts) {
  BSG_REQUIRE(h && handoff_timeouts, "diffnet_status: null argument");
  *handoff_timeouts = 0;
  if (h->flags) {
    unsigned v[2] = {0, 0};   // word 0: hand-off give-ups, word 1: values beyond the fp16 range of the split-fp16 launch
    BSG_HIP(hipMemcpy(v, h->flags + h->flags_cap, 2 * sizeof(unsigned), hipMemcpyDeviceToHost));
    *handoff_timeouts = (int32_t)(v[0] + v[1]);
  }
  if (h->split_flags) {
    unsigned v = 0;
    BSG_HIP(hipMemcpy(&v, h->split_flags + 16 * h->split_cap, sizeof(unsigned), hipMemcpyDeviceToHost));
    *handoff_timeouts += (int32_t)v;
  }
  return BSG_OK;
}

extern "C" int bsg_diffnet_health_take(bsg_diffnet* h, int32_t* counts, void* stream) {
  BSG_REQUIRE(h && counts, "diffnet_health_take: null argument");
  hipStream_t st = (hipStream_t)stream;
  counts[0] = counts[1] = 0;
  unsigned v[3] = {0, 0, 0};
  if (h->flags) BSG_HIP(hipMemcpyAsync(&v[0], h->flags + h->flags_cap, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  if (h->split_flags) BSG_HIP(hipMemcpyAsync(&v[2], h->split_flags + 16 * h->split_cap, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  BSG_HIP(hipStreamSynchronize(st));
  if (v[0] | v[1]) BSG_HIP(hipMemsetAsync(h->flags + h->flags_cap, 0, 3 * sizeof(unsigned), st));   // (word 2: the flag base of the part launch that gave up)
  if (v[2]) BSG_HIP(hipMemsetAsync(h->split_flags + 16 * h->split_cap, 0, sizeof(unsigned), st));
  counts[0] = (int32_t)(v[0] + v[2]);
  counts[1] = (int32_t)v[1];
  return BSG_OK;
}

extern "C" int bsg_diffnet_handoff_take(bsg_diffnet* h, int32_t* handoff_timeouts, void* stream) {
  BSG_REQUIRE(h && handoff_timeouts, "diffnet_handoff_take: null argument");
  int32_t c[2] = {0, 0};
  TRY(bsg_diffnet_health_take(h, c, stream));
  *handoff_timeouts = c[0] + c[1];
  return BSG_OK;
}

extern "C" int bsg_diffnet_uses_handoffs(bsg_diffnet* h, int32_t B, int32_t T, int32_t* uses) {
  BSG_REQUIRE(h && uses && B > 0 && T > 0, "diffnet_uses_handoffs: bad argument");
  TRY(num_cus(h));   // normally set by prepare(); asked before any condition was bound
  if (h->bound.ragged && h->bound.B == B && h->bound.T == T && ragged_launch_ok(h)) {   // the bound ragged batch: its stack launch hands edges between tiles
    *uses = 1;
    return BSG_OK;
  }
  // The stack launch: the whole batch's plan says it.  The channel-split (pair / 4-way) launches: conservative, any shape of at most one
  // tile per CU while they are on.  That is more than the plan's split2 / split4: in the 16-wave window the whole batch's per-layer form
  // hands nothing over, but a sampler call runs it as two half-batch chains of split launches (dual_fork), and a handle asked before
  // prepare allocated the exchange scratch has no split form yet.
  const long long tiles = (long long)B * cdiv(T, 32);
  const bool split = h->compute == BSG_COMPUTE_F32 && use_wino() && dn_switches().split && !h->split_off && h->num_cus && tiles <= h->num_cus;
  *uses = (split || plan_stack(h, B, T, nullptr).form) ? 1 : 0;
  return BSG_OK;
}

extern "C" int bsg_diffnet_set_split(bsg_diffnet* h, int32_t enable) {
  BSG_REQUIRE(h, "diffnet_set_split: null handle");
  h->split_off = enable == 0;
  return BSG_OK;
}

extern "C" int bsg_diffnet_set_h2(bsg_diffnet* h, int32_t enable) {
  BSG_REQUIRE(h, "diffnet_set_h2: null handle");
  h->h2_off = enable == 0;
  return BSG_OK;
}

// middle tier of the range guard (ABI v7): 0 takes the 16-row stack launch (its conv image holds 16 x: |x| < 3750) off this handle; shapes
// that ran it take the 32-row launch (residual_stack_h2_kernel: |x + d| < 60000, about 8 % slower) — still the 16-bit matrix pipe
extern "C" int bsg_diffnet_set_h2q(bsg_diffnet* h, int32_t enable) {
  BSG_REQUIRE(h, "diffnet_set_h2q: null handle");
  h->q_off = enable == 0;
  return BSG_OK;
}

// test hook (ABI v6): the launch epoch of the handle's stack / part launches (device memory) := epoch, so that the wrap at 2^25 — two
// hours of single-utterance serving away — can be driven by a test
extern "C" int bsg_diffnet_debug_set_epoch(bsg_diffnet* h, uint32_t epoch, void* stream) {
  BSG_REQUIRE(h && h->epoch_dev && epoch >= 1u, "diffnet_debug_set_epoch: no launch epoch yet (prepare allocates it), or epoch 0");
  hipStream_t st = (hipStream_t)stream;
  BSG_HIP(hipStreamSynchronize(st));
  const unsigned v[2] = {epoch, 0u};
  BSG_HIP(hipMemcpy(h->epoch_dev, v, sizeof(v), hipMemcpyHostToDevice));
  // flag words hold epoch x 64 + layer of launches that ran under smaller epochs: still older than every launch from here on
  return BSG_OK;
}

// fault injection (ABI v6): in the next n_launches PART launches the odd parts of every tile report another XCC id than the one they run on —
// what the parts would see under a dispatch order other than workgroup i -> XCD i mod 8
extern "C" int bsg_diffnet_debug_inject_xcc(bsg_diffnet* h, int32_t n_launches) {
  BSG_REQUIRE(h && n_launches >= 0, "diffnet_debug_inject_xcc: bad argument");
  h->inject_xcc = n_launches;
  return BSG_OK;
}

// part forms on / off for this handle (ABI v6): the first tier of the self-heal after a hand-off give-up inside a part launch — the
// one-workgroup-per-tile stack launch needs no placement on one XCD and stays; bsg_diffnet_set_split(h, 0) is the second tier
extern "C" int bsg_diffnet_set_parts(bsg_diffnet* h, int32_t enable) {
  BSG_REQUIRE(h, "diffnet_set_parts: null handle");
  h->parts_off = !enable;
  return BSG_OK;
}

extern "C" int bsg_diffnet_debug_inject_giveup(bsg_diffnet* h, int32_t n_launches) {
  BSG_REQUIRE(h, "diffnet_debug_inject_giveup: bad argument");
  // n < 0 (timing experiment, tools/part_nowait.py): the next -n PART launches skip every hand-off wait without counting anything — wrong
  // results, the same instructions otherwise: what the waits themselves cost
  h->inject_giveup = n_launches > 0 ? n_launches : 0;
  h->inject_nowait = n_launches < 0 ? -n_launches : 0;
  return BSG_OK;
}

extern "C" int bsg_diffnet_status_async(bsg_diffnet* h, int32_t* host_counts, void* stream) {
  BSG_REQUIRE(h && host_counts, "diffnet_status_async: null argument");
  hipStream_t st = (hipStream_t)stream;
  host_counts[0] = host_counts[1] = host_counts[2] = 0;
  // words 0 and 1 of the stack launches' status are adjacent: one copy fills host_counts[0] (give-ups) and [1] (range events)
  if (h->flags) BSG_HIP(hipMemcpyAsync(&host_counts[0], h->flags + h->flags_cap, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  if (h->split_flags) BSG_HIP(hipMemcpyAsync(&host_counts[2], h->split_flags + 16 * h->split_cap, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  return BSG_OK;
}

extern "C" int bsg_diffnet_debug_stack_stamps(bsg_diffnet* h, int32_t t_uniform, int32_t B, int32_t T, uint64_t* stamps, void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  TRY(check_bound(h, B, T, "diffnet_debug_stack_stamps"));
  BSG_REQUIRE(stamps, "diffnet_debug_stack_stamps: null stamps");
  const StackPlan plan = plan_stack(h, B, T, (hipStream_t)stream);
  TRY(cond_layout_for(h, plan, (hipStream_t)stream));
  BSG_REQUIRE(plan.family() != STACK_NONE && plan.rows >= B, "diffnet_debug_stack_stamps: (B=%d,T=%d) does not run as one %sstack launch", B, T,
              h->compute == BSG_COMPUTE_BF16 ? "bf16 " : "");
  return launch_stack(h, plan, nullptr, t_uniform, B, T, (hipStream_t)stream, (unsigned long long*)stamps);
}

extern "C" const char* bsg_diffnet_last_path(bsg_diffnet* h) { return h ? h->last_path : "none"; }

// test hook: the per-frame conditioner term of the bound condition in channel-quad order — behind a token binding its expansion
extern "C" int bsg_diffnet_debug_cond_quads(bsg_diffnet* h, float* out, int32_t B, int32_t T, void* stream) {
  TRY(check_bound(h, B, T, "diffnet_debug_cond_quads"));
  BSG_REQUIRE(out, "diffnet_debug_cond_quads: null argument");
  TRY(ensure_cond_quads(h, (hipStream_t)stream));
  if (!h->bound.quads) {
    set_error("diffnet_debug_cond_quads: the bound condition's term was not written in channel-quad order");
    return BSG_ESTATE;
  }
  BSG_HIP(hipMemcpyAsync(out, h->condterm_q, (size_t)h->L * 2 * C * B * T * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return BSG_OK;
}
extern "C" int bsg_diffnet_last_launch(bsg_diffnet* h, int32_t* chains, int32_t* groups) {
  BSG_REQUIRE(h && chains && groups, "diffnet_last_launch: null argument");
  *chains = h->last_chains;
  *groups = h->last_groups;
  return BSG_OK;
}

extern "C" int bsg_diffnet_clock_read(bsg_diffnet* h, double* shader_mhz, double* span_us) {
  BSG_REQUIRE(h && shader_mhz && span_us, "diffnet_clock_read: null argument");
  *shader_mhz = 0.0;
  *span_us = 0.0;
  if (!h->clk) return BSG_OK;
  unsigned long long v[4] = {0, 0, 0, 0};
  BSG_HIP(hipMemcpy(v, h->clk, sizeof(v), hipMemcpyDeviceToHost));
  if (v[3] > v[1] && v[2] > v[0]) {
    *span_us = (double)(v[3] - v[1]) / 100.0;            // s_memrealtime counts at 100 MHz
    *shader_mhz = (double)(v[2] - v[0]) / *span_us;      // s_memtime counts shader clocks
  }
  return BSG_OK;
}

extern "C" int bsg_diffnet_profile(bsg_diffnet* h, int32_t enable) {
  BSG_REQUIRE(h, "diffnet_profile: null handle");
  if (enable && h->prof_ev.empty()) {
    h->prof_ev.resize(2 * 4096);
    for (hipEvent_t& e : h->prof_ev) BSG_HIP(hipEventCreate(&e));
  }
  h->prof_on = enable != 0;
  h->prof_used = 0;
  h->prof_launches = 0;
  return BSG_OK;
}

extern "C" int bsg_diffnet_profile_read(bsg_diffnet* h, double* layer_ms_total, int64_t* n_layer_launches) {
  BSG_REQUIRE(h && layer_ms_total && n_layer_launches, "diffnet_profile_read: null argument");
  double total = 0.0;
  for (size_t i = 0; i + 1 < h->prof_used; i += 2) {
    BSG_HIP(hipEventSynchronize(h->prof_ev[i + 1]));
    float ms = 0.f;
    BSG_HIP(hipEventElapsedTime(&ms, h->prof_ev[i], h->prof_ev[i + 1]));
    total += ms;
  }
  *layer_ms_total = total;
  *n_layer_launches = (int64_t)h->prof_launches;
  return BSG_OK;
}

extern "C" int bsg_mel_finish(const float* x, const float* spec_min, const float* spec_max, const int64_t* mel2ph,
                              float* mel_out, int32_t B, int32_t M, int32_t T, void* stream) {
  BSG_REQUIRE(x && spec_min && spec_max && mel_out && B > 0 && M > 0 && M <= 512 && T > 0, "mel_finish: bad argument");
  hipLaunchKernelGGL(mel_finish_kernel, dim3(cdiv(T, 64), B), dim3(256), (size_t)M * 65 * sizeof(float), (hipStream_t)stream, x,
                     spec_min, spec_max, (const long long*)mel2ph, mel_out, M, T);
  BSG_LAUNCH_CHECK();
  return BSG_OK;
}

extern "C" int bsg_mel_start(const float* fs2_mel, const float* spec_min, const float* spec_max, const float* noise,
                             float sqrt_ac, float sqrt_1m_ac, float* x, int32_t B, int32_t M, int32_t T, void* stream) {
  BSG_REQUIRE(fs2_mel && spec_min && spec_max && noise && x && B > 0 && M > 0 && M <= 512 && T > 0, "mel_start: bad argument");
  hipLaunchKernelGGL(mel_start_kernel, dim3(cdiv(T, 64), B), dim3(256), (size_t)64 * (M + 1) * sizeof(float), (hipStream_t)stream,
                     fs2_mel, spec_min, spec_max, noise, sqrt_ac, sqrt_1m_ac, x, M, T);
  BSG_LAUNCH_CHECK();
  return BSG_OK;
}

extern "C" int bsg_ddpm_step(float* x, const float* eps, const float* noise, const bsg_schedule* s, int32_t t, int64_t n,
                             uint64_t seed, uint64_t offset, void* stream) {
  TRY(check_schedule(s, "ddpm_step", false));
  BSG_REQUIRE(x && eps && n > 0 && n % 4 == 0 && offset % 4 == 0 && t >= 0 && t < s->num_timesteps, "ddpm_step: bad argument");
  StepCoef c{s->sqrt_recip_alphas_cumprod[t], s->sqrt_recipm1_alphas_cumprod[t], s->posterior_mean_coef1[t],
             s->posterior_mean_coef2[t], s->sigma[t]};
  hipLaunchKernelGGL(ddpm_step_kernel, dim3(cdiv(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, x, eps, noise, c, (long long)(n / 4),
                     (unsigned long long)seed, (unsigned)(t + 1), (unsigned long long)(offset / 4));
  BSG_LAUNCH_CHECK();
  return BSG_OK;
}

extern "C" int bsg_philox_normal(float* x, int64_t n, uint64_t seed, uint32_t stream_id, uint64_t offset, void* stream) {
  BSG_REQUIRE(x && n > 0 && n % 4 == 0 && offset % 4 == 0, "philox_normal: n=%lld offset=%llu must be multiples of 4", (long long)n, (unsigned long long)offset);
  hipLaunchKernelGGL(philox_fill_kernel, dim3(cdiv(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, x, (long long)(n / 4),
                     (unsigned long long)seed, (unsigned)stream_id, (unsigned long long)(offset / 4));
  BSG_LAUNCH_CHECK();
  return BSG_OK;
}

// ABI v22: x [B][M][T], row b from the stream (seeds_host[b], stream_id) at its own length — what bsg_philox_normal gives the row alone
// (philox_fill_rows_kernel).  Every row is checked before the first launch; 32 rows per launch.
extern "C" int bsg_philox_normal_rows(float* x, int32_t B, int32_t M, int32_t T, const int32_t* lengths_host, const uint64_t* seeds_host,
                                      uint32_t stream_id, void* stream) {
  BSG_REQUIRE(x && seeds_host, "philox_normal_rows: null %s", x ? "seeds_host" : "x");
  BSG_REQUIRE(B > 0 && M > 0 && T > 0, "philox_normal_rows: bad argument (B=%d M=%d T=%d)", B, M, T);
  for (int b = 0; b < B; ++b) {
    const int nb = lengths_host ? lengths_host[b] : T;
    BSG_REQUIRE(nb >= 1 && nb <= T, "philox_normal_rows: lengths[%d]=%d outside 1..T=%d", b, nb, T);
    BSG_REQUIRE((long long)M * nb % 4 == 0, "philox_normal_rows: row %d draws M * n = %d * %d values, no multiple of 4 (the stream is drawn four at a time)",
                b, M, nb);
  }
  for (int b0 = 0; b0 < B; b0 += kPhiloxRowsPerLaunch) {
    PhiloxRows rows{};
    const int n = B - b0 < kPhiloxRowsPerLaunch ? B - b0 : kPhiloxRowsPerLaunch;
    long long items = 0;   // of the row with the most: its quads and the fours of its zero tail
    for (int r = 0; r < n; ++r) {
      rows.seed[r] = seeds_host[b0 + r];
      rows.len[r] = lengths_host ? lengths_host[b0 + r] : T;
      const long long it = (long long)M * rows.len[r] / 4 + cdiv((long long)M * (T - rows.len[r]), 4);
      if (it > items) items = it;
    }
    hipLaunchKernelGGL(philox_fill_rows_kernel, dim3((unsigned)cdiv(items, 256), n), dim3(256), 0, (hipStream_t)stream,
                       x + (long long)b0 * M * T, rows, (int)M, (int)T, (unsigned)stream_id);
    BSG_LAUNCH_CHECK();
  }
  return BSG_OK;
}

extern "C" int bsg_plms_sample(bsg_diffnet* h, const bsg_schedule* s, float* x, int32_t K_step, int32_t interval, int32_t B,
                               int32_t T, void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  TRY(sampler_enter(h, s, B, T, "plms_sample", true));
  BSG_REQUIRE(x && interval > 0 && K_step > 0 && K_step <= s->num_timesteps && K_step <= h->cfg.max_steps,
              "plms_sample: K_step=%d interval=%d schedule=%d", K_step, interval, s->num_timesteps);
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)B * h->M * T;
  BSG_REQUIRE(h->xpred, "plms_sample: history buffers missing (bsg_diffnet_prepare allocates them)");
  SamplerFrame f;
  TRY(sampler_begin(h, f, x, B, T, st, "plms_sample"));
  const dim3 grid(cdiv((long long)n, 256)), block(256);
  // the unfused update (first iteration); ragged: on each row's own frames only
  auto plms_step = [&](const float* xi, float* xo, const float* e0, const float* e1, const float* e2, const float* e3, const PlmsCoef& k) {
    if (f.plan.ragged())
      hipLaunchKernelGGL(plms_step_ragged_kernel, dim3(cdiv(T, 256), h->M, B), dim3(256), 0, st, xi, xo, e0, e1, e2, e3, k, (const int*)h->rg_dev, h->M, T);
    else
      hipLaunchKernelGGL(plms_step_kernel, grid, block, 0, st, xi, xo, e0, e1, e2, e3, k, (long long)n);
  };
  const bool fused = f.tail.form != TAIL_UNFUSED;
  // history ring: hist[0] = newest
  float* hist[4] = {h->eps_hist[0], h->eps_hist[1], h->eps_hist[2], h->eps_hist[3]};
  int n_hist = 0, rc = BSG_OK;
  const int last = ((K_step - 1) / interval) * interval;
  for (int i = last; i >= 0; i -= interval) {
    const int ip = i - interval > 0 ? i - interval : 0;
    PlmsCoef c{};
    c.a_t = s->alphas_cumprod[i];
    c.a_prev = s->alphas_cumprod[ip];
    float* e_new = hist[3];  // slot about to be recycled
    if (n_hist > 0 && fused) {
      // fused iteration: h->xa already holds the in-projection of x (left by the previous iteration); the tail projects the skip
      // sum to eps, stores it to the history slot, applies the multistep update to x and projects the new x for the next one
      if (f.n_sub == 0) dual_fork(h, f, true);   // the first fused iteration forks the two half-batch chains, not an earlier one
      for (int u = 0; u < f.n_sub && rc == BSG_OK; ++u) {
        TailArgs a = f.subs[u].args;
        a.plms_hist = n_hist; a.pk = c; a.e_new = e_new; a.h1 = hist[0]; a.h2 = hist[1]; a.h3 = hist[2];
        plms_blend(n_hist, a.pk);
        a.do_head = i - interval >= 0;
        rc = run_step(h, f.subs[u], i, a);
      }
      if (rc != BSG_OK) break;
      hist[3] = hist[2]; hist[2] = hist[1]; hist[1] = hist[0]; hist[0] = e_new;
      if (n_hist < 3) ++n_hist;
      continue;
    }
    TRY(forward_impl(h, f.plan, x, nullptr, i, e_new, B, T, st));
    plms_blend(n_hist, c);
    if (n_hist == 0) {
      // ragged: the predictor below writes x_pred on each row's frames only; its padding takes x's (finite, the caller's), which the
      // input projection of the second evaluation reads
      if (f.plan.ragged()) BSG_HIP(hipMemcpyAsync(h->xpred, x, n * sizeof(float), hipMemcpyDeviceToDevice, st));
      plms_step((const float*)x, h->xpred, (const float*)e_new,
                         (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, c);
      TRY(forward_impl(h, f.plan, h->xpred, nullptr, ip, h->eps, B, T, st));
      c.w0 = 1.f; c.inv = 2.f;
      plms_step((const float*)x, x, (const float*)e_new, (const float*)h->eps,
                         (const float*)nullptr, (const float*)nullptr, c);
    } else {
      plms_step((const float*)x, x, (const float*)e_new, (const float*)hist[0], n_hist >= 2 ? (const float*)hist[1] : nullptr,
                n_hist >= 3 ? (const float*)hist[2] : nullptr, c);
    }
    BSG_LAUNCH_CHECK();
    if (fused && i - interval >= 0) TRY(conv1x1(h->w_in, h->b_in, x, h->xa, C, h->M, B, T, ACT_RELU, st));   // for the fused iterations
    hist[3] = hist[2]; hist[2] = hist[1]; hist[1] = hist[0]; hist[0] = e_new;
    if (n_hist < 3) ++n_hist;
  }
  return sampler_end(h, f, rc);
}

// One PLMS update given the noise predictions (p_sample_plms :168-201 without the denoiser calls), for denoisers that are not a
// bsg_diffnet (ABI v5): x_out = x + x_delta(eps') with eps' the multistep blend of e0 (newest) and the n_hist <= 3 older predictions
// e1..e3 (NULL beyond n_hist):  n_hist = 0, avg = 0: eps' = e0 (the predictor half-step of the first iteration);  n_hist = 1, avg = 1:
// (e0 + e1) / 2 (its corrector);  n_hist = 1: (3 e0 - e1) / 2;  2: (23 e0 - 16 e1 + 5 e2) / 12;  3: (55 e0 - 59 e1 + 37 e2 - 9 e3) / 24.
extern "C" int bsg_plms_step(const float* x, float* x_out, const float* e0, const float* e1, const float* e2, const float* e3, int32_t n_hist,
                             int32_t avg, const bsg_schedule* s, int32_t t, int32_t t_prev, int64_t n, void* stream) {
  TRY(check_schedule(s, "plms_step", true));
  BSG_REQUIRE(x && x_out && e0 && n > 0 && n_hist >= 0 && n_hist <= 3 && t >= 0 && t < s->num_timesteps && t_prev >= 0 && t_prev <= t,
              "plms_step: bad argument");
  BSG_REQUIRE((n_hist < 1 || e1) && (n_hist < 2 || e2) && (n_hist < 3 || e3), "plms_step: %d history tensors expected", n_hist);
  PlmsCoef c{};
  c.a_t = s->alphas_cumprod[t];
  c.a_prev = s->alphas_cumprod[t_prev];
  if (n_hist == 1 && avg) { c.w0 = 1.f; c.inv = 2.f; }
  else plms_blend(n_hist, c);
  hipLaunchKernelGGL(plms_step_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, x_out, e0, n_hist >= 1 ? e1 : nullptr,
                     n_hist >= 2 ? e2 : nullptr, n_hist >= 3 ? e3 : nullptr, c, (long long)n);
  BSG_LAUNCH_CHECK();
  return BSG_OK;
}

// ---- ragged batches (ABI v8) -----------------------------------------------------------------------------------------------------
// First-fit decreasing of whole rows (ceil(len / tile_frames) tiles each) into launch groups of at most `cus` tiles: rows by tile count,
// longest first (ties: lower row first), each into the first group it fits.  A group's tiles run as one launch; the groups one after another.
extern "C" int bsg_ragged_plan(const int32_t* lens, int32_t B, int32_t tile_frames, int32_t cus, int32_t* group_of_row, int32_t* n_groups) {
  BSG_REQUIRE(lens && group_of_row && n_groups && B > 0 && tile_frames > 0 && cus > 0, "ragged_plan: bad argument");
  std::vector<int> order(B), tiles(B);
  for (int b = 0; b < B; ++b) {
    BSG_REQUIRE(lens[b] > 0, "ragged_plan: row %d has %d frames", b, lens[b]);
    tiles[b] = cdiv(lens[b], tile_frames);
    BSG_REQUIRE(tiles[b] <= cus, "ragged_plan: row %d of %d frames takes %d tiles of %d frames; a launch group holds %d (one per CU)", b, lens[b],
                tiles[b], tile_frames, cus);
    order[b] = b;
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return tiles[a] > tiles[b]; });
  std::vector<int> fill;
  for (int b : order) {
    size_t g = 0;
    while (g < fill.size() && fill[g] + tiles[b] > cus) ++g;
    if (g == fill.size()) fill.push_back(0);
    fill[g] += tiles[b];
    group_of_row[b] = (int32_t)g;
  }
  *n_groups = (int32_t)fill.size();
  return BSG_OK;
}

extern "C" int bsg_diffnet_prepare_ragged(bsg_diffnet* h, const float* cond, const int32_t* lens, int32_t B, int32_t T, void* stream) {
  BSG_REQUIRE(h && cond && lens, "diffnet_prepare_ragged: null argument");
  BSG_REQUIRE(B > 0 && T > 0, "diffnet_prepare_ragged: B=%d T=%d", B, T);
  hipStream_t st = (hipStream_t)stream;
  if (is_capturing(st)) {
    set_error("diffnet_prepare_ragged: a ragged batch cannot be bound or decoded under stream capture");
    return BSG_ESTATE;
  }
  for (int b = 0; b < B; ++b) BSG_REQUIRE(lens[b] >= 1 && lens[b] <= T, "diffnet_prepare_ragged: row %d has %d frames (1..T=%d)", b, lens[b], T);
  TRY(num_cus(h));
  std::vector<int32_t> grp(B);
  int32_t ng = 0;
  TRY(bsg_ragged_plan(lens, B, 64, h->num_cus, grp.data(), &ng));
  TRY(bsg_diffnet_prepare(h, cond, B, T, stream));
  // [lengths, padded to an even count][tables]: group after group, each row's tiles contiguous and in order
  const int bpad = (B + 1) & ~1;
  std::vector<int> host(bpad, 0);
  for (int b = 0; b < B; ++b) host[b] = lens[b];
  h->rg_group_off.assign(ng, 0);
  h->rg_group_tiles.assign(ng, 0);
  int off = 0;
  for (int g = 0; g < ng; ++g) {
    h->rg_group_off[g] = off;
    for (int b = 0; b < B; ++b) {
      if (grp[b] != g) continue;
      for (int j = 0; j < cdiv(lens[b], 64); ++j) { host.push_back(b); host.push_back(j); ++off; }
    }
    h->rg_group_tiles[g] = off - h->rg_group_off[g];
  }
  BSG_HIP(hipStreamSynchronize(st));   // (the previous binding's tables may still be read by launches in flight)
  TRY(grow(h, &h->rg_cap, host.size(), st));
  BSG_HIP(hipMemcpy(h->rg_dev, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice));
  h->rg_lens.assign(lens, lens + B);
  h->bound.ragged = true;
  return BSG_OK;
}

extern "C" int bsg_diffnet_ragged_native(bsg_diffnet* h, int32_t B, int32_t T, int32_t* native) {
  BSG_REQUIRE(h && native, "diffnet_ragged_native: null argument");
  *native = h->bound.ragged && h->bound.B == B && h->bound.T == T && ragged_launch_ok(h) ? 1 : 0;
  return BSG_OK;
}

// ---- per-handle range guard of the split-fp16 GEMMs (ABI v7): one implementation for the five handle kinds
namespace bsg {
Guard* guard_of_diffnet(void* h) { return &static_cast<bsg_diffnet*>(h)->guard; }
}
