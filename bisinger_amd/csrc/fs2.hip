// FastSpeech2-MIDI encoder / decoder (the condition generator of the diffusion decoder) on gfx950.
//
// Reference semantics (paths relative to /root/reference/train_bisinger):
//   modules/diffsinger_midi/fs2.py:14-65 (FastspeechMIDIEncoder), :94-197 (FastSpeech2MIDI.forward)
//   modules/fastspeech/tts_modules.py:39-58 (LayerNorm eps 1e-12), :61-153 (DurationPredictor),
//     :156-191 (LengthRegulator), :253-309 (FFTBlocks)
//   modules/commons/common_layers.py:106-179 (SinusoidalPositionalEmbedding), :282-346 (MultiheadAttention ->
//     F.multi_head_attention_forward), :598-644 (TransformerFFNLayer), :664-730 (EncSALayer), :832-860 (ESM)
//   modules/commons/espnet_positional_embedding.py:90-114 (RelPositionalEncoding)
//
// Activations live as [rows = b*T + t][C] (C contiguous), so every Linear / attention product / Conv1d-as-
// K-segmented-GEMM goes through the fp32 MFMA GEMM of gemm.hip with a fused epilogue (bias, k^-1/2 scale,
// GELU, residual add, non-padding mask).  The row-wise pieces (LayerNorm, masked softmax) are one-wave-
// per-row kernels with wavefront shuffles; gathers are coalesced 1-KB row copies.  FS2 is ~1.3 % of the
// path's FLOPs (27 MFLOP per frame vs 2.1 GFLOP for 100 diffusion steps), so it is built for exactness
// and simplicity; the unfused attention materialises the [B*H,T,T] score matrix in HBM.
#include <math.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "bsg_common.h"
#include "bsg_ws.h"
#include "diffnet_res.h"
#include "diffnet_tail.h"

namespace bsg {
namespace {

constexpr int H = 256;   // hidden size (checked at create)
// rows of the MIDI front's fixed-size tables (diffsinger_midi/fs2.py:88-92: midi_embed, is_slur_embed, lang_embed, style_embed): what
// fs2_create_impl copies and what the kernels that clamp an id clamp it to
constexpr int MIDI_ROWS = 300, SLUR_ROWS = 2, LANG_ROWS = 2, STYLE_ROWS = 3;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// Ragged front (bsg_fs2midi_encode_ragged / bsg_fs2_decode_ragged): `lens` (device, one count per utterance; null = the padded call) bounds
// utterance b by lens[b] rows while the pitch of its tensors stays T.  true: the row lies at or beyond its utterance's end.
__device__ __forceinline__ bool row_dead(const int* __restrict__ lens, long long row, int T) {
  if (!lens) return false;
  const long long b = row / T;
  return (int)(row - b * T) >= lens[b];
}

// ---- LayerNorm over C = 256: one wave per row, 4 contiguous floats per lane ---------------------
// y = (x - mean) * rsqrt(var + eps) * w + b, then * rowscale[row] (the reference's "* nonpadding").
using ln_f16x4 = __attribute__((ext_vector_type(4))) _Float16;
// yh / yl (optional, instead of y): the result as hi / lo fp16 planes of 16 x value — the activation operand of gemm_h2w_kernel
__global__ void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                 float* __restrict__ y, const float* __restrict__ rowscale, long long rows, float eps,
                                 _Float16* __restrict__ yh, _Float16* __restrict__ yl, unsigned* __restrict__ range_events,
                                 const int* __restrict__ lens, int T) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  if (row_dead(lens, row, T)) {   // ragged: nothing is read; the fp32 result is 0 (the planes are read up to the row's end only)
    if (y) reinterpret_cast<f32x4*>(y + row * H)[lane] = f32x4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  const f32x4 v = reinterpret_cast<const f32x4*>(x + row * H)[lane];
  const float mean = wave_sum(v[0] + v[1] + v[2] + v[3]) * (1.0f / H);
  const float d0 = v[0] - mean, d1 = v[1] - mean, d2 = v[2] - mean, d3 = v[3] - mean;
  const float var = wave_sum(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3) * (1.0f / H);
  const float rstd = 1.0f / sqrtf(var + eps);
  const f32x4 wv = reinterpret_cast<const f32x4*>(w)[lane], bv = reinterpret_cast<const f32x4*>(b)[lane];
  const float rs = rowscale ? rowscale[row] : 1.0f;
  f32x4 o = {(d0 * rstd * wv[0] + bv[0]) * rs, (d1 * rstd * wv[1] + bv[1]) * rs, (d2 * rstd * wv[2] + bv[2]) * rs,
             (d3 * rstd * wv[3] + bv[3]) * rs};
  if (y) reinterpret_cast<f32x4*>(y + row * H)[lane] = o;
  if (yh) {
    ln_f16x4 hv, lv;
    bool bad = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float s = o[e] * 16.0f;
      bad |= !(fabsf(s) < 65000.0f);
      hv[e] = (_Float16)s;
      lv[e] = (_Float16)(s - (float)hv[e]);
    }
    reinterpret_cast<ln_f16x4*>(yh + row * H)[lane] = hv;
    reinterpret_cast<ln_f16x4*>(yl + row * H)[lane] = lv;
    if (range_events && __builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0) atomicAdd(range_events, 1u);
  }
}

// ---- masked softmax over keys: one 256-thread workgroup per (batch*head, query) row --------------
__global__ void masked_softmax_kernel(float* __restrict__ S, const float* __restrict__ keep, int Tq, int Tk, int heads) {
  __shared__ float red[4];
  const long long row = blockIdx.x;                 // (b*heads + h)*Tq + q
  const int b = (int)(row / ((long long)heads * Tq));
  float* __restrict__ s = S + row * Tk;
  const float* __restrict__ kp = keep + (long long)b * Tk;   // 1 = real key, 0 = padded key (-> -inf)
  const int tid = threadIdx.x;
  float m = -INFINITY;
  for (int k = tid; k < Tk; k += 256) {
    const float v = kp[k] != 0.f ? s[k] : -INFINITY;
    m = fmaxf(m, v);
  }
  m = wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int k = tid; k < Tk; k += 256) {
    const float e = kp[k] != 0.f ? expf(s[k] - m) : 0.f;
    s[k] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  sum = (red[0] + red[1]) + (red[2] + red[3]);
  for (int k = tid; k < Tk; k += 256) s[k] = sum > 0.f ? s[k] / sum : 0.f;   // (a row without keys: 0, not 0 / 0)
}

// ---- fused self-attention (EncSALayer's MultiheadAttention, common_layers.py:282-370, head dim 128) -------------------
// softmax(Q K^T + key-padding mask) V without materialising the [T,T] scores, fp32 MFMA throughout.  One wave = 32 queries;
// a workgroup of NW waves shares the K / V tiles of a 32-key block in LDS.  Per block:
//   S^T[key, q] = K[32 x 128] Q^T           A = K rows from LDS (stride 129: conflict-free), B = Q from registers (64 per lane)
//   online softmax over keys: a lane owns ONE query (its accumulator column), its keys sit in its 16 registers and in the
//   partner lane (lane ^ 32): max / sum are 16 in-register steps + one cross-half shuffle; the running output is rescaled
//   in registers (exp(m_old - m_new) is per lane)
//   O^T[d, q] += V^T[d, key] P[key, q]      the S accumulator IS the B operand: MFMA step j takes key row (j&3)+8(j>>2) (+4 for
//   the upper lane half) = register j of the lane, the A operand V[key][d] is read from LDS with that same key order.
// q is pre-scaled by head_dim^-1/2 (fused into the QKV projection); masked keys (keep == 0, or beyond T) get -inf as in the
// reference's masked_fill; rows are [b*T + t][3H] with Q | K | V column blocks.
template <int NW>
__global__ __launch_bounds__(64 * NW, 2) void flash_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ keep,
                                                                float* __restrict__ out, int T, int heads, int ld, int ldo,
                                                                const int* __restrict__ lens) {
  constexpr int D = 128, BK = 32, LDK = D + 1;
  __shared__ float Ks[BK * LDK];
  __shared__ __attribute__((aligned(16))) float Vs[BK * D];
  __shared__ float kp[BK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int b = blockIdx.y / heads, hh = blockIdx.y - b * heads;
  const int q_row = (blockIdx.x * NW + wave) * 32 + l31;
  const int Tb = lens ? lens[b] : T;              // ragged: queries and keys of this utterance end at lens[b]; T stays the pitch
  if ((int)blockIdx.x * NW * 32 >= Tb) return;    // (ragged only: the whole query tile lies beyond the utterance: nothing is loaded)
  const bool q_ok = q_row < Tb;
  const float* __restrict__ base = qkv + (long long)b * T * ld + hh * D;
  float qreg[64];
  {
    const float* __restrict__ qp = base + (long long)(q_ok ? q_row : Tb - 1) * ld;
#pragma unroll
    for (int s = 0; s < 64; ++s) qreg[s] = qp[2 * s + lh];
  }
  f32x16 O[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) O[dt][r] = 0.f;
  float m = -INFINITY, l = 0.f;
  const int H3 = ld / 3;
  for (int k0 = 0; k0 < Tb; k0 += BK) {
    __syncthreads();   // the previous block's tiles are consumed
#pragma unroll
    for (int j = 0; j < 1024 / (64 * NW); ++j) {
      const int idx = tid + 64 * NW * j;
      const int key = idx >> 5, c4 = (idx & 31) << 2;
      const int kt = k0 + key;
      f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = kv;
      if (kt < Tb) {
        const float* __restrict__ rp = base + (long long)kt * ld + c4;
        kv = *reinterpret_cast<const f32x4*>(rp + H3);
        vv = *reinterpret_cast<const f32x4*>(rp + 2 * H3);
      }
      Ks[key * LDK + c4] = kv[0]; Ks[key * LDK + c4 + 1] = kv[1]; Ks[key * LDK + c4 + 2] = kv[2]; Ks[key * LDK + c4 + 3] = kv[3];
      *reinterpret_cast<f32x4*>(&Vs[key * D + c4]) = vv;
    }
    if (tid < BK) kp[tid] = (k0 + tid < Tb) ? keep[(long long)b * T + k0 + tid] : 0.f;
    __syncthreads();
    f32x16 S;
#pragma unroll
    for (int r = 0; r < 16; ++r) S[r] = 0.f;
    {
      const float* __restrict__ kr = Ks + l31 * LDK + lh;
#pragma unroll
      for (int s = 0; s < 64; ++s) S = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[2 * s], qreg[s], S, 0, 0, 0);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (kp[acc_row(r, lh)] == 0.f) S[r] = -INFINITY;
      mx = fmaxf(mx, S[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m, mx);
    const float ms = m_new == -INFINITY ? 0.f : m_new;     // a block of masked keys only must not produce inf - inf
    const float scale = expf(m - ms);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      S[r] = expf(S[r] - ms);
      ps += S[r];
    }
    ps += __shfl_xor(ps, 32);
    l = l * scale + ps;
    m = m_new;
    const bool rescale = __any(scale != 1.0f);   // wave-uniform: once the running maxima have settled nothing is rescaled
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      if (rescale) {
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dt][r] *= scale;
      }
      const float* __restrict__ vr = Vs + 4 * lh * D + 32 * dt + l31;
#pragma unroll
      for (int j = 0; j < 16; ++j) O[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[((j & 3) + 8 * (j >> 2)) * D], S[j], O[dt], 0, 0, 0);
    }
  }
  if (q_ok) {
    const float inv = l > 0.f ? 1.0f / l : 0.f;   // a row without keys (an empty utterance of the batch): O = 0 and l = 0 give 0, not 0 x inf
    float* __restrict__ op = out + ((long long)b * T + q_row) * ldo + hh * D;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) op[32 * dt + acc_row(r, lh)] = O[dt][r] * inv;
  }
}

// ---- the same fused attention with every product on the 16-bit matrix pipe (split-fp16, see gemm.hip / diffnet_h2.hip) --------------
// Q, K, V are scaled by 2^4 and split exactly into hi + lo fp16 terms (Q once, into registers; K and V while their 32-key block is staged:
// K as [key][128 d] planes, V TRANSPOSED as [d][32 keys] planes), the probabilities P = exp(S - m) in [0, 1] by 2^10 and split in
// registers; every fp32 product is hi hi + hi lo + lo hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation: 48 MFMAs of 32 matrix cycles
// per key block and wave instead of 128 of 64.  The softmax runs in fp32 on the un-scaled scores exactly as above.
//   S^T[key, q]: A = K fragment (lane = key, 8 consecutive d per lane half), B = Q fragment of the lane's query.
//   O^T[d, q] += V^T[d, key] P[key, q]: the lane's 16 probabilities are keys (r&3) + 8 (r>>2) + 4 lh; MFMA step t takes its registers
//   8t .. 8t+7 as the 8 k-values of the lane half, so the A fragment of V^T is read with that key order: two 8-byte pieces of a [d] row.
// Operands beyond the fp16 range (|v| >= 4062) are counted in the GEMMs' range-event counter (the host repeats the call on the
// fp32 pipe).
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f16x4 = __attribute__((ext_vector_type(4))) _Float16;
using u32x2_t = __attribute__((ext_vector_type(2))) unsigned;
using u32x4_t = __attribute__((ext_vector_type(4))) unsigned;

template <int NW>
__global__ __launch_bounds__(64 * NW, 2) void flash_attn_split_kernel(const float* __restrict__ qkv, const float* __restrict__ keep,
                                                                      float* __restrict__ out, int T, int heads, int ld, int ldo,
                                                                      unsigned* __restrict__ range_events, _Float16* __restrict__ out_h,
                                                                      long long out_plane, const int* __restrict__ lens) {
  constexpr int D = 128, BK = 32, KROW = 2 * D + 16, VROW = 2 * BK + 16;   // bytes per LDS row: 272 (68 dwords = 4 mod 64), 80
  constexpr float SIN = 16.0f, PSC = 1024.0f;
  __shared__ __attribute__((aligned(16))) char Kp[2 * BK * KROW];    // hi plane, lo plane
  __shared__ __attribute__((aligned(16))) char Vp[2 * D * VROW];
  __shared__ float kp[BK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int b = blockIdx.y / heads, hh = blockIdx.y - b * heads;
  const int q_row = (blockIdx.x * NW + wave) * 32 + l31;
  const int Tb = lens ? lens[b] : T;              // ragged: queries and keys of this utterance end at lens[b]; T stays the pitch
  if ((int)blockIdx.x * NW * 32 >= Tb) return;    // (ragged only: the whole query tile lies beyond the utterance: nothing is loaded)
  const bool q_ok = q_row < Tb;
  const float* __restrict__ base = qkv + (long long)b * T * ld + hh * D;
  bool bad = false;
  auto split8 = [&](const f32x4 a, const f32x4 c, f16x8& hi, f16x8& lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = (e < 4 ? a[e] : c[e - 4]) * SIN;
      bad |= !(fabsf(x) < 65000.0f);
      hi[e] = (_Float16)x;
      lo[e] = (_Float16)(x - (float)hi[e]);
    }
  };
  f16x8 qh[8], ql[8];   // d = 16 s + 8 lh + 0..7
  {
    const float* __restrict__ qp = base + (long long)(q_ok ? q_row : Tb - 1) * ld + 8 * lh;
#pragma unroll
    for (int s = 0; s < 8; ++s)
      split8(*reinterpret_cast<const f32x4*>(qp + 16 * s), *reinterpret_cast<const f32x4*>(qp + 16 * s + 4), qh[s], ql[s]);
  }
  f32x16 O[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) O[dt][r] = 0.f;
  float m = -INFINITY, l = 0.f;
  const int H3 = ld / 3;
  for (int k0 = 0; k0 < Tb; k0 += BK) {
    __syncthreads();   // the previous block's tiles are consumed
#pragma unroll 2
    for (int j = 0; j < 1024 / (64 * NW); ++j) {
      const int idx = tid + 64 * NW * j;
      const int key = idx >> 5, c4 = (idx & 31) << 2;
      const int kt = k0 + key;
      f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = kv;
      if (kt < Tb) {
        const float* __restrict__ rp = base + (long long)kt * ld + c4;
        kv = *reinterpret_cast<const f32x4*>(rp + H3);
        vv = *reinterpret_cast<const f32x4*>(rp + 2 * H3);
      }
      f16x4 kh4, kl4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = kv[e] * SIN, y = vv[e] * SIN;
        bad |= !(fabsf(x) < 65000.0f) || !(fabsf(y) < 65000.0f);
        kh4[e] = (_Float16)x;
        kl4[e] = (_Float16)(x - (float)kh4[e]);
        const _Float16 vh = (_Float16)y, vl = (_Float16)(y - (float)vh);
        *reinterpret_cast<_Float16*>(Vp + (c4 + e) * VROW + key * 2) = vh;
        *reinterpret_cast<_Float16*>(Vp + D * VROW + (c4 + e) * VROW + key * 2) = vl;
      }
      *reinterpret_cast<f16x4*>(Kp + key * KROW + c4 * 2) = kh4;
      *reinterpret_cast<f16x4*>(Kp + BK * KROW + key * KROW + c4 * 2) = kl4;
    }
    if (tid < BK) kp[tid] = (k0 + tid < Tb) ? keep[(long long)b * T + k0 + tid] : 0.f;
    __syncthreads();
    f32x16 S;
#pragma unroll
    for (int r = 0; r < 16; ++r) S[r] = 0.f;
    {
      const char* kr = Kp + l31 * KROW + 16 * lh;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const f16x8 ah = *reinterpret_cast<const f16x8*>(kr + 32 * s);
        const f16x8 al = *reinterpret_cast<const f16x8*>(kr + 32 * s + BK * KROW);
        S = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, qh[s], S, 0, 0, 0);
        S = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, ql[s], S, 0, 0, 0);
        S = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, qh[s], S, 0, 0, 0);
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      S[r] *= 1.0f / (SIN * SIN);
      if (kp[acc_row(r, lh)] == 0.f) S[r] = -INFINITY;
      mx = fmaxf(mx, S[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m, mx);
    const float ms = m_new == -INFINITY ? 0.f : m_new;     // a block of masked keys only must not produce inf - inf
    const float scale = expf(m - ms);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      S[r] = expf(S[r] - ms);
      ps += S[r];
    }
    ps += __shfl_xor(ps, 32);
    l = l * scale + ps;
    m = m_new;
    f16x8 ph[2], pl[2];   // step t: registers 8t .. 8t+7 = keys 16 t + 4 lh + (j & 3) + 8 (j >> 2)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = S[8 * t + j] * PSC;
        ph[t][j] = (_Float16)x;
        pl[t][j] = (_Float16)(x - (float)ph[t][j]);
      }
    const bool rescale = __any(scale != 1.0f);   // wave-uniform: once the running maxima have settled nothing is rescaled
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      if (rescale) {
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dt][r] *= scale;
      }
      const char* vr = Vp + (32 * dt + l31) * VROW + 8 * lh;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const u32x2_t h0 = *reinterpret_cast<const u32x2_t*>(vr + 32 * t), h1 = *reinterpret_cast<const u32x2_t*>(vr + 32 * t + 16);
        const u32x2_t l0 = *reinterpret_cast<const u32x2_t*>(vr + 32 * t + D * VROW), l1 = *reinterpret_cast<const u32x2_t*>(vr + 32 * t + 16 + D * VROW);
        const f16x8 ah = __builtin_bit_cast(f16x8, u32x4_t{h0[0], h0[1], h1[0], h1[1]});
        const f16x8 al = __builtin_bit_cast(f16x8, u32x4_t{l0[0], l0[1], l1[0], l1[1]});
        O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, ph[t], O[dt], 0, 0, 0);
        O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, pl[t], O[dt], 0, 0, 0);
        O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, ph[t], O[dt], 0, 0, 0);
      }
    }
  }
  if (q_ok && out_h) {
    // the attention output is read by the output projection only: written as the hi / lo fp16 planes of 16 x value that gemm_h2w_kernel
    // stages (registers 4 g .. 4 g + 3 of a lane are 4 consecutive d: one 8-byte store per plane)
    const float inv = l > 0.f ? 1.0f / (l * SIN * PSC) : 0.f;   // (a row without keys: 0, not 0 x inf)
    _Float16* __restrict__ oph = out_h + ((long long)b * T + q_row) * ldo + hh * D;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        f16x4 hv, lv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = O[dt][4 * gq + e] * inv * SIN;
          bad |= !(fabsf(x) < 65000.0f);
          hv[e] = (_Float16)x;
          lv[e] = (_Float16)(x - (float)hv[e]);
        }
        *reinterpret_cast<f16x4*>(oph + 32 * dt + 8 * gq + 4 * lh) = hv;
        *reinterpret_cast<f16x4*>(oph + out_plane + 32 * dt + 8 * gq + 4 * lh) = lv;
      }
  }
  if (range_events && __builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0) atomicAdd(range_events, 1u);
  if (q_ok && !out_h) {
    const float inv = l > 0.f ? 1.0f / (l * SIN * PSC) : 0.f;   // (a row without keys: 0, not 0 x inf)
    float* __restrict__ op = out + ((long long)b * T + q_row) * ldo + hh * D;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) op[32 * dt + acc_row(r, lh)] = O[dt][r] * inv;
  }
}

// ---- token embeddings ----------------------------------------------------------------------------
constexpr int FLP_LDS = 2 * (2 * 32 * 272 + 2 * 128 * 80);   // flash_attn_planes_kernel: two K and two V^T buffers = 75 776 B
// ---- round 4: the fused attention on PRE-SPLIT operands -------------------------------------------------------------------------------
// flash_attn_split_kernel splits K and V while it stages every 32-key block — and transposes V with 2-byte LDS writes — once per 64 or 128
// queries: at T = 1000 a K / V element is split 8-16 times, between two barriers and with its global loads exposed.  Here
// qkv_split_kernel (BSG_QKV_FUSED=0; by default the QKV product's own epilogue, H2wArgs::qkv_T — one launch less per layer) splits the QKV
// projection's output ONCE into fp16 planes — Q and K as [row][256] (hi, lo), V TRANSPOSED as
// [b][256 (head, d)][Tp keys] (Tp = T rounded up to 32, the padding zeroed; keys in fragment order within groups of 16) — plus one mask word per (utterance, 32-key block), and
// flash_attn_planes_kernel stages a key block as plain 16-byte copies while the MFMAs of the blocks before it run: K two blocks ahead, V^T one,
// one barrier per block, no vector arithmetic in the staging, the softmax in the log2 domain (v_exp_f32, the 2^10 of the P operand folded into the
// exponent), its two cross-half reductions as v_permlane32_swap, blocks whose mask word is all ones skip the masking.  Same products, fragments
// and key order as flash_attn_split_kernel (its comment above).
// Measured (T = 1000, decoder layer): 118 -> 88 us at B = 16, 99 -> 63 us at B = 1 against the first planes form (the split-in-kernel form: 270 /
// 200 us).  PMC of this kernel (profiles/r04_flash_planes_pmc.txt): matrix pipe busy 25 % of the wave cycles, vector issue 29 %, LDS 8 %,
// s_waitcnt 18 % — the grid is B x heads x T / 32 = 1024 waves at B = 16, ONE wave per SIMD, so nothing hides the in-order dependences of a wave.
// Batches that leave SIMDs empty split the KEYS of a query tile over gridDim.z = 2 or 4 workgroups (each a shorter serial chain of key blocks);
// the last to arrive combines the un-normalised partials in the order of z: a single utterance 63 -> 27 us per decoder layer, the 8 utterances of
// a configs[3] rank 66 -> 50 us.  (With agent-scope fences around the count the same split was SLOWER than no split — 100 against 66 us: every
// workgroup's release is an L2 write-back; write-through stores + sc1 loads, the residual launches' hand-off form, cost nothing measurable.)
// mask words of flash_attn_planes_kernel when the QKV product writes the planes itself (H2wArgs::qkv_T): one wave per (utterance, 32-key block)
__global__ __launch_bounds__(256) void key_mask_kernel(const float* __restrict__ keep, unsigned* __restrict__ kmask, int B, int T, int Tp) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, nblk = Tp / 32;
  if (w >= B * nblk) return;
  const int b = w / nblk, t = (w - b * nblk) * 32 + lane;
  const unsigned long long mk = __builtin_amdgcn_ballot_w64(lane < 32 && t < T && keep[(long long)b * T + t] != 0.f);
  if (lane == 0) kmask[w] = (unsigned)mk;
}

__global__ __launch_bounds__(256) void qkv_split_kernel(const float* __restrict__ qkv, _Float16* __restrict__ qk, long long qk_plane,
                                                        _Float16* __restrict__ vt, long long vt_plane, int T, int Tp,
                                                        const float* __restrict__ keep, unsigned* __restrict__ kmask,
                                                        unsigned* __restrict__ range_events) {
  __shared__ __attribute__((aligned(16))) _Float16 vh[32][H + 8], vl[32][H + 8];   // the tile's V rows for the transpose
  const int b = blockIdx.y, t0 = blockIdx.x * 32, tid = threadIdx.x;
  bool bad = false;
  if (tid < 64) {   // bit j of the tile's mask word: key t0 + j takes part in the softmax (keep != 0, j < T)
    const unsigned long long mk = __builtin_amdgcn_ballot_w64(tid < 32 && t0 + tid < T && keep[(long long)b * T + t0 + tid] != 0.f);
    if (tid == 0) kmask[b * (Tp / 32) + blockIdx.x] = (unsigned)mk;
  }
  // Q | K: 32 rows x 512 columns, 8 values per item -> [row][512] planes (Q = columns 0..255, K = 256..511)
  for (int it = tid; it < 32 * 96; it += 256) {
    const int r = it / 96, c8 = (it - r * 96) * 8, t = t0 + r;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, c = a;
    if (t < T) {
      const float* p = qkv + ((long long)b * T + t) * (3 * H) + c8;
      a = *reinterpret_cast<const f32x4*>(p);
      c = *reinterpret_cast<const f32x4*>(p + 4);
    }
    f16x8 h, l;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = (e < 4 ? a[e] : c[e - 4]) * 16.0f;
      bad |= !(fabsf(x) < 65000.0f);
      h[e] = (_Float16)x;
      l[e] = (_Float16)(x - (float)h[e]);
    }
    if (c8 < 2 * H) {
      if (t < T) {
        _Float16* d = qk + ((long long)b * T + t) * (2 * H) + c8;
        *reinterpret_cast<f16x8*>(d) = h;
        *reinterpret_cast<f16x8*>(d + qk_plane) = l;
      }
    } else {
      *reinterpret_cast<f16x8*>(&vh[r][c8 - 2 * H]) = h;      // rows t >= T: zeros
      *reinterpret_cast<f16x8*>(&vl[r][c8 - 2 * H]) = l;
    }
  }
  __syncthreads();
  // V^T: thread = one (head, d) row, 32 keys = 64 bytes per plane
  {
    const int d = tid;
    _Float16 th[32], tl[32];
#pragma unroll
    for (int r = 0; r < 32; ++r) { th[r] = vh[r][d]; tl[r] = vl[r][d]; }
    _Float16* dst = vt + ((long long)b * H + d) * Tp + t0;
#pragma unroll
    // within a group of 16 keys the stored order is 0-3, 8-11, 4-7, 12-15: the 8 keys one lane feeds to a P V MFMA (16 t + 4 lh + (j & 3) + 8 (j >> 2))
    // are then 16 contiguous bytes
    for (int g = 0; g < 4; ++g) {
      const int k = 16 * (g >> 1) + 4 * (g & 1);
      *reinterpret_cast<f16x8*>(dst + 8 * g) = f16x8{th[k], th[k + 1], th[k + 2], th[k + 3], th[k + 8], th[k + 9], th[k + 10], th[k + 11]};
      *reinterpret_cast<f16x8*>(dst + vt_plane + 8 * g) = f16x8{tl[k], tl[k + 1], tl[k + 2], tl[k + 3], tl[k + 8], tl[k + 9], tl[k + 10], tl[k + 11]};
    }
  }
  if (range_events && __builtin_amdgcn_ballot_w64(bad) != 0ull && (tid & 63) == 0) atomicAdd(range_events, 1u);
}

template <int NW>
__global__ __launch_bounds__(64 * NW, 1) void flash_attn_planes_kernel(const _Float16* __restrict__ qk, long long qk_plane,
                                                                       const _Float16* __restrict__ vt, long long vt_plane,
                                                                       const unsigned* __restrict__ kmask, int T, int Tp, int heads,
                                                                       _Float16* __restrict__ out_h, long long out_plane, int ldo,
                                                                       unsigned* __restrict__ range_events, float* __restrict__ part,
                                                                       unsigned* __restrict__ cnt, const int* __restrict__ lens) {
  constexpr int D = 128, BK = 32, KROW = 2 * D + 16, VROW = 2 * BK + 16;   // bytes per LDS row: 272 (68 dwords = 4 mod 64), 80
  constexpr int KB = 2 * BK * KROW, VB = 2 * D * VROW;                     // K hi | K lo, V^T hi | V^T lo of one key block
  constexpr int NTH = 64 * NW, NPC = 1024 / NTH;                           // 16-byte pieces of a block's K (or V^T) per thread
  constexpr float SIN = 16.0f;
  constexpr float C2 = 1.4426950408889634f / (SIN * SIN);                  // scores -> log2 domain (operands carry SIN each)
  extern __shared__ __attribute__((aligned(16))) char fl[];                // K buffers [2][KB] | V^T buffers [2][VB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int b = blockIdx.y / heads, hh = blockIdx.y - b * heads;
  const int q_row = (blockIdx.x * NW + wave) * 32 + l31;
  // ragged: queries and keys of this utterance end at lens[b]; T and Tp stay the pitches.  A query tile beyond the end returns before it loads
  // anything (all gridDim.z workgroups of the tile alike: the arrival counter stays 0).  Key blocks at or beyond the end are staged (the
  // pipeline below is unconditional) but never scored into a result; inside the last block the keys beyond the end are masked (kmask) and
  // their K / V rows are the zeros the QKV product stores there.
  const int Tb = lens ? lens[b] : T;
  if ((int)blockIdx.x * NW * 32 >= Tb) return;
  const bool q_ok = q_row < Tb;
  const _Float16* __restrict__ qkb = qk + (long long)b * T * (2 * H) + hh * D;          // Q of this head; K at + H
  const _Float16* __restrict__ vtb = vt + ((long long)b * H + hh * D) * Tp;
  const unsigned* __restrict__ kmb = kmask + b * (Tp / 32);
  f16x8 qh[8], ql[8];   // d = 16 s + 8 lh + 0..7
  {
    const _Float16* qp = qkb + (long long)(q_ok ? q_row : Tb - 1) * (2 * H) + 8 * lh;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      qh[s] = *reinterpret_cast<const f16x8*>(qp + 16 * s);
      ql[s] = *reinterpret_cast<const f16x8*>(qp + 16 * s + qk_plane);
    }
  }
  // staging: K of a block = 1024 16-byte pieces (plane p >> 9, key (p >> 4) & 31, chunk p & 15), V^T likewise (plane p >> 9, row d = (p >> 2) & 127,
  // chunk p & 3).  One register set serves both.  The loop is software-pipelined: iteration i forms the scores of block i + 1 (matrix pipe)
  // while the softmax of block i runs (vector pipe), so K is staged TWO blocks ahead and V^T one:
  //   iteration i reads K(i+1) from K buffer (i+1)&1 and V^T(i) from V buffer i&1, writes K(i+2) to K buffer i&1 (last read in iteration i-1) and
  //   V^T(i+1) to V buffer (i+1)&1 (last read in iteration i-1); one barrier per iteration.
  u32x4_t st[NPC], sv[NPC];
  // piece j of thread tid: K key (tid >> 4) + KPP j' (j' = j mod NPC/2), chunk tid & 15, plane j / (NPC/2); V^T row (tid >> 2) + VPP j', chunk
  // tid & 3.  Per thread ONE 32-bit offset each for K, V^T and the two LDS images; everything that depends on j or on the block is wave-uniform.
  constexpr int KPP = NTH / 16, VPP = NTH / 4, HP = NPC / 2;
  const unsigned koff = ((tid >> 4) * (2 * H) + (tid & 15) * 8) * 2, kls = (tid >> 4) * KROW + (tid & 15) * 16;
  const unsigned voff = ((tid >> 2) * Tp + (tid & 3) * 8) * 2, vls = (tid >> 2) * VROW + (tid & 3) * 16;
  const char* __restrict__ kbase = reinterpret_cast<const char*>(qkb + H);
  const char* __restrict__ vbase = reinterpret_cast<const char*>(vtb);
  auto load_k = [&](int k0) {   // rows past T (k0 is clamped to the padded length): the next utterance's keys or stale workspace — their scores are masked
    k0 = min(k0, Tp - BK);
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      const char* bj = kbase + ((long long)(k0 + KPP * (j % HP)) * (2 * H) + (j / HP ? qk_plane : 0)) * 2;
      st[j] = *reinterpret_cast<const u32x4_t*>(bj + koff);
    }
  };
  auto store_k = [&](int buf) {
    char* sb = fl + buf * KB + kls;
#pragma unroll
    for (int j = 0; j < NPC; ++j) *reinterpret_cast<u32x4_t*>(sb + (j / HP) * BK * KROW + KPP * (j % HP) * KROW) = st[j];
  };
  auto load_v = [&](int k0) {   // k0 + 32 <= Tp: the planes are padded to Tp keys and the padding is zero
    k0 = min(k0, Tp - BK);
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      const char* bj = vbase + ((long long)(VPP * (j % HP)) * Tp + k0 + (j / HP ? vt_plane : 0)) * 2;
      sv[j] = *reinterpret_cast<const u32x4_t*>(bj + voff);
    }
  };
  auto store_v = [&](int buf) {
    char* sb = fl + 2 * KB + buf * VB + vls;
#pragma unroll
    for (int j = 0; j < NPC; ++j) *reinterpret_cast<u32x4_t*>(sb + (j / HP) * D * VROW + VPP * (j % HP) * VROW) = sv[j];
  };
  auto scores = [&](int buf, f32x16& S) {   // S[key][query] = sum_d K Q, 3 fp16 products per fp32 product
    const char* kr = fl + buf * KB + l31 * KROW + 16 * lh;
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const f16x8 ah = *reinterpret_cast<const f16x8*>(kr + 32 * s);
      const f16x8 al = *reinterpret_cast<const f16x8*>(kr + 32 * s + BK * KROW);
      S = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, qh[s], s == 0 ? zero : S, 0, 0, 0);
      S = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, ql[s], S, 0, 0, 0);
      S = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, qh[s], S, 0, 0, 0);
    }
  };
  f32x16 O[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) O[dt][r] = 0.f;
  float m = -INFINITY, l = 0.f;   // running maximum (log2 domain), running sum (carries the 2^10 of the P operand)
  // One key block: S = this block's scores (formed in the previous iteration), Sn <- the next block's.  Straight-line code — the staging is
  // unconditional (past the end it moves clamped rows nobody reads) — so that the scheduler can run the Q K^T MFMAs of block i + 1 under the softmax
  // of block i and the staging under the P V MFMAs.
  auto block = [&](auto masked, auto curc, int k0, f32x16& S, f32x16& Sn, unsigned km) {
    constexpr bool MASKED = decltype(masked)::value;
    constexpr int cur = decltype(curc)::value;
    store_k(cur);            // K(i+2), requested at the start of the previous iteration
    load_k(k0 + 3 * BK);
    load_v(k0 + BK);
    scores(cur ^ 1, Sn);
    if constexpr (MASKED) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (!((km >> acc_row(r, lh)) & 1u)) S[r] = -INFINITY;
    }
    float mx = S[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, S[r]);
    {
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);   // the other 16 keys of this query
      mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
    }
    const float m_new = fmaxf(m, mx * C2);
    const float ms = m_new == -INFINITY ? 0.f : m_new;     // a block of masked keys only must not produce inf - inf
    const float scale = __builtin_amdgcn_exp2f(m - ms);
    const float off = 10.0f - ms;                          // P carries 2^10: the fp16 hi / lo split of values <= 1024
    float ps = 0.f;
    f16x8 ph[2], pl[2];   // step t: registers 8t .. 8t+7 = keys 16 t + 4 lh + (j & 3) + 8 (j >> 2)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = __builtin_amdgcn_exp2f(fmaf(S[8 * t + j], C2, off));
        ps += x;
        ph[t][j] = (_Float16)x;
        pl[t][j] = (_Float16)(x - (float)ph[t][j]);
      }
    {
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(ps), __float_as_uint(ps), false, false);
      ps = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    l = l * scale + ps;
    m = m_new;
    if (__any(scale != 1.0f)) {   // wave-uniform: once the running maxima have settled nothing is rescaled
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dt][r] *= scale;
    }
    const char* Vp = fl + 2 * KB + cur * VB;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const char* vr = Vp + (32 * dt + l31) * VROW + 16 * lh;   // the keys of a lane are contiguous (qkv_split_kernel's order): one 16-byte read, conflict-free
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const f16x8 ah = *reinterpret_cast<const f16x8*>(vr + 32 * t);
        const f16x8 al = *reinterpret_cast<const f16x8*>(vr + 32 * t + D * VROW);
        O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, ph[t], O[dt], 0, 0, 0);
        O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, pl[t], O[dt], 0, 0, 0);
        O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, ph[t], O[dt], 0, 0, 0);
      }
    }
    store_v(cur ^ 1);        // V^T(i+1)
    __syncthreads();         // this block is consumed; K(i+2) and V^T(i+1) are complete
  };
  using std::integral_constant;
  // key split (gridDim.z = KS > 1, small batches): this workgroup takes the key blocks [kbeg, kend) of its query tile and leaves an un-normalised
  // partial (O, m, l); the last of the KS workgroups to arrive combines them in the order of z (below)
  const int KS = (int)gridDim.z;
  const int nbz = (Tp / BK + KS - 1) / KS;
  const int kbeg = (int)blockIdx.z * nbz * BK, kend = min(Tb, kbeg + nbz * BK);
  load_k(kbeg);
  store_k(0);
  load_k(kbeg + BK);
  store_k(1);
  load_v(kbeg);
  store_v(0);
  load_k(kbeg + 2 * BK);
  __syncthreads();
  f32x16 S0, S1;
  scores(0, S0);
  __syncthreads();   // K buffer 0 is free for K(2)
  for (int k0 = kbeg; k0 < kend; k0 += 2 * BK) {
    const unsigned km0 = kmb[k0 >> 5];   // wave-uniform
    if (km0 == 0xffffffffu) block(integral_constant<bool, false>{}, integral_constant<int, 0>{}, k0, S0, S1, km0);
    else block(integral_constant<bool, true>{}, integral_constant<int, 0>{}, k0, S0, S1, km0);
    if (k0 + BK >= kend) break;
    const unsigned km1 = kmb[(k0 >> 5) + 1];
    if (km1 == 0xffffffffu) block(integral_constant<bool, false>{}, integral_constant<int, 1>{}, k0 + BK, S1, S0, km1);
    else block(integral_constant<bool, true>{}, integral_constant<int, 1>{}, k0 + BK, S1, S0, km1);
  }
  if (KS > 1) {
    // partial of (unit, z): O [NW][16 register quads][64 lanes][4], m [NW][64], l [NW][64] (16 bytes per lane: coalesced).  The hand-off form of
    // the residual launches (diffnet_h2.hip): write-through (sc1) stores, drained, a barrier, then the count; the combining workgroup reads with sc1
    // loads — no agent-scope fence (an L2 write-back per workgroup: measured 45 us per launch of 512 workgroups)
    constexpr int PS = NW * 64 * 66;
    const int unit = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
    const rsrc_t rp = mk_rsrc(part + (long long)unit * KS * PS, (unsigned)(KS * PS * 4));
    const int zoff = (int)blockIdx.z * PS * 4;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 v = {O[dt][4 * g4], O[dt][4 * g4 + 1], O[dt][4 * g4 + 2], O[dt][4 * g4 + 3]};
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rp, ((wave * 16 + dt * 4 + g4) * 64 + lane) * 16, zoff, 16);
      }
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, m), rp, (NW * 4096 + wave * 64 + lane) * 4, zoff, 16);
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, l), rp, (NW * 4096 + NW * 64 + wave * 64 + lane) * 4, zoff, 16);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned* arrived = reinterpret_cast<unsigned*>(fl);   // (the key buffers are dead)
    if (tid == 0) *arrived = __hip_atomic_fetch_add(cnt + unit, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (*arrived != (unsigned)(KS - 1)) return;
    if (tid == 0) __hip_atomic_store(cnt + unit, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
    float M = -INFINITY;
    for (int z = 0; z < KS; ++z)
      M = fmaxf(M, __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rp, (NW * 4096 + wave * 64 + lane) * 4, z * PS * 4, 16)));
    const float Ms = M == -INFINITY ? 0.f : M;
    l = 0.f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) O[dt][r] = 0.f;
    for (int z = 0; z < KS; ++z) {   // fixed order: the result does not depend on which workgroup combines
      const float mz = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rp, (NW * 4096 + wave * 64 + lane) * 4, z * PS * 4, 16));
      const float lz = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rp, (NW * 4096 + NW * 64 + wave * 64 + lane) * 4, z * PS * 4, 16));
      const float wz = __builtin_amdgcn_exp2f(mz - Ms);
      l = fmaf(wz, lz, l);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rp, ((wave * 16 + dt * 4 + g4) * 64 + lane) * 16, z * PS * 4, 16));
#pragma unroll
          for (int e = 0; e < 4; ++e) O[dt][4 * g4 + e] = fmaf(wz, v[e], O[dt][4 * g4 + e]);
        }
    }
  }
  bool bad = false;
  if (q_ok) {
    // the attention output is read by the output projection only: hi / lo fp16 planes of 16 x value (registers 4 g .. 4 g + 3 of a lane are 4
    // consecutive d: one 8-byte store per plane)
    const float inv = l > 0.f ? 1.0f / (l * SIN) : 0.f;   // l carries the 2^10 of P; a row without keys: 0, not 0 x inf
    _Float16* __restrict__ oph = out_h + ((long long)b * T + q_row) * ldo + hh * D;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        f16x4 hv, lv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = O[dt][4 * gq + e] * inv * SIN;
          bad |= !(fabsf(x) < 65000.0f);
          hv[e] = (_Float16)x;
          lv[e] = (_Float16)(x - (float)hv[e]);
        }
        *reinterpret_cast<f16x4*>(oph + 32 * dt + 8 * gq + 4 * lh) = hv;
        *reinterpret_cast<f16x4*>(oph + out_plane + 32 * dt + 8 * gq + 4 * lh) = lv;
      }
  }
  if (range_events && __builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0) atomicAdd(range_events, 1u);
}

// x0 = sqrt(H) * E_tok[txt]; lang_e = E_lang[lang]                      (diffsinger_midi/fs2.py:28,122)
__global__ void embed_tokens_kernel(const long long* __restrict__ txt, const long long* __restrict__ lang,
                                    const float* __restrict__ Etok, const float* __restrict__ Elang, float* __restrict__ x0,
                                    float* __restrict__ lang_e, long long rows, float scale, _Float16* __restrict__ x0h,
                                    _Float16* __restrict__ x0l, unsigned* __restrict__ range_events) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  f32x4 e = reinterpret_cast<const f32x4*>(Etok + txt[row] * H)[lane];
  e *= scale;
  reinterpret_cast<f32x4*>(x0 + row * H)[lane] = e;
  if (x0h) {   // x0 as the operand of the ESM's query projection on the pre-split GEMM: hi / lo fp16 planes of 16 x0
    ln_f16x4 hv, lv;
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float x = e[c] * 16.0f;
      bad |= !(fabsf(x) < 65000.0f);
      hv[c] = (_Float16)x;
      lv[c] = (_Float16)(x - (float)hv[c]);
    }
    reinterpret_cast<ln_f16x4*>(x0h + row * H)[lane] = hv;
    reinterpret_cast<ln_f16x4*>(x0l + row * H)[lane] = lv;
    if (range_events && __builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0) atomicAdd(range_events, 1u);
  }
  reinterpret_cast<f32x4*>(lang_e + row * H)[lane] = reinterpret_cast<const f32x4*>(Elang + lang[row] * H)[lane];
}

// x = ((((x0 + midi) + mdur) + slur) + dyn) * sqrt(H) + pe_rev[j], then * keep      (fs2.py:30-34, FFTBlocks :297)
__global__ void embed_finish_kernel(const float* __restrict__ x0, const float* __restrict__ dyn,
                                    const long long* __restrict__ txt, const long long* __restrict__ pitch_midi,
                                    const float* __restrict__ midi_dur, const long long* __restrict__ is_slur,
                                    const float* __restrict__ Emidi, const float* __restrict__ Wdur,
                                    const float* __restrict__ bdur, const float* __restrict__ Eslur,
                                    const float* __restrict__ pe, float* __restrict__ x, float* __restrict__ keep,
                                    long long rows, int Tt, float scale) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int j = (int)(row % Tt);
  const float kp = txt[row] != 0 ? 1.f : 0.f;
  const f32x4 a = reinterpret_cast<const f32x4*>(x0 + row * H)[lane];
  const f32x4 mi = reinterpret_cast<const f32x4*>(Emidi + pitch_midi[row] * H)[lane];
  const f32x4 wd = reinterpret_cast<const f32x4*>(Wdur)[lane], bd = reinterpret_cast<const f32x4*>(bdur)[lane];
  const f32x4 sl = reinterpret_cast<const f32x4*>(Eslur + is_slur[row] * H)[lane];
  const f32x4 dy = reinterpret_cast<const f32x4*>(dyn + row * H)[lane];
  const f32x4 pv = reinterpret_cast<const f32x4*>(pe + (long long)j * H)[lane];
  const float md = midi_dur[row];
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float v = __fadd_rn(a[e], mi[e]);
    v = __fadd_rn(v, __fadd_rn(__fmul_rn(md, wd[e]), bd[e]));
    v = __fadd_rn(v, sl[e]);
    v = __fadd_rn(v, dy[e]);
    o[e] = __fadd_rn(__fmul_rn(v, scale), pv[e]) * kp;
  }
  reinterpret_cast<f32x4*>(x + row * H)[lane] = o;
  if (lane == 0) keep[row] = kp;
}

// The ragged MIDI front (bsg_fs2midi_encode_ragged), embed_tokens_kernel + embed_finish_kernel in one launch: token j of utterance b with
// j < lens[b] gets the same sum in the same order, its ESM term gathered from the two-row table esm_tab[lang] (the ESM of the utterance
// alone: esm_alone_table below).  Beyond an utterance's end only the key mask is written and no input is read.  Ids outside their tables are
// clamped (torch raises): no read out of bounds.
__global__ void embed_ragged_kernel(const long long* __restrict__ txt, const long long* __restrict__ lang,
                                    const long long* __restrict__ pitch_midi, const float* __restrict__ midi_dur,
                                    const long long* __restrict__ is_slur, const float* __restrict__ Etok, const float* __restrict__ esm_tab,
                                    const float* __restrict__ Emidi, const float* __restrict__ Wdur, const float* __restrict__ bdur,
                                    const float* __restrict__ Eslur, const float* __restrict__ pe, float* __restrict__ x,
                                    float* __restrict__ keep, long long rows, int Tt, float scale, int vocab, const int* __restrict__ lens) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const long long b = row / Tt;
  const int j = (int)(row - b * Tt);
  if (j >= lens[b]) {
    if (lane == 0) keep[row] = 0.f;
    return;
  }
  auto clampi = [](long long i, int n) { return i < 0 ? 0ll : i < n ? i : (long long)n - 1; };
  const long long tok = clampi(txt[row], vocab);
  const float kp = tok != 0 ? 1.f : 0.f;
  f32x4 a = reinterpret_cast<const f32x4*>(Etok + tok * H)[lane];
  a *= scale;
  const f32x4 mi = reinterpret_cast<const f32x4*>(Emidi + clampi(pitch_midi[row], MIDI_ROWS) * H)[lane];
  const f32x4 wd = reinterpret_cast<const f32x4*>(Wdur)[lane], bd = reinterpret_cast<const f32x4*>(bdur)[lane];
  const f32x4 sl = reinterpret_cast<const f32x4*>(Eslur + clampi(is_slur[row], SLUR_ROWS) * H)[lane];
  const f32x4 dy = reinterpret_cast<const f32x4*>(esm_tab + clampi(lang[row], LANG_ROWS) * H)[lane];
  const f32x4 pv = reinterpret_cast<const f32x4*>(pe + (long long)j * H)[lane];
  const float md = midi_dur[row];
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float v = __fadd_rn(a[e], mi[e]);
    v = __fadd_rn(v, __fadd_rn(__fmul_rn(md, wd[e]), bd[e]));
    v = __fadd_rn(v, sl[e]);
    v = __fadd_rn(v, dy[e]);
    o[e] = __fadd_rn(__fmul_rn(v, scale), pv[e]) * kp;
  }
  reinterpret_cast<f32x4*>(x + row * H)[lane] = o;
  if (lane == 0) keep[row] = kp;
}

// ---- ESM attention over the BATCH axis (reference quirk, common_layers.py:853) --------------------
// q,k,v: [L=B][N=Tt][H]; for every (n, head) softmax over the L keys.  One thread per (l, n, head).
// q / o hold the Lq QUERY utterances only (all L of them, or a rank's rows: bsg_fs2midi_encode_rows); k / v all L.
template <int HD>
__global__ void esm_attention_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                     float* __restrict__ o, int L, int Lq, int N, int heads, float scale) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)Lq * N * heads;
  if (idx >= total) return;
  const int h = (int)(idx % heads);
  const int n = (int)((idx / heads) % N);
  const int l = (int)(idx / ((long long)heads * N));
  float qv[HD];
  const float* qp = q + ((long long)l * N + n) * H + h * HD;
#pragma unroll
  for (int d = 0; d < HD; ++d) qv[d] = qp[d] * scale;
  float m = -INFINITY;
  for (int j = 0; j < L; ++j) {
    const float* kp = k + ((long long)j * N + n) * H + h * HD;
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) s = fmaf(qv[d], kp[d], s);
    m = fmaxf(m, s);
  }
  float acc[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) acc[d] = 0.f;
  float sum = 0.f;
  for (int j = 0; j < L; ++j) {
    const float* kp = k + ((long long)j * N + n) * H + h * HD;
    const float* vp = v + ((long long)j * N + n) * H + h * HD;
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) s = fmaf(qv[d], kp[d], s);
    const float e = expf(s - m);
    sum += e;
#pragma unroll
    for (int d = 0; d < HD; ++d) acc[d] = fmaf(e, vp[d], acc[d]);
  }
  float* op = o + ((long long)l * N + n) * H + h * HD;
#pragma unroll
  for (int d = 0; d < HD; ++d) op[d] = acc[d] / sum;
}

// The same for L <= 64 utterances with ONE WAVE per (position n, head): lane = query utterance l; the L keys and values of (n, head) are staged in
// LDS once (128-byte rows, coalesced) and read back as broadcasts, instead of every thread streaming its own copy of them through L1 with
// 64 different cache lines per load instruction (186 us at the 64-row token front of configs[3]; this form: see DESIGN.md).  Two passes as
// above (max, then exp and sum) in the same order of operations.  ld = row stride of q / k / v; out fp32 [.][H] and / or hi / lo planes of 16 x out.
__global__ __launch_bounds__(256) void esm_attention_wave_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                 const float* __restrict__ v, int ldq, int ldkv, float* __restrict__ o,
                                                                 _Float16* __restrict__ oh, long long o_plane, int L, int Lq, int N, int heads,
                                                                 float scale, unsigned* __restrict__ range_events) {
  constexpr int HD = 32;
  __shared__ __attribute__((aligned(16))) float kv[4][2][64][HD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int unit = blockIdx.x * 4 + wave;          // (n, head)
  const bool live = unit < N * heads;              // (no early return: the barrier below is the workgroup's)
  const int n = live ? unit / heads : 0, hh = live ? unit - n * heads : 0;
  for (int it = 0; it < (L * 8 + 63) / 64; ++it) {
    const int j = it * 8 + (lane >> 3), d4 = (lane & 7) * 4;
    if (live && j < L) {
      const long long row = ((long long)j * N + n) * ldkv + hh * HD + d4;
      *reinterpret_cast<f32x4*>(&kv[wave][0][j][d4]) = *reinterpret_cast<const f32x4*>(k + row);
      *reinterpret_cast<f32x4*>(&kv[wave][1][j][d4]) = *reinterpret_cast<const f32x4*>(v + row);
    }
  }
  __syncthreads();
  if (!live || lane >= Lq) return;
  const int l = lane;   // LOCAL query row: q, o and the planes hold the Lq query utterances only; the keys are all L
  float qv[HD];
  {
    const float* qp = q + ((long long)l * N + n) * ldq + hh * HD;
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(qp + d);
      qv[d] = t[0] * scale; qv[d + 1] = t[1] * scale; qv[d + 2] = t[2] * scale; qv[d + 3] = t[3] * scale;
    }
  }
  float m = -INFINITY;
  for (int j = 0; j < L; ++j) {
    const float* kp = kv[wave][0][j];
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) s = fmaf(qv[d], kp[d], s);
    m = fmaxf(m, s);
  }
  float acc[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) acc[d] = 0.f;
  float sum = 0.f;
  for (int j = 0; j < L; ++j) {
    const float* kp = kv[wave][0][j];
    const float* vp = kv[wave][1][j];
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) s = fmaf(qv[d], kp[d], s);
    const float e = expf(s - m);
    sum += e;
#pragma unroll
    for (int d = 0; d < HD; ++d) acc[d] = fmaf(e, vp[d], acc[d]);
  }
  const long long orow = ((long long)l * N + n) * H + hh * HD;
  bool bad = false;
#pragma unroll
  for (int d = 0; d < HD; d += 4) {
    f32x4 t;
#pragma unroll
    for (int c = 0; c < 4; ++c) t[c] = acc[d + c] / sum;
    if (o) *reinterpret_cast<f32x4*>(o + orow + d) = t;
    if (oh) {
      ln_f16x4 hv, lv;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float x = t[c] * 16.0f;
        bad |= !(fabsf(x) < 65000.0f);
        hv[c] = (_Float16)x;
        lv[c] = (_Float16)(x - (float)hv[c]);
      }
      *reinterpret_cast<ln_f16x4*>(oh + orow + d) = hv;
      *reinterpret_cast<ln_f16x4*>(oh + o_plane + orow + d) = lv;
    }
  }
  if (range_events && bad) atomicAdd(range_events, 1u);
}

// ---- encoder -> frames ---------------------------------------------------------------------------
// dur_inp = (enc + spk) * src_keep                                                    (fs2.py:164)
__global__ void add_spk_kernel(const float* __restrict__ enc, const long long* __restrict__ spk_id,
                               const float* __restrict__ Espk, const float* __restrict__ keep, float* __restrict__ out,
                               long long rows, int Tt, const int* __restrict__ lens) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows || row_dead(lens, row, Tt)) return;   // (ragged: the predictor's convolutions read a row up to its end only)
  const int lane = threadIdx.x & 63;
  const int b = (int)(row / Tt);
  f32x4 e = reinterpret_cast<const f32x4*>(enc + row * H)[lane];
  if (Espk) e = e + reinterpret_cast<const f32x4*>(Espk + spk_id[b] * H)[lane];   // (no speaker table: the plain front's spk_embed = 0)
  e = e * keep[row];
  reinterpret_cast<f32x4*>(out + row * H)[lane] = e;
}

// decoder_inp[b,t] = (pad(enc)[b, mel2ph[b,t]] + spk[b] + style[b]) * (mel2ph > 0)          (fs2.py:168-189)
__global__ void gather_frames_kernel(const float* __restrict__ enc, const long long* __restrict__ mel2ph,
                                     const long long* __restrict__ spk_id, const long long* __restrict__ style_id,
                                     const float* __restrict__ Espk, const float* __restrict__ Estyle,
                                     float* __restrict__ out, long long rows, int T, int Tt, const int* __restrict__ lens_f,
                                     const int* __restrict__ lens_t) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int b = (int)(row / T);
  if (row_dead(lens_f, row, T)) {   // ragged: a frame beyond its utterance's end is 0 and reads nothing
    reinterpret_cast<f32x4*>(out + row * H)[lane] = f32x4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  const long long ph = mel2ph[row];
  f32x4 e = {0.f, 0.f, 0.f, 0.f};
  if (ph > 0 && ph <= (lens_t ? lens_t[b] : Tt)) e = reinterpret_cast<const f32x4*>(enc + ((long long)b * Tt + (ph - 1)) * H)[lane];
  if (Espk) e = e + reinterpret_cast<const f32x4*>(Espk + spk_id[b] * H)[lane];       // (the plain front: no style row, possibly no speaker table)
  if (Estyle) e = e + reinterpret_cast<const f32x4*>(Estyle + style_id[b] * H)[lane];
  const float kp = ph > 0 ? 1.f : 0.f;
  e = e * kp;
  reinterpret_cast<f32x4*>(out + row * H)[lane] = e;
}

// The same per TOKEN: out[b,k] = what gather_frames_kernel writes for a frame with mel2ph = k, k = 0 .. Tt (row 0: the padding token) — the
// same expression in the same order, so that out[b, mel2ph[b,t]] equals decoder_inp[b,t] bit for bit
__global__ void token_rows_kernel(const float* __restrict__ enc, const long long* __restrict__ spk_id, const long long* __restrict__ style_id,
                                  const float* __restrict__ Espk, const float* __restrict__ Estyle, float* __restrict__ out, long long rows,
                                  int Tt) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int b = (int)(row / (Tt + 1));
  const long long ph = row - (long long)b * (Tt + 1);
  f32x4 e = {0.f, 0.f, 0.f, 0.f};
  if (ph > 0 && ph <= Tt) e = reinterpret_cast<const f32x4*>(enc + ((long long)b * Tt + (ph - 1)) * H)[lane];
  if (Espk) e = e + reinterpret_cast<const f32x4*>(Espk + spk_id[b] * H)[lane];
  if (Estyle) e = e + reinterpret_cast<const f32x4*>(Estyle + style_id[b] * H)[lane];
  const float kp = ph > 0 ? 1.f : 0.f;
  e = e * kp;
  reinterpret_cast<f32x4*>(out + row * H)[lane] = e;
}

// FFTBlocks entry for the decoder (tts_modules.py:289-297): padding = (sum |x| == 0), positions =
// cumsum(x[...,0] != 0) * (x[...,0] != 0) (utils/__init__.py:146-158), x = (x + alpha * table[pos]) * keep.
// One wave per utterance scans T in 64-frame chunks; then every lane copies rows.
__global__ void decoder_positions_kernel(const float* __restrict__ x, int* __restrict__ pos, float* __restrict__ keep, int T,
                                         const int* __restrict__ lens) {
  const int b = blockIdx.x, lane = threadIdx.x;   // 64 threads
  const int Tb = lens ? lens[b] : T;              // (ragged: the scan stops at the utterance's end)
  int carry = 0;
  for (int t0 = 0; t0 < Tb; t0 += 64) {
    const int t = t0 + lane;
    bool nz = false;
    if (t < Tb) nz = x[((long long)b * T + t) * H] != 0.f;
    const unsigned long long bal = __ballot(nz);
    const int pre = __popcll(bal & ((1ull << lane) - 1ull)) + (nz ? 1 : 0);
    if (t < Tb) pos[(long long)b * T + t] = nz ? carry + pre : 0;
    carry += __popcll(bal);
  }
  (void)keep;
}
__global__ void decoder_entry_kernel(float* __restrict__ x, const int* __restrict__ pos, const float* __restrict__ table,
                                     const float* __restrict__ alpha, float* __restrict__ keep, long long rows, int n_pos,
                                     const int* __restrict__ lens, int T) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  if (row_dead(lens, row, T)) {   // ragged: only the key mask is written beyond an utterance's end
    if (lane == 0) keep[row] = 0.f;
    return;
  }
  f32x4 v = reinterpret_cast<const f32x4*>(x + row * H)[lane];
  const float asum = wave_sum(fabsf(v[0]) + fabsf(v[1]) + fabsf(v[2]) + fabsf(v[3]));
  const float kp = asum == 0.f ? 0.f : 1.f;
  int p = pos[row];
  p = p < n_pos ? p : n_pos - 1;
  const f32x4 pe = reinterpret_cast<const f32x4*>(table + (long long)p * H)[lane];
  const float a = alpha[0];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(v[e], __fmul_rn(a, pe[e])) * kp;
  reinterpret_cast<f32x4*>(x + row * H)[lane] = v;
  if (lane == 0) keep[row] = kp;
}

// ---- duration predictor tail + length regulator --------------------------------------------------
// dur = clamp(round(exp(xs) - 1), min=0) with xs already masked                       (tts_modules.py:124-129)
__global__ void dur_from_log_kernel(float* __restrict__ xs, long long* __restrict__ dur, long long n, const int* __restrict__ lens, int Tt) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (row_dead(lens, i, Tt)) {   // ragged: no launch wrote xs beyond an utterance's end
    xs[i] = 0.f;
    dur[i] = 0;
    return;
  }
  const float d = rintf(expf(xs[i]) - 1.0f);
  dur[i] = d > 0.f ? (long long)d : 0;
}
// mel2ph[b,j] = sum_i i * [cum_{i-1} <= j < cum_i]  (tts_modules.py:178-190); one workgroup per utterance
__global__ void length_regulator_kernel(const long long* __restrict__ dur, const long long* __restrict__ txt,
                                        long long* __restrict__ mel2ph, int Tt, int T) {
  extern __shared__ long long cum[];
  const int b = blockIdx.x;
  if (threadIdx.x == 0) {
    long long c = 0;
    for (int i = 0; i < Tt; ++i) {
      long long d = dur[(long long)b * Tt + i];
      if (txt && txt[(long long)b * Tt + i] == 0) d = 0;
      c += d;
      cum[i] = c;
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < T; j += blockDim.x) {
    // first i with cum[i] > j
    int lo = 0, hi = Tt;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cum[mid] > j) hi = mid; else lo = mid + 1;
    }
    mel2ph[(long long)b * T + j] = lo < Tt ? lo + 1 : 0;
  }
}

// conv weight [M][Cin][k] -> [k][M][Cin]  (so each tap is a plain [N,K] operand of the GEMM)
__global__ void repack_conv_kernel(const float* __restrict__ w, float* __restrict__ out, int M, int Cin, int k) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)M * Cin * k;
  if (i >= total) return;
  const int c = (int)(i % Cin);
  const int m = (int)((i / Cin) % M);
  const int tap = (int)(i / ((long long)Cin * M));
  out[i] = w[((long long)m * Cin + c) * k + tap];
}

__global__ void mask_rows_by_index_kernel(float* __restrict__ x, const long long* __restrict__ idx, long long rows, int width,
                                          const int* __restrict__ lens, int T) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * width) return;
  if (row_dead(lens, i / width, T) || idx[i / width] <= 0) x[i] = 0.f;   // (ragged: idx is not read beyond an utterance's end)
}

// ---- plain FastSpeech2 front (FastspeechEncoder.forward_embedding, tts_modules.py:342-349) -------------------------------------------
// x = (sqrt(H) * E_tok[txt] + table[pos]) * keep with pos = the count of non-pad tokens up to and including this one (make_positions of the
// token ids, utils/__init__.py:146-158; pad id 0 -> row 0 of the table, which is zero) and keep = (txt != 0) (FFTBlocks :297).  One wave per
// token: it counts the non-pad tokens before it with ballots over 64-token pieces of its utterance (8-byte reads, T_txt is a few hundred).
__global__ void token_front_kernel(const long long* __restrict__ txt, const float* __restrict__ Etok, const float* __restrict__ table,
                                   float* __restrict__ x, float* __restrict__ keep, long long rows, int Tt, float scale, int n_pos, int vocab,
                                   const int* __restrict__ lens) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const long long b = row / Tt;
  const int j = (int)(row - b * Tt);
  if (lens && j >= lens[b]) {   // ragged: only the key mask is written beyond an utterance's end; its tokens are not read
    if (lane == 0) keep[row] = 0.f;
    return;
  }
  const long long* __restrict__ tb = txt + b * Tt;
  int cnt = 0;
  for (int t0 = 0; t0 <= j; t0 += 64) {
    const int t = t0 + lane;
    cnt += __popcll(__ballot(t <= j && tb[t] != 0));
  }
  long long tok = tb[j];
  const float kp = tok != 0 ? 1.f : 0.f;
  int p = tok != 0 ? cnt : 0;
  p = p < n_pos ? p : n_pos - 1;
  tok = tok < 0 ? 0 : tok < vocab ? tok : vocab - 1;   // an id outside the table is clamped (torch raises): no read out of bounds
  const f32x4 e = reinterpret_cast<const f32x4*>(Etok + tok * H)[lane];
  const f32x4 pv = reinterpret_cast<const f32x4*>(table + (long long)p * H)[lane];
  f32x4 o;
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = __fadd_rn(__fmul_rn(scale, e[c]), pv[c]) * kp;
  reinterpret_cast<f32x4*>(x + row * H)[lane] = o;
  if (lane == 0) keep[row] = kp;
}

// ---- frame-level pitch adaptor (FastSpeech2.add_pitch, fastspeech/fs2.py:201-234; PitchPredictor, tts_modules.py:224-237) -------------
// pitch_inp[b,t] = (pad(enc)[b, mel2ph[b,t]] + spk[b]) * (mel2ph > 0)  (fs2.py:139); its first channel decides the position (make_positions
// of xs[..., 0], tts_modules.py:230): one wave per utterance scans the frames in 64-frame pieces, as decoder_positions_kernel does.
// a speaker / style id outside its table is clamped (torch raises): the new kernels never read out of bounds
__device__ __forceinline__ long long clamp_id(long long i, int n) { return i < 0 ? 0 : i < n ? i : n - 1; }
__device__ __forceinline__ float pitch_inp0(const float* __restrict__ enc, const long long* __restrict__ mel2ph, const float* __restrict__ spk,
                                            long long b, long long row, int Tt, int ntok) {
  const long long ph = mel2ph[row];
  float e = 0.f;
  if (ph > 0 && ph <= ntok) e = enc[(b * Tt + (ph - 1)) * H];
  if (spk) e = e + spk[0];
  return e * (ph > 0 ? 1.f : 0.f);
}
__global__ void pitch_positions_kernel(const float* __restrict__ enc, const long long* __restrict__ mel2ph,
                                       const long long* __restrict__ spk_id, const float* __restrict__ Espk, int* __restrict__ pos, int T,
                                       int Tt, int spk_rows, const int* __restrict__ lens_f, const int* __restrict__ lens_t) {
  const int b = blockIdx.x, lane = threadIdx.x;   // 64 threads
  const float* spk = Espk ? Espk + clamp_id(spk_id[b], spk_rows) * H : nullptr;
  const int Tb = lens_f ? lens_f[b] : T, ntok = lens_t ? lens_t[b] : Tt;   // (ragged: the scan stops at the utterance's end)
  int carry = 0;
  for (int t0 = 0; t0 < Tb; t0 += 64) {
    const int t = t0 + lane;
    bool nz = false;
    if (t < Tb) nz = pitch_inp0(enc, mel2ph, spk, b, (long long)b * T + t, Tt, ntok) != 0.f;
    const unsigned long long bal = __ballot(nz);
    const int pre = __popcll(bal & ((1ull << lane) - 1ull)) + (nz ? 1 : 0);
    if (t < Tb) pos[(long long)b * T + t] = nz ? carry + pre : 0;
    carry += __popcll(bal);
  }
}
// x = pitch_inp + alpha * table[pos]: the predictor's input, one wave per frame.  Padded frames (pitch_inp == 0) take row 0 of the table (zero).
__global__ void pitch_entry_kernel(const float* __restrict__ enc, const long long* __restrict__ mel2ph, const long long* __restrict__ spk_id,
                                   const float* __restrict__ Espk, const int* __restrict__ pos, const float* __restrict__ table,
                                   const float* __restrict__ alpha, float* __restrict__ x, long long rows, int T, int Tt, int n_pos, int spk_rows,
                                   const int* __restrict__ lens_f, const int* __restrict__ lens_t) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows || row_dead(lens_f, row, T)) return;   // (ragged: the predictor reads a row up to its end only)
  const int lane = threadIdx.x & 63;
  const long long b = row / T;
  const long long ph = mel2ph[row];
  f32x4 e = {0.f, 0.f, 0.f, 0.f};
  if (ph > 0 && ph <= (lens_t ? lens_t[b] : Tt)) e = reinterpret_cast<const f32x4*>(enc + (b * Tt + (ph - 1)) * H)[lane];
  if (Espk) e = e + reinterpret_cast<const f32x4*>(Espk + clamp_id(spk_id[b], spk_rows) * H)[lane];
  e = e * (ph > 0 ? 1.f : 0.f);
  int p = pos[row];
  p = p < n_pos ? p : n_pos - 1;
  const f32x4 pe = reinterpret_cast<const f32x4*>(table + (long long)p * H)[lane];
  const float a = alpha[0];
#pragma unroll
  for (int c = 0; c < 4; ++c) e[c] = __fadd_rn(e[c], __fmul_rn(a, pe[c]));
  reinterpret_cast<f32x4*>(x + row * H)[lane] = e;
}

// f0_to_coarse (utils/pitch_utils.py:22-31) with the reference's fp32 operation order; a NaN (which the reference's own assert refuses) takes bin 1
__device__ __forceinline__ long long f0_coarse_bin(float f0) {
  const float mel_min = 77.75496616579426f;   // 1127 ln(1 + 50 / 700), rounded to fp32 as the reference's Python scalar is
  const float mel_span = 986.6532669978451f;  // 1127 ln(1 + 1100 / 700) - mel_min
  float m = __fmul_rn(1127.0f, logf(__fadd_rn(1.0f, __fdiv_rn(f0, 700.0f))));
  if (m > 0.f) m = __fadd_rn(__fdiv_rn(__fmul_rn(__fsub_rn(m, mel_min), 254.0f), mel_span), 1.0f);
  if (!(m > 1.0f)) m = 1.0f;
  if (m > 255.0f) m = 255.0f;
  return (long long)__fadd_rn(m, 0.5f);
}

// The adaptor's frame-level tail, one wave per frame (4 channels per lane):
//   the LAST predictor layer's LayerNorm (eps 1e-12) of the ReLU-ed convolution `c`, Linear(256 -> 2) as two shuffle-reduced dots -> pitch_pred;
//   f0 = supplied or pred[0], uv = supplied or pred[1] > 0 (use_uv);  f0_denorm = 2^f0, 0 where uv or padded;  bin = f0_to_coarse(f0_denorm);
//   decoder_inp = (((pad(enc)[mel2ph] + pitch_embed[bin]) + spk) + style) * (mel2ph > 0)                              (fs2.py:142-146, midi :181-189)
// pitch_pred, f0_denorm and bins may each be NULL.
__global__ void pitch_tail_kernel(const float* __restrict__ c, const float* __restrict__ lnw, const float* __restrict__ lnb,
                                  const float* __restrict__ lin_w, const float* __restrict__ lin_b, const float* __restrict__ f0_in,
                                  const float* __restrict__ uv_in, int use_uv, const float* __restrict__ enc,
                                  const long long* __restrict__ mel2ph, const long long* __restrict__ spk_id,
                                  const long long* __restrict__ style_id, const float* __restrict__ Espk, const float* __restrict__ Estyle,
                                  const float* __restrict__ Epitch, float* __restrict__ pitch_pred, float* __restrict__ f0_denorm,
                                  long long* __restrict__ bins, float* __restrict__ out, long long rows, int T, int Tt, int spk_rows,
                                  const int* __restrict__ lens_f, const int* __restrict__ lens_t) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const long long b = row / T;
  if (row_dead(lens_f, row, T)) {   // ragged: beyond an utterance's end nothing is read; floats are 0, the bin is f0_to_coarse(0) = 1
    if (lane == 0) {
      if (pitch_pred) { pitch_pred[2 * row] = 0.f; pitch_pred[2 * row + 1] = 0.f; }
      if (f0_denorm) f0_denorm[row] = 0.f;
      if (bins) bins[row] = 1;
    }
    reinterpret_cast<f32x4*>(out + row * H)[lane] = f32x4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  const f32x4 v = reinterpret_cast<const f32x4*>(c + row * H)[lane];
  const float mean = wave_sum(v[0] + v[1] + v[2] + v[3]) * (1.0f / H);
  const float d0 = v[0] - mean, d1 = v[1] - mean, d2 = v[2] - mean, d3 = v[3] - mean;
  const float var = wave_sum(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3) * (1.0f / H);
  const float rstd = 1.0f / sqrtf(var + 1e-12f);
  const f32x4 wv = reinterpret_cast<const f32x4*>(lnw)[lane], bv = reinterpret_cast<const f32x4*>(lnb)[lane];
  const f32x4 y = {d0 * rstd * wv[0] + bv[0], d1 * rstd * wv[1] + bv[1], d2 * rstd * wv[2] + bv[2], d3 * rstd * wv[3] + bv[3]};
  const f32x4 w0 = reinterpret_cast<const f32x4*>(lin_w)[lane], w1 = reinterpret_cast<const f32x4*>(lin_w + H)[lane];
  const float p0 = wave_sum(y[0] * w0[0] + y[1] * w0[1] + y[2] * w0[2] + y[3] * w0[3]) + lin_b[0];
  const float p1 = wave_sum(y[0] * w1[0] + y[1] * w1[1] + y[2] * w1[2] + y[3] * w1[3]) + lin_b[1];
  const long long ph = mel2ph[row];
  const float f0 = f0_in ? f0_in[row] : p0;
  const bool unvoiced = use_uv && (uv_in ? uv_in[row] > 0.f : p1 > 0.f);
  float fd = exp2f(f0);
  if (unvoiced || ph == 0) fd = 0.f;
  const long long bin = f0_coarse_bin(fd);
  if (lane == 0) {
    // (the reference's f0[pitch_padding] = 0, fs2.py:230, writes through its view of pitch_pred when f0 is the predicted one: the
    // returned pitch_pred[..., 0] is 0 on padded frames then, and untouched with a supplied f0)
    if (pitch_pred) { pitch_pred[2 * row] = (!f0_in && ph == 0) ? 0.f : p0; pitch_pred[2 * row + 1] = p1; }
    if (f0_denorm) f0_denorm[row] = fd;
    if (bins) bins[row] = bin;
  }
  f32x4 e = {0.f, 0.f, 0.f, 0.f};
  if (ph > 0 && ph <= (lens_t ? lens_t[b] : Tt)) e = reinterpret_cast<const f32x4*>(enc + (b * Tt + (ph - 1)) * H)[lane];
  e = e + reinterpret_cast<const f32x4*>(Epitch + bin * H)[lane];
  if (Espk) e = e + reinterpret_cast<const f32x4*>(Espk + clamp_id(spk_id[b], spk_rows) * H)[lane];
  if (Estyle) e = e + reinterpret_cast<const f32x4*>(Estyle + clamp_id(style_id[b], STYLE_ROWS) * H)[lane];
  e = e * (ph > 0 ? 1.f : 0.f);
  reinterpret_cast<f32x4*>(out + row * H)[lane] = e;
}

}  // namespace
}  // namespace bsg

// ================================================================================================
using namespace bsg;

#define TRY(expr)                  \
  do {                             \
    int _rc = (expr);              \
    if (_rc != BSG_OK) return _rc; \
  } while (0)

struct FftLayerW {
  float *ln1w, *ln1b, *in_proj, *out_proj, *ln2w, *ln2b, *ffn1 /*[k][4H][H]*/, *ffn1b, *ffn2, *ffn2b;
  H2wWeights p_in, p_out, p_ffn1, p_ffn2;   // the four weight matrices once more as pre-split fp16 fragments (gemm_h2w.hip)
};

struct bsg_fs2midi {
  bsg_fs2midi_cfg cfg;
  Guard guard;   // this handle's range-event word and split-fp16 GEMM switch
  DevOwned owned;
  // weights
  float *Etok, *dec_alpha, *dec_lnw, *dec_lnb, *mel_w, *mel_b, *Espk, *dur_lin_w, *dur_lin_b;
  std::vector<FftLayerW> enc, dec;
  std::vector<float*> dur_conv, dur_convb, dur_lnw, dur_lnb;
  float *esm_in_w, *esm_in_b, *esm_out_w, *esm_out_b, *esm_f0w, *esm_f0b, *esm_f2w, *esm_f2b, *esm_ln1w, *esm_ln1b, *esm_ln2w, *esm_ln2b;
  H2wWeights p_esm_q, p_esm_kv, p_esm_out, p_esm_f0, p_esm_f2;   // the ESM's Linear layers as pre-split fragments (K and V projections as one product)
  float *enc_lnw, *enc_lnb, *Emidi, *Wdur, *bdur, *Eslur, *Elang, *Estyle;
  float *dec_table, *rel_table;   // rel_table: the token-level position table (plain front: the sinusoidal table the tokens index)
  // bsg_fs2_create (ABI v16): the front and the frame-level pitch adaptor; bsg_fs2midi_create leaves the defaults
  int front = BSG_FS2_FRONT_MIDI;
  int use_pitch = 0, pitch_layers = 0, pitch_kernel = 0, use_uv = 0, n_pitch_pos = 0;
  float *Epitch = nullptr, *pit_alpha = nullptr, *pit_lin_w = nullptr, *pit_lin_b = nullptr, *pit_table = nullptr;
  std::vector<float*> pit_conv, pit_convb, pit_lnw, pit_lnb;
  // workspace
  size_t cap_rows = 0, cap_scores = 0;
  float *w_x = nullptr, *w_a = nullptr, *w_b = nullptr, *w_qkv = nullptr, *w_ffn = nullptr, *w_keep = nullptr, *w_scores = nullptr;
  float *w_c = nullptr;
  int* w_pos = nullptr;
  unsigned short *w_ap = nullptr, *w_fp = nullptr;   // activation planes [2][rows][H] / [2][rows][4H] fp16 (operands of gemm_h2w_kernel)
  float* w_fsk = nullptr;                            // key-split partials of flash_attn_planes_kernel (small batches) and their arrival counters
  unsigned* w_fcnt = nullptr;
  size_t cap_fsk = 0, cap_fcnt = 0;
  unsigned* pack_bad = nullptr;                      // device word: packed weights beyond the fp16 range (then the pre-split GEMMs are not used)
  bool h2w_ok = false;
  bool planes_lds = false;                           // this handle's device grants flash_attn_planes_kernel<2> its FLP_LDS (asked at create)
  int *w_lens_t = nullptr, *w_lens_f = nullptr;      // ragged calls: the utterances' token and frame counts on the device, filled by the call itself (lens_fill)
  size_t cap_lens = 0;
  float* esm_scr = nullptr;                          // MIDI front: [6][2][H] scratch of the two-row ESM table of the ragged encode (esm_alone_table)
  int last_token_rows = 0;   // rows (utterances x tokens) the last encode ran its encoder on; rows of the last FFT stack (bsg_fs2midi_last_rows)
  int last_stack_rows = 0;
  std::string path;          // the launch forms of the last encode and of the decode after it (bsg_fs2midi_last_path, bsg_fftden_last_path)
  size_t path_enc_len = 0;   // where the encode's tokens end: a decode replaces what follows
};

// One token per launch FORM, appended at the branch that launched (never derived from the thresholds again): "<stack>.<site>:<form>", in
// launch order; a form that a stack launches again (every layer, as a rule) is named once.
static void path_add(bsg_fs2midi* h, const char* tag, const char* tok) {
  const std::string full = std::string(tag) + tok;
  if ((" " + h->path + " ").find(" " + full + " ") != std::string::npos) return;
  if (!h->path.empty()) h->path += ' ';
  h->path += full;
}

static int fs2_copy(bsg_fs2midi* h, float** dst, const void* src, size_t n, hipStream_t st) {
  TRY(own_alloc(h->owned, dst, n));
  BSG_HIP(hipMemcpyAsync(*dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st));
  return BSG_OK;
}
static int fs2_conv(bsg_fs2midi* h, float** dst, const void* src, int M, int Cin, int k, hipStream_t st) {
  TRY(own_alloc(h->owned, dst, (size_t)M * Cin * k));
  const long long total = (long long)M * Cin * k;
  hipLaunchKernelGGL(repack_conv_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, (const float*)src, *dst, M, Cin, k);
  BSG_LAUNCH_CHECK();
  return BSG_OK;
}

// The handle's shape-sized workspaces (bsg_ws.h): destroy, grow() and the poison hook all walk this one table.  cap_rows: token / frame rows.
// What depends on the attention form has capacities of its own, sized from the plan (launch_fft): the key-split partials, their arrival
// counters (zeroed when (re)allocated: the kernel leaves every counter at zero; never poisoned: they must stay zero between launches) and
// the score tensor.  The position words are not poisoned either.
static std::vector<WsBuf> ws_table(bsg_fs2midi* h) {
  const size_t f = sizeof(float), s = sizeof(unsigned short);
  return {
      {&h->cap_rows, (void**)&h->w_x, H * f, 0, WS_POISON},       {&h->cap_rows, (void**)&h->w_a, H * f, 0, WS_POISON},
      {&h->cap_rows, (void**)&h->w_b, H * f, 0, WS_POISON},       {&h->cap_rows, (void**)&h->w_c, H * f, 0, WS_POISON},
      {&h->cap_rows, (void**)&h->w_qkv, 3 * H * f, 0, WS_POISON}, {&h->cap_rows, (void**)&h->w_ffn, 4 * H * f, 0, WS_POISON},
      {&h->cap_rows, (void**)&h->w_keep, f, 0, WS_POISON},        {&h->cap_rows, (void**)&h->w_pos, sizeof(int)},
      {&h->cap_rows, (void**)&h->w_ap, 2 * H * s, 0, WS_POISON},  {&h->cap_rows, (void**)&h->w_fp, 2 * 4 * H * s, 0, WS_POISON},
      {&h->cap_scores, (void**)&h->w_scores, f, 0, WS_POISON},
      {&h->cap_fsk, (void**)&h->w_fsk, f, 0, WS_POISON},
      {&h->cap_fcnt, (void**)&h->w_fcnt, sizeof(unsigned), 0, WS_ZERO},
      {&h->cap_lens, (void**)&h->w_lens_t, sizeof(int)},          {&h->cap_lens, (void**)&h->w_lens_f, sizeof(int)},
  };
}
// (the capacity test comes first, so that a call that grows nothing builds no table)
static int grow(bsg_fs2midi* h, size_t* cap, size_t need, hipStream_t st) {
  return need <= *cap ? BSG_OK : ws_grow(ws_table(h), "fs2", cap, need, st);
}

extern "C" void bsg_fs2midi_destroy(bsg_fs2midi* h) {
  if (!h) return;
  guard_free(&h->guard);
  h->owned.free_all();
  ws_free(ws_table(h));
  if (h->pack_bad) (void)hipFree(h->pack_bad);
  for (std::vector<FftLayerW>* v : {&h->enc, &h->dec})
    for (FftLayerW& L : *v) { h2w_free(&L.p_in); h2w_free(&L.p_out); h2w_free(&L.p_ffn1); h2w_free(&L.p_ffn2); }
  for (H2wWeights* p : {&h->p_esm_q, &h->p_esm_kv, &h->p_esm_out, &h->p_esm_f0, &h->p_esm_f2}) h2w_free(p);
  delete h;
}

static int load_fft_layers(bsg_fs2midi* h, std::vector<FftLayerW>& out, const void* const* w, int n_layers, int ksz, hipStream_t st) {
  out.resize(n_layers);
  if (!h->pack_bad) {
    BSG_HIP(hipMalloc((void**)&h->pack_bad, sizeof(unsigned)));
    BSG_HIP(hipMemsetAsync(h->pack_bad, 0, sizeof(unsigned), st));
  }
  for (int i = 0; i < n_layers; ++i) {
    const void* const* lw = w + 10 * i;
    FftLayerW& L = out[i];
    TRY(fs2_copy(h, &L.ln1w, lw[0], H, st));
    TRY(fs2_copy(h, &L.ln1b, lw[1], H, st));
    TRY(fs2_copy(h, &L.in_proj, lw[2], (size_t)3 * H * H, st));
    TRY(fs2_copy(h, &L.out_proj, lw[3], (size_t)H * H, st));
    TRY(fs2_copy(h, &L.ln2w, lw[4], H, st));
    TRY(fs2_copy(h, &L.ln2b, lw[5], H, st));
    TRY(fs2_conv(h, &L.ffn1, lw[6], 4 * H, H, ksz, st));
    TRY(fs2_copy(h, &L.ffn1b, lw[7], 4 * H, st));
    TRY(fs2_copy(h, &L.ffn2, lw[8], (size_t)H * 4 * H, st));
    TRY(fs2_copy(h, &L.ffn2b, lw[9], H, st));
    // pre-split fragments: Linear weights [N][K]; the conv from its original [4H][H][k] layout (tap stride 1, k stride `ksz`)
    TRY(h2w_pack(&L.p_in, (const float*)lw[2], 3 * H, H, 1, 0, H, 1, h->pack_bad, st));
    TRY(h2w_pack(&L.p_out, (const float*)lw[3], H, H, 1, 0, H, 1, h->pack_bad, st));
    if (ksz <= 17) TRY(h2w_pack(&L.p_ffn1, (const float*)lw[6], 4 * H, H, ksz, 1, (long long)H * ksz, ksz, h->pack_bad, st));
    TRY(h2w_pack(&L.p_ffn2, (const float*)lw[8], H, 4 * H, 1, 0, 4 * H, 1, h->pack_bad, st));
  }
  return BSG_OK;
}

// pitch_embed.weight, pitch_predictor.{pos_embed_alpha, conv.l.1.{weight,bias}, conv.l.3.{weight,bias}, linear.{weight,bias},
// embed_positions._float_tensor}  (fastspeech/fs2.py:55-81, tts_modules.py:194-222)
static int load_pitch(bsg_fs2midi* h, const void* const* w, int& i, hipStream_t st) {
  const int L = h->pitch_layers;
  TRY(fs2_copy(h, &h->Epitch, w[i++], (size_t)300 * H, st));
  TRY(fs2_copy(h, &h->pit_alpha, w[i++], 1, st));
  h->pit_conv.resize(L); h->pit_convb.resize(L); h->pit_lnw.resize(L); h->pit_lnb.resize(L);
  for (int l = 0; l < L; ++l) {
    TRY(fs2_conv(h, &h->pit_conv[l], w[i++], H, H, h->pitch_kernel, st));
    TRY(fs2_copy(h, &h->pit_convb[l], w[i++], H, st));
    TRY(fs2_copy(h, &h->pit_lnw[l], w[i++], H, st));
    TRY(fs2_copy(h, &h->pit_lnb[l], w[i++], H, st));
  }
  TRY(fs2_copy(h, &h->pit_lin_w, w[i++], (size_t)2 * H, st));
  TRY(fs2_copy(h, &h->pit_lin_b, w[i++], 2, st));
  i++;  // pitch_predictor.embed_positions._float_tensor: placeholder buffer of the reference
  return BSG_OK;
}

static int load_dur(bsg_fs2midi* h, const void* const* w, int& i, hipStream_t st) {
  const bsg_fs2midi_cfg& c = h->cfg;
  h->dur_conv.resize(c.dur_layers); h->dur_convb.resize(c.dur_layers); h->dur_lnw.resize(c.dur_layers); h->dur_lnb.resize(c.dur_layers);
  for (int l = 0; l < c.dur_layers; ++l) {
    TRY(fs2_conv(h, &h->dur_conv[l], w[i++], H, H, c.dur_kernel, st));
    TRY(fs2_copy(h, &h->dur_convb[l], w[i++], H, st));
    TRY(fs2_copy(h, &h->dur_lnw[l], w[i++], H, st));
    TRY(fs2_copy(h, &h->dur_lnb[l], w[i++], H, st));
  }
  TRY(fs2_copy(h, &h->dur_lin_w, w[i++], H, st));
  TRY(fs2_copy(h, &h->dur_lin_b, w[i++], 1, st));
  return BSG_OK;
}

// decoder.*, mel_out, [spk_embed_proj], dur_predictor, [pitch_embed, pitch_predictor]: one run of tensors in the state_dict() of both fronts
static int load_decoder(bsg_fs2midi* h, const void* const* w, int& i, hipStream_t st) {
  const bsg_fs2midi_cfg& c = h->cfg;
  TRY(fs2_copy(h, &h->dec_alpha, w[i++], 1, st));
  i++;  // decoder.embed_positions._float_tensor: placeholder buffer of the reference, no meaning
  TRY(load_fft_layers(h, h->dec, w + i, c.dec_layers, c.dec_ffn_kernel_size, st));
  i += 10 * c.dec_layers;
  TRY(fs2_copy(h, &h->dec_lnw, w[i++], H, st));
  TRY(fs2_copy(h, &h->dec_lnb, w[i++], H, st));
  TRY(fs2_copy(h, &h->mel_w, w[i++], (size_t)c.out_dims * H, st));
  TRY(fs2_copy(h, &h->mel_b, w[i++], c.out_dims, st));
  if (c.spk_rows > 0) TRY(fs2_copy(h, &h->Espk, w[i++], (size_t)c.spk_rows * H, st));
  TRY(load_dur(h, w, i, st));
  if (h->use_pitch) TRY(load_pitch(h, w, i, st));
  return BSG_OK;
}

// The end of every create: the position tables (tok_table: none for the FFT denoiser), the read-back of the packing (h2w_ok), and the
// question whether this handle's device grants the planes attention its LDS (a refusal is no error: no planes attention on this handle)
static int create_tail(bsg_fs2midi* h, const float* dec_table, const float* tok_table, const float* pitch_table, hipStream_t st) {
  const bsg_fs2midi_cfg& c = h->cfg;
  TRY(fs2_copy(h, &h->dec_table, dec_table, (size_t)c.n_pos * H, st));
  if (tok_table) TRY(fs2_copy(h, &h->rel_table, tok_table, (size_t)c.n_rel * H, st));
  if (h->use_pitch) TRY(fs2_copy(h, &h->pit_table, pitch_table, (size_t)h->n_pitch_pos * H, st));
  unsigned bad = 0;
  BSG_HIP(hipMemcpyAsync(&bad, h->pack_bad, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  BSG_HIP(hipStreamSynchronize(st));
  h->h2w_ok = bad == 0 && c.enc_ffn_kernel_size <= 17 && c.dec_ffn_kernel_size <= 17;
  h->planes_lds = hipFuncSetAttribute(reinterpret_cast<const void*>(flash_attn_planes_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, FLP_LDS) == hipSuccess;
  if (!h->planes_lds) (void)hipGetLastError();
  return BSG_OK;
}

// The plain FastSpeech2 (fastspeech/fs2.py:24-89) in state_dict() order: encoder_embed_tokens, encoder.{layers, layer_norm, embed_tokens
// (alias), embed_positions._float_tensor}, decoder.{pos_embed_alpha, embed_positions._float_tensor, layers, layer_norm}, mel_out,
// [spk_embed_proj], dur_predictor, [pitch_embed, pitch_predictor]
static int fs2_create_plain(bsg_fs2midi* h, const void* const* w, const float* dec_table, const float* tok_table, const float* pitch_table,
                            hipStream_t st) {
  const bsg_fs2midi_cfg& c = h->cfg;
  int i = 0;
  TRY(fs2_copy(h, &h->Etok, w[i++], (size_t)c.vocab * H, st));
  TRY(load_fft_layers(h, h->enc, w + i, c.enc_layers, c.enc_ffn_kernel_size, st));
  i += 10 * c.enc_layers;
  TRY(fs2_copy(h, &h->enc_lnw, w[i++], H, st));
  TRY(fs2_copy(h, &h->enc_lnb, w[i++], H, st));
  i += 2;  // encoder.embed_tokens (alias of encoder_embed_tokens), encoder.embed_positions._float_tensor
  TRY(load_decoder(h, w, i, st));
  return create_tail(h, dec_table, tok_table, pitch_table, st);
}

static int fs2_create_impl(bsg_fs2midi* h, const void* const* w, const float* dec_table, const float* rel_table, const float* pitch_table,
                           hipStream_t st) {
  const bsg_fs2midi_cfg& c = h->cfg;
  int i = 0;
  TRY(fs2_copy(h, &h->Etok, w[i++], (size_t)c.vocab * H, st));
  TRY(load_decoder(h, w, i, st));
  TRY(fs2_copy(h, &h->esm_in_w, w[i++], (size_t)3 * H * H, st));
  TRY(fs2_copy(h, &h->esm_in_b, w[i++], 3 * H, st));
  TRY(fs2_copy(h, &h->esm_out_w, w[i++], (size_t)H * H, st));
  TRY(fs2_copy(h, &h->esm_out_b, w[i++], H, st));
  TRY(fs2_copy(h, &h->esm_f0w, w[i++], (size_t)H * H, st));
  TRY(fs2_copy(h, &h->esm_f0b, w[i++], H, st));
  TRY(fs2_copy(h, &h->esm_f2w, w[i++], (size_t)H * H, st));
  TRY(fs2_copy(h, &h->esm_f2b, w[i++], H, st));
  TRY(fs2_copy(h, &h->esm_ln1w, w[i++], H, st));
  TRY(fs2_copy(h, &h->esm_ln1b, w[i++], H, st));
  TRY(fs2_copy(h, &h->esm_ln2w, w[i++], H, st));
  TRY(fs2_copy(h, &h->esm_ln2b, w[i++], H, st));
  TRY(h2w_pack(&h->p_esm_q, h->esm_in_w, H, H, 1, 0, H, 1, h->pack_bad, st));
  TRY(h2w_pack(&h->p_esm_kv, h->esm_in_w + (size_t)H * H, 2 * H, H, 1, 0, H, 1, h->pack_bad, st));
  TRY(h2w_pack(&h->p_esm_out, h->esm_out_w, H, H, 1, 0, H, 1, h->pack_bad, st));
  TRY(h2w_pack(&h->p_esm_f0, h->esm_f0w, H, H, 1, 0, H, 1, h->pack_bad, st));
  TRY(h2w_pack(&h->p_esm_f2, h->esm_f2w, H, H, 1, 0, H, 1, h->pack_bad, st));
  TRY(load_fft_layers(h, h->enc, w + i, c.enc_layers, c.enc_ffn_kernel_size, st));
  i += 10 * c.enc_layers;
  TRY(fs2_copy(h, &h->enc_lnw, w[i++], H, st));
  TRY(fs2_copy(h, &h->enc_lnb, w[i++], H, st));
  i += 1 + 12;  // encoder.embed_tokens / encoder.esm.*: aliases of encoder_embed_tokens / esm.* (fs2.py:84-87)
  TRY(fs2_copy(h, &h->Emidi, w[i++], (size_t)MIDI_ROWS * H, st));
  TRY(fs2_copy(h, &h->Wdur, w[i++], H, st));
  TRY(fs2_copy(h, &h->bdur, w[i++], H, st));
  TRY(fs2_copy(h, &h->Eslur, w[i++], (size_t)SLUR_ROWS * H, st));
  TRY(fs2_copy(h, &h->Elang, w[i++], (size_t)LANG_ROWS * H, st));
  TRY(fs2_copy(h, &h->Estyle, w[i++], (size_t)STYLE_ROWS * H, st));
  TRY(own_alloc(h->owned, &h->esm_scr, (size_t)6 * 2 * H));
  return create_tail(h, dec_table, rel_table, pitch_table, st);
}

extern "C" int bsg_fs2midi_n_weights(const bsg_fs2midi_cfg* c) {
  return 3 + 10 * c->dec_layers + 2 + 2 + 1 + 4 * c->dur_layers + 2 + 12 + 10 * c->enc_layers + 2 + 1 + 12 + 6;
}

// every refusal of bsg_fs2_create / bsg_fs2midi_create / bsg_fs2_n_weights, before any device call
static int fs2_cfg_check(const bsg_fs2_cfg* cfg, const char* who) {
  BSG_REQUIRE(cfg, "%s: null config", who);
  const bsg_fs2midi_cfg& b = cfg->base;
  BSG_REQUIRE(cfg->front == BSG_FS2_FRONT_MIDI || cfg->front == BSG_FS2_FRONT_PLAIN, "%s: front=%d (0 = MIDI + ESM, 1 = plain)", who, cfg->front);
  BSG_REQUIRE(b.hidden_size == H, "%s: hidden_size=%d; kernels are built for 256", who, b.hidden_size);
  BSG_REQUIRE(b.num_heads > 0 && H % b.num_heads == 0 && (H / b.num_heads) % 4 == 0, "%s: num_heads=%d", who, b.num_heads);
  BSG_REQUIRE(cfg->front == BSG_FS2_FRONT_PLAIN || b.esm_heads == 8, "%s: esm_heads=%d (the reference fixes 8, fs2.py:83)", who, b.esm_heads);
  BSG_REQUIRE(b.enc_layers > 0 && b.dec_layers > 0 && b.dur_layers > 0 && b.vocab > 0 && b.out_dims > 0 && b.out_dims % 4 == 0 && b.n_pos > 1 &&
                  b.n_rel > 0,
              "%s: bad config", who);
  BSG_REQUIRE(cfg->front == BSG_FS2_FRONT_PLAIN ? b.spk_rows >= 0 : b.spk_rows > 0, "%s: spk_rows=%d (0 = no speaker table: the plain front only)",
              who, b.spk_rows);
  BSG_REQUIRE(b.enc_ffn_kernel_size % 2 == 1 && b.dec_ffn_kernel_size % 2 == 1 && b.dur_kernel % 2 == 1, "%s: SAME padding needs odd kernels", who);
  BSG_REQUIRE(cfg->use_pitch_embed == 0 || cfg->use_pitch_embed == 1, "%s: use_pitch_embed=%d", who, cfg->use_pitch_embed);
  if (cfg->use_pitch_embed) {
    BSG_REQUIRE(cfg->pitch_layers > 0 && cfg->pitch_layers <= 16, "%s: pitch_layers=%d (1 .. 16)", who, cfg->pitch_layers);
    BSG_REQUIRE(cfg->pitch_kernel > 0 && cfg->pitch_kernel % 2 == 1 && cfg->pitch_kernel <= 31, "%s: pitch_kernel=%d (odd, at most 31: SAME padding)",
                who, cfg->pitch_kernel);
    BSG_REQUIRE(cfg->use_uv == 0 || cfg->use_uv == 1, "%s: use_uv=%d", who, cfg->use_uv);
    BSG_REQUIRE(cfg->n_pitch_pos > 1, "%s: n_pitch_pos=%d rows of the pitch position table", who, cfg->n_pitch_pos);
  }
  return BSG_OK;
}

extern "C" int bsg_fs2_n_weights(const bsg_fs2_cfg* cfg) {
  TRY(fs2_cfg_check(cfg, "fs2_n_weights"));
  const bsg_fs2midi_cfg& b = cfg->base;
  const int pitch = cfg->use_pitch_embed ? 1 + 1 + 4 * cfg->pitch_layers + 2 + 1 : 0;
  if (cfg->front == BSG_FS2_FRONT_MIDI) return bsg_fs2midi_n_weights(&b) + pitch;
  return 1 + 10 * b.enc_layers + 2 + 2 + 2 + 10 * b.dec_layers + 2 + 2 + (b.spk_rows > 0 ? 1 : 0) + 4 * b.dur_layers + 2 + pitch;
}

// the body of both create entries; `who` keeps each entry's messages under its own name
static int fs2_create(const char* who, bsg_fs2midi** out, const bsg_fs2_cfg* cfg, const void* const* dev_weights, int32_t n_weights,
                      const float* dec_pos_table, const float* tok_pos_table, const float* pitch_pos_table, hipStream_t st) {
  TRY(fs2_cfg_check(cfg, who));
  BSG_REQUIRE(out && dev_weights && dec_pos_table && tok_pos_table, "%s: null argument", who);
  BSG_REQUIRE(!cfg->use_pitch_embed || pitch_pos_table, "%s: use_pitch_embed without a pitch position table", who);
  const int want = bsg_fs2_n_weights(cfg);
  BSG_REQUIRE(n_weights == want, "%s: expected %d weight tensors, got %d", who, want, n_weights);
  for (int i = 0; i < n_weights; ++i) BSG_REQUIRE(dev_weights[i] != nullptr, "%s: weight %d is null", who, i);
  bsg_fs2midi* h = new bsg_fs2midi();
  h->cfg = cfg->base;
  h->front = cfg->front;
  h->use_pitch = cfg->use_pitch_embed;
  if (h->use_pitch) { h->pitch_layers = cfg->pitch_layers; h->pitch_kernel = cfg->pitch_kernel; h->use_uv = cfg->use_uv; h->n_pitch_pos = cfg->n_pitch_pos; }
  int rc = guard_init(&h->guard, st);
  if (rc == BSG_OK)
    rc = (h->front == BSG_FS2_FRONT_MIDI ? fs2_create_impl : fs2_create_plain)(h, dev_weights, dec_pos_table, tok_pos_table, pitch_pos_table, st);
  if (rc != BSG_OK) {
    bsg_fs2midi_destroy(h);
    return rc;
  }
  *out = h;
  return BSG_OK;
}

extern "C" int bsg_fs2_create(bsg_fs2midi** out, const bsg_fs2_cfg* cfg, const void* const* dev_weights, int32_t n_weights,
                              const float* dec_pos_table, const float* tok_pos_table, const float* pitch_pos_table, void* stream) {
  return fs2_create("fs2_create", out, cfg, dev_weights, n_weights, dec_pos_table, tok_pos_table, pitch_pos_table, (hipStream_t)stream);
}

// the extended configuration of the older entry: MIDI front, no pitch embedding
extern "C" int bsg_fs2midi_create(bsg_fs2midi** out, const bsg_fs2midi_cfg* cfg, const void* const* dev_weights,
                                  int32_t n_weights, const float* dec_pos_table, const float* rel_pos_table, void* stream) {
  BSG_REQUIRE(cfg, "fs2midi_create: null argument");
  const bsg_fs2_cfg x{*cfg, BSG_FS2_FRONT_MIDI};
  return fs2_create("fs2midi_create", out, &x, dev_weights, n_weights, dec_pos_table, rel_pos_table, nullptr, (hipStream_t)stream);
}

// launch_gemm / launch_gemm_h2w; with `rec`, the form it picked is added to that handle's launch record under `tag`
template <class Args>
static int launch_rec(int (*launch)(const Args&, hipStream_t), bsg_fs2midi* rec, const char* tag, Args& g, hipStream_t st) {
  const char* form = nullptr;
  g.form_out = rec ? &form : nullptr;
  const int rc = launch(g, st);
  if (form) path_add(rec, tag, form);
  return rc;
}
static int gemm_rec(bsg_fs2midi* rec, const char* tag, GemmArgs& g, hipStream_t st) { return launch_rec(launch_gemm, rec, tag, g, st); }
static int h2w_rec(bsg_fs2midi* rec, const char* tag, H2wArgs& g, hipStream_t st) { return launch_rec(launch_gemm_h2w, rec, tag, g, st); }
// a token its stack names once, after the first launch it names (the QKV producer, the attention form): appended, never searched for
static void path_name(bsg_fs2midi* h, bool first, const char* stack, const char* site, const char* form) {
  if (!first) return;   // (the later layers of a stack launch the plan's same forms)
  if (!h->path.empty()) h->path += ' ';
  h->path.append(stack).append(site).append(form);
}

// lens / T (ragged calls): the batched form (M = T, batch = rows / T) bounded per utterance by GemmArgs::lens — rows at or beyond an
// utterance's end are neither read nor written, and a tile beyond it returns before its first load
static int linear(const float* X, const float* W, const float* bias, float* Y, long long rows, int N, int K, int act,
                  const float* R, const float* rowscale, hipStream_t st, float alpha = 1.f, int alpha_ncols = 0,
                  bsg_fs2midi* rec = nullptr, const char* tag = "", const int* lens = nullptr, int T = 0) {
  GemmArgs g{};
  g.A = X; g.B = W; g.C = Y; g.M = (int)rows; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N; g.trans_b = 1; g.taps = 1;
  g.bias_n = bias; g.alpha = alpha; g.alpha_ncols = alpha_ncols; g.act = act; g.R = R; g.ldr = N; g.rowscale = rowscale; g.batch = 1;
  if (lens) {
    g.M = T; g.batch = (int)(rows / T); g.sA = (long long)T * K; g.sC = (long long)T * N; g.sR = (long long)T * N; g.sRS = T; g.lens = lens;
  }
  return gemm_rec(rec, tag, g, st);
}

// lens / T (ragged calls; null = padded): rows at or beyond their utterance's end are not read, y is 0 there
static int ln(const float* x, const float* w, const float* b, float* y, const float* rowscale, long long rows, float eps, hipStream_t st,
              const int* lens = nullptr, int T = 0) {
  hipLaunchKernelGGL(layernorm_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, x, w, b, y, rowscale, rows, eps, (_Float16*)nullptr,
                     (_Float16*)nullptr, (unsigned*)nullptr, lens, T);
  BSG_LAUNCH_CHECK();
  return BSG_OK;
}
// LayerNorm whose result is read by a pre-split GEMM only: hi / lo fp16 planes [2][rows][H]
static int ln_planes(const float* x, const float* w, const float* b, unsigned short* planes, long long rows, float eps, hipStream_t st,
                     const int* lens = nullptr, int T = 0) {
  hipLaunchKernelGGL(layernorm_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, x, w, b, (float*)nullptr, (const float*)nullptr, rows, eps,
                     reinterpret_cast<_Float16*>(planes), reinterpret_cast<_Float16*>(planes) + rows * H, gemm_range_counter(), lens, T);
  BSG_LAUNCH_CHECK();
  return BSG_OK;
}
// y[rows][N] = epi(planes[rows][K] W^T): Linear through gemm_h2w_kernel (W pre-split); `planes_out`: the result as planes [2][rows][N] instead
static int linear_h2w(bsg_fs2midi* rec, const char* tag, const unsigned short* planes, const H2wWeights& W, int N, const float* bias, float* Y, unsigned short* planes_out, long long rows,
                      int act, const float* R, const float* rowscale, hipStream_t st, float alpha = 1.f, int alpha_ncols = 0,
                      long long act_plane = 0, const int* lens = nullptr, int T = 0) {
  H2wArgs g{};
  g.act = planes; g.act_plane = act_plane ? act_plane : rows * W.K; g.lda = W.K; g.wpack = W.pack; g.rows = (int)rows; g.K = W.K; g.Wn = W.Wn; g.taps = 1;
  g.act_is_a = 1; g.C = Y; g.ldc = N; g.out = planes_out; g.out_plane = rows * N; g.ldo = N; g.bias = bias; g.alpha = alpha;
  g.alpha_ncols = alpha_ncols; g.act_fn = act; g.R = R; g.ldr = N; g.rowscale = rowscale; g.batch = 1;
  if (lens) {   // ragged: one batch item per utterance, bounded by H2wArgs::lens
    g.rows = T; g.batch = (int)(rows / T); g.sAct = (long long)T * W.K; g.sC = (long long)T * N; g.sO = (long long)T * N; g.sR = (long long)T * N;
    g.sRS = T; g.lens = lens;
  }
  return h2w_rec(rec, tag, g, st);
}

// The environment switches of the FFT stack and of the ESM front: read by the first call that asks and never again in the process.  (What a
// device answers is no switch: bsg_fs2midi::planes_lds.)
struct FftSwitches {
  bool gemm_h2w = env_int("BSG_GEMM_H2W", 1);         // =0: gemm_split_kernel (operands split while staged) instead of the pre-split GEMMs
  bool esm_h2w = env_int("BSG_ESM_H2W", 1);           // =0: the ESM's Linear layers on gemm_split_kernel and the thread-per-query attention
  bool flash = !getenv("BSG_NO_FLASH_ATTN");          // set at all: the score tensor + masked_softmax_kernel instead of a fused attention
  bool flash_split = env_int("BSG_FLASH_SPLIT", 1);   // =0: the fp32-MFMA attention even while the GEMMs run split-fp16
  bool flash_planes = env_int("BSG_FLASH_PLANES", 1); // =0: flash_attn_split_kernel (K / V split while staged) instead of the pre-split attention
  bool qkv_fused = env_int("BSG_QKV_FUSED", 1);       // =0: fp32 QKV tensor + qkv_split_kernel instead of the QKV product's own plane output
  int flash_ks = env_int("BSG_FLASH_KS", 0);          // 0 = auto, 1 = never split, 2 / 4 / 8 = that many key splits whenever the sequence allows
};
static const FftSwitches& fft_switches() { static const FftSwitches sw; return sw; }

// What one FFT stack launches at (B, T): chosen once per call by plan_fft, the same for every layer.
enum FftAttn { ATTN_PLANES, ATTN_SPLIT, ATTN_FLASH, ATTN_SOFTMAX };   // flash_attn_planes_kernel<2> · flash_attn_split_kernel<NW> · flash_attn_kernel<NW> · score tensor
enum FftQkv { QKV_FUSED, QKV_SPLIT_KERNEL, QKV_H2W, QKV_GEMM };       // who writes what the attention reads (the index of QKV_TOKEN)
static const char* const QKV_TOKEN[] = {"fused", "split_kernel", "h2w", "gemm"};
struct FftPlan {
  int B, T, Tp, ksz, heads, hd;
  long long rows;
  float qscale;
  bool h2w;            // every product on launch_gemm_h2w (operands pre-split by their producers) · on launch_gemm (split while staged)
  FftQkv qkv;
  FftAttn attn;
  int nw, ks;          // waves per workgroup of the attention; planes: the workgroups that share the keys of a query tile
  const char* attn_tok;   // the form as last_path names it, set where the form is chosen
  dim3 grid, block;    // of the attention launch (softmax: of masked_softmax_kernel)
  size_t need_fsk, need_fcnt, need_scores;   // elements the call needs of w_fsk / w_fcnt / w_scores; 0 where the form needs none
  // Operand views of the pre-split path: Q | K planes [2][rows][2H] in the (not yet written) FFN planes buffer w_fp; V^T planes [2][B][H][Tp] in
  // the fp32 FFN buffer that path does not use; the key mask words [B][Tp / 32] behind them.  attn_*: where the attention writes, fp32 rows
  // for the staged GEMM, planes (w_ap) for the pre-split one.
  _Float16 *qk, *vt, *attn_planes;
  long long qk_plane, vt_plane, attn_plane;
  unsigned* km;
  float* attn_out;
};

// Pure: reads the handle (h2w_ok, heads, its workspace pointers, gemm_split_enabled() under the call's guard scope), the switches and the
// shape; writes nothing, allocates and launches nothing.  Every threshold is a workgroup count of the shape against a constant.
// ragged: the call carries per-utterance lengths.  The attention's thresholds are those of the padded call at (B, T); the forms that are not
// built with lengths (the score tensor, qkv_split_kernel) are not chosen: the ragged entries refuse, before any device call, where the
// score tensor would be the only one left (rag_plan_check).
static FftPlan plan_fft(const bsg_fs2midi* h, int B, int T, int ksz, bool ragged = false) {
  const FftSwitches& sw = fft_switches();
  FftPlan p{};
  p.B = B; p.T = T; p.Tp = cdiv(T, 32) * 32; p.ksz = ksz; p.heads = h->cfg.num_heads; p.hd = H / p.heads;
  p.rows = (long long)B * T; p.qscale = (float)sqrt(1.0 / (double)p.hd);
  const bool split_ok = gemm_split_enabled(), flash = p.hd == 128 && sw.flash;
  p.h2w = sw.gemm_h2w && h->h2w_ok && split_ok && sw.flash_split && flash && h2w_supports(T, 4 * H, H, ksz, H) &&
          h2w_supports((int)p.rows, 3 * H, H, 1, H) && p.rows * 4 * H * 2 < (1LL << 31);
  if (p.h2w && sw.flash_planes && h->planes_lds && p.Tp <= 3 * T && p.rows >= 32 && (!ragged || sw.qkv_fused)) {
    // 2 waves (64 queries) per workgroup at every size: the pipelined loop keeps two score tiles live and does not fit 4 waves x 2 workgroups.
    // Small batches: the keys of a query tile over ks workgroups (a single utterance is 32 workgroups, each a serial chain of 32 key blocks)
    p.attn = ATTN_PLANES; p.nw = 2; p.qkv = sw.qkv_fused ? QKV_FUSED : QKV_SPLIT_KERNEL;
    const int units = cdiv(T, 64) * B * p.heads, nb = p.Tp / 32;
    p.ks = 1;
    if (sw.flash_ks == 0) { while (p.ks < 4 && units * p.ks * 2 <= 512 && nb / (p.ks * 2) >= 4) p.ks *= 2; }
    else { while (p.ks < sw.flash_ks && nb / (p.ks * 2) >= 1) p.ks *= 2; }
    p.attn_tok = p.ks == 1 ? "planes/ks1" : p.ks == 2 ? "planes/ks2" : p.ks == 4 ? "planes/ks4" : p.ks == 8 ? "planes/ks8" : "planes/ks16+";
    p.grid = dim3(cdiv(T, 64), B * p.heads, p.ks); p.block = dim3(128);
    if (p.ks > 1) { p.need_fsk = (size_t)units * p.ks * (2 * 64 * 66); p.need_fcnt = (size_t)units; }
  } else if (flash) {
    // fused attention without planes: 2 waves per workgroup when 4 would leave CUs idle; fp32 MFMA unless the GEMMs run split-fp16
    p.attn = p.h2w || (sw.flash_split && split_ok) ? ATTN_SPLIT : ATTN_FLASH;
    p.nw = (long long)cdiv(T, 128) * B * p.heads >= 512 ? 4 : 2;
    p.attn_tok = p.attn == ATTN_SPLIT ? (p.nw == 4 ? "split/nw4" : "split/nw2") : (p.nw == 4 ? "flash/nw4" : "flash/nw2");
    p.qkv = p.h2w ? QKV_H2W : QKV_GEMM;
    p.grid = dim3(cdiv(T, 32 * p.nw), B * p.heads); p.block = dim3(64 * p.nw);
  } else {
    // [B*heads, T, T] scores: only this form (BSG_NO_FLASH_ATTN, or a head dim other than 128) needs them
    p.attn = ATTN_SOFTMAX; p.attn_tok = "softmax"; p.qkv = QKV_GEMM;
    p.grid = dim3((unsigned)((long long)B * p.heads * T)); p.block = dim3(256);
    p.need_scores = (size_t)B * p.heads * T * T;
  }
  p.qk = reinterpret_cast<_Float16*>(h->w_fp); p.qk_plane = p.rows * 2 * H;
  p.vt = reinterpret_cast<_Float16*>(h->w_ffn); p.vt_plane = (long long)B * H * p.Tp;
  p.km = reinterpret_cast<unsigned*>(p.vt + 2 * p.vt_plane);
  if (p.h2w) { p.attn_planes = reinterpret_cast<_Float16*>(h->w_ap); p.attn_plane = p.rows * H; } else p.attn_out = h->w_a;
  return p;
}

// Q | K | V of a layer on the pre-split path, from the LayerNorm planes in h->w_ap
static int qkv_h2w(bsg_fs2midi* h, const char* gtag, const FftPlan& p, const FftLayerW& L, const float* keep, hipStream_t st, const int* lens) {
  if (p.qkv == QKV_FUSED) {
    H2wArgs g{};   // the QKV product writes the attention's planes itself (H2wArgs::qkv_T): no fp32 QKV tensor, no split launch
    g.act = h->w_ap; g.act_plane = p.rows * H; g.lda = H; g.wpack = L.p_in.pack; g.rows = (int)p.rows; g.K = H; g.Wn = 3 * H; g.taps = 1; g.act_is_a = 1;
    g.out = h->w_fp; g.out_plane = p.qk_plane; g.ldo = 2 * H; g.alpha = p.qscale; g.alpha_ncols = H; g.act_fn = ACT_NONE; g.batch = 1;
    g.qkv_T = p.T; g.qkv_Tp = p.Tp; g.qkv_H = H; g.vt = reinterpret_cast<unsigned short*>(p.vt); g.vt_plane = p.vt_plane;
    if (lens) {   // ragged: one batch item per utterance (its tiles start at the utterance's first row: every K / V row the attention stages up to
                  // the end of the utterance's last 32-key block lies in a tile that is computed, and is 0 beyond the end)
      g.rows = p.T; g.batch = p.B; g.sAct = (long long)p.T * H; g.sO = (long long)p.T * 2 * H; g.lens = lens;
    }
    return h2w_rec(h, gtag, g, st);
  }
  TRY(linear_h2w(h, gtag, h->w_ap, L.p_in, 3 * H, nullptr, h->w_qkv, nullptr, p.rows, ACT_NONE, nullptr, nullptr, st, p.qscale, H, 0, lens, p.T));
  if (p.qkv == QKV_SPLIT_KERNEL) {
    hipLaunchKernelGGL(qkv_split_kernel, dim3(p.Tp / 32, p.B), dim3(256), 0, st, (const float*)h->w_qkv, p.qk, p.qk_plane, p.vt, p.vt_plane, p.T, p.Tp, keep, p.km, gemm_range_counter());
    BSG_LAUNCH_CHECK();
  }
  return BSG_OK;
}

// The attention of a layer: the one launch site of every form, named once its kernel has been launched
static int attention(bsg_fs2midi* h, bool first, const char* stack, const char* gtag, const FftPlan& p, const float* keep, hipStream_t st,
                     const int* lens) {
  const int T = p.T, heads = p.heads;
  const float* qkv = h->w_qkv;
  switch (p.attn) {
    case ATTN_PLANES:
      hipLaunchKernelGGL(flash_attn_planes_kernel<2>, p.grid, p.block, FLP_LDS, st, (const _Float16*)p.qk, p.qk_plane, (const _Float16*)p.vt, p.vt_plane, (const unsigned*)p.km, T, p.Tp, heads, p.attn_planes, p.attn_plane, H, gemm_range_counter(), h->w_fsk, h->w_fcnt, lens);
      break;
    case ATTN_SPLIT:
      if (p.nw == 4) hipLaunchKernelGGL(flash_attn_split_kernel<4>, p.grid, p.block, 0, st, qkv, keep, p.attn_out, T, heads, 3 * H, H, gemm_range_counter(), p.attn_planes, p.attn_plane, lens);
      else hipLaunchKernelGGL(flash_attn_split_kernel<2>, p.grid, p.block, 0, st, qkv, keep, p.attn_out, T, heads, 3 * H, H, gemm_range_counter(), p.attn_planes, p.attn_plane, lens);
      break;
    case ATTN_FLASH:   // no [B*heads, T, T] score tensor (flash_attn_kernel)
      if (p.nw == 4) hipLaunchKernelGGL(flash_attn_kernel<4>, p.grid, p.block, 0, st, qkv, keep, p.attn_out, T, heads, 3 * H, H, lens);
      else hipLaunchKernelGGL(flash_attn_kernel<2>, p.grid, p.block, 0, st, qkv, keep, p.attn_out, T, heads, 3 * H, H, lens);
      break;
    case ATTN_SOFTMAX: {   // (never with lengths: rag_plan_check refused the call)
      const int hd = p.hd, nbh = p.B * heads;
      GemmArgs s{};   // S[b,h] = Q K^T
      s.A = qkv; s.B = qkv + H; s.C = h->w_scores; s.M = T; s.N = T; s.K = hd; s.lda = 3 * H; s.ldb = 3 * H; s.ldc = T;
      s.trans_b = 1; s.taps = 1; s.alpha = 1.f; s.batch = nbh; s.batch2 = heads;
      s.sA = (long long)T * 3 * H; s.sA2 = hd; s.sB = (long long)T * 3 * H; s.sB2 = hd;
      s.sC = (long long)heads * T * T; s.sC2 = (long long)T * T;
      TRY(gemm_rec(h, gtag, s, st));
      hipLaunchKernelGGL(masked_softmax_kernel, p.grid, p.block, 0, st, h->w_scores, keep, T, T, heads);
      BSG_LAUNCH_CHECK();
      path_name(h, first, stack, "attn:", p.attn_tok);
      GemmArgs o{};   // O[b,:,h] = P V
      o.A = h->w_scores; o.B = qkv + 2 * H; o.C = p.attn_out; o.M = T; o.N = hd; o.K = T; o.lda = T; o.ldb = 3 * H; o.ldc = H;
      o.trans_b = 0; o.taps = 1; o.alpha = 1.f; o.batch = nbh; o.batch2 = heads;
      o.sA = (long long)heads * T * T; o.sA2 = (long long)T * T; o.sB = (long long)T * 3 * H; o.sB2 = hd;
      o.sC = (long long)T * H; o.sC2 = hd;
      return gemm_rec(h, gtag, o, st);
    }
  }
  BSG_LAUNCH_CHECK();
  path_name(h, first, stack, "attn:", p.attn_tok);
  return BSG_OK;
}

// EncSALayer x FFTBlocks tail (common_layers.py:706-730, tts_modules.py:298-305); x [B*T, H] in place.  plan_fft decides, grow()
// allocates, the loops only launch.  Every GEMM launch of every layer goes through path_add; the QKV and attention tokens are named in the
// first layer only (`first`), the later layers launching the plan's same forms.
// lens (ragged calls; null = the padded call, which launches exactly what it did): utterance b is lens[b] rows long.  The layout stays padded
// ([B][T] rows, the pitch of every tensor) and every launch takes the lengths: LayerNorm and the GEMMs neither read nor compute rows at or
// beyond an utterance's end (the k-tap convolution reads zeros there), the attention's query tiles and key blocks stop at it, and whole
// tiles beyond it return before their first load.  The caller sets last_stack_rows (it knows the lengths on the host).
static int launch_fft(bsg_fs2midi* h, const std::vector<FftLayerW>& layers, const float* lnw, const float* lnb, int ksz,
                      float* x, const float* keep, int B, int T, hipStream_t st, const char* stack, const int* lens = nullptr) {
  const FftPlan p = plan_fft(h, B, T, ksz, lens != nullptr);
  const long long rows = p.rows;
  if (!lens) h->last_stack_rows = (int)rows;
  TRY(grow(h, &h->cap_fsk, p.need_fsk, st));
  TRY(grow(h, &h->cap_fcnt, p.need_fcnt, st));
  TRY(grow(h, &h->cap_scores, p.need_scores, st));
  const std::string gemm_tag = std::string(stack) + "gemm:";
  const char* gtag = gemm_tag.c_str();
  const float ffn_alpha = (float)pow((double)ksz, -0.5);
  bool first = true;
  if (p.qkv == QKV_FUSED) {   // the key mask words once per stack: qkv_split_kernel writes them itself, the fused QKV product does not
    hipLaunchKernelGGL(key_mask_kernel, dim3(cdiv(B * (p.Tp / 32), 4)), dim3(256), 0, st, keep, p.km, B, T, p.Tp);
    BSG_LAUNCH_CHECK();
  }
  if (p.h2w) {
    // Every product on the 16-bit matrix pipe with PRE-SPLIT operands (gemm_h2w.hip): the weights were split into hi / lo fp16 fragments at
    // create, and each activation is written as hi / lo fp16 planes by the kernel that produces it (LayerNorm, the fused attention, the
    // GELU epilogue of the FFN convolution) — no kernel splits an operand while it stages it.  Same arithmetic as the loop below.
    for (const FftLayerW& L : layers) {
      TRY(ln_planes(x, L.ln1w, L.ln1b, h->w_ap, rows, 1e-5f, st, lens, T));
      TRY(qkv_h2w(h, gtag, p, L, keep, st, lens));
      path_name(h, first, stack, "qkv:", QKV_TOKEN[p.qkv]);
      TRY(attention(h, first, stack, gtag, p, keep, st, lens));
      TRY(linear_h2w(h, gtag, h->w_ap, L.p_out, H, nullptr, h->w_b, nullptr, rows, ACT_NONE, x, keep, st, 1.f, 0, 0, lens, T));   // x1 = (x + attn) * keep
      TRY(ln_planes(h->w_b, L.ln2w, L.ln2b, h->w_ap, rows, 1e-5f, st, lens, T));
      H2wArgs g{};   // Conv1d(H -> 4H, k, SAME) * k^-1/2 -> GELU, written as the planes the second Linear reads
      g.act = h->w_ap; g.act_plane = rows * H; g.lda = H; g.sAct = (long long)T * H; g.wpack = L.p_ffn1.pack; g.rows = T; g.K = H; g.Wn = 4 * H;
      g.taps = ksz; g.tap_shift0 = -(ksz / 2); g.act_is_a = 1; g.out = h->w_fp; g.out_plane = rows * 4 * H; g.ldo = 4 * H; g.sO = (long long)T * 4 * H;
      g.bias = L.ffn1b; g.alpha = ffn_alpha; g.act_fn = ACT_GELU; g.batch = B; g.lens = lens;   // (ragged: the taps read zeros beyond the utterance's end)
      TRY(h2w_rec(h, gtag, g, st));
      TRY(linear_h2w(h, gtag, h->w_fp, L.p_ffn2, H, L.ffn2b, x, nullptr, rows, ACT_NONE, h->w_b, keep, st, 1.f, 0, 0, lens, T));   // x = (x1 + ffn) * keep
      first = false;
    }
  } else {
    for (const FftLayerW& L : layers) {
      TRY(ln(x, L.ln1w, L.ln1b, h->w_a, nullptr, rows, 1e-5f, st, lens, T));
      TRY(linear(h->w_a, L.in_proj, nullptr, h->w_qkv, rows, 3 * H, H, ACT_NONE, nullptr, nullptr, st, p.qscale, H, h, gtag, lens, T));
      path_name(h, first, stack, "qkv:", QKV_TOKEN[p.qkv]);
      TRY(attention(h, first, stack, gtag, p, keep, st, lens));
      TRY(linear(h->w_a, L.out_proj, nullptr, h->w_b, rows, H, H, ACT_NONE, x, keep, st, 1.f, 0, h, gtag, lens, T));   // x1 = (x + attn) * keep
      TRY(ln(h->w_b, L.ln2w, L.ln2b, h->w_a, nullptr, rows, 1e-5f, st, lens, T));
      GemmArgs g{};   // Conv1d(H -> 4H, k, SAME) * k^-1/2 -> GELU
      g.A = h->w_a; g.B = L.ffn1; g.C = h->w_ffn; g.M = T; g.N = 4 * H; g.K = H; g.lda = H; g.ldb = H; g.ldc = 4 * H;
      g.trans_b = 1; g.taps = ksz; g.tap_shift0 = -(ksz / 2); g.sTapB = (long long)4 * H * H;
      g.bias_n = L.ffn1b; g.alpha = ffn_alpha; g.act = ACT_GELU; g.batch = B;
      g.sA = (long long)T * H; g.sC = (long long)T * 4 * H; g.lens = lens;   // (ragged: the taps read zeros beyond the utterance's end)
      TRY(gemm_rec(h, gtag, g, st));
      TRY(linear(h->w_ffn, L.ffn2, L.ffn2b, x, rows, H, 4 * H, ACT_NONE, h->w_b, keep, st, 1.f, 0, h, gtag, lens, T));   // x = (x1 + ffn) * keep
      first = false;
    }
  }
  return ln(x, lnw, lnb, x, keep, rows, 1e-5f, st, lens, T);   // (ragged: 0 beyond an utterance's end — what the call returns there)
}

// duration predictor (tts_modules.py:108-133) on (x + spk) * keep for the nb utterances of x (their keep in w_keep); spk_id: these rows'
// lens (ragged calls): the predictor is masked per layer already, so the lengths only skip the padded rows; dur_xs and dur are 0 beyond an
// utterance's end
static int dur_predict(bsg_fs2midi* h, const float* x, const int64_t* spk_id, int32_t nb, int32_t Tt, float* dur_xs, int64_t* dur, hipStream_t st,
                       const int* lens = nullptr) {
  const long long lrows = (long long)nb * Tt;
  const dim3 lg(cdiv(lrows, 4)), rb(256);
  // duration predictor (tts_modules.py:108-133) on (enc + spk) * keep
  float* a = h->w_a;
  float* b = h->w_b;
  hipLaunchKernelGGL(add_spk_kernel, lg, rb, 0, st, (const float*)x, (const long long*)spk_id, h->Espk, h->w_keep, a, lrows, Tt, lens);
  BSG_LAUNCH_CHECK();
  const int ks = h->cfg.dur_kernel;
  for (int l = 0; l < h->cfg.dur_layers; ++l) {
    GemmArgs g{};
    g.A = a; g.B = h->dur_conv[l]; g.C = b; g.M = Tt; g.N = H; g.K = H; g.lda = H; g.ldb = H; g.ldc = H; g.trans_b = 1;
    g.taps = ks; g.tap_shift0 = -(ks / 2); g.sTapB = (long long)H * H; g.bias_n = h->dur_convb[l]; g.alpha = 1.f;
    g.act = ACT_RELU; g.batch = nb; g.sA = (long long)Tt * H; g.sC = (long long)Tt * H; g.lens = lens;
    TRY(launch_gemm(g, st));
    TRY(ln(b, h->dur_lnw[l], h->dur_lnb[l], a, h->w_keep, lrows, 1e-12f, st, lens, Tt));
  }
  TRY(linear(a, h->dur_lin_w, h->dur_lin_b, dur_xs, lrows, 1, H, ACT_NONE, nullptr, h->w_keep, st, 1.f, 0, nullptr, "", lens, Tt));
  hipLaunchKernelGGL(dur_from_log_kernel, dim3(cdiv(lrows, 256)), dim3(256), 0, st, dur_xs, (long long*)dur, lrows, lens, Tt);
  BSG_LAUNCH_CHECK();
  return BSG_OK;
}

// Token-level front for the batch rows [row0, row0 + nb) of a batch of B utterances.  Only the ESM couples rows (it attends over the BATCH
// axis, common_layers.py:853), and only through K / V = projections of LN(lang_embed[lang]) of every row (:850-853): the other rows
// contribute their `lang` ints and nothing else.  So K / V are projected for all B rows, and everything else — Q, the attention's queries,
// the ESM's FFN, the embedding sum, the 4-layer FFT encoder, the duration predictor — runs on the nb rows asked for.  row0 = 0, nb = B is
// the whole batch (bsg_fs2midi_encode); a rank of a sharded run asks for its own rows (bsg_fs2midi_encode_rows): the same arithmetic
// on an eighth of the tokens at configs[3].
static int encode_impl(bsg_fs2midi* h, const int64_t* txt, const int64_t* pitch_midi, const float* midi_dur, const int64_t* is_slur,
                       const int64_t* lang, const int64_t* spk_id, int32_t B, int32_t Tt, int32_t row0, int32_t nb, float* enc_out,
                       float* dur_xs, int64_t* dur, hipStream_t st) {
  const long long rows = (long long)B * Tt;        // every utterance: the lang embedding and K / V
  const long long lrows = (long long)nb * Tt;      // the rows asked for
  const long long off = (long long)row0 * Tt;
  TRY(grow(h, &h->cap_rows, (size_t)rows, st));
  h->last_token_rows = (int)lrows;
  const dim3 rg(cdiv(rows, 4)), lg(cdiv(lrows, 4)), rb(256);
  const float sq = sqrtf((float)H);
  float* x0 = h->w_x;      // sqrt(H) * tok                [rows][H]
  float* lange = h->w_b;   // lang embedding LP            [rows][H]
  const FftSwitches& sw = fft_switches();
  const bool esm_h2w = sw.esm_h2w && sw.gemm_h2w && h->h2w_ok && gemm_split_enabled() && B <= 64 && h2w_supports((int)rows, H, H, 1, H) &&
                       h2w_supports((int)lrows, H, H, 1, H) && rows * 4 * H * 2 < (1LL << 31);
  if (esm_h2w) {
    // ---- ESM (common_layers.py:848-860) on the pre-split GEMM: every operand is written as hi / lo planes by its producer; the K and V
    // projections (both of LN(lang)) are ONE product of 512 weight rows; the attention runs one wave per (position, head)
    unsigned short* ap = h->w_ap;   // [2][rows][H]
    unsigned short* fp = h->w_fp;   // x0 planes, later the FFN's hidden planes ([2][rows][H] of its [2][rows][4H])
    hipLaunchKernelGGL(embed_tokens_kernel, rg, rb, 0, st, (const long long*)txt, (const long long*)lang, h->Etok, h->Elang, x0, lange, rows, sq,
                       reinterpret_cast<_Float16*>(fp), reinterpret_cast<_Float16*>(fp) + rows * H, gemm_range_counter());
    BSG_LAUNCH_CHECK();
    TRY(ln_planes(lange, h->esm_ln1w, h->esm_ln1b, ap, rows, 1e-5f, st));
    float* q = h->w_qkv;                // [lrows][H]
    float* kvp = h->w_qkv + rows * H;   // [rows][2H]: K | V
    TRY(linear_h2w(h, "esm.gemm:", fp + off * H, h->p_esm_q, H, h->esm_in_b, q, nullptr, lrows, ACT_NONE, nullptr, nullptr, st, 1.f, 0, rows * H));
    TRY(linear_h2w(h, "esm.gemm:", ap, h->p_esm_kv, 2 * H, h->esm_in_b + H, kvp, nullptr, rows, ACT_NONE, nullptr, nullptr, st));
    hipLaunchKernelGGL(esm_attention_wave_kernel, dim3(cdiv(Tt * 8, 4)), dim3(256), 0, st, (const float*)q, (const float*)kvp, (const float*)(kvp + H), H,
                       2 * H, (float*)nullptr, reinterpret_cast<_Float16*>(ap), lrows * H, B, nb, Tt, 8, (float)sqrt(1.0 / 32.0), gemm_range_counter());
    BSG_LAUNCH_CHECK();
    path_add(h, "esm:", "wave");
    float* Mo = h->w_c;
    TRY(linear_h2w(h, "esm.gemm:", ap, h->p_esm_out, H, h->esm_out_b, Mo, nullptr, lrows, ACT_NONE, lange + off * H, nullptr, st));   // Mo = out_proj + LP
    TRY(ln_planes(Mo, h->esm_ln2w, h->esm_ln2b, ap, lrows, 1e-5f, st));
    TRY(linear_h2w(h, "esm.gemm:", ap, h->p_esm_f0, H, h->esm_f0b, nullptr, fp, lrows, ACT_RELU, nullptr, nullptr, st));
    TRY(linear_h2w(h, "esm.gemm:", fp, h->p_esm_f2, H, h->esm_f2b, h->w_a, nullptr, lrows, ACT_NONE, Mo, nullptr, st));          // Fo = ffn + Mo
  } else {
  hipLaunchKernelGGL(embed_tokens_kernel, rg, rb, 0, st, (const long long*)txt, (const long long*)lang, h->Etok, h->Elang, x0, lange, rows, sq,
                     (_Float16*)nullptr, (_Float16*)nullptr, (unsigned*)nullptr);
  BSG_LAUNCH_CHECK();
  // ---- ESM (common_layers.py:848-860): attention over the batch axis
  float* lpn = h->w_a;
  TRY(ln(lange, h->esm_ln1w, h->esm_ln1b, lpn, nullptr, rows, 1e-5f, st));
  float* q = h->w_qkv;                     // [lrows][H]
  float* k = h->w_qkv + rows * H;          // [rows][H]
  float* v = h->w_qkv + 2 * rows * H;
  TRY(linear(x0 + off * H, h->esm_in_w, h->esm_in_b, q, lrows, H, H, ACT_NONE, nullptr, nullptr, st, 1.f, 0, h, "esm.gemm:"));
  TRY(linear(lpn, h->esm_in_w + (size_t)H * H, h->esm_in_b + H, k, rows, H, H, ACT_NONE, nullptr, nullptr, st, 1.f, 0, h, "esm.gemm:"));
  TRY(linear(lpn, h->esm_in_w + (size_t)2 * H * H, h->esm_in_b + 2 * H, v, rows, H, H, ACT_NONE, nullptr, nullptr, st, 1.f, 0, h, "esm.gemm:"));
  float* att = h->w_a;   // lpn is dead once k, v exist
  {
    const long long total = lrows * 8;
    hipLaunchKernelGGL(esm_attention_kernel<32>, dim3(cdiv(total, 128)), dim3(128), 0, st, (const float*)q, (const float*)k,
                       (const float*)v, att, B, nb, Tt, 8, (float)sqrt(1.0 / 32.0));
    BSG_LAUNCH_CHECK();
    path_add(h, "esm:", "thread");
  }
  float* Mo = h->w_c;
  TRY(linear(att, h->esm_out_w, h->esm_out_b, Mo, lrows, H, H, ACT_NONE, lange + off * H, nullptr, st, 1.f, 0, h, "esm.gemm:"));       // Mo = out_proj + LP
  float* t1 = h->w_a;
  float* t2 = h->w_qkv;   // (q, k, v are dead; w_b still holds the lang embedding of every row)
  TRY(ln(Mo, h->esm_ln2w, h->esm_ln2b, t1, nullptr, lrows, 1e-5f, st));
  TRY(linear(t1, h->esm_f0w, h->esm_f0b, t2, lrows, H, H, ACT_RELU, nullptr, nullptr, st, 1.f, 0, h, "esm.gemm:"));
  TRY(linear(t2, h->esm_f2w, h->esm_f2b, h->w_a, lrows, H, H, ACT_NONE, Mo, nullptr, st, 1.f, 0, h, "esm.gemm:"));      // Fo = ffn + Mo
  }
  // ---- sum of embeddings, *sqrt(H) + reversed positional table, mask (the rows asked for; row0 * Tt is a multiple of Tt: the position of a
  // row inside its utterance is unchanged)
  float* x = h->w_c;
  hipLaunchKernelGGL(embed_finish_kernel, lg, rb, 0, st, (const float*)(x0 + off * H), (const float*)h->w_a, (const long long*)txt + off,
                     (const long long*)pitch_midi + off, midi_dur + off, (const long long*)is_slur + off, h->Emidi, h->Wdur, h->bdur, h->Eslur,
                     h->rel_table, x, h->w_keep, lrows, Tt, sq);
  BSG_LAUNCH_CHECK();
  TRY(launch_fft(h, h->enc, h->enc_lnw, h->enc_lnb, h->cfg.enc_ffn_kernel_size, x, h->w_keep, nb, Tt, st, "enc."));
  BSG_HIP(hipMemcpyAsync(enc_out, x, lrows * H * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (dur) TRY(dur_predict(h, x, spk_id ? spk_id + row0 : nullptr, nb, Tt, dur_xs, dur, st));
  return BSG_OK;
}

extern "C" int bsg_fs2midi_encode(bsg_fs2midi* h, const int64_t* txt, const int64_t* pitch_midi, const float* midi_dur,
                                  const int64_t* is_slur, const int64_t* lang, const int64_t* spk_id, int32_t B, int32_t Tt,
                                  float* enc_out, float* dur_xs, int64_t* dur, void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  BSG_REQUIRE(h && txt && pitch_midi && midi_dur && is_slur && lang && spk_id && enc_out, "fs2midi_encode: null argument");
  BSG_REQUIRE(h->front == BSG_FS2_FRONT_MIDI, "fs2midi_encode: the handle has the plain front (bsg_fs2_encode_plain)");
  BSG_REQUIRE(B > 0 && Tt > 0 && Tt <= h->cfg.n_rel, "fs2midi_encode: B=%d T_txt=%d (rel-pos table has %d rows)", B, Tt, h->cfg.n_rel);
  BSG_REQUIRE((dur_xs == nullptr) == (dur == nullptr), "fs2midi_encode: dur_xs and dur go together");
  h->path.clear();
  const int rc = encode_impl(h, txt, pitch_midi, midi_dur, is_slur, lang, spk_id, B, Tt, 0, B, enc_out, dur_xs, dur, (hipStream_t)stream);
  h->path_enc_len = h->path.size();
  return rc;
}

extern "C" int bsg_fs2midi_encode_rows(bsg_fs2midi* h, const int64_t* txt, const int64_t* pitch_midi, const float* midi_dur,
                                       const int64_t* is_slur, const int64_t* lang, const int64_t* spk_id, int32_t B, int32_t Tt,
                                       int32_t row0, int32_t n_rows, float* enc_out, float* dur_xs, int64_t* dur, void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  BSG_REQUIRE(h && txt && pitch_midi && midi_dur && is_slur && lang && spk_id && enc_out, "fs2midi_encode_rows: null argument");
  BSG_REQUIRE(h->front == BSG_FS2_FRONT_MIDI, "fs2midi_encode_rows: the handle has the plain front (bsg_fs2_encode_plain)");
  BSG_REQUIRE(B > 0 && Tt > 0 && Tt <= h->cfg.n_rel, "fs2midi_encode_rows: B=%d T_txt=%d (rel-pos table has %d rows)", B, Tt, h->cfg.n_rel);
  BSG_REQUIRE(row0 >= 0 && n_rows > 0 && row0 + n_rows <= B, "fs2midi_encode_rows: rows [%d, %d) of a batch of %d", row0, row0 + n_rows, B);
  BSG_REQUIRE((dur_xs == nullptr) == (dur == nullptr), "fs2midi_encode_rows: dur_xs and dur go together");
  h->path.clear();
  const int rc = encode_impl(h, txt, pitch_midi, midi_dur, is_slur, lang, spk_id, B, Tt, row0, n_rows, enc_out, dur_xs, dur, (hipStream_t)stream);
  h->path_enc_len = h->path.size();
  return rc;
}

// The plain front (fastspeech/fs2.py:100-129): token embedding + positions in one launch, the FFT encoder, the duration predictor.  Nothing
// couples the utterances of a batch, so the rows [row0, row0 + n_rows) are simply the rows that run.
extern "C" int bsg_fs2_encode_plain(bsg_fs2midi* h, const int64_t* txt, const int64_t* spk_id, int32_t B, int32_t Tt, int32_t row0,
                                    int32_t n_rows, float* enc_out, float* dur_xs, int64_t* dur, void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  BSG_REQUIRE(h && txt && enc_out, "fs2_encode_plain: null argument");
  BSG_REQUIRE(h->front == BSG_FS2_FRONT_PLAIN, "fs2_encode_plain: the handle has the MIDI front (bsg_fs2midi_encode)");
  BSG_REQUIRE((spk_id != nullptr) == (h->cfg.spk_rows > 0), "fs2_encode_plain: spk_id goes with a speaker table (spk_rows=%d)", h->cfg.spk_rows);
  BSG_REQUIRE(B > 0 && Tt > 0 && Tt < h->cfg.n_rel, "fs2_encode_plain: B=%d T_txt=%d (position table has %d rows)", B, Tt, h->cfg.n_rel);
  BSG_REQUIRE(row0 >= 0 && n_rows > 0 && row0 + n_rows <= B, "fs2_encode_plain: rows [%d, %d) of a batch of %d", row0, row0 + n_rows, B);
  BSG_REQUIRE((dur_xs == nullptr) == (dur == nullptr), "fs2_encode_plain: dur_xs and dur go together");
  hipStream_t st = (hipStream_t)stream;
  h->path.clear();
  const long long lrows = (long long)n_rows * Tt, off = (long long)row0 * Tt;
  TRY(grow(h, &h->cap_rows, (size_t)lrows, st));
  h->last_token_rows = (int)lrows;
  float* x = h->w_c;
  hipLaunchKernelGGL(token_front_kernel, dim3(cdiv(lrows, 4)), dim3(256), 0, st, (const long long*)txt + off, h->Etok, h->rel_table, x, h->w_keep,
                     lrows, Tt, sqrtf((float)H), h->cfg.n_rel, h->cfg.vocab, (const int*)nullptr);
  BSG_LAUNCH_CHECK();
  path_add(h, "tok:", "front");
  TRY(launch_fft(h, h->enc, h->enc_lnw, h->enc_lnb, h->cfg.enc_ffn_kernel_size, x, h->w_keep, n_rows, Tt, st, "enc."));
  BSG_HIP(hipMemcpyAsync(enc_out, x, lrows * H * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (dur) TRY(dur_predict(h, x, spk_id ? spk_id + row0 : nullptr, n_rows, Tt, dur_xs, dur, st));
  h->path_enc_len = h->path.size();
  return BSG_OK;
}

// ---- ragged batches through the front (ABI v20): every utterance as the B = 1 call on its own tokens and frames --------------------------
// The counts come from a HOST array, are checked before any device call, and reach the kernels through the handle's own device rows
// (w_lens_t / w_lens_f), which launches of the call itself fill (lens_fill): a captured call replays its counts.
static int rag_check(const char* who, const char* what, const int32_t* n, int B, int lo, int hi) {
  BSG_REQUIRE(n, "%s: %s is null", who, what);
  for (int b = 0; b < B; ++b) BSG_REQUIRE(n[b] >= lo && n[b] <= hi, "%s: %s[%d]=%d outside %d..%d", who, what, b, n[b], lo, hi);
  return BSG_OK;
}
// rows that a ragged stack computes, as bsg_fs2midi_last_rows reports them: every utterance rounded up to the 32-row granule (the smallest
// tile of any launch of the stack: a 32-query wave of the attention, a 32-row GEMM tile; the 64- and 128-row tiles round further)
static int rag_rows(const int32_t* n, int B, int T) {
  long long r = 0;
  for (int b = 0; b < B; ++b) r += std::min(T, (n[b] + 31) / 32 * 32);
  return (int)r;
}

// The plan is pure, so a ragged entry asks it before its first device call: a stack whose attention could only be the score tensor is
// refused here, with nothing enqueued (under capture: nothing in the graph).
static int rag_plan_check(const bsg_fs2midi* h, const char* who, int B, int T, int ksz) {
  BSG_REQUIRE(plan_fft(h, B, T, ksz, true).attn != ATTN_SOFTMAX,
              "%s: the ragged front is built on the fused attention (head dim 128, BSG_NO_FLASH_ATTN unset), not on the score tensor", who);
  return BSG_OK;
}

// The ESM of an utterance ALONE (common_layers.py:848-860 at B = 1): the attention over the batch axis has one key, its softmax is exactly 1,
// so the attention's output is V and Q / K drop out:  Mo = out_proj(v_proj(LN1(E_lang[l]))) + E_lang[l],  Fo = ffn(LN2(Mo)) + Mo — a function of
// the token's lang id only.  Two rows (one per row of lang_embed) on the handle's LayerNorm / GEMM launches (split-fp16: fp32-grade).
static int esm_alone_table(bsg_fs2midi* h, const float** tab, hipStream_t st) {
  float* s = h->esm_scr;   // [6][2][H]
  float *lpn = s, *v = s + 2 * H, *Mo = s + 4 * H, *t1 = s + 6 * H, *t2 = s + 8 * H, *Fo = s + 10 * H;
  TRY(ln(h->Elang, h->esm_ln1w, h->esm_ln1b, lpn, nullptr, 2, 1e-5f, st));
  TRY(linear(lpn, h->esm_in_w + (size_t)2 * H * H, h->esm_in_b + 2 * H, v, 2, H, H, ACT_NONE, nullptr, nullptr, st, 1.f, 0, h, "esm.gemm:"));
  TRY(linear(v, h->esm_out_w, h->esm_out_b, Mo, 2, H, H, ACT_NONE, h->Elang, nullptr, st, 1.f, 0, h, "esm.gemm:"));
  TRY(ln(Mo, h->esm_ln2w, h->esm_ln2b, t1, nullptr, 2, 1e-5f, st));
  TRY(linear(t1, h->esm_f0w, h->esm_f0b, t2, 2, H, H, ACT_RELU, nullptr, nullptr, st, 1.f, 0, h, "esm.gemm:"));
  TRY(linear(t2, h->esm_f2w, h->esm_f2b, Fo, 2, H, H, ACT_NONE, Mo, nullptr, st, 1.f, 0, h, "esm.gemm:"));
  path_add(h, "esm:", "alone");
  *tab = Fo;
  return BSG_OK;
}

// what both ragged encodes share once the front's rows are in w_c / w_keep
static int encode_ragged_tail(bsg_fs2midi* h, const int64_t* spk_id, const int32_t* n_tok_host, int32_t B, int32_t Tt, float* enc_out,
                              float* dur_xs, int64_t* dur, hipStream_t st) {
  const long long rows = (long long)B * Tt;
  float* x = h->w_c;
  TRY(launch_fft(h, h->enc, h->enc_lnw, h->enc_lnb, h->cfg.enc_ffn_kernel_size, x, h->w_keep, B, Tt, st, "enc.", h->w_lens_t));
  h->last_token_rows = h->last_stack_rows = rag_rows(n_tok_host, B, Tt);
  BSG_HIP(hipMemcpyAsync(enc_out, x, rows * H * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (dur) TRY(dur_predict(h, x, spk_id, B, Tt, dur_xs, dur, st, h->w_lens_t));
  h->path_enc_len = h->path.size();
  return BSG_OK;
}

extern "C" int bsg_fs2midi_encode_ragged(bsg_fs2midi* h, const int64_t* txt, const int64_t* pitch_midi, const float* midi_dur,
                                         const int64_t* is_slur, const int64_t* lang, const int64_t* spk_id, const int32_t* n_tok_host,
                                         int32_t B, int32_t Tt, float* enc_out, float* dur_xs, int64_t* dur, void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  BSG_REQUIRE(h && txt && pitch_midi && midi_dur && is_slur && lang && spk_id && enc_out, "fs2midi_encode_ragged: null argument");
  BSG_REQUIRE(h->front == BSG_FS2_FRONT_MIDI, "fs2midi_encode_ragged: the handle has the plain front (bsg_fs2_encode_plain_ragged)");
  BSG_REQUIRE(B > 0 && B <= 65535 && Tt > 0 && Tt <= h->cfg.n_rel, "fs2midi_encode_ragged: B=%d T_txt=%d (rel-pos table has %d rows)", B, Tt, h->cfg.n_rel);
  BSG_REQUIRE((dur_xs == nullptr) == (dur == nullptr), "fs2midi_encode_ragged: dur_xs and dur go together");
  TRY(rag_check("fs2midi_encode_ragged", "n_tok_host", n_tok_host, B, 1, Tt));
  TRY(rag_plan_check(h, "fs2midi_encode_ragged", B, Tt, h->cfg.enc_ffn_kernel_size));
  hipStream_t st = (hipStream_t)stream;
  h->path.clear();
  const long long rows = (long long)B * Tt;
  TRY(grow(h, &h->cap_rows, (size_t)rows, st));
  TRY(grow(h, &h->cap_lens, (size_t)B, st));
  TRY(lens_fill(h->w_lens_t, n_tok_host, B, st));
  const float* tab = nullptr;
  TRY(esm_alone_table(h, &tab, st));
  hipLaunchKernelGGL(embed_ragged_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, (const long long*)txt, (const long long*)lang,
                     (const long long*)pitch_midi, midi_dur, (const long long*)is_slur, h->Etok, tab, h->Emidi, h->Wdur, h->bdur, h->Eslur,
                     h->rel_table, h->w_c, h->w_keep, rows, Tt, sqrtf((float)H), h->cfg.vocab, (const int*)h->w_lens_t);
  BSG_LAUNCH_CHECK();
  path_add(h, "tok:", "ragged");
  return encode_ragged_tail(h, spk_id, n_tok_host, B, Tt, enc_out, dur_xs, dur, st);
}

extern "C" int bsg_fs2_encode_plain_ragged(bsg_fs2midi* h, const int64_t* txt, const int64_t* spk_id, const int32_t* n_tok_host, int32_t B,
                                           int32_t Tt, float* enc_out, float* dur_xs, int64_t* dur, void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  BSG_REQUIRE(h && txt && enc_out, "fs2_encode_plain_ragged: null argument");
  BSG_REQUIRE(h->front == BSG_FS2_FRONT_PLAIN, "fs2_encode_plain_ragged: the handle has the MIDI front (bsg_fs2midi_encode_ragged)");
  BSG_REQUIRE((spk_id != nullptr) == (h->cfg.spk_rows > 0), "fs2_encode_plain_ragged: spk_id goes with a speaker table (spk_rows=%d)", h->cfg.spk_rows);
  BSG_REQUIRE(B > 0 && B <= 65535 && Tt > 0 && Tt < h->cfg.n_rel, "fs2_encode_plain_ragged: B=%d T_txt=%d (position table has %d rows)", B, Tt, h->cfg.n_rel);
  BSG_REQUIRE((dur_xs == nullptr) == (dur == nullptr), "fs2_encode_plain_ragged: dur_xs and dur go together");
  TRY(rag_check("fs2_encode_plain_ragged", "n_tok_host", n_tok_host, B, 1, Tt));
  TRY(rag_plan_check(h, "fs2_encode_plain_ragged", B, Tt, h->cfg.enc_ffn_kernel_size));
  hipStream_t st = (hipStream_t)stream;
  h->path.clear();
  const long long rows = (long long)B * Tt;
  TRY(grow(h, &h->cap_rows, (size_t)rows, st));
  TRY(grow(h, &h->cap_lens, (size_t)B, st));
  TRY(lens_fill(h->w_lens_t, n_tok_host, B, st));
  hipLaunchKernelGGL(token_front_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, (const long long*)txt, h->Etok, h->rel_table, h->w_c, h->w_keep,
                     rows, Tt, sqrtf((float)H), h->cfg.n_rel, h->cfg.vocab, (const int*)h->w_lens_t);
  BSG_LAUNCH_CHECK();
  path_add(h, "tok:", "ragged");
  return encode_ragged_tail(h, spk_id, n_tok_host, B, Tt, enc_out, dur_xs, dur, st);
}

extern "C" int bsg_fs2midi_last_rows(const bsg_fs2midi* h, int32_t* token_rows, int32_t* stack_rows) {
  BSG_REQUIRE(h && token_rows && stack_rows, "fs2midi_last_rows: null argument");
  *token_rows = h->last_token_rows;
  *stack_rows = h->last_stack_rows;
  return BSG_OK;
}

extern "C" const char* bsg_fs2midi_last_path(bsg_fs2midi* h) { return h && !h->path.empty() ? h->path.c_str() : "none"; }

// Test hook: every activation workspace of the handle, at its current capacity, filled with 0xFF bytes (a NaN as fp16 and as fp32) — data
// that a correct kernel never lets into a result.  Not the arrival counters of the key split (they must stay zero between launches), not
// the position words, not weights.
extern "C" int bsg_fs2midi_debug_poison_workspace(bsg_fs2midi* h, void* stream) {
  BSG_REQUIRE(h, "fs2midi_debug_poison_workspace: null handle");
  return ws_poison(ws_table(h), (hipStream_t)stream);
}

extern "C" int bsg_length_regulator(const int64_t* dur, const int64_t* txt, int64_t* mel2ph, int32_t B, int32_t Tt, int32_t T,
                                    void* stream) {
  BSG_REQUIRE(dur && mel2ph, "length_regulator: null %s", dur ? "mel2ph" : "dur");
  BSG_REQUIRE(B > 0 && Tt > 0 && T > 0, "length_regulator: B=%d T_txt=%d T=%d (each must be positive)", B, Tt, T);
  BSG_REQUIRE(Tt <= 8192, "length_regulator: T_txt=%d (at most 8192: the running sums of an utterance live in 64 KiB of LDS)", Tt);
  hipLaunchKernelGGL(length_regulator_kernel, dim3(B), dim3(256), Tt * sizeof(long long), (hipStream_t)stream,
                     (const long long*)dur, (const long long*)txt, (long long*)mel2ph, Tt, T);
  BSG_LAUNCH_CHECK();
  return BSG_OK;
}

// The pitch adaptor in front of the decoder: scan + entry (positions), per predictor layer the k-tap convolution as a K-segmented GEMM with
// bias + ReLU in its epilogue and (but for the last layer) a LayerNorm launch — NO mask between the layers (tts_modules.py:233-234: padded
// frames carry bias-driven values into the last real frames through the taps) — and pitch_tail_kernel.
static int pitch_adaptor(bsg_fs2midi* h, const float* enc_out, const int64_t* mel2ph, const int64_t* spk_id, const int64_t* speechsing,
                         const float* f0, const float* uv, int32_t B, int32_t Tt, int32_t T, float* pitch_pred, float* f0_denorm,
                         int64_t* pitch_bin, float* decoder_inp, hipStream_t st, const int* lens_f, const int* lens_t) {
  // lens_f / lens_t (ragged calls; null = padded): the utterances' frame and token counts.  With them the predictor's convolutions read zeros
  // beyond an utterance's end in EVERY layer (the utterance alone), and nothing is computed there.
  const long long rows = (long long)B * T;
  const dim3 rg(cdiv(rows, 4)), rb(256);
  float *cur = h->w_a, *cv = h->w_b;
  int n_launch = 0;   // counted where each launch is made: the record's last token
  hipLaunchKernelGGL(pitch_positions_kernel, dim3(B), dim3(64), 0, st, enc_out, (const long long*)mel2ph, (const long long*)spk_id, h->Espk,
                     h->w_pos, T, Tt, h->cfg.spk_rows, lens_f, lens_t);
  BSG_LAUNCH_CHECK();
  path_add(h, "pit.", "pos");
  ++n_launch;
  hipLaunchKernelGGL(pitch_entry_kernel, rg, rb, 0, st, enc_out, (const long long*)mel2ph, (const long long*)spk_id, h->Espk,
                     (const int*)h->w_pos, h->pit_table, h->pit_alpha, cur, rows, T, Tt, h->n_pitch_pos, h->cfg.spk_rows, lens_f, lens_t);
  BSG_LAUNCH_CHECK();
  path_add(h, "pit.", "entry");
  ++n_launch;
  const int ks = h->pitch_kernel, L = h->pitch_layers;
  for (int l = 0; l < L; ++l) {
    GemmArgs g{};
    g.A = cur; g.B = h->pit_conv[l]; g.C = cv; g.M = T; g.N = H; g.K = H; g.lda = H; g.ldb = H; g.ldc = H; g.trans_b = 1;
    g.taps = ks; g.tap_shift0 = -(ks / 2); g.sTapB = (long long)H * H; g.bias_n = h->pit_convb[l]; g.alpha = 1.f;
    g.act = ACT_RELU; g.batch = B; g.sA = (long long)T * H; g.sC = (long long)T * H; g.lens = lens_f;
    TRY(gemm_rec(h, "pit.gemm:", g, st));
    ++n_launch;
    if (l + 1 < L) {
      TRY(ln(cv, h->pit_lnw[l], h->pit_lnb[l], cur, nullptr, rows, 1e-12f, st, lens_f, T));
      path_add(h, "pit.", "ln");
      ++n_launch;
    }
  }
  hipLaunchKernelGGL(pitch_tail_kernel, rg, rb, 0, st, (const float*)cv, h->pit_lnw[L - 1], h->pit_lnb[L - 1], h->pit_lin_w, h->pit_lin_b, f0, uv,
                     h->use_uv, enc_out, (const long long*)mel2ph, (const long long*)spk_id, (const long long*)speechsing, h->Espk, h->Estyle,
                     h->Epitch, pitch_pred, f0_denorm, (long long*)pitch_bin, decoder_inp, rows, T, Tt, h->cfg.spk_rows, lens_f, lens_t);
  BSG_LAUNCH_CHECK();
  path_add(h, "pit.", "tail");
  ++n_launch;
  path_add(h, "pit.launches:", std::to_string(n_launch).c_str());
  return BSG_OK;
}

static int decode_impl(bsg_fs2midi* h, const char* who, const float* enc_out, const int64_t* mel2ph, const int64_t* spk_id,
                       const int64_t* speechsing, const float* f0, const float* uv, int32_t B, int32_t Tt, int32_t T, float* pitch_pred,
                       float* f0_denorm, int64_t* pitch_bin, float* decoder_inp, float* mel_out, hipStream_t st,
                       const int32_t* n_tok_host = nullptr, const int32_t* n_frames_host = nullptr, bool ragged = false) {
  BSG_REQUIRE(h && enc_out && mel2ph && decoder_inp, "%s: null argument", who);
  BSG_REQUIRE((spk_id != nullptr) == (h->Espk != nullptr), "%s: spk_id goes with a speaker table (spk_rows=%d)", who, h->cfg.spk_rows);
  BSG_REQUIRE((speechsing != nullptr) == (h->front == BSG_FS2_FRONT_MIDI), "%s: speechsing goes with the MIDI front", who);
  BSG_REQUIRE(B > 0 && Tt > 0 && T > 0 && T < h->cfg.n_pos, "%s: B=%d T_txt=%d T=%d (position table has %d rows)", who, B, Tt, T, h->cfg.n_pos);
  BSG_REQUIRE(h->use_pitch || (!f0 && !uv && !pitch_pred && !f0_denorm && !pitch_bin), "%s: f0 / uv / pitch outputs on a handle without use_pitch_embed", who);
  BSG_REQUIRE(!h->use_pitch || T < h->n_pitch_pos, "%s: T=%d (pitch position table has %d rows)", who, T, h->n_pitch_pos);
  if (ragged) {   // every refusal before any device call
    BSG_REQUIRE(B <= 65535, "%s: B=%d", who, B);
    TRY(rag_check(who, "n_tok_host", n_tok_host, B, 1, Tt));
    TRY(rag_check(who, "n_frames_host", n_frames_host, B, 0, T));
    if (mel_out) TRY(rag_plan_check(h, who, B, T, h->cfg.dec_ffn_kernel_size));
  }
  h->path.resize(h->path_enc_len);   // the record keeps the encode this decode follows
  const long long rows = (long long)B * T;
  TRY(grow(h, &h->cap_rows, (size_t)rows, st));
  const int *lens_f = nullptr, *lens_t = nullptr;
  if (ragged) {
    TRY(grow(h, &h->cap_lens, (size_t)B, st));
    TRY(lens_fill(h->w_lens_t, n_tok_host, B, st));
    TRY(lens_fill(h->w_lens_f, n_frames_host, B, st));
    lens_f = h->w_lens_f; lens_t = h->w_lens_t;
    path_add(h, "dec.", "ragged");
  }
  const dim3 rg(cdiv(rows, 4)), rb(256);
  if (h->use_pitch) {
    TRY(pitch_adaptor(h, enc_out, mel2ph, spk_id, speechsing, f0, uv, B, Tt, T, pitch_pred, f0_denorm, pitch_bin, decoder_inp, st, lens_f, lens_t));
  } else {
    hipLaunchKernelGGL(gather_frames_kernel, rg, rb, 0, st, enc_out, (const long long*)mel2ph, (const long long*)spk_id,
                       (const long long*)speechsing, h->Espk, h->Estyle, decoder_inp, rows, T, Tt, lens_f, lens_t);
    BSG_LAUNCH_CHECK();
  }
  if (!mel_out) return BSG_OK;   // skip_decoder
  float* x = h->w_x;
  BSG_HIP(hipMemcpyAsync(x, decoder_inp, rows * H * sizeof(float), hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(decoder_positions_kernel, dim3(B), dim3(64), 0, st, (const float*)x, h->w_pos, h->w_keep, T, lens_f);
  BSG_LAUNCH_CHECK();
  hipLaunchKernelGGL(decoder_entry_kernel, rg, rb, 0, st, x, (const int*)h->w_pos, h->dec_table, h->dec_alpha, h->w_keep, rows, h->cfg.n_pos, lens_f, T);
  BSG_LAUNCH_CHECK();
  TRY(launch_fft(h, h->dec, h->dec_lnw, h->dec_lnb, h->cfg.dec_ffn_kernel_size, x, h->w_keep, B, T, st, "dec.", lens_f));
  if (ragged) h->last_stack_rows = rag_rows(n_frames_host, B, T);
  // mel_out = Linear(H -> M)(x) * (mel2ph > 0)                                        (fastspeech/fs2.py:236-240)
  TRY(linear(x, h->mel_w, h->mel_b, mel_out, rows, h->cfg.out_dims, H, ACT_NONE, nullptr, nullptr, st, 1.f, 0, nullptr, "", lens_f, T));
  // ... * tgt_nonpadding, which comes from mel2ph (not from the decoder's own |x| test)
  hipLaunchKernelGGL(mask_rows_by_index_kernel, dim3(cdiv(rows * h->cfg.out_dims, 256)), dim3(256), 0, st, mel_out,
                     (const long long*)mel2ph, rows, h->cfg.out_dims, lens_f, T);
  BSG_LAUNCH_CHECK();
  return BSG_OK;
}

extern "C" int bsg_fs2midi_decode(bsg_fs2midi* h, const float* enc_out, const int64_t* mel2ph, const int64_t* spk_id,
                                  const int64_t* speechsing, int32_t B, int32_t Tt, int32_t T, float* decoder_inp,
                                  float* mel_out, void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  // (spk_id / speechsing: required on a MIDI handle, NULL where a plain-front handle has no such table — decode_impl says which)
  return decode_impl(h, "fs2midi_decode", enc_out, mel2ph, spk_id, speechsing, nullptr, nullptr, B, Tt, T, nullptr, nullptr, nullptr, decoder_inp,
                     mel_out, (hipStream_t)stream);
}

extern "C" int bsg_fs2midi_token_rows(bsg_fs2midi* h, const float* enc_out, const int64_t* spk_id, const int64_t* speechsing, int32_t B,
                                      int32_t Tt, float* cond_tok, void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  BSG_REQUIRE(h && enc_out && cond_tok, "fs2midi_token_rows: null argument");
  BSG_REQUIRE(!h->use_pitch, "fs2midi_token_rows: with a frame-level pitch embedding the condition is per frame");
  BSG_REQUIRE((spk_id != nullptr) == (h->Espk != nullptr), "fs2midi_token_rows: spk_id goes with a speaker table (spk_rows=%d)", h->cfg.spk_rows);
  BSG_REQUIRE((speechsing != nullptr) == (h->front == BSG_FS2_FRONT_MIDI), "fs2midi_token_rows: speechsing goes with the MIDI front");
  BSG_REQUIRE(B > 0 && Tt > 0, "fs2midi_token_rows: B=%d T_txt=%d", B, Tt);
  const long long rows = (long long)B * (Tt + 1);
  hipLaunchKernelGGL(token_rows_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, enc_out, (const long long*)spk_id,
                     (const long long*)speechsing, h->Espk, h->Estyle, cond_tok, rows, Tt);
  BSG_LAUNCH_CHECK();
  return BSG_OK;
}

extern "C" int bsg_fs2_decode(bsg_fs2midi* h, const float* enc_out, const int64_t* mel2ph, const int64_t* spk_id, const int64_t* speechsing,
                              const float* f0, const float* uv, int32_t B, int32_t Tt, int32_t T, float* pitch_pred, float* f0_denorm,
                              int64_t* pitch_bin, float* decoder_inp, float* mel_out, void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  return decode_impl(h, "fs2_decode", enc_out, mel2ph, spk_id, speechsing, f0, uv, B, Tt, T, pitch_pred, f0_denorm, pitch_bin, decoder_inp, mel_out,
                     (hipStream_t)stream);
}

// ABI v20: bsg_fs2_decode on a ragged batch.  Utterance b has n_tok_host[b] tokens and n_frames_host[b] frames; serves handles without the
// adaptor too (the five adaptor pointers NULL), and both fronts.
extern "C" int bsg_fs2_decode_ragged(bsg_fs2midi* h, const float* enc_out, const int64_t* mel2ph, const int64_t* spk_id, const int64_t* speechsing,
                                     const float* f0, const float* uv, const int32_t* n_tok_host, const int32_t* n_frames_host, int32_t B,
                                     int32_t Tt, int32_t T, float* pitch_pred, float* f0_denorm, int64_t* pitch_bin, float* decoder_inp,
                                     float* mel_out, void* stream) {
  GuardScope guard_scope(h ? &h->guard : nullptr);
  return decode_impl(h, "fs2_decode_ragged", enc_out, mel2ph, spk_id, speechsing, f0, uv, B, Tt, T, pitch_pred, f0_denorm, pitch_bin, decoder_inp,
                     mel_out, (hipStream_t)stream, n_tok_host, n_frames_host, true);
}

// ================================================================================================
// the `FFT` candidate denoiser (DIFF_DECODERS['fft'], usr/diff/candidate_decoder.py:39-100):
// input projection -> concat[x, cond, step embedding] -> Linear(3C -> H) -> FastspeechDecoder stack -> Linear(H -> M).
// The concat-Linear is split by columns: the cond part is step-invariant (hoisted to prepare), the step part is one
// vector per utterance, so per call only x * W_x^T runs over all frames.  Reuses launch_fft() of the FS2 decoder.
// ================================================================================================
namespace bsg {
namespace {
// in [B][R][Cc] -> out [B][Cc][R]
__global__ void transpose_brc_kernel(const float* __restrict__ in, float* __restrict__ out, int R, int Cc) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: 32 x 8
  for (int j = ty; j < 32; j += 8) {
    const int r = r0 + j, c = c0 + tx;
    tile[j][tx] = (r < R && c < Cc) ? in[((long long)b * R + r) * Cc + c] : 0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int c = c0 + j, r = r0 + tx;
    if (c < Cc && r < R) out[((long long)b * Cc + c) * R + r] = tile[tx][j];
  }
}
__global__ void gather_rows_kernel(const float* __restrict__ table, const long long* __restrict__ idx, float* __restrict__ out, int n,
                                   int width, int n_rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * width) return;
  long long r = idx[i / width];
  r = r < 0 ? 0 : (r >= n_rows ? n_rows - 1 : r);
  out[i] = table[r * width + (i % width)];
}

// Ragged forms of the two layout changes (bsg_fftden_prepare_ragged): row b has lens[b] frames, the pitch of every tensor stays T.
// in [B][R][T] -> out [B][T][R] on the frames < lens[b]: nothing at or beyond a row's end is read or written, and a tile that lies
// beyond it returns before its first load.  Grid as transpose_brc_kernel(in, out, R, T).
__global__ void transpose_in_rag_kernel(const float* __restrict__ in, float* __restrict__ out, int R, int T, const int* __restrict__ lens) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, r0 = blockIdx.y * 32, c0 = blockIdx.x * 32, nb = lens[b];
  if (c0 >= nb) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: 32 x 8
  for (int j = ty; j < 32; j += 8) {
    const int r = r0 + j, c = c0 + tx;
    tile[j][tx] = (r < R && c < nb) ? in[((long long)b * R + r) * T + c] : 0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int c = c0 + j, r = r0 + tx;
    if (c < nb && r < R) out[((long long)b * T + c) * R + r] = tile[tx][j];
  }
}
// in [B][T][Cc] -> out [B][Cc][T]: the frames < lens[b] transposed, the frames from there to T written as 0 without a read.
// Grid as transpose_brc_kernel(in, out, T, Cc).
__global__ void transpose_out_rag_kernel(const float* __restrict__ in, float* __restrict__ out, int T, int Cc, const int* __restrict__ lens) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, r0 = blockIdx.y * 32, c0 = blockIdx.x * 32, nb = lens[b];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int j = ty; j < 32; j += 8) {
    const int r = r0 + j, c = c0 + tx;
    tile[j][tx] = (r < nb && c < Cc) ? in[((long long)b * T + r) * Cc + c] : 0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int c = c0 + j, r = r0 + tx;
    if (c < Cc && r < T) out[((long long)b * Cc + c) * T + r] = tile[tx][j];
  }
}

// ------------------------------------------------------------------------------------------------
// The sampler step's tail of the FFT denoiser, one launch (bsg_fftden_ddpm_sample / bsg_fftden_plms_sample): for a tile of 64 frames
// of one row
//   eps  = get_mel_out(xs)                 Linear(256 -> M) on the stack's output rows                       (candidate_decoder.py:98)
//   x   <- p_sample(x, eps, noise)         the arithmetic of ddpm_step_kernel                   (shallow_diffusion_tts.py:149-166)
//   or   p_sample_plms(x, eps, history)    plms_update, eps stored to the history slot as well                         (:168-201)
// in place of the Linear launch, the [B][T][M] -> [B][M][T] transpose, the draws' launch and the generic step launch.
// Lanes run along the frames, so x, the noise and the history are read and written as 256-byte rows of [B][M][T] and the product needs
// no transpose: the tile of xs goes through LDS in four 64-column pieces (row pitch 65 floats: a column read is conflict free), wave w
// keeps the M / 4 mel rows w, w + 4, .. of its 64 frames in registers, and the weight row of a mel bin is the same for a whole wave (scalar
// loads).  Every sum is one fmaf chain in ascending k, in registers, whatever the grid: the same call gives the same bits.  The product
// is on the vector pipe: 41 kFLOP per frame against 23 MFLOP per frame in the stack, and the fp32 matrix pipe has the same rate.
// Ragged: a tile beyond its row's end returns before its first load, and the frames beyond it inside a tile are neither read nor written.
// ------------------------------------------------------------------------------------------------
constexpr int FT_F = 64, FT_KC = 64, FT_MJ = 20;   // frames per tile; staged columns per piece; mel rows per wave (M <= 4 FT_MJ)
enum { FT_DDPM = 0, FT_PLMS = 1, FT_PLMS_CORRECT = 2 };
struct FftTailArgs {
  const float* xs;      // [B][T][H]: the stack's output
  const float* w;       // get_mel_out.weight [M][H]
  const float* bias;    // [M]
  const float* x_in;    // [B][M][T]
  float* x_out;         // [B][M][T] (may be x_in)
  const int* lens;      // device, one frame count per row; null: every row has T frames
  int T, M, mode;
  // FT_DDPM
  const float* noise;   // [B][M][T] supplied draws, or null: Philox
  const unsigned long long* row_seeds;   // device [B]: row b draws element m n_b + f of the stream (row_seeds[b], stream); null: (seed, stream) at elem0 + flat index
  unsigned long long seed, elem0;
  unsigned stream;
  StepCoef k;
  // FT_PLMS: eps -> e_new (if set), x_out = plms_update(x_in, eps, h1, h2, h3).  FT_PLMS_CORRECT (the first iteration's second evaluation):
  // x_out = plms_update(x_in, h1, eps) with the average's weights, eps is not kept
  int n_hist;
  PlmsCoef pk;
  float* e_new;
  const float *h1, *h2, *h3;
};
template <int MODE>   // FT_DDPM / FT_PLMS / FT_PLMS_CORRECT: one update per instantiation, so that the epilogue holds one of the three
__global__ __launch_bounds__(256) void fftden_tail_kernel(FftTailArgs a) {
  __shared__ float tile[FT_F][FT_KC + 1];
  const int b = blockIdx.y, f0 = blockIdx.x * FT_F;
  const int nb = a.lens ? a.lens[b] : a.T;
  if (f0 >= nb) return;
  const int live = nb - f0 < FT_F ? nb - f0 : FT_F;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float acc[FT_MJ];
#pragma unroll
  for (int j = 0; j < FT_MJ; ++j) acc[j] = 0.f;
  const float* xs = a.xs + ((long long)b * a.T + f0) * H;
  for (int kc = 0; kc < H; kc += FT_KC) {
    if (kc) __syncthreads();
#pragma unroll
    for (int i = 0; i < FT_F * FT_KC / 4 / 256; ++i) {
      const int idx = (int)threadIdx.x + i * 256, fr = idx / (FT_KC / 4), q = idx % (FT_KC / 4);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (fr < live) v = *reinterpret_cast<const f32x4*>(xs + (long long)fr * H + kc + q * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) tile[fr][q * 4 + e] = v[e];
    }
    __syncthreads();
#pragma unroll 1
    for (int k4 = 0; k4 < FT_KC; k4 += 4) {   // four columns at a time: 20 weight quads fit the scalar registers
      float av[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) av[e] = tile[lane][k4 + e];
#pragma unroll
      for (int j = 0; j < FT_MJ; ++j) {
        const int m = wave + 4 * j < a.M ? wave + 4 * j : a.M - 1;   // (a row beyond M repeats the last one; its sum is not stored)
        const float* wr = a.w + (long long)m * H + kc + k4;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j] = fmaf(av[e], wr[e], acc[j]);
      }
    }
  }
  if (lane >= live) return;
  const int f = f0 + lane;
#pragma unroll
  for (int j = 0; j < FT_MJ; ++j) {
    const int m = wave + 4 * j;
    if (m >= a.M) break;
    const float eps = acc[j] + a.bias[m];
    const long long idx = ((long long)b * a.M + m) * a.T + f;
    const float xv = a.x_in[idx];
    if constexpr (MODE == FT_DDPM) {
      float nz = 0.f;
      if (a.noise) nz = a.noise[idx];
      else if (a.k.sigma != 0.f)
        nz = a.row_seeds ? philox_normal1(a.row_seeds[b], a.stream, (unsigned long long)m * nb + f) : philox_normal1(a.seed, a.stream, a.elem0 + (unsigned long long)idx);
      // every product / sum rounded separately, as ddpm_step_kernel
      float x0 = __fsub_rn(__fmul_rn(a.k.recip, xv), __fmul_rn(a.k.recipm1, eps));
      x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
      const float mean = __fadd_rn(__fmul_rn(a.k.pc1, x0), __fmul_rn(a.k.pc2, xv));
      a.x_out[idx] = __fadd_rn(mean, __fmul_rn(a.k.sigma, nz));
    } else if constexpr (MODE == FT_PLMS_CORRECT) {
      a.x_out[idx] = plms_update(xv, a.h1[idx], eps, 0.f, 0.f, 1, a.pk, nullptr);
    } else {
      if (a.e_new) a.e_new[idx] = eps;
      const float e1 = a.n_hist >= 1 ? a.h1[idx] : 0.f, e2 = a.n_hist >= 2 ? a.h2[idx] : 0.f, e3 = a.n_hist >= 3 ? a.h3[idx] : 0.f;
      a.x_out[idx] = plms_update(xv, eps, e1, e2, e3, a.n_hist, a.pk, nullptr);
    }
  }
}
}  // namespace
}  // namespace bsg

struct bsg_fftden {
  bsg_fs2midi* core = nullptr;   // owns weights + the FFT-stack workspaces
  int M = 0, S = 0, n_pos = 0, ksz = 9;
  std::vector<FftLayerW> layers;
  float *alpha, *lnw, *lnb, *in_w, *in_b, *mel_w, *mel_b, *gdi_w, *gdi_b, *dtab;
  size_t cap = 0;   // rows (B x T) of the per-call buffers below
  int B = 0, T = 0;
  float *condpart = nullptr, *xT = nullptr, *xp = nullptr, *te = nullptr, *tvec = nullptr, *mel = nullptr;
  // ragged binding (bsg_fftden_prepare_ragged): the rows' frame counts on the device, filled by the binding call itself (lens_fill), and
  // once more on the host (the rows a ragged stack computes; what the row-keyed draws need to be multiples of 4)
  bool ragged = false;
  size_t cap_lens = 0;   // rows (B) of lens / seeds
  int* lens = nullptr;
  unsigned long long* seeds = nullptr;   // bsg_fftden_ddpm_sample with seeds_host: the rows' Philox keys, filled by the call itself
  std::vector<int32_t> lens_host;
  // sampler entries: the step part of the concat-Linear for every timestep [S][H] (every row of a sampler call shares t), and the PLMS
  // history with the predictor's x
  float* tvtab = nullptr;
  size_t cap_smp = 0;    // rows (B x T) of hist / xpred
  float *hist[4] = {nullptr, nullptr, nullptr, nullptr}, *xpred = nullptr;
};

// the handle's own per-call buffers (the FFT stack's are the core's).  `condpart` is not poisoned: bsg_fftden_prepare's result is an input
// of every forward, and so are the lengths of a ragged binding.  te: [B][H] used; rows >= B for any later (B,T) that fits
static std::vector<WsBuf> ws_table(bsg_fftden* h) {
  const size_t f = sizeof(float);
  static const char* const smp_lazy = "fftden_plms_sample: the history buffers have to grow for this shape, which a capturing stream cannot do; run the shape once eagerly before capturing";
  static const char* const seeds_lazy = "fftden_ddpm_sample: the rows' seeds need a buffer of this batch size, which a capturing stream cannot allocate; run the shape once eagerly before capturing";
  return {
      {&h->cap, (void**)&h->condpart, H * f},          {&h->cap, (void**)&h->xT, H * f, 0, WS_POISON},   {&h->cap, (void**)&h->xp, H * f, 0, WS_POISON},
      {&h->cap, (void**)&h->te, H * f, 0, WS_POISON},  {&h->cap, (void**)&h->tvec, H * f, 0, WS_POISON}, {&h->cap, (void**)&h->mel, h->M * f, 0, WS_POISON},
      {&h->cap_lens, (void**)&h->lens, sizeof(int), 0, 0, seeds_lazy}, {&h->cap_lens, (void**)&h->seeds, sizeof(unsigned long long), 0, 0, seeds_lazy},
      {&h->cap_smp, (void**)&h->hist[0], h->M * f, 0, WS_POISON, smp_lazy}, {&h->cap_smp, (void**)&h->hist[1], h->M * f, 0, WS_POISON, smp_lazy},
      {&h->cap_smp, (void**)&h->hist[2], h->M * f, 0, WS_POISON, smp_lazy}, {&h->cap_smp, (void**)&h->hist[3], h->M * f, 0, WS_POISON, smp_lazy},
      {&h->cap_smp, (void**)&h->xpred, h->M * f, 0, WS_POISON, smp_lazy},
  };
}

extern "C" void bsg_fftden_destroy(bsg_fftden* h) {
  if (!h) return;
  ws_free(ws_table(h));
  for (FftLayerW& L : h->layers) { h2w_free(&L.p_in); h2w_free(&L.p_out); h2w_free(&L.p_ffn1); h2w_free(&L.p_ffn2); }
  bsg_fs2midi_destroy(h->core);
  delete h;
}

extern "C" int bsg_fftden_n_weights(int32_t n_layers) { return 2 + 10 * n_layers + 2 + 2 + 4 + 2 + 2; }

// FFT.state_dict(): pos_embed_alpha, embed_positions._float_tensor, layers.*, layer_norm.{w,b}, input_projection.{w,b},
// mlp.0.{w,b}, mlp.2.{w,b}, get_mel_out.{w,b}, get_decode_inp.{w,b}
static int fftden_load(bsg_fftden* h, int n_layers, const void* const* w, const float* step_table, const float* pos_table, hipStream_t st) {
  bsg_fs2midi* c = h->core;
  const int M = h->M;
  int i = 0;
  TRY(guard_init(&c->guard, st));
  GuardScope guard_scope(&c->guard);
  TRY(fs2_copy(c, &h->alpha, w[i++], 1, st));
  i++;
  TRY(load_fft_layers(c, h->layers, w + i, n_layers, h->ksz, st));
  i += 10 * n_layers;
  TRY(fs2_copy(c, &h->lnw, w[i++], H, st));
  TRY(fs2_copy(c, &h->lnb, w[i++], H, st));
  TRY(fs2_copy(c, &h->in_w, w[i++], (size_t)H * M, st));
  TRY(fs2_copy(c, &h->in_b, w[i++], H, st));
  const float *m0w = (const float*)w[i], *m0b = (const float*)w[i + 1], *m2w = (const float*)w[i + 2], *m2b = (const float*)w[i + 3];
  i += 4;
  TRY(fs2_copy(c, &h->mel_w, w[i++], (size_t)M * H, st));
  TRY(fs2_copy(c, &h->mel_b, w[i++], M, st));
  TRY(fs2_copy(c, &h->gdi_w, w[i++], (size_t)H * 3 * H, st));
  TRY(fs2_copy(c, &h->gdi_b, w[i++], H, st));
  // step-embedding MLP tabulated for every timestep (candidate_decoder.py:60-62)
  float* hid = nullptr;
  TRY(own_alloc(c->owned, &hid, (size_t)h->S * 4 * H));
  TRY(own_alloc(c->owned, &h->dtab, (size_t)h->S * H));
  TRY(linear(step_table, m0w, m0b, hid, h->S, 4 * H, H, ACT_MISH, nullptr, nullptr, st));
  TRY(linear(hid, m2w, m2b, h->dtab, h->S, H, 4 * H, ACT_NONE, nullptr, nullptr, st));
  // ... and its part of the concat-Linear with the bias (:63-70), for the sampler entries: one row per timestep
  TRY(own_alloc(c->owned, &h->tvtab, (size_t)h->S * H));
  {
    GemmArgs g{};
    g.A = h->dtab; g.B = h->gdi_w + 2 * H; g.C = h->tvtab; g.M = h->S; g.N = H; g.K = H; g.lda = H; g.ldb = 3 * H; g.ldc = H; g.trans_b = 1;
    g.taps = 1; g.bias_n = h->gdi_b; g.alpha = 1.f; g.batch = 1;
    TRY(launch_gemm(g, st));
  }
  return create_tail(c, pos_table, nullptr, nullptr, st);   // the frame position table: c->dec_table
}

extern "C" int bsg_fftden_create(bsg_fftden** out, int32_t in_dims, int32_t n_layers, int32_t num_heads, int32_t ffn_kernel,
                                 int32_t max_steps, int32_t n_pos, const void* const* w, int32_t n_weights, const float* step_table,
                                 const float* pos_table, void* stream) {
  BSG_REQUIRE(out && w && step_table && pos_table, "fftden_create: null argument");
  BSG_REQUIRE(in_dims > 0 && in_dims % 4 == 0 && n_layers > 0 && num_heads > 0 && H % num_heads == 0 && (H / num_heads) % 4 == 0 &&
                  ffn_kernel % 2 == 1 && max_steps > 0 && n_pos > 1, "fftden_create: bad config");
  BSG_REQUIRE(n_weights == bsg_fftden_n_weights(n_layers), "fftden_create: expected %d weight tensors, got %d", bsg_fftden_n_weights(n_layers), n_weights);
  for (int i = 0; i < n_weights; ++i) BSG_REQUIRE(w[i] != nullptr, "fftden_create: weight %d is null", i);
  bsg_fftden* h = new bsg_fftden();
  h->core = new bsg_fs2midi();
  h->core->cfg = bsg_fs2midi_cfg{};
  h->core->cfg.num_heads = num_heads;
  h->core->cfg.dec_ffn_kernel_size = ffn_kernel;   // (create_tail reads these two)
  h->core->cfg.n_pos = n_pos;
  h->M = in_dims; h->S = max_steps; h->n_pos = n_pos; h->ksz = ffn_kernel;
  const int rc = fftden_load(h, n_layers, w, step_table, pos_table, (hipStream_t)stream);
  if (rc != BSG_OK) {
    bsg_fftden_destroy(h);
    return rc;
  }
  *out = h;
  return BSG_OK;
}

extern "C" int bsg_fftden_prepare(bsg_fftden* h, const float* cond, int32_t B, int32_t T, void* stream) {
  GuardScope guard_scope(h && h->core ? &h->core->guard : nullptr);
  BSG_REQUIRE(h && cond && B > 0 && T > 0 && T < h->n_pos, "fftden_prepare: bad argument (T=%d)", T);
  hipStream_t st = (hipStream_t)stream;
  const size_t rows = (size_t)B * T;
  if (rows > h->cap) TRY(ws_grow(ws_table(h), "fftden", &h->cap, rows, st));
  TRY(grow(h->core, &h->core->cap_rows, rows, st));
  h->B = B; h->T = T; h->ragged = false;
  // cond [B][H][T] -> [B*T][H]; condpart = cond_t * W[:, C:2C]^T                           (candidate_decoder.py:63-70)
  hipLaunchKernelGGL(transpose_brc_kernel, dim3(cdiv(T, 32), cdiv(H, 32), B), dim3(256), 0, st, cond, h->xT, H, T);
  BSG_LAUNCH_CHECK();
  GemmArgs g{};
  g.A = h->xT; g.B = h->gdi_w + H; g.C = h->condpart; g.M = (int)rows; g.N = H; g.K = H; g.lda = H; g.ldb = 3 * H; g.ldc = H;
  g.trans_b = 1; g.taps = 1; g.alpha = 1.f; g.batch = 1;
  return launch_gemm(g, st);
}

// ABI v22 (addition): bsg_fftden_prepare for a ragged batch.  Row b has lengths_host[b] frames; the calls that follow on the handle decode
// it as the B = 1 call on those frames alone.  The counts are read and checked before the first device call and reach the kernels through the
// handle's own device row, which launches of this call fill (lens_fill).  condpart is projected on the live frames only.
extern "C" int bsg_fftden_prepare_ragged(bsg_fftden* h, const float* cond, const int32_t* lengths_host, int32_t B, int32_t T, void* stream) {
  GuardScope guard_scope(h && h->core ? &h->core->guard : nullptr);
  TRY(lens_check(lengths_host, B, T, "fftden_prepare_ragged"));
  BSG_REQUIRE(h && cond, "fftden_prepare_ragged: null %s", h ? "cond" : "handle");
  BSG_REQUIRE(T < h->n_pos, "fftden_prepare_ragged: bad argument (T=%d, position table has %d rows)", T, h->n_pos);
  hipStream_t st = (hipStream_t)stream;
  if (is_capturing(st)) {
    set_error("fftden_prepare_ragged: a ragged batch cannot be bound under stream capture");
    return BSG_ESTATE;
  }
  TRY(rag_plan_check(h->core, "fftden_prepare_ragged", B, T, h->ksz));
  const size_t rows = (size_t)B * T;
  if (rows > h->cap) TRY(ws_grow(ws_table(h), "fftden", &h->cap, rows, st));
  if ((size_t)B > h->cap_lens) TRY(ws_grow(ws_table(h), "fftden", &h->cap_lens, (size_t)B, st));
  TRY(grow(h->core, &h->core->cap_rows, rows, st));
  h->B = B; h->T = T; h->ragged = true;
  h->lens_host.assign(lengths_host, lengths_host + B);
  TRY(lens_fill(h->lens, lengths_host, B, st));
  hipLaunchKernelGGL(transpose_in_rag_kernel, dim3(cdiv(T, 32), cdiv(H, 32), B), dim3(256), 0, st, cond, h->xT, H, T, (const int*)h->lens);
  BSG_LAUNCH_CHECK();
  GemmArgs g{};   // one batch item per row, bounded by its length
  g.A = h->xT; g.B = h->gdi_w + H; g.C = h->condpart; g.M = T; g.N = H; g.K = H; g.lda = H; g.ldb = 3 * H; g.ldc = H;
  g.trans_b = 1; g.taps = 1; g.alpha = 1.f; g.batch = B; g.sA = (long long)T * H; g.sC = (long long)T * H; g.lens = h->lens;
  return launch_gemm(g, st);
}

// The denoiser up to the stack's last LayerNorm: the result [B*T][H] is left in the core's w_x.  `t`: one step per row, on the device
// (bsg_fftden_forward); null: every row at step t_all, its step vector read from the table of all steps (the sampler entries).  On a
// ragged binding every launch takes the rows' lengths; the padded call launches exactly what it did.
static int fftden_stack(bsg_fftden* h, const float* x, const int64_t* t, int t_all, int B, int T, hipStream_t st) {
  const long long rows = (long long)B * T;
  bsg_fs2midi* c = h->core;
  const int* lens = h->ragged ? h->lens : nullptr;
  c->path.clear();
  if (lens) path_add(c, "den.", "ragged");
  // x [B][M][T] -> [B*T][M]; xp = input_projection                                        (:57-58)
  if (lens) hipLaunchKernelGGL(transpose_in_rag_kernel, dim3(cdiv(T, 32), cdiv(h->M, 32), B), dim3(256), 0, st, x, h->xT, h->M, T, lens);
  else hipLaunchKernelGGL(transpose_brc_kernel, dim3(cdiv(T, 32), cdiv(h->M, 32), B), dim3(256), 0, st, x, h->xT, h->M, T);
  BSG_LAUNCH_CHECK();
  TRY(linear(h->xT, h->in_w, h->in_b, h->xp, rows, H, h->M, ACT_NONE, nullptr, nullptr, st, 1.f, 0, nullptr, "", lens, T));
  // step part: tvec[b] = mlp(emb(t_b)) * W[:, 2C:3C]^T + bias                               (:59-66)
  if (t) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3(cdiv(B * H, 256)), dim3(256), 0, st, (const float*)h->dtab, (const long long*)t, h->te, B, H, h->S);
    BSG_LAUNCH_CHECK();
    GemmArgs g{};
    g.A = h->te; g.B = h->gdi_w + 2 * H; g.C = h->tvec; g.M = B; g.N = H; g.K = H; g.lda = H; g.ldb = 3 * H; g.ldc = H; g.trans_b = 1;
    g.taps = 1; g.bias_n = h->gdi_b; g.alpha = 1.f; g.batch = 1;
    TRY(launch_gemm(g, st));
  }
  float* xs = c->w_x;
  {
    GemmArgs g{};   // decoder_inp = xp W_x^T + condpart + tvec[b]
    g.A = h->xp; g.B = h->gdi_w; g.C = xs; g.M = T; g.N = H; g.K = H; g.lda = H; g.ldb = 3 * H; g.ldc = H; g.trans_b = 1; g.taps = 1;
    g.bias_n = h->tvec; g.sBiasN = H; g.alpha = 1.f; g.R = h->condpart; g.ldr = H; g.sR = (long long)T * H; g.batch = B;
    g.sA = (long long)T * H; g.sC = (long long)T * H; g.lens = lens;
    if (!t) { g.bias_n = h->tvtab + (long long)t_all * H; g.sBiasN = 0; }
    TRY(launch_gemm(g, st));
  }
  const dim3 rg(cdiv(rows, 4)), rb(256);
  hipLaunchKernelGGL(decoder_positions_kernel, dim3(B), dim3(64), 0, st, (const float*)xs, c->w_pos, c->w_keep, T, lens);
  BSG_LAUNCH_CHECK();
  hipLaunchKernelGGL(decoder_entry_kernel, rg, rb, 0, st, xs, (const int*)c->w_pos, c->dec_table, h->alpha, c->w_keep, rows, h->n_pos, lens, T);
  BSG_LAUNCH_CHECK();
  TRY(launch_fft(c, h->layers, h->lnw, h->lnb, h->ksz, xs, c->w_keep, B, T, st, "den.", lens));
  if (lens) c->last_stack_rows = rag_rows(h->lens_host.data(), B, T);
  return BSG_OK;
}

extern "C" int bsg_fftden_forward(bsg_fftden* h, const float* x, const int64_t* t, float* eps, int32_t B, int32_t T, void* stream) {
  GuardScope guard_scope(h && h->core ? &h->core->guard : nullptr);
  BSG_REQUIRE(h && x && t && eps, "fftden_forward: null argument");
  BSG_REQUIRE(h->cap > 0 && h->B == B && h->T == T, "fftden_forward: (B=%d,T=%d) does not match bsg_fftden_prepare (B=%d,T=%d)", B, T, h->B, h->T);
  hipStream_t st = (hipStream_t)stream;
  const long long rows = (long long)B * T;
  TRY(fftden_stack(h, x, t, 0, B, T, st));
  const float* xs = h->core->w_x;
  if (h->ragged) {   // get_mel_out on the live frames; eps is written as 0 from a row's end to T
    TRY(linear(xs, h->mel_w, h->mel_b, h->mel, rows, h->M, H, ACT_NONE, nullptr, nullptr, st, 1.f, 0, nullptr, "", h->lens, T));
    hipLaunchKernelGGL(transpose_out_rag_kernel, dim3(cdiv(h->M, 32), cdiv(T, 32), B), dim3(256), 0, st, (const float*)h->mel, eps, T, h->M, (const int*)h->lens);
    BSG_LAUNCH_CHECK();
    return BSG_OK;
  }
  TRY(linear(xs, h->mel_w, h->mel_b, h->mel, rows, h->M, H, ACT_NONE, nullptr, nullptr, st));       // get_mel_out (:98)
  hipLaunchKernelGGL(transpose_brc_kernel, dim3(cdiv(h->M, 32), cdiv(T, 32), B), dim3(256), 0, st, (const float*)h->mel, eps, T, h->M);
  BSG_LAUNCH_CHECK();
  return BSG_OK;
}

// ---- the sampler loops over this denoiser (ABI v22, additions): every step enqueued on the stream, nothing waited for ------------------
// What both entries check before anything is enqueued; `plms`: which schedule arrays the loop reads.
static int fftden_sampler_enter(bsg_fftden* h, const bsg_schedule* s, const float* x, int B, int T, const char* who, bool plms) {
  BSG_REQUIRE(h, "%s: null handle", who);
  TRY(check_schedule(s, who, plms));
  BSG_REQUIRE(x, "%s: null x", who);
  BSG_REQUIRE(h->cap > 0 && h->B == B && h->T == T, "%s: (B=%d,T=%d) does not match the handle's binding (B=%d,T=%d)", who, B, T, h->B, h->T);
  BSG_REQUIRE(h->M <= 4 * FT_MJ, "%s: the fused step tail is built for up to %d mel bins (in_dims=%d)", who, 4 * FT_MJ, h->M);
  return BSG_OK;
}
// the step tail on the stack's output of the evaluation just enqueued
static int fftden_tail(bsg_fftden* h, FftTailArgs a, int B, int T, hipStream_t st) {
  a.xs = h->core->w_x; a.w = h->mel_w; a.bias = h->mel_b; a.lens = h->ragged ? h->lens : nullptr; a.T = T; a.M = h->M;
  const dim3 grid(cdiv(T, FT_F), B), block(256);
  if (a.mode == FT_DDPM) hipLaunchKernelGGL(fftden_tail_kernel<FT_DDPM>, grid, block, 0, st, a);
  else if (a.mode == FT_PLMS) hipLaunchKernelGGL(fftden_tail_kernel<FT_PLMS>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(fftden_tail_kernel<FT_PLMS_CORRECT>, grid, block, 0, st, a);
  BSG_LAUNCH_CHECK();
  return BSG_OK;
}

// bsg_ddpm_sample / bsg_ddpm_sample_rows over the FFT denoiser, on the handle's binding (padded or ragged).  Per step: the denoiser up to
// the stack's last LayerNorm, then ONE launch for get_mel_out, the draw and p_sample (fftden_tail_kernel).  Draws: `noise`
// [n_steps][B][M][T] · seeds_host (host, B keys): row b from the stream (seeds_host[b], i + 1) at its own bound length, the values of
// bsg_philox_normal_rows · neither: (seed, i + 1) by global row and padded stride (row0, B_total).  A ragged row's x beyond its end is
// left as given.
extern "C" int bsg_fftden_ddpm_sample(bsg_fftden* h, const bsg_schedule* s, float* x, const float* noise, uint64_t seed, const uint64_t* seeds_host,
                                      int32_t t_start, int32_t n_steps, int32_t B, int32_t T, int32_t row0, int32_t B_total, void* stream) {
  GuardScope guard_scope(h && h->core ? &h->core->guard : nullptr);
  const char* who = "fftden_ddpm_sample";
  TRY(fftden_sampler_enter(h, s, x, B, T, who, false));
  BSG_REQUIRE(!(noise && seeds_host), "%s: supplied noise and seeds_host exclude each other", who);
  BSG_REQUIRE(t_start < s->num_timesteps && t_start < h->S && n_steps >= 0 && t_start - n_steps + 1 >= 0,
              "%s: steps [%d..%d] outside the schedule (%d) / step table (%d)", who, t_start - n_steps + 1, t_start, s->num_timesteps, h->S);
  BSG_REQUIRE(row0 >= 0 && row0 + B <= B_total, "%s: rows [%d,%d) outside the global batch %d", who, row0, row0 + B, B_total);
  BSG_REQUIRE((long long)B * h->M * T % 4 == 0, "%s: B*M*T must be a multiple of 4", who);
  hipStream_t st = (hipStream_t)stream;
  if (seeds_host) {   // what bsg_philox_normal_rows would refuse is refused here, before a step is enqueued
    for (int b = 0; b < B; ++b) {
      const int nb = h->ragged ? h->lens_host[b] : T;
      BSG_REQUIRE((long long)h->M * nb % 4 == 0, "%s: row %d draws M * n = %d * %d values, no multiple of 4", who, b, h->M, nb);
    }
    // (a ragged binding sized the group for its B already: only a padded one grows it here)
    if ((size_t)B > h->cap_lens) TRY(ws_grow(ws_table(h), "fftden", &h->cap_lens, (size_t)B, st, GROW_LAZY));
    std::vector<int32_t> words(2 * (size_t)B);   // the keys as 32-bit words, low word first: the order the device reads a 64-bit value in
    for (int b = 0; b < B; ++b) {
      words[2 * b] = (int32_t)(uint32_t)(seeds_host[b] & 0xFFFFFFFFull);
      words[2 * b + 1] = (int32_t)(uint32_t)(seeds_host[b] >> 32);
    }
    TRY(lens_fill(reinterpret_cast<int*>(h->seeds), words.data(), 2 * B, st));
  }
  const long long n = (long long)B * h->M * T;
  for (int k = 0; k < n_steps; ++k) {
    const int i = t_start - k;
    TRY(fftden_stack(h, x, nullptr, i, B, T, st));
    FftTailArgs a{};
    a.mode = FT_DDPM; a.x_in = x; a.x_out = x;
    a.noise = noise ? noise + k * n : nullptr; a.row_seeds = seeds_host ? h->seeds : nullptr;
    a.seed = seed; a.elem0 = (unsigned long long)row0 * h->M * T; a.stream = (unsigned)(i + 1);
    a.k = StepCoef{s->sqrt_recip_alphas_cumprod[i], s->sqrt_recipm1_alphas_cumprod[i], s->posterior_mean_coef1[i], s->posterior_mean_coef2[i], s->sigma[i]};
    TRY(fftden_tail(h, a, B, T, st));
  }
  return BSG_OK;
}

// bsg_plms_sample over the FFT denoiser (p_sample_plms :168-201), on the handle's binding: the 4-deep history of the noise predictions
// lives in handle workspace; the first iteration is the predictor / corrector pair (two evaluations); t - interval clamps at 0.  Every
// evaluation ends in the one tail launch, which also stores eps to the history slot.
extern "C" int bsg_fftden_plms_sample(bsg_fftden* h, const bsg_schedule* s, float* x, int32_t K_step, int32_t interval, int32_t B, int32_t T,
                                      void* stream) {
  GuardScope guard_scope(h && h->core ? &h->core->guard : nullptr);
  const char* who = "fftden_plms_sample";
  TRY(fftden_sampler_enter(h, s, x, B, T, who, true));
  BSG_REQUIRE(interval > 0 && K_step > 0 && K_step <= s->num_timesteps && K_step <= h->S, "%s: K_step=%d interval=%d schedule=%d step table=%d", who,
              K_step, interval, s->num_timesteps, h->S);
  hipStream_t st = (hipStream_t)stream;
  const size_t rows = (size_t)B * T;
  if (rows > h->cap_smp) TRY(ws_grow(ws_table(h), "fftden", &h->cap_smp, rows, st, GROW_LAZY));
  float* hist[4] = {h->hist[0], h->hist[1], h->hist[2], h->hist[3]};   // ring: hist[0] = newest
  int n_hist = 0;
  const int last = ((K_step - 1) / interval) * interval;
  for (int i = last; i >= 0; i -= interval) {
    const int ip = i - interval > 0 ? i - interval : 0;
    FftTailArgs a{};
    a.pk.a_t = s->alphas_cumprod[i];
    a.pk.a_prev = s->alphas_cumprod[ip];
    float* e_new = hist[3];   // the slot about to be recycled
    TRY(fftden_stack(h, x, nullptr, i, B, T, st));
    a.mode = FT_PLMS; a.n_hist = n_hist; a.e_new = e_new; a.x_in = x; a.x_out = x;
    a.h1 = hist[0]; a.h2 = hist[1]; a.h3 = hist[2];
    plms_blend(n_hist, a.pk);
    if (n_hist == 0) {
      // predictor into xpred (a ragged row: its own frames only; the second evaluation reads no others), then the corrector on x
      a.x_out = h->xpred;
      TRY(fftden_tail(h, a, B, T, st));
      TRY(fftden_stack(h, h->xpred, nullptr, ip, B, T, st));
      a.mode = FT_PLMS_CORRECT; a.x_out = x; a.h1 = e_new; a.e_new = nullptr;
      a.pk.w0 = 1.f; a.pk.inv = 2.f;   // (eps + eps_prev) / 2
    }
    TRY(fftden_tail(h, a, B, T, st));
    hist[3] = hist[2]; hist[2] = hist[1]; hist[1] = hist[0]; hist[0] = e_new;
    if (n_hist < 3) ++n_hist;
  }
  return BSG_OK;
}

extern "C" const char* bsg_fftden_last_path(bsg_fftden* h) { return h && h->core && !h->core->path.empty() ? h->core->path.c_str() : "none"; }

// as bsg_fs2midi_debug_poison_workspace, plus this handle's own per-call buffers (not `condpart`: bsg_fftden_prepare's result is an input of
// every forward)
extern "C" int bsg_fftden_debug_poison_workspace(bsg_fftden* h, void* stream) {
  BSG_REQUIRE(h && h->core, "fftden_debug_poison_workspace: null handle");
  hipStream_t st = (hipStream_t)stream;
  TRY(ws_poison(ws_table(h->core), st));
  return ws_poison(ws_table(h), st);
}

namespace bsg {
Guard* guard_of_fs2midi(void* h) { return &static_cast<bsg_fs2midi*>(h)->guard; }
Guard* guard_of_fftden(void* h) { return &static_cast<bsg_fftden*>(h)->core->guard; }
}
