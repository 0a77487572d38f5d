// The Parallel WaveGAN generator (modules/parallel_wavegan/models/parallel_wavegan.py:135-168, layers/residual_block.py:91-129,
// layers/upsample.py) on gfx950: `vocoder: pwg`.
//
// One residual layer is ONE launch (pwg_layer_kernel).  For one batch row and a run of samples t, with d the layer's dilation:
//   y[g][t] = b[g] + sum_tap sum_ci W[g][ci][tap] x[ci][t + (tap - 1) d] + sum_ch Wa[g][ch] c[ch][t]        g < 128   (x is zero outside the row)
//   z[k][t] = tanh(y[k][t]) sigmoid(y[64 + k][t])                                                             k < 64
//   x'[r][t] = (bo[r] + sum_k Wo[r][k] z[k][t] + x[r][t]) sqrt(1/2);   skip[r][t] += bs[r] + sum_k Ws[r][k] z[k][t]
// All four products run on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32: an exact-f32 fmaf chain, no operand range to guard, no status
// word, nothing to repeat).  A wave owns 64 consecutive samples and all 128 rows: samples lie on the lanes (B operand, read from global
// memory as they stand, 128 contiguous bytes per half wave), output channels in the accumulator registers, so that tanh and sigmoid of
// one gate pair meet in one lane and one register index, and z is the B operand of the second product with no movement between lanes: the
// k index of that product is taken in the order in which the accumulator holds it (acc_row), and the weights are packed in that order.
// A workgroup (4 waves, 256 samples per tile) keeps the dilated-convolution and the 1x1 weights of the layer in LDS (129 KB of the 160 KB)
// as MFMA A fragments in execution order, reads the auxiliary weights (40 KB, the same for every workgroup) from L2, and walks over tiles with a grid
// stride; waves never wait for each other after the weights are in.  A tile's result does not depend on which workgroup computes it:
// a batch row equals the row alone bit for bit.
//
// Around the stack, small plain launches: the pitch front, conv_in, the up-sampler (one launch per scale), the first 1x1 convolution
// and the tail (ReLU, 1x1, ReLU, 1x1 from the scaled skip sum).
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "bsg_common.h"
#include "bsg_ws.h"

namespace bsg {
namespace {

constexpr int PW_R = 64;          // residual = skip channels
constexpr int PW_G = 128;         // gate channels
constexpr int PW_A = 80;          // aux channels
constexpr int PW_WCOLS = 64;      // samples per wave
constexpr int PW_TILE = 256;      // samples per workgroup tile
constexpr int PW_S1 = 3 * PW_R / 2;    // k-steps of the dilated convolution (2 k per MFMA)
constexpr int PW_SA = PW_A / 2;        // k-steps of the aux term
constexpr int PW_S2 = PW_R / 2;        // k-steps of the two 1x1 products
constexpr int PW_IMG = (PW_S1 + PW_S2) * 4 * 64 + 2 * PW_G;   // floats of a layer's LDS image: W1 | W2 | b1 | b2
constexpr int PW_AUXW = PW_SA * 4 * 64;                       // floats of a layer's aux fragments
constexpr uint32_t PW_PHILOX_STREAM = 0x505747;               // 'PWG': the stream id of z in the Philox family

struct LayerArgs {
  const float* xin;    // [B][64][L]
  float* xout;         // [B][64][L] (not xin: neighbouring tiles read xin at t +- d)
  float* skip;         // [B][64][L]
  const float* c;      // [B][80][L]
  const float* img;    // PW_IMG floats
  const float* auxw;   // PW_AUXW floats
  int L, dil, tiles_per_row, ntiles, first, last;
};
// ragged (RAG) only: frames per row | the rows' tile counts as a prefix table pre[0 .. B], pre[B] = ntiles; L stays the pitch of a row
struct LayerRag {
  const int* lens;
  const int* pre;
  int hop;
};

// acc[m][j] += A_step[m] (x) B_step[j] over `NS` k-steps; A and B are fetched U steps ahead of the products that use them
template <int NS, typename AF, typename BF>
__device__ __forceinline__ void steps_product(f32x16 (&acc)[4][2], AF afetch, BF bfetch) {
  constexpr int U = 4;
  static_assert(NS % U == 0, "k-steps per prefetch group");
  float an[U][4], bn[U][2];
  auto load = [&](int s0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int m = 0; m < 4; ++m) an[u][m] = afetch(s0 + u, m);
#pragma unroll
      for (int j = 0; j < 2; ++j) bn[u][j] = bfetch(s0 + u, j);
    }
  };
  load(0);
  for (int s0 = 0; s0 < NS; s0 += U) {
    float ac[U][4], bc[U][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int m = 0; m < 4; ++m) ac[u][m] = an[u][m];
#pragma unroll
      for (int j = 0; j < 2; ++j) bc[u][j] = bn[u][j];
    }
    if (s0 + U < NS) load(s0 + U);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[u][m], bc[u][j], acc[m][j], 0, 0, 0);
  }
}

// RAG (bsg_pwg_forward_ragged): row b ends at Lb = lens[b] hop inside the pitch L, and the workgroups walk the LIVE tiles only: tile ->
// (row, tile of the row) through the prefix table.  A workgroup's tiles ascend, so its row only ever advances: two wave-uniform loads per
// row passed (its tile count and its length), kept in scalar registers — a tile that stays in the row loads nothing before its first
// sample.  The padded instantiation is the kernel without any of it.
template <bool RAG>
__global__ __launch_bounds__(256) void pwg_layer_kernel(const LayerArgs a, const LayerRag g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // PW_IMG floats
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  {
    const float4* __restrict__ src = reinterpret_cast<const float4*>(a.img);
    float4* dst = reinterpret_cast<float4*>(lds);
    for (int i = tid; i < PW_IMG / 4; i += 256) dst[i] = src[i];
  }
  __syncthreads();
  const float* w1 = lds;
  const float* w2 = lds + PW_S1 * 256;
  const float* b1 = w2 + PW_S2 * 256;
  const float* b2 = b1 + PW_G;
  const float* __restrict__ auxw = a.auxw;
  const int L = a.L, dil = a.dil;
  // RAG: the row of the last tile, its tiles [rlo, rhi) and its samples rL — the bound where the padded form has L (which it names itself
  // below: it compiles to the kernel it was before RAG existed)
  int rb = 0, rlo = 0, rhi = 0, rL = 0;
  if (RAG) {
    rhi = __builtin_amdgcn_readfirstlane(g.pre[1]);
    rL = __builtin_amdgcn_readfirstlane(g.lens[0]) * g.hop;
  }

  // no barrier below: every wave walks its own 64 samples of every tile of this workgroup
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    int b, t0;
    if (RAG) {
      while (tile >= rhi) {            // tile < ntiles = pre[B]: ends at a row b < B
        ++rb;
        rlo = rhi;
        rhi = __builtin_amdgcn_readfirstlane(g.pre[rb + 1]);
        rL = __builtin_amdgcn_readfirstlane(g.lens[rb]) * g.hop;
      }
      b = rb;
      t0 = (tile - rlo) * PW_TILE + wave * PW_WCOLS;
    } else {
      b = tile / a.tiles_per_row;
      t0 = (tile - b * a.tiles_per_row) * PW_TILE + wave * PW_WCOLS;
    }
    if (t0 >= (RAG ? rL : L)) continue;
    const float* __restrict__ xin = a.xin + (long long)b * PW_R * L;
    const float* __restrict__ cc = a.c + (long long)b * PW_A * L;
    float* __restrict__ xout = a.xout + (long long)b * PW_R * L;
    float* __restrict__ skip = a.skip + (long long)b * PW_R * L;

    f32x16 acc[4][2];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float bv = b1[32 * m + acc_row(r, lh)];
        acc[m][0][r] = bv;
        acc[m][1][r] = bv;
      }
    // the dilated convolution: step s = tap * 32 + s', k = (tap, ci = 2 s' + lh); a sample outside the row is zero and never read
    steps_product<PW_S1>(
        acc, [&](int s, int m) { return w1[(s * 4 + m) * 64 + lane]; },
        [&](int s, int j) {
          const int tap = s >> 5, ci = 2 * (s & 31) + lh;
          const int t = t0 + 32 * j + l31 + (tap - 1) * dil;
          return (t >= 0 && t < (RAG ? rL : L)) ? xin[(long long)ci * L + t] : 0.f;
        });
    // the aux term: k = ch = 2 s + lh
    steps_product<PW_SA>(
        acc, [&](int s, int m) { return auxw[(s * 4 + m) * 64 + lane]; },
        [&](int s, int j) {
          const int t = t0 + 32 * j + l31;
          return t < (RAG ? rL : L) ? cc[(long long)(2 * s + lh) * L + t] : 0.f;
        });

    // the gate: tanh first (residual_block.py:121)
    f32x16 z[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) z[h][j][r] = tanhf(acc[h][j][r]) * (1.f / (1.f + expf(-acc[h + 2][j][r])));

    // rows 0..63: conv1x1_out, rows 64..127: conv1x1_skip; k = 32 h + acc_row(r, lh) at step (h, r) — the order z lies in
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float bv = b2[32 * m + acc_row(r, lh)];
        acc[m][0][r] = bv;
        acc[m][1][r] = bv;
      }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float af[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) af[m] = w2[((h * 16 + r) * 4 + m) * 64 + lane];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m], z[h][j][r], acc[m][j], 0, 0, 0);
      }

    const float rs = 0.70710678118654752440f;     // (float)sqrt(0.5)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int t = t0 + 32 * j + l31;
      if (t < (RAG ? rL : L)) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const long long o = (long long)(32 * m + acc_row(r, lh)) * L + t;
            if (!a.last) xout[o] = (acc[m][j][r] + xin[o]) * rs;
            const float s = acc[m + 2][j][r];
            skip[o] = a.first ? s : skip[o] + s;
          }
      }
    }
  }
}

// c'[b][o][f] = bc[o] + sum_i Wc[o][i] c[b][i][f] + sum_i Wc[o][80 + i] E[pitch[b][f]][i]   (parallel_wavegan.py:150-151)
// RAG: Tp is the unpadded T (the front is per frame: edge-padding its output is its output on the edge-padded input), frames f < lens[b]
template <bool RAG>
__global__ void pwg_pitch_front_kernel(const float* __restrict__ c, const long long* __restrict__ pitch, const float* __restrict__ emb,
                                       const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out, int B, int Tp,
                                       int n_emb, const int* __restrict__ lens) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)B * PW_A * Tp) return;
  const int f = (int)(idx % Tp), o = (int)((idx / Tp) % PW_A), b = (int)(idx / ((long long)Tp * PW_A));
  if (RAG && f >= lens[b]) return;
  long long p = pitch[(long long)b * Tp + f];
  p = p < 0 ? 0 : (p >= n_emb ? n_emb - 1 : p);      // torch raises on an index outside the table; nothing outside it is read here
  const float* __restrict__ cb = c + (long long)b * PW_A * Tp + f;
  const float* __restrict__ e = emb + p * PW_A;
  const float* __restrict__ wr = w + (long long)o * 2 * PW_A;
  float s = 0.f;
  for (int i = 0; i < PW_A; ++i) s = fmaf(wr[i], cb[(long long)i * Tp], s);
  for (int i = 0; i < PW_A; ++i) s = fmaf(wr[PW_A + i], e[i], s);
  out[idx] = s + bias[o];
}

// conv_in: out[b][o][f] = sum_i sum_k W[o][i][k] c[b][i][f + k], f < T (no padding: the caller padded by the window, upsample.py:157)
// RAG: c is [B][80][T], unpadded; frame f + k of the row's own edge padding is frame clamp(f + k - w, 0, lens[b] - 1), f < lens[b]; the
// same fmaf order
template <bool RAG>
__global__ void pwg_conv_in_kernel(const float* __restrict__ c, const float* __restrict__ w, float* __restrict__ out, int B, int T, int K,
                                   const int* __restrict__ lens) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)B * PW_A * T) return;
  const int f = (int)(idx % T), o = (int)((idx / T) % PW_A), b = (int)(idx / ((long long)T * PW_A));
  const float* __restrict__ wr = w + (long long)o * PW_A * K;
  float s = 0.f;
  if (RAG) {
    const int n = lens[b], hw = (K - 1) / 2;
    if (f >= n) return;
    const float* __restrict__ cb = c + (long long)b * PW_A * T;
    for (int i = 0; i < PW_A; ++i)
      for (int k = 0; k < K; ++k) {
        const int g = f + k - hw;
        s = fmaf(wr[i * K + k], cb[(long long)i * T + (g < 0 ? 0 : (g >= n ? n - 1 : g))], s);
      }
  } else {
    const int Tp = T + K - 1;
    const float* __restrict__ cb = c + (long long)b * PW_A * Tp + f;
    for (int i = 0; i < PW_A; ++i)
      for (int k = 0; k < K; ++k) s = fmaf(wr[i * K + k], cb[(long long)i * Tp + k], s);
  }
  out[idx] = s;
}

// one scale of the up-sampler (upsample.py:85-99): nearest stretch by s, then a (2 s + 1)-tap convolution with zero padding s, per row
// RAG: batch row b ends at lens[b] mul, mul = T-to-Lout rate (the scales so far, this one included): the zero padding sits there, and
// nothing at or beyond it is read or written; Lin and Lout stay the pitches
template <bool RAG>
__global__ void pwg_upsample_kernel(const float* __restrict__ in, const float* __restrict__ w, float* __restrict__ out, long long rows, int Lin,
                                    int s, const int* __restrict__ lens, int mul) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int Lout = Lin * s;
  if (idx >= rows * Lout) return;
  const int t = (int)(idx % Lout);
  const int Lb = RAG ? lens[(idx / Lout) / PW_A] * mul : Lout;
  if (RAG && t >= Lb) return;
  const float* __restrict__ r = in + (idx / Lout) * Lin;
  float v = 0.f;
  for (int j = 0; j <= 2 * s; ++j) {
    const int q = t + j - s;
    if (q >= 0 && q < Lb) v = fmaf(w[j], r[q / s], v);
  }
  out[idx] = v;
}

// first_conv: x[b][ch][t] = w[ch] z[b][t] + bias[ch]      (RAG: t < lens[b] hop)
template <bool RAG>
__global__ void pwg_first_kernel(const float* __restrict__ z, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ x,
                                 int B, int L, const int* __restrict__ lens, int hop) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)B * L) return;
  const int b = (int)(idx / L), t = (int)(idx % L);
  if (RAG && t >= lens[b] * hop) return;
  const float zv = z[idx];
  float* __restrict__ xb = x + (long long)b * PW_R * L + t;
#pragma unroll 8
  for (int ch = 0; ch < PW_R; ++ch) xb[(long long)ch * L] = fmaf(w[ch], zv, bias[ch]);
}

// the tail (parallel_wavegan.py:161-166): y = b4 + w4 . relu(b3 + W3 relu(skips sqrt(1 / layers)))      (RAG: y = 0 at t >= lens[b] hop)
template <bool RAG>
__global__ __launch_bounds__(256) void pwg_tail_kernel(const float* __restrict__ skip, const float* __restrict__ w3, const float* __restrict__ b3,
                                                       const float* __restrict__ w4, const float* __restrict__ b4, float* __restrict__ y, int B,
                                                       int L, float scale, const int* __restrict__ lens, int hop) {
  __shared__ __attribute__((aligned(16))) float sw[PW_R * PW_R + 2 * PW_R];
  for (int i = threadIdx.x; i < PW_R * PW_R; i += 256) sw[i] = w3[i];
  if (threadIdx.x < PW_R) {
    sw[PW_R * PW_R + threadIdx.x] = b3[threadIdx.x];
    sw[PW_R * PW_R + PW_R + threadIdx.x] = w4[threadIdx.x];
  }
  __syncthreads();
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)B * L) return;
  const int b = (int)(idx / L), t = (int)(idx % L);
  if (RAG && t >= lens[b] * hop) {
    y[idx] = 0.f;
    return;
  }
  const float* __restrict__ sb = skip + (long long)b * PW_R * L + t;
  float v[PW_R];
#pragma unroll
  for (int ch = 0; ch < PW_R; ++ch) v[ch] = fmaxf(sb[(long long)ch * L] * scale, 0.f);
  float out = 0.f;
#pragma unroll 2
  for (int o = 0; o < PW_R; ++o) {
    const float4* wr = reinterpret_cast<const float4*>(sw + o * PW_R);
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < PW_R / 4; ++q) {
      const float4 w = wr[q];
      s = fmaf(w.x, v[4 * q], s);
      s = fmaf(w.y, v[4 * q + 1], s);
      s = fmaf(w.z, v[4 * q + 2], s);
      s = fmaf(w.w, v[4 * q + 3], s);
    }
    out = fmaf(sw[PW_R * PW_R + PW_R + o], fmaxf(s + sw[PW_R * PW_R + o], 0.f), out);
  }
  y[idx] = out + b4[0];
}

}  // namespace
}  // namespace bsg

using namespace bsg;

struct bsg_pwg {
  bsg_pwg_cfg cfg{};
  int hop = 0, cus = 0;
  std::vector<int> dil;
  float* wdev = nullptr;        // every packed weight, one allocation
  // offsets (floats) into wdev
  size_t o_first_w = 0, o_first_b = 0, o_cin = 0, o_up[8] = {}, o_img = 0, o_aux = 0, o_w3 = 0, o_b3 = 0, o_w4 = 0, o_b4 = 0, o_emb = 0, o_cw = 0,
         o_cb = 0;
  float* ws = nullptr;          // the workspaces, one allocation
  size_t ws_bytes = 0;
  int* lens = nullptr;          // ragged forwards: lens[0 .. B) frames per row | pre[0 .. B] tiles before row b, written by launches of the call itself
  size_t lens_cap = 0;          // rows
  int tiles = 0;                // 256-sample tiles one layer launch of the last forward walked
  std::string path;
};

// the handle's shape-sized buffers (bsg_ws.h): the workspaces, one allocation that the forward grows, destroy frees and the test hook
// poisons; and the lengths array of the ragged forward (2 lens_cap + 1 ints, not poisoned: the call itself fills it)
static std::vector<WsBuf> ws_table(bsg_pwg* h) {
  return {{&h->ws_bytes, (void**)&h->ws, 1, 0, WS_POISON}, {&h->lens_cap, (void**)&h->lens, 2 * sizeof(int), sizeof(int)}};
}

static int pwg_expected_weights(const bsg_pwg_cfg* c) { return 2 + 1 + c->n_scales + 7 * c->layers + 4 + (c->use_pitch_embed ? 3 : 0); }

extern "C" int bsg_pwg_n_weights(const bsg_pwg_cfg* cfg) { return cfg ? pwg_expected_weights(cfg) : 0; }

extern "C" void bsg_pwg_destroy(bsg_pwg* h) {
  if (!h) return;
  if (h->wdev) (void)hipFree(h->wdev);
  ws_free(ws_table(h));
  delete h;
}

extern "C" const char* bsg_pwg_last_path(bsg_pwg* h) { return h && !h->path.empty() ? h->path.c_str() : "none"; }

extern "C" int bsg_pwg_create(bsg_pwg** out, const bsg_pwg_cfg* cfg, const void* const* dev_weights, int32_t n_weights, void* stream) {
  BSG_REQUIRE(out, "pwg_create: null argument");
  *out = nullptr;
  BSG_REQUIRE(cfg && dev_weights, "pwg_create: null argument");
  // what is built: refusals name the value, and come before any device call
  BSG_REQUIRE(cfg->in_channels == 1 && cfg->out_channels == 1, "pwg_create: in_channels=%d, out_channels=%d: only 1 and 1 are built",
              cfg->in_channels, cfg->out_channels);
  BSG_REQUIRE(cfg->kernel_size == 3, "pwg_create: kernel_size=%d is not built; accepted: 3", cfg->kernel_size);
  BSG_REQUIRE(!cfg->use_causal_conv, "pwg_create: use_causal_conv=%d (the causal form) is not built; accepted: 0", cfg->use_causal_conv);
  BSG_REQUIRE(cfg->residual_channels == PW_R, "pwg_create: residual_channels=%d is not built; accepted: 64", cfg->residual_channels);
  BSG_REQUIRE(cfg->skip_channels == PW_R, "pwg_create: skip_channels=%d is not built; accepted: 64", cfg->skip_channels);
  BSG_REQUIRE(cfg->gate_channels == PW_G, "pwg_create: gate_channels=%d is not built; accepted: 128", cfg->gate_channels);
  BSG_REQUIRE(cfg->aux_channels == PW_A, "pwg_create: aux_channels=%d is not built; accepted: 80", cfg->aux_channels);
  BSG_REQUIRE(cfg->bias, "pwg_create: bias=%d (layers without bias) is not built; accepted: 1", cfg->bias);
  BSG_REQUIRE(cfg->upsample_net == 0, "pwg_create: upsample_net code %d is not built; accepted: 0 (ConvInUpsampleNetwork)", cfg->upsample_net);
  BSG_REQUIRE(cfg->interpolate_nearest == 1 && cfg->freq_axis_kernel_size == 1,
              "pwg_create: interpolate_nearest=%d, freq_axis_kernel_size=%d: only the nearest stretch with a 1 x (2 scale + 1) kernel is built",
              cfg->interpolate_nearest, cfg->freq_axis_kernel_size);
  BSG_REQUIRE(cfg->aux_context_window >= 0 && cfg->aux_context_window <= 8, "pwg_create: aux_context_window=%d outside 0 .. 8",
              cfg->aux_context_window);
  BSG_REQUIRE(cfg->layers >= 1 && cfg->layers <= 64 && cfg->stacks >= 1 && cfg->layers % cfg->stacks == 0,
              "pwg_create: layers=%d, stacks=%d: layers must be 1 .. 64 and a multiple of stacks", cfg->layers, cfg->stacks);
  BSG_REQUIRE(cfg->layers / cfg->stacks <= 16, "pwg_create: layers / stacks = %d: dilations beyond 2^15 are not built", cfg->layers / cfg->stacks);
  BSG_REQUIRE(cfg->n_scales >= 1 && cfg->n_scales <= 8, "pwg_create: %d upsample_scales: 1 .. 8 are built", cfg->n_scales);
  long long prod = 1;
  for (int i = 0; i < cfg->n_scales; ++i) {
    BSG_REQUIRE(cfg->upsample_scales[i] >= 1 && cfg->upsample_scales[i] <= 64, "pwg_create: upsample_scales[%d]=%d outside 1 .. 64", i,
                cfg->upsample_scales[i]);
    prod *= cfg->upsample_scales[i];
  }
  BSG_REQUIRE(prod == cfg->hop_size, "pwg_create: the product of upsample_scales is %lld but hop_size=%d: they must be equal", prod, cfg->hop_size);
  BSG_REQUIRE(!cfg->use_pitch_embed || cfg->n_pitch >= 1, "pwg_create: use_pitch_embed with n_pitch=%d embedding rows", cfg->n_pitch);
  const int want = pwg_expected_weights(cfg);
  BSG_REQUIRE(n_weights == want, "pwg_create: %d weights given, %d expected (folded state-dict order)", n_weights, want);
  for (int i = 0; i < n_weights; ++i) BSG_REQUIRE(dev_weights[i], "pwg_create: weight %d is null", i);

  hipStream_t st = (hipStream_t)stream;
  const int NL = cfg->layers, KC = 2 * cfg->aux_context_window + 1;
  // the folded state-dict order (a folded convolution lists its bias before its weight):
  //   first_conv.{bias, weight}, upsample_net.conv_in.weight, upsample_net.upsample.up_layers.{1, 3, ..}.weight,
  //   conv_layers.i.{conv.bias, conv.weight, conv1x1_aux.weight, conv1x1_out.bias, conv1x1_out.weight, conv1x1_skip.bias, conv1x1_skip.weight},
  //   last_conv_layers.1.{bias, weight}, last_conv_layers.3.{bias, weight} (, pitch_embed.weight, c_proj.weight, c_proj.bias)
  std::vector<size_t> sizes;
  sizes.push_back(PW_R); sizes.push_back(PW_R);
  sizes.push_back((size_t)PW_A * PW_A * KC);
  for (int i = 0; i < cfg->n_scales; ++i) sizes.push_back(2 * cfg->upsample_scales[i] + 1);
  for (int l = 0; l < NL; ++l) {
    const size_t s7[7] = {PW_G, (size_t)PW_G * PW_R * 3, (size_t)PW_G * PW_A, PW_R, (size_t)PW_R * PW_R, PW_R, (size_t)PW_R * PW_R};
    sizes.insert(sizes.end(), s7, s7 + 7);
  }
  sizes.push_back(PW_R); sizes.push_back((size_t)PW_R * PW_R); sizes.push_back(1); sizes.push_back(PW_R);
  if (cfg->use_pitch_embed) {
    sizes.push_back((size_t)cfg->n_pitch * PW_A); sizes.push_back((size_t)PW_A * 2 * PW_A); sizes.push_back(PW_A);
  }
  std::vector<std::vector<float>> W(n_weights);
  for (int i = 0; i < n_weights; ++i) {
    W[i].resize(sizes[i]);
    BSG_HIP(hipMemcpyAsync(W[i].data(), dev_weights[i], sizes[i] * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  BSG_HIP(hipStreamSynchronize(st));

  bsg_pwg* h = new bsg_pwg();
  h->cfg = *cfg;
  h->hop = cfg->hop_size;
  for (int l = 0; l < NL; ++l) h->dil.push_back(1 << (l % (NL / cfg->stacks)));
  std::vector<float> P;
  auto put = [&](const std::vector<float>& v) {
    while (P.size() % 4) P.push_back(0.f);      // 16-byte alignment of every block
    const size_t o = P.size();
    P.insert(P.end(), v.begin(), v.end());
    return o;
  };
  int wi = 0;
  h->o_first_b = put(W[wi++]); h->o_first_w = put(W[wi++]);
  h->o_cin = put(W[wi++]);
  for (int i = 0; i < cfg->n_scales; ++i) h->o_up[i] = put(W[wi++]);
  std::vector<float> img((size_t)NL * PW_IMG), aux((size_t)NL * PW_AUXW);
  for (int l = 0; l < NL; ++l) {
    const std::vector<float>&cb = W[wi], &cw = W[wi + 1], &aw = W[wi + 2], &ob = W[wi + 3], &ow = W[wi + 4], &sb = W[wi + 5], &sw = W[wi + 6];
    wi += 7;
    float* I = img.data() + (size_t)l * PW_IMG;
    float* w1 = I;
    float* w2 = I + PW_S1 * 256;
    float* b1 = w2 + PW_S2 * 256;
    float* b2 = b1 + PW_G;
    for (int s = 0; s < PW_S1; ++s)
      for (int m = 0; m < 4; ++m)
        for (int lane = 0; lane < 64; ++lane) {
          const int tap = s >> 5, ci = 2 * (s & 31) + (lane >> 5), g = 32 * m + (lane & 31);
          w1[(s * 4 + m) * 64 + lane] = cw[((size_t)g * PW_R + ci) * 3 + tap];
        }
    for (int s = 0; s < PW_SA; ++s)
      for (int m = 0; m < 4; ++m)
        for (int lane = 0; lane < 64; ++lane)
          aux[(size_t)l * PW_AUXW + (s * 4 + m) * 64 + lane] = aw[(size_t)(32 * m + (lane & 31)) * PW_A + 2 * s + (lane >> 5)];
    for (int hh = 0; hh < 2; ++hh)
      for (int r = 0; r < 16; ++r)
        for (int m = 0; m < 4; ++m)
          for (int lane = 0; lane < 64; ++lane) {
            const int k = 32 * hh + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), row = 32 * m + (lane & 31);
            w2[((hh * 16 + r) * 4 + m) * 64 + lane] = row < PW_R ? ow[(size_t)row * PW_R + k] : sw[(size_t)(row - PW_R) * PW_R + k];
          }
    for (int g = 0; g < PW_G; ++g) b1[g] = cb[g];
    for (int r = 0; r < PW_R; ++r) { b2[r] = ob[r]; b2[PW_R + r] = sb[r]; }
  }
  h->o_img = put(img);
  h->o_aux = put(aux);
  h->o_b3 = put(W[wi++]); h->o_w3 = put(W[wi++]); h->o_b4 = put(W[wi++]); h->o_w4 = put(W[wi++]);
  if (cfg->use_pitch_embed) { h->o_emb = put(W[wi++]); h->o_cw = put(W[wi++]); h->o_cb = put(W[wi++]); }

  auto fail = [&](hipError_t e, const char* what) {
    set_error("pwg_create: %s -> %s", what, hipGetErrorString(e));
    bsg_pwg_destroy(h);
    return e == hipErrorOutOfMemory ? BSG_ENOMEM : BSG_EHIP;
  };
  hipError_t e;
  if ((e = hipMalloc((void**)&h->wdev, P.size() * sizeof(float))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMemcpyAsync(h->wdev, P.data(), P.size() * sizeof(float), hipMemcpyHostToDevice, st)) != hipSuccess) return fail(e, "hipMemcpyAsync");
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(e, "hipStreamSynchronize");
  if ((e = hipFuncSetAttribute((const void*)pwg_layer_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               PW_IMG * (int)sizeof(float))) != hipSuccess ||
      (e = hipFuncSetAttribute((const void*)pwg_layer_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               PW_IMG * (int)sizeof(float))) != hipSuccess)
    return fail(e, "hipFuncSetAttribute");
  int dev = 0;
  hipDeviceProp_t prop;
  if ((e = hipGetDevice(&dev)) != hipSuccess || (e = hipGetDeviceProperties(&prop, dev)) != hipSuccess) return fail(e, "hipGetDeviceProperties");
  h->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  *out = h;
  return BSG_OK;
}

// test hook: NaN bytes into the workspaces (the lengths array is the call's own and stays)
extern "C" int bsg_pwg_debug_poison_workspace(bsg_pwg* h, void* stream) {
  BSG_REQUIRE(h, "pwg_debug_poison_workspace: null handle");
  return ws_poison(ws_table(h), (hipStream_t)stream);
}

extern "C" int bsg_pwg_last_tiles(bsg_pwg* h) { return h ? h->tiles : 0; }

#define TRY(expr)                  \
  do {                             \
    int _rc = (expr);              \
    if (_rc != BSG_OK) return _rc; \
  } while (0)

// The forward, padded (RAG = false: c [B][80][T + 2 w], lengths_host null) or ragged (c = mel [B][80][T]): the same launches in the same
// order over the same workspaces, each bounding row b by its own length; only the layer launch has another grid (the live tiles).
template <bool RAG>
static int pwg_forward_any(bsg_pwg* h, const float* z, const float* c, const int64_t* pitch, const int32_t* lengths_host, float* y, int32_t B,
                           int32_t T, uint64_t seed, void* stream, const char* who) {
  if (RAG) TRY(lens_check(lengths_host, B, T, who));      // first: refused before anything is grown, enqueued or written
  BSG_REQUIRE(B >= 1 && T >= 1, "%s: B=%d, T=%d: both must be >= 1", who, B, T);
  BSG_REQUIRE(h && c && y, "%s: null argument", who);
  const bsg_pwg_cfg& cf = h->cfg;
  BSG_REQUIRE(!cf.use_pitch_embed || pitch, "%s: this generator has the pitch front (use_pitch_embed): pitch is required", who);
  BSG_REQUIRE(cf.use_pitch_embed || !pitch, "%s: pitch given but this generator was built without use_pitch_embed", who);
  const int hop = h->hop;
  const long long L = (long long)T * hop;
  BSG_REQUIRE((long long)B * L * PW_A < (1ll << 40) && L < (1ll << 30), "%s: B=%d rows of %lld samples are more than one call carries", who, B, L);
  BSG_REQUIRE(z || (B * L) % 4 == 0, "%s: B * T * hop = %lld is no multiple of 4: supply z (the Philox stream is drawn four at a time)", who,
              B * L);
  hipStream_t st = (hipStream_t)stream;
  const int w = cf.aux_context_window, Tp = T + 2 * w;
  // the workspaces: c' [B][80][Tp] | c2 [B][80][T] | cfull [B][80][L] | ctmp [B][80][L / s_last] | x0, x1, skip [B][64][L] | z [B][L]
  // (ragged: the same sizes; c' is [B][80][T] at the front of its part)
  const int s_last = cf.upsample_scales[cf.n_scales - 1];
  auto al = [](size_t n) { return (n + 63) & ~(size_t)63; };
  const size_t n_cp = al((size_t)B * PW_A * Tp), n_c2 = al((size_t)B * PW_A * T), n_cf = al((size_t)B * PW_A * L),
               n_ct = al((size_t)B * PW_A * (L / s_last)), n_x = al((size_t)B * PW_R * L), n_z = al((size_t)B * L);
  const size_t need = (n_cp + n_c2 + n_cf + n_ct + 3 * n_x + n_z) * sizeof(float);
  if (need > h->ws_bytes) TRY(ws_grow(ws_table(h), "pwg", &h->ws_bytes, need, st));
  const int tiles_per_row = cdiv(L, PW_TILE);
  int ntiles = B * tiles_per_row;
  const int* lens = nullptr;
  const int* pre = nullptr;
  if (RAG) {
    // the counts and the prefix table of the rows' tile counts travel in kernel arguments (lens_fill): a captured forward replays them
    if ((size_t)B > h->lens_cap) TRY(ws_grow(ws_table(h), "pwg", &h->lens_cap, (size_t)B, st));
    std::vector<int32_t> pre_host((size_t)B + 1);
    pre_host[0] = 0;
    for (int b = 0; b < B; ++b) pre_host[b + 1] = pre_host[b] + cdiv((long long)lengths_host[b] * hop, PW_TILE);
    ntiles = pre_host[B];
    TRY(lens_fill(h->lens, lengths_host, B, st));
    TRY(lens_fill(h->lens + B, pre_host.data(), B + 1, st));
    lens = h->lens;
    pre = h->lens + B;
  }
  float* cp = h->ws;
  float* c2 = cp + n_cp;
  float* cfull = c2 + n_c2;
  float* ctmp = cfull + n_cf;
  float* x0 = ctmp + n_ct;
  float* x1 = x0 + n_x;
  float* skip = x1 + n_x;
  float* zbuf = skip + n_x;
  const float* Wd = h->wdev;
  h->path.clear();
  h->tiles = 0;
  auto tok = [&](const std::string& s) { if (!h->path.empty()) h->path += ' '; h->path += s; };
  if (RAG) tok("ragged");

  const float* cin = c;
  if (cf.use_pitch_embed) {
    const int Tf = RAG ? T : Tp;      // ragged: the front runs on the unpadded frames
    hipLaunchKernelGGL(pwg_pitch_front_kernel<RAG>, dim3(cdiv((long long)B * PW_A * Tf, 256)), dim3(256), 0, st, c, (const long long*)pitch,
                       Wd + h->o_emb, Wd + h->o_cw, Wd + h->o_cb, cp, B, Tf, cf.n_pitch, lens);
    BSG_LAUNCH_CHECK();
    tok("pitch");
    cin = cp;
  }
  hipLaunchKernelGGL(pwg_conv_in_kernel<RAG>, dim3(cdiv((long long)B * PW_A * T, 256)), dim3(256), 0, st, cin, Wd + h->o_cin, c2, B, T, 2 * w + 1,
                     lens);
  BSG_LAUNCH_CHECK();
  tok("conv_in");
  const float* uin = c2;
  int Lin = T, mul = 1;
  for (int i = 0; i < cf.n_scales; ++i) {
    float* uout = ((cf.n_scales - 1 - i) & 1) ? ctmp : cfull;
    const int s = cf.upsample_scales[i];
    mul *= s;
    hipLaunchKernelGGL(pwg_upsample_kernel<RAG>, dim3(cdiv((long long)B * PW_A * Lin * s, 256)), dim3(256), 0, st, uin, Wd + h->o_up[i], uout,
                       (long long)B * PW_A, Lin, s, lens, mul);
    BSG_LAUNCH_CHECK();
    tok("up" + std::to_string(i) + ":x" + std::to_string(s));
    uin = uout;
    Lin *= s;
  }
  if (!z) {
    TRY(bsg_philox_normal(zbuf, (long long)B * L, seed, PW_PHILOX_STREAM, 0, stream));
    tok("philox");
    z = zbuf;
  }
  hipLaunchKernelGGL(pwg_first_kernel<RAG>, dim3(cdiv((long long)B * L, 256)), dim3(256), 0, st, z, Wd + h->o_first_w, Wd + h->o_first_b, x0, B,
                     (int)L, lens, hop);
  BSG_LAUNCH_CHECK();
  tok("first");
  LayerArgs a{};
  a.c = cfull; a.skip = skip; a.L = (int)L;
  a.tiles_per_row = tiles_per_row;
  a.ntiles = ntiles;
  const LayerRag rag{lens, pre, hop};
  const int grid = a.ntiles < h->cus ? a.ntiles : h->cus;
  float* xa = x0;
  float* xb = x1;
  for (int l = 0; l < cf.layers; ++l) {
    a.xin = xa; a.xout = xb; a.dil = h->dil[l]; a.first = l == 0; a.last = l == cf.layers - 1;
    a.img = Wd + h->o_img + (size_t)l * PW_IMG;
    a.auxw = Wd + h->o_aux + (size_t)l * PW_AUXW;
    hipLaunchKernelGGL(pwg_layer_kernel<RAG>, dim3(grid), dim3(256), PW_IMG * sizeof(float), st, a, rag);
    BSG_LAUNCH_CHECK();
    tok("layer" + std::to_string(l) + ":f32/d" + std::to_string(a.dil));
    float* t = xa; xa = xb; xb = t;
  }
  hipLaunchKernelGGL(pwg_tail_kernel<RAG>, dim3(cdiv((long long)B * L, 256)), dim3(256), 0, st, skip, Wd + h->o_w3, Wd + h->o_b3, Wd + h->o_w4,
                     Wd + h->o_b4, y, B, (int)L, (float)sqrt(1.0 / cf.layers), lens, hop);
  BSG_LAUNCH_CHECK();
  tok("tail");
  h->tiles = ntiles;
  return BSG_OK;
}

extern "C" int bsg_pwg_forward(bsg_pwg* h, const float* z, const float* c, const int64_t* pitch, float* y, int32_t B, int32_t T, uint64_t seed,
                               void* stream) {
  return pwg_forward_any<false>(h, z, c, pitch, nullptr, y, B, T, seed, stream, "pwg_forward");
}

// Ragged batches: row b is the generator on its own n_b = lengths_host[b] frames (1 .. T) inside the (B, T) tensors, edge-padded at ITS
// end by the library, bit for bit the B = 1, T = n_b call; the layer launches walk the live tiles only (include/bisinger_hip.h).
extern "C" int bsg_pwg_forward_ragged(bsg_pwg* h, const float* z, const float* mel, const int64_t* pitch, const int32_t* lengths_host, float* y,
                                      int32_t B, int32_t T, uint64_t seed, void* stream) {
  return pwg_forward_any<true>(h, z, mel, pitch, lengths_host, y, B, T, seed, stream, "pwg_forward_ragged");
}

