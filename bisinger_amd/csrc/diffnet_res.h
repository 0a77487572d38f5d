// Shared by the fp32 (diffnet.hip) and bf16-operand (diffnet_bf16.hip) forms of the fused residual block.
#pragma once
#include "bsg_common.h"

namespace bsg {

constexpr int C = 256;     // residual channels == encoder hidden (checked at create)
constexpr int HALO = 8;    // max dilation 2^3

struct ResArgs {
  const float* x_in;     // [B][C][T]
  float* x_out;          // [B][C][T]
  float* skip;           // [B][C][T]
  const float* condterm; // this layer's [B][2C][T]: conditioner_projection(cond) + b_cond + b_dil
  const float* dproj;    // [S][L][C] table: diffusion_projection_l(mlp(emb(step)))
  const long long* t_dev;  // [B] or null
  int t_uniform;
  const float* apack1;   // dilated conv, packed  [16][96][64][4]
  const float* apack2;   // output projection     [16][32][64][4]
  const float* apackw;   // dilated conv in Winograd F(2,3) form, packed for 16x16x4 MFMAs [4][32][16][64][4]
  const float* apackw43; // dilated conv in Winograd F(4,3) form (diffnet_f43.hip) [6][32][16][64][4]
  const unsigned short* apack1h;  // bf16 operand path: dilated conv packed for 32x32x16 bf16 MFMAs [16][48][64][8]
  const unsigned short* apack2h;  // bf16 operand path: output projection                           [16][16][64][8]
  // bf16-operand path: conditioner term and running skip sum are STORED as bf16 in channel-quad order
  // [B][rows/4][T][4] (one 8-byte access per lane = 4 consecutive channels of one frame, 256-B coalesced)
  const unsigned short* condterm_h;  // this layer's [B][2C/4][T][4]
  unsigned short* skip_h;            // [B][C/4][T][4]
  const float* bias_out; // [2C]
  int B, T, L, layer, dil, tiles_per_row;
  int first;             // layer 0: skip is stored, not accumulated
  float skip_div;        // last layer: skip_sum / sqrt(L) (net.py:126); 1 otherwise
  unsigned long long* stamps;  // diagnostic build only (STAMP = true): [workgroup][wave][8] s_memtime values
};

// arguments of the stack launches (all L layers of a group of rows in one launch, residual stream on chip):
// residual_stack_h2_kernel (diffnet_h2.hip), residual_stack_f43_kernel (diffnet_f43.hip), residual_stack_bf16_kernel (diffnet_bf16.hip)
struct StackArgs {
  const float* x_in;      // [B][C][T] in-projected x of this launch's rows
  float* skip;            // [B][C][T] output: skip sum / sqrt(L)
  unsigned short* skip_h; // bf16 form: the same as bf16 channel quads [B][C/4][T][4]
  const float* condterm;  // layer 0, this launch's rows: [B][2C][T]; + l * ct_stride for layer l
  const float* condterm_q; // 16-row stack launch: the same in channel-quad order [B][2C/4][T][4] (null: `condterm`); + l * ct_stride
  const float* dproj;     // [S][L][C]
  const float* dconv;     // 16-row stack launch: [S][L][4][2C] = W_tap d for tap 0, 1, 2 and their sum (the step term's share of the dilated conv)
  const long long* t_dev; // [B] or null
  const float* apackw;    // layer 0; + l * aw_stride
  const float* apackw43;  // F(4,3) form (diffnet_f43.hip), layer 0; + l * 6*2C*C
  const unsigned short* apack1h;     // bf16 form: dilated conv fragments, layer 0; + l * 2C*3C
  const unsigned short* apack2h;     // bf16 form: output projection fragments, layer 0; + l * 2C*C
  const unsigned short* condterm_h;  // bf16 form: conditioner term in channel-quad order, layer 0 / this launch's rows; + l * ct_stride
  const float* apack2;    // layer 0; + l * a2_stride
  const unsigned short* apack1s;  // split-fp16 form (diffnet_h2.hip): hi / lo fp16 fragments of the dilated conv, layer 0; + l * 2*2C*3C
  const unsigned short* apack2s;  // split-fp16 form: output projection, layer 0; + l * 2*2C*C
  const float* h2_scale;          // split-fp16 form: [L][4] = s1, 1/s1, s2 * 2^10, 1/(s2 * 2^10)
  const unsigned short* apack1q;  // quad form: the same weights as 16-row fragments of v_mfma_f32_16x16x32_f16, layer 0; + l * 2*2C*3C
  const unsigned short* apack2q;  // quad form: output projection, layer 0; + l * 2*2C*C
  const float* bias_out;  // layer 0; + l * 2C
  long long ct_stride;
  float* hx;              // [2 parities][n_tiles][2 sides][C][8] edge exchange
  unsigned* flags;        // [n_tiles]
  unsigned* status;       // += 1 for every spin that gave up
  int t_uniform, T, L, tiles_per_row, n_tiles, cycle;
  unsigned fbase;         // launch epoch * 64: flag value = fbase + layers published (host-side epoch: diagnostics; otherwise `epoch`)
  // Round 4: the launch epoch lives in DEVICE memory, so that a captured launch can be replayed (a replay repeats its kernel arguments):
  // epoch[0] = epoch of the launch that runs next, epoch[1] = workgroups of the running launch that are through their layers.  Every
  // workgroup takes fbase = epoch[0] * 64 at entry; the LAST one through its layer loop (all others have read the epoch long ago)
  // advances it — and, before the 32-bit flag values could come round, zeroes every flag word and starts the epochs again.
  unsigned* epoch;        // null: p.fbase
  int flag_words;         // words of `flags` to zero at a wrap (the status words behind them are not touched)
  int pflag_words;        // the same for `pflags` (part forms)
  // zeroed at an epoch wrap by WHATEVER launch wraps (round 5): the handle's part-form flags even when this launch does not wait on
  // them (p.pflags null) — a wrap inside a whole-tile launch used to leave them near 2^31 while the epochs restarted at 1, and the next part
  // launch then saw every flag 'published'
  unsigned* wrap_pflags;
  int wrap_pflag_words;
  int stamp_mode;         // diagnostics (BSG_STAMP_MODE, part forms): 1 = stamp slots 1 / 2 mark the gate phase's inner boundaries instead of GEMM1's
  int inject;             // fault injection: consumers do not wait
  // part forms of the split-fp16 launch (residual_part_h2_kernel, small batches): exchange of the P channel parts of a tile
  unsigned short* zx;     // [n_tiles][P parts][2 planes][tile frames][C/P] fp16: gated activation parts
  unsigned short* ix;     // [2 parities][n_tiles][P parts][2 planes][tile frames][C/P] fp16: image parts (core frames; neighbours read the edges)
  unsigned* pflags;       // [2][n_tiles][P parts]: [0] image flags (layers prepared), [1] z flags
  unsigned long long* stamps;   // diagnostic (bsg_diffnet_debug_stack_stamps) or null: [n_tiles][L][8] s_memrealtime at the phase boundaries
  unsigned long long* clk;      // null, or [4]: tile 0 stores s_memtime / s_memrealtime at its start and end (sustained shader clock, bench.py)
  // ragged launch (residual_stack_q_kernel<.., VARLEN = true>, residual_stack_bf16_varlen_kernel; bsg_diffnet_prepare_ragged); null otherwise
  const int2* vl_tiles;   // [n_tiles] {row of the bound batch, column tile in the row}: each row's tiles contiguous, in order
  const int* vl_len;      // [B] frames of every row of the bound batch (<= T, the row stride)
  // token form of the 16-row launch (residual_stack_q_kernel<.., Q_TOK>; bsg_diffnet_prepare_tokens); null / 0 otherwise
  const int* tok;         // [rows][T] token id of every frame of this launch's rows, in [0, tok_K); condterm_q is then [L][B][2C/4][tok_K][4]
  int tok_K;              // token rows per utterance (row 0: the padding token)
};

// Launch epoch in device memory (StackArgs::epoch): taken at entry by every workgroup ...
__device__ __forceinline__ unsigned stack_epoch_take(const StackArgs& p) {
  if (!p.epoch) return p.fbase;
  return (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(p.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) * 64u;
}
// ... and advanced by the last of the launch's `n_wgs` workgroups to leave its layer loop (one thread of each calls this once)
__device__ __forceinline__ void stack_epoch_done(const StackArgs& p, unsigned fbase, int n_wgs) {
  if (!p.epoch) return;
  const unsigned done = atomicAdd(p.epoch + 1, 1u);
  if (done + 1u != (unsigned)n_wgs) return;
  unsigned next = fbase / 64u + 1u;
  if (next >= (1u << 25)) {   // flag values = epoch * 64 + layer in 32 bits: start again from zeroed flags, as nothing else runs on them now
    for (int i = 0; i < p.flag_words; ++i) p.flags[i] = 0u;
    if (p.wrap_pflags)
      for (int i = 0; i < p.wrap_pflag_words; ++i) p.wrap_pflags[i] = 0u;
    next = 1u;
  }
  __hip_atomic_store(p.epoch + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(p.epoch, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (the launch forms that take these arguments: diffnet_forms.h)

// split-fp16 weight fragments and their scales (diffnet_h2.hip)
int pack_a_frag_q(const float* src, unsigned short* out, int M, int K, int Kc, long long sm, long long sc, long long stp, const float* tab,
                  int is_gemm2, hipStream_t st);
int h2_scales(const float* const* w1, const float* const* w2, int L, unsigned* maxbits, float* tab, hipStream_t st);
int pack_a_frag_h2(const float* src, unsigned short* out, int M, int K, int Kc, long long sm, long long sc, long long stp, const float* tab,
                   int is_gemm2, hipStream_t st);

int pack_wino43(const float* w, float* out, hipStream_t st);   // [2C][C][3] -> [6][32][16][64][4]

// fp32 [M][K] weights -> bf16 A fragments of v_mfma_f32_32x32x16_bf16 (see diffnet_bf16.hip)
int pack_a_frag_bf16(const float* src, unsigned short* out, int M, int K, int Kc, long long sm, long long sc, long long stp,
                     hipStream_t st);

// fp32 [B][rows][T] <-> bf16 channel-quad order [B][rows/4][T][4] (rows % 4 == 0)
int f32_to_quad_bf16(const float* src, unsigned short* dst, int B, int rows, int T, hipStream_t st);
int quad_bf16_to_f32(const unsigned short* src, float* dst, int B, int rows, int T, hipStream_t st);

__device__ __forceinline__ float bf16_lo(unsigned v) { return __builtin_bit_cast(float, v << 16); }
__device__ __forceinline__ float bf16_hi(unsigned v) { return __builtin_bit_cast(float, v & 0xffff0000u); }

// fast gate math: v_exp_f32 / v_rcp_f32 based (abs error ~2e-7, far inside the 1e-3 mel budget); the libm
// versions cost ~60 VALU instructions per element and the gate phase runs with the MFMA pipe idle.
__device__ __forceinline__ float fast_sigmoid(float x) { return __frcp_rn(1.0f + __expf(-x)); }
__device__ __forceinline__ float fast_tanh(float x) { return 1.0f - 2.0f * __frcp_rn(1.0f + __expf(2.0f * x)); }
// sigmoid(g) * tanh(f) with two exponentials and ONE reciprocal: (1 - e^{-2f}) / ((1 + e^{-g}) (1 + e^{-2f})); f is clamped to +-15
// (tanh = +-1 to 1e-13 there) so that e^{-2f} stays finite.  Relative error ~2e-7 (two v_exp_f32, one v_rcp_f32): used where the result is rounded to bf16
// anyway, and by the F(4,3) stack launch, whose rounding differs from the other fp32 kernels' already.
__device__ __forceinline__ float gate1(float g, float f) {
  f = fminf(fmaxf(f, -15.0f), 15.0f);
  const float eg = __expf(-g), ef = __expf(-2.0f * f);
  return (1.0f - ef) * __frcp_rn((1.0f + eg) * (1.0f + ef));
}

// gate1 for two elements on packed fp32 math (v_pk_mul / v_pk_add / v_pk_fma: two elements per instruction; only the exponentials and the
// reciprocals are per element): `num` x sigmoid(g / s) tanh(f / s) from accumulators that carry a scale s — cg = -log2(e) / s,
// cf = -2 log2(e) / s, lim = 15 s; s = 1, num = 1 is gate1 itself
using f32x2 = __attribute__((ext_vector_type(2))) float;
__device__ __forceinline__ f32x2 gate2_scaled(f32x2 g, f32x2 f, float cg, float cf, float lim, float num) {
  f[0] = __builtin_amdgcn_fmed3f(f[0], -lim, lim);   // (one instruction for the clamp; a NaN comes out as -lim in both forms)
  f[1] = __builtin_amdgcn_fmed3f(f[1], -lim, lim);
  const f32x2 a = g * cg, b = f * cf;
  const f32x2 eg = f32x2{__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])};
  const f32x2 ef = f32x2{__builtin_amdgcn_exp2f(b[0]), __builtin_amdgcn_exp2f(b[1])};
  const f32x2 den = (eg + 1.0f) * (ef + 1.0f);
  const f32x2 r = f32x2{__builtin_amdgcn_rcpf(den[0]), __builtin_amdgcn_rcpf(den[1])};
  return (num - num * ef) * r;
}

// Buffer (SRSRC) addressing: one wave-uniform 128-bit descriptor per tensor, a per-lane 32-bit byte offset that
// is computed once, and a wave-uniform SGPR offset per access — the 32 row-strided loads of an accumulator tile
// then need ONE address VGPR instead of 32 64-bit pairs (what keeps the kernel at <= 80 VGPRs = 3 workgroups/CU).
using rsrc_t = __amdgpu_buffer_rsrc_t;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
__device__ __forceinline__ rsrc_t mk_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float ldf(rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ f32x4 ldf4(rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ __forceinline__ void stf(float v, rsrc_t r, int voff, int soff) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, 0);
}
// uniform part of acc_row(): register r of a 32x32 accumulator covers row (r&3) + 8*(r>>2) (+ 4 for lanes >= 32)
__device__ __forceinline__ constexpr int acc_row0(int r) { return (r & 3) + 8 * (r >> 2); }

// The run-time switches of the denoiser (diffnet.hip, diffnet_h2q.hip; environment), read on first use and never again.  Host side only.
struct DnSwitches {
  int gemm_h2w = env_int("BSG_GEMM_H2W", 1);                  // 0: the conditioner projections on gemm_split_kernel (operands split while staged) instead of the pre-split GEMM
  int cond_quad = env_int("BSG_COND_QUAD", 1);                // 0: prepare writes no channel-quad copy of the conditioner term (nor under BSG_H2_Q=0)
  int cond_bf16_direct = env_int("BSG_COND_BF16_DIRECT", 1);  // 0: bf16 configuration: the term as fp32 rows first, converted to bf16 quads by 20 launches
  int cond_rows = env_int("BSG_COND_ROWS", 0);                // 1: prepare writes the row layout of the term as well as the quads (round 5's way)
  int wino = env_int("BSG_WINO", 2);                          // GEMM1 of the residual block: 2: Winograd F(2,3) kernels and the F(4,3) stack launch; 1: F(2,3) only; 0: the direct K=768 form
  int split = env_int("BSG_SPLIT", 1);                        // 0: no channel-split / 16-wave launches; 2: no 4-way split; 3: pair form only (A/B measurements)
  int stack_bf16 = env_int("BSG_STACK_BF16", 1);              // 0: bf16 configuration on per-layer launches
  int h2 = env_int("BSG_H2", 1);                              // 0: no split-fp16 launches (the kernels of the fp32 matrix pipe)
  int h2_nct = env_int("BSG_H2_NCT", 0);                      // 1 / 2: force 32- / 64-frame tiles of the split-fp16 stack launch (and no part forms)
  int h2_part = env_int("BSG_H2_PART", 1);                    // 0: no part forms
  int h2_quad = env_int("BSG_H2_QUAD", 1);                    // 0: no quads of 32-frame tiles
  int h2_quad64 = env_int("BSG_H2_QUAD64", 1);                // 0: no quads of 64-frame tiles
  int h2_pair64 = env_int("BSG_H2_PAIR64", 1);                // 0: no pairs of 64-frame tiles
  int h2_q = env_int("BSG_H2_Q", 1);                          // 0: the 32-row stack launch (residual_stack_h2_kernel) instead of the 16-row one
  int stack43 = env_int("BSG_STACK43", 1);                    // 0: no F(4,3) stack launch; 2: at any shape (tests)
  int h2_tail = env_int("BSG_H2_TAIL", 1);                    // 0: the step tail as its own launch behind a split-fp16 stack / part launch
  int dual = env_int("BSG_DUAL", 1);                          // 0: no half-batch chains; 2: for big batches only
  int debug_wrap_r04 = env_int("BSG_DEBUG_WRAP_R04", 0);      // 1: round 4's behaviour (only a PART launch zeroes the part flags at a wrap): the negative control of tests/test_gpu_handoff.py
  int h2q_diag = env_int("BSG_H2Q_DIAG", 0);                  // 1 .. 6: timing experiments on the 16-row launches of 64-frame tiles (diffnet_h2q.hip h2q_form; all but 3: wrong results)
  int h2q_fair = env_int("BSG_H2Q_FAIR", 1);                  // 0: no time-sliced issue priority between the two waves of a SIMD
  int cond_tok = env_int("BSG_COND_TOK", 1);                  // 0: behind bsg_diffnet_prepare_tokens the stack launch reads the per-frame term (expanded), not the token table
};
inline const DnSwitches& dn_switches() { static const DnSwitches s; return s; }

// Three switches are NOT cached: they are read again on every call, because tests flip them between calls of one process
// (monkeypatch.setenv of BSG_NO_FUSED_TAIL in tests/test_gpu_sampler.py and of BSG_TAIL_BF16 in tests/test_gpu_bf16.py); BSG_STAMP_MODE
// (tools/stack_stamps.py, tools/wave_stamps.py) has always been read per stamped launch and stays so.
inline bool live_no_fused_tail() { return getenv("BSG_NO_FUSED_TAIL") != nullptr; }   // set to anything: the samplers' unfused loops
inline bool live_tail_bf16() { return env_int("BSG_TAIL_BF16", 1) != 0; }              // 0: bf16 configuration with the fp32 step tail
inline int live_stamp_mode() { return env_int("BSG_STAMP_MODE", 0); }                  // stamp contents of the debug stack launch (0 | 2 | 3 | 5)


}  // namespace bsg
