/* bisinger_hip.h — C ABI of libbisinger_hip.so: the MI355X (gfx950) mel-generation hot path of BiSinger.
 *
 * The reference (BiSinger-SVS/BiSinger) is pure Python on PyTorch and has no FFI of its own; its
 * plug points for this path are Python callables/registries.  Each entry point below
 * names the reference interface it stands behind (paths relative to /root/reference/train_bisinger).
 * The Python drop-ins in bisinger_amd/ (same class names, constructor arguments, state_dict keys) bind
 * these with ctypes: see INTEGRATION.md.
 *
 * Conventions
 *   - return 0 on success, a negative BSG_E* code on failure; never throws; bsg_last_error() gives
 *     the thread-local message of the last failure on the calling thread.
 *   - every tensor argument is a caller-owned, contiguous DEVICE pointer unless it says "host";
 *     float = IEEE fp32, indices = int64 (torch.long), exactly the reference's dtypes.
 *   - the library owns packed copies of the weights and its workspaces (sized at create /
 *     prepare time; nothing is allocated by *_forward / *_sample, which only enqueue on `stream`
 *     and never synchronise the host, so they can be captured into a hipGraph).
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *   - a handle is single-stream and not re-entrant; distinct handles are independent.
 */
#ifndef BISINGER_HIP_H
#define BISINGER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSG_ABI_VERSION 22

#define BSG_OK 0
#define BSG_EINVAL (-22)  /* bad argument / shape the kernels do not support            */
#define BSG_ENOMEM (-12)  /* hipMalloc failed                                            */
#define BSG_EHIP (-5)     /* a HIP runtime call failed (message has hipGetErrorString)   */
#define BSG_ESTATE (-1)   /* call order violated (e.g. forward before prepare)           */

int bsg_abi_version(void);
const char* bsg_last_error(void);
/* Name of device 0's architecture ("gfx950"...), or NULL when no HIP device is usable. */
const char* bsg_device_arch(void);

/* ------------------------------------------------------------------------------------------------
 * DiffNet — the WaveNet noise predictor.
 * Stands behind: DIFF_DECODERS['wavenet'] = lambda hp: DiffNet(hp['audio_num_mel_bins'])
 *   (usr/diffsinger_task.py:24-29) with contract
 *   denoise_fn(spec [B,1,M,T] f32, t [B] i64, cond [B,H,T] f32) -> [B,1,M,T]  (usr/diff/net.py:107-130).
 * ---------------------------------------------------------------------------------------------- */
typedef struct bsg_diffnet bsg_diffnet;

typedef struct {
  int32_t in_dims;               /* M: mel bins, DiffNet(in_dims)                 net.py:82     */
  int32_t residual_channels;     /* C: hparams['residual_channels'] (must be 256) net.py:88     */
  int32_t encoder_hidden;        /* H: hparams['hidden_size']      (must be 256)  net.py:86     */
  int32_t residual_layers;       /* L: hparams['residual_layers']                 net.py:87     */
  int32_t dilation_cycle_length; /* dilation of layer i = 2^(i % cycle), <= 8     net.py:99     */
  int32_t max_steps;             /* rows of step_table (>= diffusion timesteps)                 */
} bsg_diffnet_cfg;

/* dev_weights: 10 + 8*L device pointers in DiffNet.state_dict() order (net.py:91-105):
 *   input_projection.{weight[C,M,1],bias[C]}, mlp.0.{weight[4C,C],bias}, mlp.2.{weight[C,4C],bias},
 *   residual_layers.i.{dilated_conv.weight[2C,C,3],bias, diffusion_projection.weight[C,C],bias,
 *                      conditioner_projection.weight[2C,H,1],bias, output_projection.weight[2C,C,1],bias},
 *   skip_projection.{weight[C,C,1],bias}, output_projection.{weight[M,C,1],bias}.
 * step_table: device [max_steps, C] = SinusoidalPosEmb(C)(arange(max_steps)) (net.py:32-44), built by
 *   the host with the same fp32 ops as the reference so the embedding is bit-identical.
 * The call packs the weights into MFMA fragment order and tabulates mlp(step_table) and every layer's
 * diffusion_projection of it (net.py:119-120, :67) — work that does not depend on the input.
 * Synchronises `stream` before returning (the caller may free/modify its weight tensors afterwards). */
int bsg_diffnet_create(bsg_diffnet** out, const bsg_diffnet_cfg* cfg, const void* const* dev_weights,
                       int32_t n_weights, const float* step_table, void* stream);
void bsg_diffnet_destroy(bsg_diffnet* h);

/* Bind a condition: cond [B,H,T] (= decoder_inp^T, shallow_diffusion_tts.py:235).  Computes every
 * layer's conditioner_projection(cond) + its bias + the dilated conv's bias once ([L,B,2C,T], the
 * step-invariant part of net.py:68-71) and sizes the workspaces for (B,T).  May allocate. */
int bsg_diffnet_prepare(bsg_diffnet* h, const float* cond, int32_t B, int32_t T, void* stream);

/* eps = DiffNet(x, t, cond bound by prepare).  x, eps: [B,M,T] (the reference's [B,1,M,T]); t: [B] i64. */
int bsg_diffnet_forward(bsg_diffnet* h, const float* x, const int64_t* t, float* eps, int32_t B,
                        int32_t T, void* stream);

/* ABI v8, ragged batches: every row at its own length, no padding semantics.
 * bsg_diffnet_prepare_ragged binds cond [B,H,T] (as bsg_diffnet_prepare, which it calls) together with lens (HOST [B], 1 <= lens[b] <= T).
 *   The bsg_diffnet_forward / bsg_ddpm_sample / bsg_plms_sample calls that follow at this (B,T) decode row b on frames [0, lens[b]) as if it
 *   were alone at T = lens[b]: nothing of frames >= lens[b] is read by a frame below it.  T stays the row stride of x, eps, noise and cond.
 *   eps is 0 at frames >= lens[b]; the samplers leave x there as the caller gave it.  Philox draws keep their index (global row, stride T);
 *   bsg_ddpm_sample_rows (ABI v22) draws every row from its own seed at its own length instead: the lone call's draws.
 *   Whole rows are packed into launch groups of at most one 64-frame tile per CU (bsg_ragged_plan); the groups run one after another on
 *   `stream`.  BSG_EINVAL for a row longer than one group; BSG_ESTATE under stream capture (binding and calls).  Both configurations:
 *   fp32 (the ragged 16-row stack launch) and bf16 (bsg_diffnet_set_compute BF16: the ragged bf16 stack launch and bf16 step tail).
 *   A plain bsg_diffnet_prepare clears the ragged binding.
 * bsg_diffnet_ragged_native: *native = 1 when the handle's CURRENT state has the ragged launch for the bound (B,T) — not after
 *   bsg_diffnet_set_h2q / set_h2 / set_split(h, 0) (fp32), not after set_split(h, 0) or with BSG_STACK_BF16=0 / BSG_TAIL_BF16=0 (bf16).
 *   With 0 the compute calls above return BSG_ESTATE on a
 *   ragged binding: the caller decodes the rows one by one (bisinger_amd/diffnet.py does).
 * bsg_ragged_plan: the packing, a pure host function (no device needed): row b of lens[b] frames takes ceil(lens[b] / tile_frames) tiles;
 *   first-fit decreasing into groups of at most `cus` tiles; group_of_row [B] receives each row's group (0-based, launch order). */
int bsg_diffnet_prepare_ragged(bsg_diffnet* h, const float* cond, const int32_t* lens, int32_t B, int32_t T, void* stream);
int bsg_diffnet_ragged_native(bsg_diffnet* h, int32_t B, int32_t T, int32_t* native);
int bsg_ragged_plan(const int32_t* lens, int32_t B, int32_t tile_frames, int32_t cus, int32_t* group_of_row, int32_t* n_groups);

/* ABI v17, a condition that is constant over the frames of a token (the FastSpeech2-MIDI front without a frame-level pitch embedding:
 * decoder_inp[f] = (enc[mel2ph[f]] + spk + style) (mel2ph[f] > 0), fs2.py:225-228): bind it per TOKEN.
 * bsg_diffnet_prepare_tokens: cond_tok [B,K,H] fp32 (K token rows, row 0 = the padding token), tok [B,T] i64 with values in [0,K).
 *   Equivalent to bsg_diffnet_prepare on cond[b][:,f] = cond_tok[b][tok[b][f]]: same workspaces, flags and guard scope.  The hoisted
 *   projection runs on the B K token columns only and is kept as a table [L,B,2C/4,K,4]; no per-frame term is written.  The fp32 16-row
 *   stack launch on 64-frame tiles gathers from the table (bsg_diffnet_last_path "stack_h2q_tok" / "stack_h2q_tok_tail"; BSG_COND_TOK=0:
 *   not); every other launch form reads the per-frame term, expanded from the table by a copy the first time such a launch runs (under
 *   stream capture only when an eager call has allocated it).  Under BSG_COMPUTE_BF16, or where the handle's state has no pre-split
 *   projection, the call expands the condition and takes the per-frame path of bsg_diffnet_prepare itself.
 *   BSG_EINVAL for an id outside [0,K) (checked on the device; the call waits for `stream`.  Under stream capture it cannot wait: ids are
 *   clamped to token 0 there).  A plain bsg_diffnet_prepare (and so bsg_diffnet_prepare_ragged) clears the token binding. */
int bsg_diffnet_prepare_tokens(bsg_diffnet* h, const float* cond_tok, const int64_t* tok, int32_t B, int32_t K, int32_t T, void* stream);

/* Test hook: out [L,B,2C/4,T,4] = the per-frame conditioner term of the bound condition in channel-quad order (what the 16-row stack
 * launch loads); behind bsg_diffnet_prepare_tokens the expansion of the token table.  BSG_ESTATE where the bound state has no quads. */
int bsg_diffnet_debug_cond_quads(bsg_diffnet* h, float* out, int32_t B, int32_t T, void* stream);

/* Per-layer fused residual block alone (net.py:66-78), exported for unit tests and micro-benchmarks:
 * x_in [B,C,T], t [B] -> x_out [B,C,T]; skip [B,C,T] is read-modify-written unless layer == 0
 * (first layer stores); the last layer stores skip_sum / sqrt(L) (net.py:126). */
int bsg_diffnet_residual_layer(bsg_diffnet* h, int32_t layer, const float* x_in, const int64_t* t,
                               float* x_out, float* skip, int32_t B, int32_t T, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Samplers.  Stand behind GaussianDiffusion.p_sample / p_sample_plms and the inference loops
 * (usr/diff/shallow_diffusion_tts.py:159-201, :258-267).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t num_timesteps;
  /* host arrays [num_timesteps] = the module's fp32 buffers (shallow_diffusion_tts.py:103-122) */
  const float* sqrt_recip_alphas_cumprod;
  const float* sqrt_recipm1_alphas_cumprod;
  const float* posterior_mean_coef1;
  const float* posterior_mean_coef2;
  const float* sigma;          /* exp(0.5*posterior_log_variance_clipped), sigma[0] = 0 (:165-166) */
  const float* alphas_cumprod; /* PLMS only (:175-176)                                            */
} bsg_schedule;

/* DDPM ancestral loop B (:265-267): for i = t_start, t_start-1, ..., t_start-n_steps+1:
 *     x <- p_sample(x, full((B,), i), cond)
 * x: [B,M,T] in (x_{t_start+1}) / out.  noise: [n_steps,B,M,T] N(0,1) draws, one per executed step
 * (parity mode), or NULL: draws come from the on-device Philox4x32-10 stream (seed, global row, step)
 * documented in bisinger_amd/synth.py (bench mode).  row0/B_total: global batch row of this shard's
 * row 0 and global batch size, so a sharded run reproduces the unsharded noise.
 * For batches with more 32-frame tiles than the device has CUs the loop runs as two concurrent launch chains over half the
 * rows each: a handle-owned second stream is forked off `stream` and joined back before the call returns (BSG_DUAL=0
 * disables); results are bit-identical either way.
 * On the split-fp16 launches (the default) a call that continues at t_start - n_steps where another call stopped gives the bits of
 * one call over all the steps; on the fp32-pipe and bf16 tails the two agree to rounding. */
int bsg_ddpm_sample(bsg_diffnet* h, const bsg_schedule* s, float* x, const float* noise, uint64_t seed,
                    int32_t t_start, int32_t n_steps, int32_t B, int32_t T, int32_t row0,
                    int32_t B_total, void* stream);

/* One ancestral update given eps (p_sample :159-166 without the denoiser call), for denoisers that are not a
 * bsg_diffnet (the FFT candidate below): x, eps, noise (or NULL = Philox stream of timestep t) are n floats. */
int bsg_ddpm_step(float* x, const float* eps, const float* noise, const bsg_schedule* s, int32_t t, int64_t n,
                  uint64_t seed, uint64_t offset, void* stream);

/* One PLMS update given the noise predictions (p_sample_plms :168-201 without the denoiser calls; ABI v5), for denoisers that are not a
 * bsg_diffnet — DIFF_DECODERS['fft'] under pndm_speedup: x_out = x + x_delta(eps'), eps' = the multistep blend of e0 (the newest prediction)
 * with the n_hist <= 3 older ones e1..e3 (NULL beyond n_hist): n_hist 0: e0 (the predictor half-step of the first iteration); n_hist 1 with
 * avg: (e0 + e1) / 2 (its corrector); 1: (3 e0 - e1) / 2; 2: (23 e0 - 16 e1 + 5 e2) / 12; 3: (55 e0 - 59 e1 + 37 e2 - 9 e3) / 24.
 * alphas_cumprod at t and t_prev = max(t - interval, 0).  x_out may alias x. */
int bsg_plms_step(const float* x, float* x_out, const float* e0, const float* e1, const float* e2, const float* e3, int32_t n_hist,
                  int32_t avg, const bsg_schedule* s, int32_t t, int32_t t_prev, int64_t n, void* stream);

/* x[0..n) <- N(0,1) from the same Philox4x32-10 stream family: element i = lane i%4 of counter
 * ((offset+i)/4, stream_id, 0, 0), key = seed (x_T under gaussian_start uses stream_id 0, the step with
 * timestep i uses stream_id i+1).  n and offset must be multiples of 4. */
int bsg_philox_normal(float* x, int64_t n, uint64_t seed, uint32_t stream_id, uint64_t offset, void* stream);

/* ABI v22, row-keyed draws: a batched row draws what it draws alone.  The unkeyed sampler addresses a step's draws by (global row, padded
 * stride T) under ONE seed, so a row's noise depends on where it sits in its batch and on the batch's longest row.  Keyed, row b has a seed
 * of its own and draws element m n_b + c of the stream (seeds[b], stream_id) at frame c of mel bin m — the lone call's draw at T = n_b,
 * row0 = 0 under seed = seeds[b].
 * bsg_philox_normal_rows: x [B,M,T]; n_b = lengths_host[b] (HOST [B]; NULL: every row is T long); seeds_host: HOST [B].
 *   x[b][m][c] for c < n_b is, bit for bit, what bsg_philox_normal(y, M n_b, seeds_host[b], stream_id, 0) writes to y[m n_b + c]; x[b][m][c] = 0
 *   for n_b <= c < T.  M = 1 covers the flat layouts whose lone prefix is contiguous (the NSF noise [B][L NH], Parallel WaveGAN's z [B][L]).
 *   Seeds and lengths travel in the launches' arguments (32 rows per launch): no device table, no copy, no host synchronisation — the
 *   call only enqueues and can be captured.  BSG_EINVAL, naming the row, with nothing enqueued: x or seeds_host NULL, B <= 0, n_b outside
 *   1..T, M n_b no multiple of 4 (bsg_philox_normal refuses that n as well).
 * bsg_ddpm_sample_rows: bsg_ddpm_sample(h, s, x, NULL, ., t_start, n_steps, B, T, 0, B, stream) with the draws of the step at timestep i
 *   from bsg_philox_normal_rows(stream id i + 1) over the row lengths of the handle's binding (bsg_diffnet_prepare_ragged's lens; T behind
 *   any other prepare): filled into a handle-owned [B,M,T] buffer in front of the step's launches and read by them as supplied noise.  Where
 *   the loop runs as two half-batch chains each half's draws are enqueued on that half's stream.  The buffer is allocated by the first
 *   eager call of a shape (BSG_EINVAL under stream capture until then).  The same launch forms as bsg_ddpm_sample with `noise`. */
int bsg_philox_normal_rows(float* x, int32_t B, int32_t M, int32_t T, const int32_t* lengths_host, const uint64_t* seeds_host,
                           uint32_t stream_id, void* stream);
int bsg_ddpm_sample_rows(bsg_diffnet* h, const bsg_schedule* s, float* x, const uint64_t* seeds_host, int32_t t_start, int32_t n_steps,
                         int32_t B, int32_t T, void* stream);

/* Glue of GaussianDiffusion.forward around the loop (shallow_diffusion_tts.py:244-272), all [B,M,T] <-> [B,T,M]:
 *   bsg_mel_start : x = sqrt_ac * norm_spec(fs2_mel)^T + sqrt_1m_ac * noise      (q_sample at t = K_step-1, :249-252)
 *   bsg_mel_finish: mel_out = denorm_spec(x^T) * (mel2ph > 0)   (mel2ph NULL: no mask, the non-singing branch :271-272)
 * spec_min / spec_max: device [M] (the module's buffers). */
int bsg_mel_start(const float* fs2_mel, const float* spec_min, const float* spec_max, const float* noise,
                  float sqrt_ac, float sqrt_1m_ac, float* x, int32_t B, int32_t M, int32_t T, void* stream);
int bsg_mel_finish(const float* x, const float* spec_min, const float* spec_max, const int64_t* mel2ph,
                   float* mel_out, int32_t B, int32_t M, int32_t T, void* stream);

/* Live timing of the dominant kernel (bench.py's roofline): while enabled, every DiffNet evaluation records
 * a hipEvent pair around its L fused residual-layer launches on the launch stream.  profile_read waits for the
 * recorded events and returns the summed device time and the number of layer-equivalents they cover (L per evaluation,
 * also when the L layers run as one stack launch). */
int bsg_diffnet_profile(bsg_diffnet* h, int32_t enable);
int bsg_diffnet_profile_read(bsg_diffnet* h, double* layer_ms_total, int64_t* n_layer_launches);
/* Arithmetic of the fused residual layers (BASELINE config "bf16 diffusion mel-gen"):
 *   BSG_COMPUTE_F32  (default) fp32 operands, fp32 MFMA — the parity configuration (<= 1e-3 on the mel);
 *   BSG_COMPUTE_BF16 MFMA operands (weights, staged x + d, gated z) rounded to bf16 (RNE), fp32 accumulation, fp32
 *                    gate/epilogue, and x / conditioner term / skip kept fp32 in HBM — a throughput configuration
 *                    whose deviation from the fp32 path is reported by tests/test_gpu_bf16.py and bench.py.
 * Takes effect on the next forward / sample call on the handle. */
#define BSG_COMPUTE_F32 0
#define BSG_COMPUTE_BF16 1
int bsg_diffnet_set_compute(bsg_diffnet* h, int32_t mode);
/* Synchronous health check of the launches that hand data between workgroups (the on-chip stack launch, whose neighbouring
 * tiles exchange their edges every layer, and the channel-split launch used for small batches): number of inter-workgroup hand-off spins that
 * gave up since the handle was bound (must be 0; non-zero means a result is invalid). */
int bsg_diffnet_status(bsg_diffnet* h, int32_t* handoff_timeouts);
/* Asynchronous form (ABI v5: THREE words): enqueues copies of the handle's health words into host_counts[0..2] (pinned host memory,
 * caller-owned) on `stream` and returns; the values are valid once the stream has passed that point (e.g. an event recorded after the
 * call): [0] hand-off give-ups of the stack / part launches, [1] values beyond the fp16 range seen by the split-fp16 stack / part / tail
 * launches (16-row stack launch: |x| >= 3750; 32-row launch, part forms and tails: |x + d| >= 60000: the result is invalid, repeat with
 * bsg_diffnet_set_h2q(h, 0) after a 16-row launch, with bsg_diffnet_set_h2(h, 0) otherwise), [2] give-ups of the channel-split launches.
 * Nothing is reset (bsg_diffnet_health_take does that).  Lets a caller fail loudly — or repeat — one call later without adding a
 * synchronisation to the path: what a replayed capture of the sampler loop (round 4: the stack / part launches keep their launch epoch in
 * device memory and can be captured) and the `deferred` guard mode of the Python drop-ins use. */
int bsg_diffnet_status_async(bsg_diffnet* h, int32_t* host_counts, void* stream);
/* Same-call form (what the Python drop-ins use): waits for `stream`, returns the give-up count accumulated since the last
 * take and resets it.  bsg_diffnet_uses_handoffs says whether launches of shape (B,T) on this handle may hand data between
 * workgroups at all (small batches: B*ceil(T/32) <= CUs); when it says 0 no check — and no synchronisation — is needed.
 * bsg_diffnet_set_split(h, 0) makes the handle use one-workgroup-per-tile launches only (no hand-offs): the caller's
 * recovery after a non-zero take is set_split(0) + re-running the evaluation, which then cannot give up. */
int bsg_diffnet_handoff_take(bsg_diffnet* h, int32_t* handoff_timeouts, void* stream);
/* The same take with the two causes apart (ABI v4): counts[0] = hand-off spins that gave up (a partner workgroup was not resident:
 * recovery = bsg_diffnet_set_split(h, 0)); counts[1] = values beyond the fp16 range seen by the split-fp16 stack launch (data, not
 * residency: recovery = bsg_diffnet_set_h2(h, 0), the fp32-matrix-pipe kernels, for this input only).  Waits for `stream`; resets both.
 * bsg_diffnet_handoff_take returns their sum. */
int bsg_diffnet_health_take(bsg_diffnet* h, int32_t* counts, void* stream);
int bsg_diffnet_uses_handoffs(bsg_diffnet* h, int32_t B, int32_t T, int32_t* uses);
int bsg_diffnet_set_split(bsg_diffnet* h, int32_t enable);
/* Fault injection for tests: in the next n_launches channel-split (or stack) launches on the handle the consumers give up every
 * hand-off without waiting (counted exactly like a timed-out spin) and one producer per tile (pair) never publishes, so the
 * consumers deterministically read stale exchange data. */
int bsg_diffnet_debug_inject_giveup(bsg_diffnet* h, int32_t n_launches);
/* Fault injection (ABI v6): in the next n_launches PART launches (several workgroups per tile on CUs of one XCD) the odd parts report
 * another XCC id than the one they run on — a dispatch order other than workgroup i -> XCD i mod 8.  Counted as hand-off give-ups. */
int bsg_diffnet_debug_inject_xcc(bsg_diffnet* h, int32_t n_launches);
/* Part forms on (1, default) / off (0) for this handle (ABI v6): with them off small batches run the one-workgroup-per-tile stack launch,
 * which exchanges only tile edges with write-through stores and needs no placement on one XCD.  First tier of the recovery after a
 * give-up inside a part launch; bsg_diffnet_set_split(h, 0) (no hand-off launches at all) is the second. */
int bsg_diffnet_set_parts(bsg_diffnet* h, int32_t enable);
/* Test hook (ABI v6): sets the device-side launch epoch of the handle's stack / part launches (hand-off flag values are epoch x 64 + layer;
 * the epoch restarts at 1, with every flag array of the handle zeroed, once it reaches 2^25).  Waits for `stream`.  epoch >= 1. */
int bsg_diffnet_debug_set_epoch(bsg_diffnet* h, uint32_t epoch, void* stream);
/* Name of the form the last residual-layer launch on the handle took.  All L layers in one launch with the residual stream on chip:
 * "stack_h2_quad" / "stack_h2_quad64" / "stack_h2_pair64" (a tile as 4 / 4 / 2 workgroups), "stack_h2q" / "stack_h2" (16- / 32-row
 * split-fp16 launch), "stack_f43", "stack_bf16"; "_tail" behind a name: the sampler's step tail ran inside the launch; "_ragged": a
 * ragged batch.  One launch per layer: "layer" (one workgroup per tile), "split2" / "split4" (a tile as 2 / 4 workgroups), "wide" (one
 * 16-wave workgroup per tile), "bf16".  "none" before the first launch.  Static string. */
const char* bsg_diffnet_last_path(bsg_diffnet* h);
/* ABI v14: what last_path does not say.  chains: launch chains of the handle's last bsg_ddpm_sample / bsg_plms_sample (2: the two
 * half-batch chains on two streams, 1: one chain or a call that returned before its loop ended, 0: no sampler call yet); groups: launch groups of whole rows of the last stack launch
 * (0: the last residual-layer launch was no stack launch).  Host state only: no wait, no launch. */
int bsg_diffnet_last_launch(bsg_diffnet* h, int32_t* chains, int32_t* groups);
/* Shader clock the chip held over the last PROFILED stack launch (bsg_diffnet_profile on): tile 0 of the launch stores s_memtime (shader
 * clocks) and s_memrealtime (100 MHz) at its start and end; shader_mhz = their ratio, span_us = the launch's in-kernel span.  Synchronous
 * copy; 0 when no profiled stack launch has run (ABI v4). */
int bsg_diffnet_clock_read(bsg_diffnet* h, double* shader_mhz, double* span_us);

/* Diagnostic run of the stack launch on whatever h->xa holds (timing only): the L layers of the bound batch (which must fit one
 * launch) at timestep t_uniform, with s_memrealtime (100 MHz) stamps per tile and layer at
 * {0 xs complete, 1 GEMM1 done, 2 z in LDS, 3 residual half done, 4 skip half done, 5 edges drained, 6 neighbours' flags seen,
 *  7 halo barrier passed} into stamps [B*ceil(T/32)][L][8] (device, uint64).  Used by tools/stack_stamps.py. */
int bsg_diffnet_debug_stack_stamps(bsg_diffnet* h, int32_t t_uniform, int32_t B, int32_t T, uint64_t* stamps, void* stream);

/* Diagnostic build of the fused residual layer (separate kernel instantiation; the product kernel executes no
 * stamp): same computation, plus s_memtime stamps per wave at the phase boundaries
 * {0 start, 1 staged, 2 acc init, 3 GEMM1 done, 4 gate done, 5 z in LDS, 6 GEMM2 residual pass, 7 skip pass}
 * into stamps [B*ceil(T/32)][8 waves][10] (device, uint64; slots 8, 9 = s_memrealtime (100 MHz) at start / end, which
 * gives the shader clock the chip held).  Never timed; used by tools/stamp_layer.py. */
int bsg_diffnet_debug_stamps(bsg_diffnet* h, int32_t layer, const float* x_in, const int64_t* t, float* x_out,
                             float* skip, int32_t B, int32_t T, uint64_t* stamps, void* stream);

/* PLMS / PNDM loop A (:258-264, p_sample_plms :168-201): for i in reversed(range(0,K_step,interval)).
 * Batched semantics = element-wise clamp of t-interval (the reference raises for B>1, :189). */
int bsg_plms_sample(bsg_diffnet* h, const bsg_schedule* s, float* x, int32_t K_step, int32_t interval,
                    int32_t B, int32_t T, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FastSpeech2-MIDI: phoneme/pitch encoder -> per-frame condition, and the FFT mel decoder.
 * Stands behind FastSpeech2MIDI.forward (modules/diffsinger_midi/fs2.py:94-197), split at the one
 * data-dependent point of the reference (the length regulator's output length, tts_modules.py:182):
 *   encode  = embeddings + ESM + FastspeechMIDIEncoder (+ DurationPredictor.inference)     fs2.py:111-165
 *   bsg_length_regulator = LengthRegulator.forward                                 tts_modules.py:161-191
 *   decode  = gather by mel2ph, +spk +style, mask -> decoder_inp; FastspeechDecoder + mel_out  fs2.py:166-195
 * ---------------------------------------------------------------------------------------------- */
typedef struct bsg_fs2midi bsg_fs2midi;

typedef struct {
  int32_t hidden_size;          /* must be 256                                  hparams['hidden_size']   */
  int32_t vocab;                /* len(phone_encoder)                           fastspeech/fs2.py:94     */
  int32_t enc_layers, dec_layers, num_heads;
  int32_t enc_ffn_kernel_size, dec_ffn_kernel_size;
  int32_t out_dims;             /* mel bins                                                              */
  int32_t dur_layers, dur_kernel;
  int32_t spk_rows;             /* num_spk + 1                                  fastspeech/fs2.py:40     */
  int32_t esm_heads;            /* 8                                            diffsinger_midi/fs2.py:83 */
  int32_t n_pos;                /* rows of dec_pos_table (frames T must be < n_pos)                      */
  int32_t n_rel;                /* rows of rel_pos_table (T_txt must be <= n_rel)                        */
} bsg_fs2midi_cfg;

/* Number of entries of FastSpeech2MIDI.state_dict() for this configuration (143 for BiSinger). */
int bsg_fs2midi_n_weights(const bsg_fs2midi_cfg* cfg);

/* dev_weights: device pointers in FastSpeech2MIDI.state_dict() order (tests/golden/state_dict_spec.json,
 * keys 'fs2.*'): encoder_embed_tokens, decoder.{pos_embed_alpha, embed_positions._float_tensor,
 * layers.i.op.{layer_norm1.w,b, self_attn.in_proj_weight, self_attn.out_proj.weight, layer_norm2.w,b,
 * ffn.ffn_1.w,b, ffn.ffn_2.w,b}, layer_norm.w,b}, mel_out.w,b, spk_embed_proj, dur_predictor.{conv.i.1.w,b,
 * conv.i.3.w,b, linear.w,b}, esm.{mh.in_proj_weight, in_proj_bias, out_proj.w,b, ffn.0.w,b, ffn.2.w,b,
 * ln1.w,b, ln2.w,b}, encoder.{layers..., layer_norm.w,b, embed_tokens (alias), esm.* (alias)},
 * midi_embed, midi_dur_layer.w,b, is_slur_embed, lang_embed, style_embed.
 * dec_pos_table [n_pos,H]: SinusoidalPositionalEmbedding table (common_layers.py:124-146, row 0 zero);
 * rel_pos_table [n_rel,H]: RelPositionalEncoding's reversed table rows 0..n_rel-1 of max_len 5000
 * (espnet_positional_embedding.py:25-46) — both built by the host with the reference's own fp32 ops.
 * The library keeps its own (re-packed) copies; synchronises `stream` before returning. */
int bsg_fs2midi_create(bsg_fs2midi** out, const bsg_fs2midi_cfg* cfg, const void* const* dev_weights,
                       int32_t n_weights, const float* dec_pos_table, const float* rel_pos_table, void* stream);
void bsg_fs2midi_destroy(bsg_fs2midi* h);

/* txt, pitch_midi, is_slur, lang: [B,T_txt] i64; midi_dur [B,T_txt] f32; spk_id [B] i64.
 * enc_out [B,T_txt,H].  dur_xs [B,T_txt] f32 (log-domain predictor output, ret['dur']) and dur [B,T_txt] i64
 * (ret['dur_choice']) are both NULL (mel2ph given) or both set (mel2ph predicted).  May grow workspaces. */
int bsg_fs2midi_encode(bsg_fs2midi* h, const int64_t* txt, const int64_t* pitch_midi, const float* midi_dur,
                       const int64_t* is_slur, const int64_t* lang, const int64_t* spk_id, int32_t B,
                       int32_t T_txt, float* enc_out, float* dur_xs, int64_t* dur, void* stream);

/* ABI v7 (one rank of a sharded batch): the same front for the batch rows [row0, row0 + n_rows) only.  The inputs are the
 * WHOLE batch's ([B,T_txt] / [B]); enc_out [n_rows,T_txt,H], dur_xs / dur [n_rows,T_txt].  Only the ESM couples the utterances of a batch
 * (it attends over the batch axis, common_layers.py:853) and only through K / V = projections of LN(lang_embed[lang]) (:850-853): K / V
 * are projected for all B rows; Q, the ESM's FFN, the embedding sum, the FFT encoder (tts_modules.py:312-328) and the duration predictor
 * run on the n_rows rows asked for.  Row for row the result equals bsg_fs2midi_encode's on the whole batch (same kernels, same order of
 * summation per row).  row0 = 0, n_rows = B is bsg_fs2midi_encode. */
int bsg_fs2midi_encode_rows(bsg_fs2midi* h, const int64_t* txt, const int64_t* pitch_midi, const float* midi_dur,
                            const int64_t* is_slur, const int64_t* lang, const int64_t* spk_id, int32_t B, int32_t T_txt,
                            int32_t row0, int32_t n_rows, float* enc_out, float* dur_xs, int64_t* dur, void* stream);

/* ABI v7, introspection (tests): token rows (utterances x T_txt) the last encode ran its ENCODER on, and rows of the last FFT stack
 * (encoder or decoder) — how a test sees that a rank's front did not encode the other ranks' utterances. */
int bsg_fs2midi_last_rows(const bsg_fs2midi* h, int32_t* token_rows, int32_t* stack_rows);

/* ABI v11: the launch forms of the handle's last bsg_fs2midi_encode[_rows] and of the last bsg_fs2midi_decode after it, as tokens separated
 * by blanks in launch order; "none" for a null handle or before the first call.  A token is written at the branch that launched, so it
 * names what ran, not what the thresholds would choose; a form that a stack launches again (in every layer, as a rule) is named once.
 * An encode starts the record anew; a decode replaces the tokens of the decode before it.
 *   esm:wave | esm:thread                              esm_attention_wave_kernel | esm_attention_kernel<32>
 *   <s>.qkv:fused | split_kernel | h2w | gemm          Q / K / V^T planes from the QKV product's own epilogue | fp32 QKV + qkv_split_kernel |
 *                                                      fp32 QKV of the pre-split GEMM | of launch_gemm
 *   <s>.attn:planes/ks<n>                              flash_attn_planes_kernel<2>, the keys over n workgroups
 *   <s>.attn:split/nw2 | split/nw4 | flash/nw2 | flash/nw4 | softmax
 *                                                      flash_attn_split_kernel<NW> | flash_attn_kernel<NW> | score tensor + masked_softmax_kernel
 *   <s>.gemm:h2w/<32|64|128>/<ring4|ring8|ring16|deep> gemm_h2w_kernel: rows per tile, steps of the weight ring (deep: 256-deep slices)
 *   <s>.gemm:gemm_split/<64|128> | gemm_fast/<64|128> | gemm_f32
 *                                                      launch_gemm: split-fp16 | fp32 matrix pipe | the unaligned form
 *   tok:front                                          token_front_kernel (the plain front's embedding, ABI v16)
 *   esm:alone tok:ragged dec.ragged                    the ragged entries (ABI v20, below): the ESM's two-row table, the ragged embedding launch, a ragged decode
 *   pit.pos pit.entry pit.gemm:<form as above> pit.ln pit.tail pit.launches:<n>   the pitch adaptor of a decode (ABI v16, bsg_fs2_decode)
 * with <s> = esm (the ESM's Linear layers), enc, dec (the FFT stacks); bsg_fftden_last_path: den, cleared by every bsg_fftden_forward.
 * The string belongs to the handle: valid until its next call or its destruction. */
const char* bsg_fs2midi_last_path(bsg_fs2midi* h);

/* ABI v11, test hook: fills every activation workspace of the handle, at its current capacity, with 0xFF bytes (NaN as fp16 and as fp32)
 * on `stream` — stale data that no result may depend on (tests/test_gpu_fs2_shapes.py).  Weights, the key split's arrival counters and,
 * for bsg_fftden, the result of bsg_fftden_prepare are left alone. */
int bsg_fs2midi_debug_poison_workspace(bsg_fs2midi* h, void* stream);

/* mel2ph [B,T] from dur [B,T_txt] (padded tokens, txt == 0, count 0 when txt != NULL); T = max_b sum(dur). */
int bsg_length_regulator(const int64_t* dur, const int64_t* txt, int64_t* mel2ph, int32_t B, int32_t T_txt,
                         int32_t T, void* stream);

/* decoder_inp [B,T,H] (ret['decoder_inp']); mel_out [B,T,out_dims] (ret['mel_out']) or NULL = skip_decoder. */
int bsg_fs2midi_decode(bsg_fs2midi* h, const float* enc_out, const int64_t* mel2ph, const int64_t* spk_id,
                       const int64_t* speechsing, int32_t B, int32_t T_txt, int32_t T, float* decoder_inp,
                       float* mel_out, void* stream);

/* ABI v17: the condition per TOKEN, for bsg_diffnet_prepare_tokens: cond_tok [B,T_txt+1,H], row 0 = the padding token (what a frame with
 * mel2ph = 0 gets), row k = enc_out[k-1] + spk + style — the expression and order of the decode's gather, so that cond_tok[b][mel2ph[b][f]]
 * equals decoder_inp[b][f] bit for bit.  Handles without use_pitch_embed only (with it the condition is per frame: BSG_EINVAL). */
int bsg_fs2midi_token_rows(bsg_fs2midi* h, const float* enc_out, const int64_t* spk_id, const int64_t* speechsing, int32_t B,
                           int32_t T_txt, float* cond_tok, void* stream);

/* ABI v16: the frame-level pitch adaptor (hparams['use_pitch_embed'], FastSpeech2.add_pitch, modules/fastspeech/fs2.py:201-234, with
 * pitch_type: frame, pitch_ar: false, pitch_norm: log) and the plain FastSpeech2 front (use_midi absent or false, fs2.py:24-152:
 * FastspeechEncoder, tts_modules.py:312-349, without rel_pos).  bsg_fs2_create returns the SAME handle type as bsg_fs2midi_create:
 * bsg_fs2midi_decode, _last_path, _last_rows, _debug_poison_workspace, the per-handle range-guard calls and bsg_fs2midi_destroy work on
 * it unchanged; with front = BSG_FS2_FRONT_MIDI and use_pitch_embed = 0 it is bsg_fs2midi_create. */
#define BSG_FS2_FRONT_MIDI 0   /* FastSpeech2MIDI: ESM + MIDI / slur / language embeddings, style row in the decoder input */
#define BSG_FS2_FRONT_PLAIN 1  /* FastSpeech2: sqrt(H) * embed_tokens[txt] + sinusoidal positions counted over the non-pad tokens */

typedef struct {
  bsg_fs2midi_cfg base;      /* plain front: esm_heads is ignored, spk_rows may be 0 (use_spk_id: false), n_rel = rows of tok_pos_table */
  int32_t front;             /* BSG_FS2_FRONT_*                                                                                     */
  int32_t use_pitch_embed;   /* 0 | 1; the four fields below are read only when it is 1                                             */
  int32_t pitch_layers;      /* hparams['predictor_layers']                                                       fs2.py:75-81      */
  int32_t pitch_kernel;      /* hparams['predictor_kernel'] (odd: ffn_padding SAME)                                                 */
  int32_t use_uv;            /* hparams['use_uv']: uv = pitch_pred[..., 1] > 0 zeroes f0_denorm                   fs2.py:226-227    */
  int32_t n_pitch_pos;       /* rows of pitch_pos_table (frames T must be < n_pitch_pos)                                            */
} bsg_fs2_cfg;

/* Entries of the model's state_dict() for this configuration (114 for the PopCS chain: plain front, no speaker table, 2-layer duration
 * and pitch predictors), or BSG_EINVAL for a configuration bsg_fs2_create refuses. */
int bsg_fs2_n_weights(const bsg_fs2_cfg* cfg);

/* dev_weights in state_dict() order.  MIDI front: as bsg_fs2midi_create, with pitch_embed.weight [300,H] and pitch_predictor.{pos_embed_alpha,
 * conv.l.1.{weight [H,H,k], bias}, conv.l.3.{weight, bias}, linear.{weight [2,H], bias}, embed_positions._float_tensor} between
 * dur_predictor.* and esm.* when use_pitch_embed.  Plain front: encoder_embed_tokens, encoder.{layers.*, layer_norm.w,b, embed_tokens (alias),
 * embed_positions._float_tensor}, decoder.{pos_embed_alpha, embed_positions._float_tensor, layers.*, layer_norm.w,b}, mel_out.w,b,
 * spk_embed_proj (when spk_rows > 0), dur_predictor.*, then the pitch entries.
 * tok_pos_table [n_rel,H]: MIDI front: rel_pos_table of bsg_fs2midi_create; plain front: the sinusoidal table the token positions index
 * (T_txt must be < n_rel).  pitch_pos_table [n_pitch_pos,H] (NULL without use_pitch_embed): the sinusoidal table of PitchPredictor
 * (tts_modules.py:221).  A bad configuration is BSG_EINVAL with a message before any device call. */
int bsg_fs2_create(bsg_fs2midi** out, const bsg_fs2_cfg* cfg, const void* const* dev_weights, int32_t n_weights,
                   const float* dec_pos_table, const float* tok_pos_table, const float* pitch_pos_table, void* stream);

/* The plain front's encode (fs2.py:100-129): txt [B,T_txt] i64 (pad id 0), spk_id [B] i64 or NULL (no speaker table), for the batch rows
 * [row0, row0 + n_rows) (nothing couples the rows of a batch: row0 = 0, n_rows = B is the whole batch).  enc_out [n_rows,T_txt,H];
 * dur_xs / dur [n_rows,T_txt] as for bsg_fs2midi_encode.  One launch forms the embedding (tok:front in the launch record). */
int bsg_fs2_encode_plain(bsg_fs2midi* h, const int64_t* txt, const int64_t* spk_id, int32_t B, int32_t T_txt, int32_t row0,
                         int32_t n_rows, float* enc_out, float* dur_xs, int64_t* dur, void* stream);

/* bsg_fs2midi_decode with the adaptor's inputs and outputs.  spk_id NULL without a speaker table, speechsing NULL on the plain front.
 * f0 [B,T] f32 (log2 Hz) and uv [B,T] f32 (> 0 = unvoiced) are supplied values or NULL = the predictor's (uv is ignored without use_uv);
 * neither is written.  pitch_pred [B,T,2] (the predictor runs with supplied f0 too, as the reference's does; with predicted f0 its
 * [..., 0] is 0 where mel2ph == 0, as the reference returns it: its in-place f0[pitch_padding] = 0 goes through a view), f0_denorm [B,T] =
 * 2^f0, 0 where unvoiced or mel2ph == 0, pitch_bin [B,T] i64 = f0_to_coarse(f0_denorm) (utils/pitch_utils.py:22-31): each may be NULL.
 * Without use_pitch_embed all five must be NULL.  decoder_inp = (enc[mel2ph] + pitch_embed[bin] + spk (+ style)) * (mel2ph > 0).
 * Launch record: pit.pos, pit.entry, pit.gemm:<form> (the predictor's k-tap convolutions with bias + ReLU), pit.ln (the LayerNorm launches
 * between the layers; absent with one layer), pit.tail (the last layer's LayerNorm, Linear(256 -> 2), exp2, zeroing, bin, embedding gather,
 * sum and mask in one launch, one wavefront per frame) and pit.launches:<n>, the adaptor's launches of this decode counted where they
 * were made (a form launched in every layer is named once, so the count is what tells a missing layer).
 * Token, speaker and style ids outside their tables are clamped by the kernels of this ABI version's additions (torch raises).
 * On a plain-front handle bsg_fs2midi_decode takes the same NULLs (spk_id without a speaker table, speechsing always). */
int bsg_fs2_decode(bsg_fs2midi* h, const float* enc_out, const int64_t* mel2ph, const int64_t* spk_id, const int64_t* speechsing,
                   const float* f0, const float* uv, int32_t B, int32_t T_txt, int32_t T, float* pitch_pred, float* f0_denorm,
                   int64_t* pitch_bin, float* decoder_inp, float* mel_out, void* stream);

/* ABI v20: ragged batches through the front — every utterance as the B = 1 call on its own tokens and frames, worded after
 * bsg_hifigan_forward_ragged / bsg_pitchext_forward_ragged.  The tensors keep their padded shapes ([B,T_txt] / [B,T]: the pitches); the
 * counts are HOST arrays read before the call returns: n_tok_host[b] in 1 .. T_txt tokens (the non-pad tokens, a prefix of the row),
 * n_frames_host[b] in 0 .. T frames (the frames with mel2ph > 0, a prefix).  A null array or a count outside its range is BSG_EINVAL with
 * a message before any device call.  Every output of utterance b on [:n_tok] / [:n_frames] is what the padded entry returns for the
 * B = 1 call on txt[b, :n_tok], ..., mel2ph[b, :n_frames] (to rounding: the sums are blocked differently); beyond an utterance's end
 * every float output is 0, dur is 0 and pitch_bin is 1 (f0_to_coarse(0)), and NO input is read there.  What differs from the padded call:
 *   the ESM (MIDI front) is the utterance's own: at B = 1 its attention over the batch axis has one key, so its result is a function of
 *   the token's lang id — a two-row table per call, gathered in the embedding sum (esm:alone, tok:ragged in the launch record);
 *   the k-tap convolutions of the FFT stacks and of the pitch predictor read zeros beyond an utterance's end in every layer (the padded
 *   call reads LayerNorm's bias there);
 *   nothing is computed beyond an utterance's end: LayerNorm rows, GEMM tiles, attention query tiles and key blocks that lie there return
 *   before their first load.  bsg_fs2midi_last_rows then reports sum_b min(T, 32 * ceil(n_b / 32)) — rows in 32-row granules, the smallest
 *   tile of any launch (64- and 128-row tiles round further) — for token_rows and stack_rows after an encode, stack_rows after a decode.
 * The launch record adds tok:ragged / dec.ragged.  The QKV and attention forms are the padded call's at (B, T); the GEMM tile heights follow
 * the same rules applied to (T rows, batch B) — the row-wise products go out as B problems of T rows — so near a threshold a tile token can
 * differ from the padded call's.  A stack whose only attention form would be the score tensor (head dim other than 128,
 * BSG_NO_FLASH_ATTN) is BSG_EINVAL before any device call.
 * bsg_fs2_decode_ragged serves handles without the adaptor too (the five adaptor pointers NULL) and both fronts.  Workspaces grow as in
 * every entry: a capturing stream that would have to grow one is refused before anything is touched. */
int bsg_fs2midi_encode_ragged(bsg_fs2midi* h, const int64_t* txt, const int64_t* pitch_midi, const float* midi_dur, const int64_t* is_slur,
                              const int64_t* lang, const int64_t* spk_id, const int32_t* n_tok_host, int32_t B, int32_t T_txt, float* enc_out,
                              float* dur_xs, int64_t* dur, void* stream);
int bsg_fs2_encode_plain_ragged(bsg_fs2midi* h, const int64_t* txt, const int64_t* spk_id, const int32_t* n_tok_host, int32_t B, int32_t T_txt,
                                float* enc_out, float* dur_xs, int64_t* dur, void* stream);
int bsg_fs2_decode_ragged(bsg_fs2midi* h, const float* enc_out, const int64_t* mel2ph, const int64_t* spk_id, const int64_t* speechsing,
                          const float* f0, const float* uv, const int32_t* n_tok_host, const int32_t* n_frames_host, int32_t B, int32_t T_txt,
                          int32_t T, float* pitch_pred, float* f0_denorm, int64_t* pitch_bin, float* decoder_inp, float* mel_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FFT candidate denoiser: DIFF_DECODERS['fft'] = FFT(hidden, dec_layers, dec_ffn_kernel_size,
 * num_heads) (usr/diffsinger_task.py:26-28, usr/diff/candidate_decoder.py:39-100); same denoise_fn contract as DiffNet.
 * dev_weights in FFT.state_dict() order: pos_embed_alpha, embed_positions._float_tensor, layers.i.op.* (10 per layer),
 * layer_norm.{w,b}, input_projection.{w,b}, mlp.0.{w,b}, mlp.2.{w,b}, get_mel_out.{w,b}, get_decode_inp.{w,b}.
 * step_table [max_steps,256] and pos_table [n_pos,256] as for bsg_diffnet_create / bsg_fs2midi_create.
 * ---------------------------------------------------------------------------------------------- */
typedef struct bsg_fftden bsg_fftden;
int bsg_fftden_n_weights(int32_t n_layers);
int bsg_fftden_create(bsg_fftden** out, int32_t in_dims, int32_t n_layers, int32_t num_heads, int32_t ffn_kernel,
                      int32_t max_steps, int32_t n_pos, const void* const* dev_weights, int32_t n_weights,
                      const float* step_table, const float* pos_table, void* stream);
void bsg_fftden_destroy(bsg_fftden* h);
int bsg_fftden_prepare(bsg_fftden* h, const float* cond, int32_t B, int32_t T, void* stream);
int bsg_fftden_forward(bsg_fftden* h, const float* x, const int64_t* t, float* eps, int32_t B, int32_t T, void* stream);
/* ABI v11: as bsg_fs2midi_last_path / bsg_fs2midi_debug_poison_workspace, for the stack of the last bsg_fftden_forward ("den." tokens) */
const char* bsg_fftden_last_path(bsg_fftden* h);
int bsg_fftden_debug_poison_workspace(bsg_fftden* h, void* stream);
/* ABI v22 (additions, as the PWG ragged entries were to v20): ragged batches through the FFT denoiser.
 * bsg_fftden_prepare_ragged binds `cond` [B,256,T] for a batch whose row b has lengths_host[b] frames (HOST array, B ints in 1..T, read
 * before the call returns; they reach the kernels through a device row of the handle that launches of the call fill).  A bad length or
 * argument is BSG_EINVAL with a message before any device call; a capturing stream is BSG_ESTATE with nothing enqueued; a head dimension
 * other than 128 or BSG_NO_FLASH_ATTN (the score-tensor attention has no lengths) is BSG_EINVAL.  The hoisted condition part is projected on
 * the live frames only.  A later bsg_fftden_prepare makes the handle padded again.
 * On a ragged-bound handle bsg_fftden_forward(h, x, t, eps, B, T) gives row b ALONE: eps[b, :, :n_b] is the denoiser on x[b:b+1, :, :n_b],
 * t[b], cond[b:b+1, :, :n_b] (B = 1, T = n_b) — positions count the row's own frames, attention keys end at n_b, the k-tap FFN convolution
 * reads zeros beyond n_b in every layer, the last LayerNorm and get_mel_out run on live frames only — and eps[b, :, n_b:] = 0.  Nothing at
 * or beyond a row's end is read (x and cond may hold NaN there; what an earlier call left in the workspaces does not matter) and no dead
 * frame is computed.  bsg_fftden_last_path of a ragged call starts with the token "den.ragged"; the padded call's record is unchanged. */
int bsg_fftden_prepare_ragged(bsg_fftden* h, const float* cond, const int32_t* lengths_host, int32_t B, int32_t T, void* stream);
/* The sampler loops over this denoiser, worded after bsg_ddpm_sample / bsg_ddpm_sample_rows / bsg_plms_sample.  Both run on whatever
 * binding the handle has (padded or ragged; (B, T) must be the binding's), enqueue every step on `stream` and never synchronise.  Per
 * evaluation: the denoiser up to its last LayerNorm, then ONE launch that does get_mel_out (256 -> in_dims <= 80), the DDPM or PLMS update
 * with the schedule values of the step, the draw, and the store into x [B,M,T] (and, PLMS, of eps into the history slot).  The step vector
 * comes from a table of all timesteps made at create (every row of a sampler call shares t).  A ragged row's x beyond its end is left as
 * given; dead frames are neither read nor written.
 * bsg_fftden_ddpm_sample: steps t_start, t_start - 1, .. (n_steps of them).  Draws, as GaussianDiffusion.sample documents them:
 *   noise      device [n_steps, B, M, T], supplied draws (not with seeds_host);
 *   seeds_host host, B keys: row b draws from the stream (seeds_host[b], i + 1) at its own bound length — bit for bit the values of
 *              bsg_philox_normal_rows / bsg_ddpm_sample_rows (M * n_b must be a multiple of 4); seed / row0 / B_total are not read;
 *   neither    Philox (seed, i + 1) indexed by global row (row0 of B_total) and padded stride T, as bsg_ddpm_step's offset.
 * bsg_fftden_plms_sample: p_sample_plms (:168-201) over i = last, last - interval, .., 0 with last = floor((K_step - 1) / interval) *
 * interval; the 4-deep history lives in handle workspace (grown by the call: not under capture until the shape has run once), the first
 * iteration is the predictor / corrector pair (two evaluations), t - interval clamps at 0. */
int bsg_fftden_ddpm_sample(bsg_fftden* h, const bsg_schedule* s, float* x, const float* noise, uint64_t seed, const uint64_t* seeds_host,
                           int32_t t_start, int32_t n_steps, int32_t B, int32_t T, int32_t row0, int32_t B_total, void* stream);
int bsg_fftden_plms_sample(bsg_fftden* h, const bsg_schedule* s, float* x, int32_t K_step, int32_t interval, int32_t B, int32_t T,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * HiFi-GAN generator forward (mel -> waveform).
 * Stands behind HifiGanGenerator(h)(x [B,80,T]) -> [B,1,T*prod(upsample_rates)]  (modules/hifigan/hifigan.py:104-173)
 * as used by HifiGAN.spec2wav (vocoders/hifigan.py:55-69).  The NSF variant (use_pitch_embed) is bsg_hifigan_forward_nsf below.
 * ---------------------------------------------------------------------------------------------- */
typedef struct bsg_hifigan bsg_hifigan;

typedef struct {
  int32_t n_mel;                      /* 80 (conv_pre in-channels, hifigan.py:119)                       */
  int32_t upsample_initial_channel;   /* h['upsample_initial_channel']                                   */
  int32_t n_ups;                      /* len(h['upsample_rates'])                                        */
  int32_t upsample_rates[8];
  int32_t upsample_kernel_sizes[8];
  int32_t n_kernels;                  /* len(h['resblock_kernel_sizes']); kernels must be 3, 5, 7 or 11  */
  int32_t resblock_kernel_sizes[8];
  int32_t n_dil;                      /* dilations per ResBlock1 (3)                                     */
  int32_t resblock_dilations[8][4];
  int32_t weight_norm;                /* 1: weights come as (bias, weight_g, weight_v) triples           */
  int32_t use_nsf;                    /* h['use_pitch_embed']: NSF harmonic source (hifigan.py:111-132)   */
  int32_t sample_rate;                /* h['audio_sample_rate'] (NSF only)                               */
  int32_t harmonic_num;               /* 8 (hifigan.py:112)                                              */
  int32_t resblock;                   /* ABI v5: h['resblock']: 1 = ResBlock1 (hifigan.py:30-52), 2 = ResBlock2 (:70-91: per dilation
                                         ONE conv, x = conv_d(lrelu(x)) + x; 0 reads as 1)                   */
} bsg_hifigan_cfg;

int bsg_hifigan_n_weights(const bsg_hifigan_cfg* cfg);
/* dev_weights in HifiGanGenerator.state_dict() order: conv_pre, ups.i, resblocks.r.convs1.m (all m), then
 * resblocks.r.convs2.m (ResBlock2: resblocks.r.convs.m only), ..., conv_post; each conv contributes (bias, weight) — the layout after
 * remove_weight_norm() — or (bias, weight_g, weight_v) when cfg->weight_norm (checkpoint layout; folded here
 * as w = g * v / ||v||, norm over dims != 0).  Synchronises `stream` before returning. */
int bsg_hifigan_create(bsg_hifigan** out, const bsg_hifigan_cfg* cfg, const void* const* dev_weights,
                       int32_t n_weights, void* stream);
void bsg_hifigan_destroy(bsg_hifigan* h);
/* mel [B,n_mel,T] -> wav [B,1,T*prod(upsample_rates)].  May grow the workspace when B*T grows. */
int bsg_hifigan_forward(bsg_hifigan* h, const float* mel, float* wav, int32_t B, int32_t T, void* stream);
/* NSF-HiFiGAN: with cfg->use_nsf the weight list starts with m_source.l_linear.{weight,bias}
 * and noise_convs.i.{weight,bias} (state_dict order).  f0 [B,T] (Hz, 0 = unvoiced); the reference's two random draws
 * are supplied: rand_ini [B,harmonic_num+1] uniform[0,1) (torch.rand, source.py:53; column 0 is ignored) and
 * noise [B, T*hop, harmonic_num+1] N(0,1) (torch.randn_like, source.py:130). */
int bsg_hifigan_forward_nsf(bsg_hifigan* h, const float* mel, const float* f0, const float* rand_ini, const float* noise,
                            float* wav, int32_t B, int32_t T, void* stream);
/* ABI v10: the launches of the handle's last bsg_hifigan_forward[_nsf], one token "<site>:<form>[/<tile variant>]" per launch in launch
 * order, separated by blanks; "none" before the first forward.  Each token is written at the branch that launched, so it names what ran,
 * not what the thresholds would choose.  Sites: src (NSF source), pre, up<i>, src<i> (NSF source add of stage i), rb<i>.<j> (a whole
 * ResBlock in one launch) or rb<i>.<j>.<m> (its m-th convolution pair / convolution), post.  Forms: h2w (pre-split GEMM), conv, conv1,
 * conv2 (conv1d_kernel, /TT1 /TT2 /TT4 = samples per lane), up2 (upsample2_kernel), upk (upsample_kernel), poly (polyphase conv1d_kernel,
 * /TT*), convT (conv_transpose1d_kernel), chain (resblock_chain_h16_kernel, /NC4 /NC8), pair_h16, pair_h2, pair_mfma (/NB1 /NB2),
 * pair_valu (resblock_pair_kernel, /TT*), post4 (conv_post_kernel), nsf, add.  The string belongs to the handle: it is valid until the
 * handle's next forward or its destruction.  A forward that fails leaves the launches made up to the failure.
 * ABI v18: after a ragged forward the string is the token "ragged" followed by the tokens of the padded call at the same (B, T). */
const char* bsg_hifigan_last_path(bsg_hifigan* h);

/* ABI v18: ragged batches — every row at its own length inside the padded tensors.  mel [B,n_mel,T] (NSF: f0 [B,T], rand_ini, noise
 * [B,T*hop,NH] as above), lengths_host: B frame counts on the HOST, 1 <= lengths_host[b] <= T (read before the call returns; a captured
 * forward replays them).  With n_b = lengths_host[b]:
 *   wav[b, 0, :n_b*hop] is the generator applied to mel[b, :, :n_b] alone (NSF: with f0[b, :n_b], rand_ini[b] and noise[b, :n_b*hop]) — what
 *                       vocoders/hifigan.py:55-69 computes for that utterance; it depends on row b alone;
 *   wav[b, 0, n_b*hop:] is written as 0;
 *   nothing at or beyond a row's end is read: not the inputs, not the stage tensors of an earlier call, not the planes of the GEMM forms.
 * The plan, the grids and the launches are those of the padded call at (B, T) (all lengths = T gives its result bit for bit); each launch
 * bounds row b by n_b x (the upsample rates so far), and a workgroup whose first output lies beyond its row's end leaves at once.
 * A length outside 1..T: BSG_EINVAL with a message naming the row, before anything is enqueued. */
int bsg_hifigan_forward_ragged(bsg_hifigan* h, const float* mel, const int32_t* lengths_host, float* wav, int32_t B, int32_t T, void* stream);
int bsg_hifigan_forward_nsf_ragged(bsg_hifigan* h, const float* mel, const float* f0, const float* rand_ini, const float* noise,
                                   const int32_t* lengths_host, float* wav, int32_t B, int32_t T, void* stream);
/* test hook, as bsg_pwg_ / bsg_fftden_ have: NaN bytes into every stage buffer, the NSF source buffers and the planes of the GEMM forms */
int bsg_hifigan_debug_poison_workspace(bsg_hifigan* h, void* stream);

/* ABI v9, building block exported for unit tests: the NSF harmonic source alone (source.py:352-399 as bsg_hifigan_forward_nsf runs it).
 * f0 [B,T], rand_ini [B,NH], noise [B,T*hop,NH] as there; lin_w [NH], lin_b [1] = m_source.l_linear.{weight,bias}.
 * har [B,T*hop] = tanh(l_linear(sine_waves)).  sines (may be NULL): [B][NH][T*hop], the per-harmonic sine_waves (sines * uv + noise,
 * :130-134) before the merge.  With sines NULL a workspace is allocated and `stream` is synchronised before returning. */
int bsg_nsf_source(const float* f0, const float* rand_ini, const float* noise, const float* lin_w, const float* lin_b, float* har,
                   float* sines, int32_t B, int32_t T, int32_t hop, int32_t NH, int32_t sample_rate, void* stream);

/* PitchExtractor: mel [B,T,n_mel] -> pitch_pred [B,T,2] (may be NULL) and f0_denorm_pred [B,T]
 * (modules/fastspeech/pe.py:120-149; pitch_norm 'log', pitch_type 'frame').  dev_weights in PitchExtractor.state_dict()
 * order; pos_table [n_pos,256] = SinusoidalPositionalEmbedding table (row 0 zero), built by the host. */
typedef struct bsg_pitchext bsg_pitchext;
typedef struct {
  int32_t hidden_size;        /* 256 */
  int32_t n_mel;              /* 80  */
  int32_t conv_layers;        /* 2   (pe.py:121)                  */
  int32_t predictor_layers;   /* 5   (pe.py:134)                  */
  int32_t predictor_kernel;   /* hparams['predictor_kernel'] = 5  */
  int32_t use_uv;             /* hparams['pitch_type']=='frame' and hparams['use_uv'] */
  int32_t n_pos;
} bsg_pitchext_cfg;
int bsg_pitchext_n_weights(const bsg_pitchext_cfg* cfg);
int bsg_pitchext_create(bsg_pitchext** out, const bsg_pitchext_cfg* cfg, const void* const* dev_weights, int32_t n_weights,
                        const float* pos_table, void* stream);
void bsg_pitchext_destroy(bsg_pitchext* h);
int bsg_pitchext_forward(bsg_pitchext* h, const float* mel, float* pitch_pred, float* f0, int32_t B, int32_t T, void* stream);

/* ABI v19: ragged batches through the pitch extractor — every row at its own length inside the padded tensors, worded after
 * bsg_hifigan_forward_ragged.  mel [B,T,n_mel], lengths_host: B frame counts on the HOST, 1 <= lengths_host[b] <= T (read before the call
 * returns; they travel in kernel arguments into a handle-owned device array, so a captured forward replays them).  With n_b = lengths_host[b]:
 *   pitch_pred[b, :n_b] and f0[b, :n_b] are the extractor applied to mel[b, :n_b] alone (B = 1, T = n_b) — what the reference, which vocodes
 *                       every utterance alone, computes: GroupNorm's statistics run over n_b x 16, the convolutions see zeros beyond n_b,
 *                       the predictor's positions stop counting at n_b.  They depend on row b alone.  Frames inside a row whose mel is
 *                       exactly 0 keep the reference's `keep` mask (pe.py:29, :142), as in the padded call;
 *   pitch_pred[b, n_b:] and f0[b, n_b:] are written as 0;
 *   nothing at or beyond a row's end is read: not the mel (which may hold NaN there), not the workspaces of an earlier call.  The 1x1
 *                       projections are bounded like the convolutions, so a NaN tail raises no range event of the split-fp16 GEMMs.
 * The launches are those of the padded call at (B, T), and so are the grids and GEMM forms of the convolutions and row kernels; the 1x1
 * projections are issued as B problems of T rows (B x ceil(T / tile) row tiles instead of ceil(B T / tile); the form by the same rule on that
 * count) so that one row bound serves every product.  An element's sum order depends on neither the tile height nor the tile's place, and
 * each ragged kernel walks a row as the B = 1, T = n_b launch does: all lengths = T gives the padded call's result bit for bit, and row b
 * equals the row-alone call bit for bit.  A workgroup (of the row kernels: a wave) whose first frame lies beyond its row's end returns
 * before its first load.
 * lengths_host NULL ("lengths_host is null") or a length outside 1..T ("lengths[b]=.. outside 1..T=..", naming the row): BSG_EINVAL before
 * anything is enqueued or written. */
int bsg_pitchext_forward_ragged(bsg_pitchext* h, const float* mel, const int32_t* lengths_host, float* pitch_pred, float* f0, int32_t B,
                                int32_t T, void* stream);
/* test hook, as bsg_hifigan_ has: NaN bytes into every shape-sized buffer of the handle (a / b / c / keep / pred / pos); the lengths array,
 * which every ragged call fills itself, is left alone */
int bsg_pitchext_debug_poison_workspace(bsg_pitchext* h, void* stream);

/* ABI v12: the spectral post-filter of the vocoder output, hparams['vocoder_denoise_c'] (vocoders/hifigan.py:66-69 -> vocoders/vocoder_utils.py:7-15:
 * librosa.stft(center, zero padding, periodic Hann of win_size points) -> |S| - v clipped at 0 with the phase kept -> librosa.istft), as one
 * launch for a batch (csrc/wavden.hip).  NOT the FFT-transformer denoiser of the diffusion model, which is bsg_fftden_*.
 *   bsg_wavden_create   accepted (fft_size, hop_size, win_size): fft_size 512 or 1024, hop_size = fft_size / 4, fft_size / 2 <= win_size <= fft_size
 *                       (every BiSinger chain is (512, 128, 512), configs/tts/base.yaml (1024, 256, 1024)).  Anything else: BSG_EINVAL and a message
 *                       naming the accepted set, before any device call.  Builds the two transform bases (float64 on the host) and uploads them
 *                       on `stream`, which it waits for.
 *   bsg_wavden_forward  wav, out: device [B][stride] fp32.  n: HOST array of B sample counts, read during the call (NULL: every row has `stride`
 *                       samples).  Row b is filtered as if it were alone at length n[b]: samples at and beyond n[b] are never read, its
 *                       result does not depend on the other rows (bit for bit), out is written up to `stride`: hop_size * (n[b] / hop_size)
 *                       filtered samples, then zeros.  v >= 0 is the magnitude subtracted from every bin.  `out` must not overlap `wav`
 *                       (BSG_EINVAL): not in place.  B < 1, stride < 1, v < 0 or not finite, n[b] outside 0 .. stride: BSG_EINVAL, checked before
 *                       the handle is looked at.  No allocation, no wait, no device-side communication between workgroups: capturable; the
 *                       lengths are baked into a captured launch.  All products run on the fp32 matrix pipe: there is no operand range, no
 *                       status word and nothing to repeat. */
typedef struct bsg_wavden bsg_wavden;
int bsg_wavden_create(bsg_wavden** out, int32_t n_fft, int32_t hop, int32_t win, void* stream);
void bsg_wavden_destroy(bsg_wavden* h);
int bsg_wavden_forward(bsg_wavden* h, const float* wav, float* out, const int32_t* n, int32_t B, int32_t stride, float v, void* stream);

/* ABI v13: the Parallel WaveGAN generator, `vocoder: pwg` (modules/parallel_wavegan/models/parallel_wavegan.py:18-201 with
 * layers/residual_block.py:39-129 and layers/upsample.py:125-183; vocoders/pwg.py:18-105), csrc/pwg.hip.  One residual layer is one launch:
 * the dilated convolution, the aux term, the gate, both 1 x 1 products and the skip sum, all products on the fp32 matrix pipe (exact f32:
 * no operand range, no status word, nothing to repeat, and no entry in the bsg_handle_* guard family).
 *   bsg_pwg_create   dev_weights: bsg_pwg_n_weights(cfg) device pointers in the order of the generator's state dict AFTER remove_weight_norm()
 *                    (a folded convolution lists its bias before its weight):
 *                      first_conv.{bias[64], weight[64,1,1]}, upsample_net.conv_in.weight[80,80,2w+1],
 *                      upsample_net.upsample.up_layers.{1,3,..}.weight[1,1,1,2s+1] (one per scale),
 *                      conv_layers.i.{conv.bias[128], conv.weight[128,64,3], conv1x1_aux.weight[128,80,1], conv1x1_out.bias[64],
 *                      conv1x1_out.weight[64,64,1], conv1x1_skip.bias[64], conv1x1_skip.weight[64,64,1]} for every layer,
 *                      last_conv_layers.1.{bias[64], weight[64,64,1]}, last_conv_layers.3.{bias[1], weight[1,64,1]},
 *                      and with use_pitch_embed pitch_embed.weight[n_pitch,80], c_proj.weight[80,160], c_proj.bias[80].
 *                    Accepted: in = out = 1 channel, kernel_size 3, non-causal, residual = skip = 64, gate = 128, aux = 80, bias,
 *                    ConvInUpsampleNetwork with the nearest stretch and freq_axis_kernel_size 1, layers % stacks == 0, the product of
 *                    upsample_scales == hop_size.  Anything else: BSG_EINVAL with a message naming the value, before any device call.
 *                    Copies and packs the weights (waits for `stream`).
 *   bsg_pwg_forward  c [B][80][T + 2 w] (the caller edge-padded the mel by w = aux_context_window frames), pitch [B][T + 2 w] int64 (coarse
 *                    pitch, required with use_pitch_embed, NULL without), z and y [B][1][T hop].  z == NULL: z is drawn from the Philox
 *                    family of bsg_philox_normal, stream id 0x505747, key `seed`, element b T hop + t (B T hop must be a multiple of 4).
 *                    Row b does not depend on the other rows, bit for bit.  Workspaces grow when (B, T) exceed what the handle has seen
 *                    (then, and only then, the call waits for `stream` and allocates: not inside a capture); otherwise it only enqueues.
 *                    A pitch index outside 0 .. n_pitch - 1 is clamped to that range (torch's embedding raises; the call cannot look at
 *                    device data without a wait).  Like every handle here, a bsg_pwg is single-stream: the growth waits for `stream`
 *                    only, so a forward of the same handle still in flight on another stream would lose its buffers.
 *   bsg_pwg_n_weights  the length of dev_weights that create expects for cfg (221, 224 with use_pitch_embed, for the 30-layer config).
 *   bsg_pwg_last_path  the launches of the handle's last forward in launch order, separated by blanks: [pitch] conv_in up<i>:x<scale> ..
 *                    [philox] first layer<i>:f32/d<dilation> .. tail; "none" for a null handle or before the first forward.
 *   bsg_pwg_debug_poison_workspace  test hook: fills the workspaces, at their current capacity, with 0xFF bytes (NaN) on `stream`. */
typedef struct bsg_pwg bsg_pwg;
typedef struct {
  int32_t in_channels, out_channels, kernel_size, layers, stacks;
  int32_t residual_channels, gate_channels, skip_channels, aux_channels, aux_context_window;
  int32_t bias, use_causal_conv;
  int32_t upsample_net;          /* 0: ConvInUpsampleNetwork; any other network: another code */
  int32_t interpolate_nearest;   /* 1: upsample_params['interpolate_mode'] == 'nearest' */
  int32_t freq_axis_kernel_size;
  int32_t n_scales;
  int32_t upsample_scales[8];
  int32_t use_pitch_embed;
  int32_t n_pitch;               /* rows of pitch_embed (300) */
  int32_t hop_size;              /* config['hop_size']: samples per mel frame */
} bsg_pwg_cfg;
int bsg_pwg_n_weights(const bsg_pwg_cfg* cfg);
int bsg_pwg_create(bsg_pwg** out, const bsg_pwg_cfg* cfg, const void* const* dev_weights, int32_t n_weights, void* stream);
void bsg_pwg_destroy(bsg_pwg* h);
int bsg_pwg_forward(bsg_pwg* h, const float* z, const float* c, const int64_t* pitch, float* y, int32_t B, int32_t T, uint64_t seed, void* stream);
const char* bsg_pwg_last_path(bsg_pwg* h);
int bsg_pwg_debug_poison_workspace(bsg_pwg* h, void* stream);

/* Additions to v20 (no version bump, as bsg_pwg_n_weights was added beyond v13): ragged batches through the PWG generator — every row as
 * the generator applied to that utterance alone, worded after bsg_hifigan_forward_ragged / bsg_pitchext_forward_ragged.
 *   bsg_pwg_forward_ragged  mel [B][80][T] is UNPADDED: the library edge-pads each row at its own end.  pitch [B][T] int64 (required with
 *                    use_pitch_embed, NULL without), z and y [B][1][T hop].  lengths_host: B frame counts on the HOST, each in 1 .. T, read
 *                    before the call returns: they travel in kernel arguments into a handle-owned device array, so a captured forward
 *                    replays them and the host array is dead on return.  With n_b = lengths_host[b], L_b = n_b hop:
 *                      y[b,0,:L_b] is, BIT FOR BIT, what bsg_pwg_forward returns at B = 1, T = n_b for c = edge-pad(mel[b,:,:n_b], w),
 *                      pitch = edge-pad(pitch[b,:n_b], w) and z[b,0,:L_b]; it depends on row b alone.  y[b,0,L_b:] is written as 0.
 *                      Nothing at or beyond a row's end is read: mel and z may hold NaN there, pitch any integer, and what an earlier
 *                      call left in the workspaces is not read.  All lengths = T: the padded call's result on the edge-padded input, bit
 *                      for bit.
 *                    z == NULL: the Philox draws keep the PADDED call's index — element b T hop + t, stream 0x505747, key `seed` — so a
 *                    row sees the draws it sees in the padded call at (B, T) (as the NSF noise and the sampler do); a batched row with
 *                    drawn noise is therefore NOT the lone call's waveform.
 *                    BSG_EINVAL before anything is enqueued or written: lengths_host NULL ("lengths_host is null"), a length outside
 *                    1 .. T ("lengths[b]=.. outside 1..T=..", naming the row) — the lengths are looked at first, before the handle — and
 *                    what bsg_pwg_forward refuses.  Workspaces grow as for the padded call at (B, T) (the lengths array with B); otherwise
 *                    the call only enqueues and is capturable.  The launches are the padded call's, each bounding row b by its own
 *                    length (the pitch front runs over T frames, not T + 2 w); the residual-layer launches walk the LIVE 256-sample
 *                    tiles only, sum_b ceil(L_b / 256) of them, through a prefix table of the rows' tile counts beside the lengths.
 *                    bsg_pwg_last_path: the token `ragged`, then the padded call's tokens.  bsg_pwg_debug_poison_workspace leaves the
 *                    lengths array alone.
 *   bsg_pwg_last_tiles  the 256-sample tiles one residual-layer launch of the handle's last forward walked: B ceil(T hop / 256) after a
 *                    padded forward, sum_b ceil(L_b / 256) after a ragged one; 0 before the first forward or for a null handle. */
int bsg_pwg_forward_ragged(bsg_pwg* h, const float* z, const float* mel, const int64_t* pitch, const int32_t* lengths_host, float* y, int32_t B,
                           int32_t T, uint64_t seed, void* stream);
int bsg_pwg_last_tiles(bsg_pwg* h);

/* w[d0,...] = g[d0] * v[d0,...] / ||v[d0,...]||   (remove_weight_norm, hifigan.py:175-182) */
int bsg_weight_norm_fold(const float* g, const float* v, float* w, int32_t dim0, int32_t inner, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Building block exported for unit tests: C[b] = op(A[b]) * B[b] (+bias)(+epilogue), fp32 MFMA.
 *   A: [M,K] row-major (lda);  B: trans_b ? [N,K] row-major : [K,N] row-major (ldb);  C: [M,N] (ldc).
 * ---------------------------------------------------------------------------------------------- */
int bsg_gemm_f32(const float* A, const float* Bm, float* C, const float* bias_m, const float* bias_n,
                 int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t ldc, int32_t trans_b,
                 int32_t batch, int64_t strideA, int64_t strideB, int64_t strideC, int32_t relu,
                 void* stream);

/* ABI v15, test entry that reaches ALL of the generic GEMM (csrc/gemm.hip launch_gemm): bsg_gemm_desc mirrors its arguments,
 *   C[z] = rowscale[zo][i] * ( post( act( alpha' * ( sum_tap A[z][i + tap_shift0 + tap][:] . B_tap[z] + bias_n[zo][j] + bias_m[i] ) ) ) + R[zo][i][j] )
 * with A rows outside [0, M) of the same batch item read as zero, alpha' = alpha on columns < alpha_ncols (0: all columns) and 1 elsewhere,
 * post(v) = v * post_scale_n[j] + post_shift_n[j].  z = 0 .. batch-1; with batch2 > 1, z = zo * batch2 + zi and an operand's offset is
 * zo * s + zi * s2 (bias_n, R and rowscale move with zo only); otherwise zo = z.  Strides and leading dimensions count elements.
 *   force_form  0: dispatch as every other caller; 1 gemm_split/64, 2 gemm_split/128, 3 gemm_fast/64, 4 gemm_fast/128, 5 gemm_f32.
 *               1-4 need the 16-byte alignment rule of those kernels (K, lda, ldb, sA, sA2, sB, sB2, sTapB multiples of 4, N too
 *               unless trans_b, A and B on 16-byte boundaries): BSG_EINVAL otherwise
 *   form        NULL, or receives the name of the form that was launched (a string literal)
 * BSG_EINVAL with a message, before any device call: a null A, B or C, a non-positive dimension, post_scale_n without post_shift_n (or
 * the reverse), R without ldr, a force_form outside 0..5, a forced aligned form on an unaligned problem. */
typedef struct {
  const float* A;
  const float* B;
  float* C;
  int32_t M, N, K;
  int32_t lda, ldb, ldc;
  int64_t sA, sB, sC;           /* batch strides of the outer batch index */
  int32_t batch2;               /* inner batch count (0 / 1: none) */
  int64_t sA2, sB2, sC2;
  int32_t trans_b;              /* 1: B is [N,K] row-major; 0: B is [K,N] row-major */
  int32_t taps, tap_shift0;     /* conv as GEMM over shifted A rows: A row = i + tap_shift0 + tap */
  int64_t sTapB;                /* B offset per tap */
  const float* bias_m;          /* per output row, or NULL */
  const float* bias_n;          /* per output column, or NULL */
  int64_t sBiasN;               /* batch stride of bias_n (0: shared) */
  float alpha;
  int32_t alpha_ncols;
  int32_t act;                  /* 0 none, 1 ReLU, 2 GELU (erf), 3 Mish */
  const float* post_scale_n;    /* both or neither */
  const float* post_shift_n;
  const float* R;               /* residual, or NULL */
  int32_t ldr;
  int64_t sR;
  const float* rowscale;        /* or NULL */
  int64_t sRS;
  int32_t batch;
} bsg_gemm_desc;
int bsg_gemm_ex(const bsg_gemm_desc* d, int32_t force_form, const char** form, void* stream);

/* The GEMMs outside the residual stack form fp32 products on the 16-bit matrix pipe from hi + lo fp16 splits of both operands
 * (csrc/gemm.hip gemm_split_kernel; fp32-grade, |operand| < 4062).  A staged operand outside that range is counted instead of being
 * clipped silently: bsg_gemm_range_events waits for `stream`, returns the count (and resets it), and bsg_gemm_set_split(0) moves every
 * later GEMM to the fp32 matrix pipe — what the Python drop-ins do before they repeat the call (bisinger_amd/diffnet.py guarded). */
int bsg_gemm_set_split(int32_t enable);
int bsg_diffnet_set_h2(bsg_diffnet* h, int32_t enable);   /* 0: this handle's residual stack on the fp32 matrix pipe only (as BSG_H2=0) */
/* ABI v7, the tier in between: 0 = not the 16-row stack launch (residual_stack_q_kernel: its conv image holds 16 x, so its range guard
 * trips at |x| >= 3750) but the 32-row one (residual_stack_h2_kernel: |x + d| < 60000, about 8 % slower), as BSG_H2_Q=0 does for the
 * process.  Recovery order of a range event (status word 1) in the 16-row launch: bsg_diffnet_set_h2q(h, 0), repeat; only if that launch
 * trips too bsg_diffnet_set_h2(h, 0) (the fp32 matrix pipe, about 2x slower). */
int bsg_diffnet_set_h2q(bsg_diffnet* h, int32_t enable);
int bsg_gemm_range_events(int32_t* events, int32_t reset, void* stream);
/* ABI v5, non-blocking: enqueues a copy of the counter into *host_word (pinned host memory) on `stream`; nothing is reset. */
int bsg_gemm_range_events_async(int32_t* host_word, void* stream);

/* ABI v7: the range guard is PER HANDLE.  Every bsg_diffnet / bsg_fs2midi / bsg_hifigan / bsg_pitchext / bsg_fftden owns the device word
 * its split-fp16 kernels count out-of-range operands into, and its own switch between the split-fp16 products and the fp32 matrix pipe:
 * an out-of-range input to one model demotes THAT handle only ("distinct handles are independent", top of this file); inside a handle's
 * compute entries the state is looked up thread-locally, so two host threads on two handles do not see each other.  The two process-wide
 * functions above remain as the guard of the handle-less entries (bsg_gemm_f32, bsg_gemm_presplit_f32) and as a test hook:
 * bsg_gemm_set_split(0) (like BSG_GEMM_SPLIT=0 in the environment) is AND-ed into every handle's switch.
 *   kind: which handle type `handle` points to.
 *   bsg_handle_range_events        waits for `stream`; *events = waves of this handle's kernels that staged an operand beyond the fp16 range
 *                                  (|16 v| >= 65000, i.e. |v| >= 4062) since the last reset; reset != 0 zeroes the word when it is non-zero
 *   bsg_handle_range_events_async  no wait: enqueues the copy of the word into *host_word (pinned host memory) on `stream`
 *   bsg_handle_set_gemm_split      0: this handle's GEMMs / fused attention / ResBlock convolutions on the fp32 matrix pipe; 1: split-fp16 again
 *   bsg_handle_get_gemm_split      the EFFECTIVE switch (handle AND process-wide) */
enum { BSG_HANDLE_DIFFNET = 0, BSG_HANDLE_FS2MIDI = 1, BSG_HANDLE_HIFIGAN = 2, BSG_HANDLE_PITCHEXT = 3, BSG_HANDLE_FFTDEN = 4 };
int bsg_handle_range_events(int32_t kind, void* handle, int32_t* events, int32_t reset, void* stream);
int bsg_handle_range_events_async(int32_t kind, void* handle, int32_t* host_word, void* stream);
int bsg_handle_set_gemm_split(int32_t kind, void* handle, int32_t enable);
int bsg_handle_get_gemm_split(int32_t kind, void* handle, int32_t* enabled);

/* Round 4: the same products with PRE-SPLIT operands (csrc/gemm_h2w.hip gemm_h2w_kernel) — weights split once into hi / lo fp16 MFMA
 * fragments at create, activations written as hi / lo fp16 planes by their producers; FS2's Linear / Conv1d-FFN layers
 * (TB/modules/commons/common_layers.py:625-644,706-730) and the hoisted conditioner projections (TB/usr/diff/net.py:68) run on it
 * (BSG_GEMM_H2W=0: gemm_split_kernel).  Exported for unit tests and micro-benchmarks: out = epi(conv_taps(act, w) + bias), SAME padding,
 *   act [batch][rows][K], w [taps][Wn][K], out act_is_a ? [batch][rows][Wn] : [batch][Wn][rows];  Wn % 128 == 0, K % 64 == 0, taps <= 17;
 *   the launch is repeated `reps` times (timing); waits for `stream`. */
int bsg_gemm_presplit_f32(const float* act, const float* w, float* out, const float* bias, int32_t rows, int32_t Wn, int32_t K,
                          int32_t taps, int32_t act_is_a, int32_t batch, int32_t relu, int32_t reps, void* stream);

/* ABI v21, test entry that reaches ALL of the pre-split GEMM (csrc/gemm_h2w.hip launch_gemm_h2w): bsg_h2w_desc mirrors every field a caller of
 * it sets, with fp32 operands.  Per batch index z (activation item za = z % zdiv, weight set zw = z / zdiv; zdiv = 0: one weight set):
 *   v(i, n) = sum_tap sum_k act[za][i + tap_shift0 + tap][k] * W[zw](tap, n, k)      rows outside [0, rows) (with lens: [0, lens[za])) are zero
 *   v = (v + bias[zw][n]) * alpha' ;  v = act_fn(v) ;  v += R[z](i, n) ;  v *= rowscale[za][i]       alpha' = alpha on weight rows n < alpha_ncols (0: all)
 * and v goes to C[z] ([rows][ldc] with act_is_a, [Wn][ldc] without), to the channel-quad copies Cq / Ch ([Wn / 4][rows][4], fp32 / bf16), to the
 * hi / lo fp16 planes `out` of 16 v, to the V^T planes `vt` of the QKV mode or to the polyphase positions C[co][8 q + r - up_p], as H2wArgs
 * (csrc/bsg_common.h) documents them.  On every call the entry packs the weights (W(tap, n, k) at w[zw * sW + tap * ts + n * rs + k * ks]) and
 * builds the activation planes: a buffer of fp16 NaNs (bytes 0x7e) into which only the logical rows x K windows are split (rows < lens[za]
 * with lengths), row stride lda and item stride sAct of their own — what the kernel fails to mask reads NaN.  Waits for `stream`, frees what it
 * allocated.  A packed weight beyond the fp16 range is BSG_EINVAL after the call; activations count into bsg_gemm_range_events.
 *   force_form  0: dispatch as every other caller; 1 h2w/32/deep, 2 h2w/32/ring16, 3 h2w/32/ring8, 4 h2w/32/ring4, 5 h2w/64/ring8,
 *               6 h2w/64/ring4, 7 h2w/128/ring4 (tile height / weight ring).  Refused with BSG_EINVAL before anything is launched: a 32-row
 *               form (1-4) with act_is_a = 0; 1 without taps == 1 && K % 256 == 0; a ring that does not divide the K / 16 * taps k-steps;
 *               with lens, any form but the six ragged ones (1 plain, 2 conv, 5, 7)
 *   form        NULL, or receives the name of the form that was launched (a string literal) */
typedef struct {
  const float* act;             /* fp32 activation: item za at act + za * sAct_src, row i at + i * lda_src (16-byte aligned rows) */
  int32_t lda_src;
  int64_t sAct_src;
  int32_t lda;                  /* row stride of the planes the entry builds (halfs; >= K, % 8) */
  int64_t sAct;                 /* their item stride (halfs; >= rows * lda, % 8) */
  const float* w;               /* fp32 weights */
  int64_t ts, rs, ks;           /* tap, row and k stride of one weight set */
  int64_t sW;                   /* stride between weight sets (elements) */
  int32_t rows, K, Wn, taps, tap_shift0, act_is_a, batch, zdiv;
  float* C;
  int32_t ldc;
  int64_t sC;
  float* Cq;
  uint16_t* Ch;
  uint16_t* out;
  int64_t out_plane;
  int32_t ldo;
  int64_t sO;
  const float* bias;
  int64_t sBias;
  float alpha;
  int32_t alpha_ncols;
  int32_t act_fn;               /* 0 none, 1 ReLU, 2 GELU (erf) */
  const float* R;
  int32_t ldr;
  int64_t sR;
  const float* rowscale;
  int64_t sRS;
  int32_t up_u, up_p, up_lout;
  int32_t qkv_T, qkv_Tp, qkv_H;
  uint16_t* vt;
  int64_t vt_plane;
  const int32_t* lens;          /* device, one row count per activation item, or NULL */
} bsg_h2w_desc;
int bsg_gemm_h2w_ex(const bsg_h2w_desc* d, int32_t force_form, const char** form, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BISINGER_HIP_H */
