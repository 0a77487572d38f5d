// The spectral post-filter of the vocoder output, hparams['vocoder_denoise_c'] (vocoders/hifigan.py:66-69 -> vocoders/vocoder_utils.py:7-15:
// librosa.stft -> |S| - v clipped at 0, phase kept -> librosa.istft), as ONE launch for a batch of waveforms on gfx950.
//
// Semantics, for one waveform y of n samples (N = n_fft, hop = N / 4, T = n / hop):
//   ypad = y with N / 2 zeros on both sides; frame i = ypad[i hop .. i hop + N), i = 0 .. T; w = periodic Hann of `win` points, zero-padded
//   symmetrically to N;  S_i = rfft(frame_i w);  S'_i = S_i max(|S_i| - v, 0) / |S_i|  (0 where |S_i| = 0);  frame'_i = irfft(S'_i) w;
//   out[o] = sum_i frame'_i[o + N / 2 - i hop] / sum_i w^2[o + N / 2 - i hop]  (the quotient only where the envelope exceeds FLT_MIN), o < hop T.
//
// A workgroup owns RUN = 29 consecutive output hops of one row and computes all 32 frames that overlap them (3 halo frames are recomputed,
// not exchanged): nothing is communicated between workgroups, the summation order is fixed, and a row's result depends on that row alone.
// Both transforms are products against N x N real bases built on the host in float64 (the window is folded into them), on the fp32 matrix
// pipe (v_mfma_f32_32x32x2_f32: exact f32, no operand range to guard).  The real spectrum is packed the usual way: bin-row r < N / 2 is
// Re S_r, bin-row N / 2 + k is Im S_k for k > 0 and the (real) Nyquist bin for k = 0, so that Re and Im of one bin meet in one lane and one
// register index of two accumulators.  The bin-rows are the ROWS of the forward product (frames on the lanes), so the clipped spectrum
// goes to LDS as [bin-row][32 frames] and is the B operand of the inverse product as it stands.  LDS (32 N floats) holds, one after the
// other: the wave segment (hop blocks skewed by one float: the 32 frames of a B-operand read lie `hop` samples apart), the clipped
// spectrum, and the windowed output frames [frame][n ^ frame] for the overlap-add.  The wave is read once and written once.
#include <float.h>
#include <math.h>

#include <vector>

#include "bsg_common.h"

struct bsg_wavden {
  int n_fft = 0, hop = 0, win = 0;
  float* fwd = nullptr;   // [n][bin-row]: analysis basis x window
  float* inv = nullptr;   // [bin-row][n]: synthesis basis x window / N
  float* wsq = nullptr;   // [n]: window squared
};

namespace bsg {
namespace {

constexpr int FR = 32;         // frames per workgroup: one 32-column MFMA tile
constexpr int RUN = FR - 3;    // output hops per workgroup (n_fft / hop - 1 = 3 halo frames)
constexpr int MAXB = 64;       // rows per launch: their sample counts travel in the kernel arguments

struct WavdenArgs {
  const float* wav;
  float* out;
  const float* fwd;
  const float* inv;
  const float* wsq;
  int stride;
  float v;
  int n[MAXB];
};

// acc[a] += basis[k][rowbase[a] + 0..31] (x) B[k][0..31] over k = 0 .. N - 1; lane l holds B[k = 2 s + (l >> 5)][l & 31] = lds[bidx(k)].
// The basis rows are loaded U k-steps ahead of the products that use them.
template <int N, int NA, typename BIdx>
__device__ __forceinline__ void basis_product(f32x16 (&acc)[NA], const float* __restrict__ basis, const int (&rowbase)[NA], const float* lds,
                                              BIdx bidx, int l31, int lh) {
  constexpr int U = 4;
  float an[U][NA], bn[U];
  auto load = [&](int s0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = 2 * (s0 + u) + lh;
#pragma unroll
      for (int a = 0; a < NA; ++a) an[u][a] = basis[(long long)k * N + rowbase[a] + l31];
      bn[u] = lds[bidx(k)];
    }
  };
  load(0);
  for (int s0 = 0; s0 < N / 2; s0 += U) {
    float ac[U][NA], bc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      bc[u] = bn[u];
#pragma unroll
      for (int a = 0; a < NA; ++a) ac[u][a] = an[u][a];
    }
    if (s0 + U < N / 2) load(s0 + U);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int a = 0; a < NA; ++a) acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[u][a], bc[u], acc[a], 0, 0, 0);
  }
}

__device__ __forceinline__ float shrink_real(float x, float v) {
  const float m = fabsf(x);
  return m > 0.f ? x * (fmaxf(m - v, 0.f) / m) : 0.f;
}

template <int N>
__global__ __launch_bounds__(256) void wavden_kernel(const WavdenArgs a) {
  constexpr int HOP = N / 4, NA = N / 128, NH = NA / 2;   // NA accumulators per wave: NH Re tiles and NH Im tiles, then NA output tiles
  extern __shared__ __attribute__((aligned(16))) float lds[];   // FR * N floats
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int row = blockIdx.y;
  const int n = a.n[row];
  const int T = n / HOP;                    // frames 0 .. T; output hops 0 .. T - 1
  const int j0 = blockIdx.x * RUN;          // first output hop of this workgroup
  const float* __restrict__ wav = a.wav + (long long)row * a.stride;
  float* __restrict__ out = a.out + (long long)row * a.stride;
  const int o0 = j0 * HOP;
  if (j0 >= T) {                            // beyond the row's length: zeros (uniform over the workgroup)
    for (int idx = tid; idx < RUN * HOP; idx += 256)
      if (o0 + idx < a.stride) out[o0 + idx] = 0.f;
    return;
  }

  // the wave segment under frames j0 - 1 .. j0 + 30: ypad[(j0 - 1) hop + p], p < 35 hop; samples outside [0, n) are zero and never read
  for (int p = tid; p < (FR + 3) * HOP; p += 256) {
    const int g = (j0 - 3) * HOP + p;
    lds[p + p / HOP] = (g >= 0 && g < n) ? wav[g] : 0.f;
  }
  __syncthreads();

  f32x16 acc[NA];
  int rowbase[NA];
#pragma unroll
  for (int t = 0; t < NA; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    rowbase[t] = t < NH ? 32 * (wave * NH + t) : N / 2 + 32 * (wave * NH + t - NH);
  }
  basis_product<N, NA>(acc, a.fwd, rowbase, lds, [&](int k) { return l31 * (HOP + 1) + k + k / HOP; }, l31, lh);

  // S' = S max(|S| - v, 0) / |S|; a frame outside 0 .. T is no frame of this row
  const int fi = j0 - 1 + l31;
  const bool frame_ok = fi >= 0 && fi <= T;
  const float v = a.v;
#pragma unroll
  for (int t = 0; t < NH; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float re = acc[t][r], im = acc[t + NH][r];
      if (rowbase[t] + acc_row(r, lh) == 0) {       // DC and Nyquist: two real bins
        re = shrink_real(re, v);
        im = shrink_real(im, v);
      } else {
        const float m = sqrtf(re * re + im * im);
        const float g = m > 0.f ? fmaxf(m - v, 0.f) / m : 0.f;
        re *= g;
        im *= g;
      }
      acc[t][r] = frame_ok ? re : 0.f;
      acc[t + NH][r] = frame_ok ? im : 0.f;
    }
  __syncthreads();      // every wave has read the segment
#pragma unroll
  for (int t = 0; t < NA; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) lds[(rowbase[t] + acc_row(r, lh)) * FR + l31] = acc[t][r];
  __syncthreads();

#pragma unroll
  for (int t = 0; t < NA; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    rowbase[t] = 32 * (wave * NA + t);
  }
  basis_product<N, NA>(acc, a.inv, rowbase, lds, [&](int k) { return k * FR + l31; }, l31, lh);
  __syncthreads();      // every wave has read the spectrum
#pragma unroll
  for (int t = 0; t < NA; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) lds[l31 * N + ((rowbase[t] + acc_row(r, lh)) ^ l31)] = acc[t][r];
  __syncthreads();

  // overlap-add in a fixed order (earliest frame first), envelope from the row's own frame count, one coalesced store
  const float* __restrict__ wsq = a.wsq;
  for (int idx = tid; idx < RUN * HOP; idx += 256) {
    const int jj = idx / HOP, m = idx % HOP, j = j0 + jj, o = o0 + idx;
    if (o >= a.stride) break;
    float y = 0.f;
    if (j < T) {
      float env = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = j - 1 + c, f = jj + c, off = (3 - c) * HOP + m;
        if (i >= 0 && i <= T) {
          y += lds[f * N + (off ^ f)];
          env += wsq[off];
        }
      }
      if (env > FLT_MIN) y /= env;
    }
    out[o] = y;
  }
}

template <int N>
int wavden_launch(const WavdenArgs& a, int rows, hipStream_t st) {
  const dim3 grid(cdiv(a.stride, RUN * (N / 4)), rows);
  hipLaunchKernelGGL(wavden_kernel<N>, grid, dim3(256), (size_t)FR * N * sizeof(float), st, a);
  BSG_LAUNCH_CHECK();
  return BSG_OK;
}

}  // namespace
}  // namespace bsg

using namespace bsg;

#define BSG_WAVDEN_ACCEPTED "n_fft 512 or 1024, hop_size = n_fft / 4, n_fft / 2 <= win_size <= n_fft"

extern "C" void bsg_wavden_destroy(bsg_wavden* h) {
  if (!h) return;
  float* bufs[] = {h->fwd, h->inv, h->wsq};
  for (float* p : bufs)
    if (p) (void)hipFree(p);
  delete h;
}

extern "C" int bsg_wavden_create(bsg_wavden** out, int32_t n_fft, int32_t hop, int32_t win, void* stream) {
  BSG_REQUIRE(out, "wavden_create: null argument");
  *out = nullptr;
  BSG_REQUIRE((n_fft == 512 || n_fft == 1024) && hop * 4 == n_fft && win >= n_fft / 2 && win <= n_fft,
              "wavden_create: (fft_size, hop_size, win_size) = (%d, %d, %d) is not built; accepted: " BSG_WAVDEN_ACCEPTED, n_fft, hop, win);
  const int N = n_fft;
  const double PI = 3.14159265358979323846;
  std::vector<double> w(N, 0.0);
  const int lp = (N - win) / 2;
  for (int i = 0; i < win; ++i) w[lp + i] = 0.5 - 0.5 * cos(2.0 * PI * i / win);      // periodic Hann
  std::vector<double> cs(N), sn(N);
  for (int i = 0; i < N; ++i) { cs[i] = cos(2.0 * PI * i / N); sn[i] = sin(2.0 * PI * i / N); }
  std::vector<float> fwd((size_t)N * N), inv((size_t)N * N), wsq(N);
  for (int nn = 0; nn < N; ++nn) {
    wsq[nn] = (float)(w[nn] * w[nn]);
    for (int r = 0; r < N; ++r) {
      const int k = r < N / 2 ? r : r - N / 2;
      const int ph = (int)(((long long)k * nn) % N);
      double f, g;      // S = sum_n x e^{-i 2 pi k n / N};  x = (1 / N) (S_0 + (-1)^n S_{N/2} + 2 sum_{0<k<N/2} (Re S_k cos - Im S_k sin))
      if (r < N / 2) { f = cs[ph]; g = (k == 0 ? 1.0 : 2.0) * cs[ph]; }
      else if (k == 0) { f = (nn & 1) ? -1.0 : 1.0; g = f; }
      else { f = -sn[ph]; g = -2.0 * sn[ph]; }
      fwd[(size_t)nn * N + r] = (float)(f * w[nn]);
      inv[(size_t)r * N + nn] = (float)(g * w[nn] / N);
    }
  }
  bsg_wavden* h = new bsg_wavden();
  h->n_fft = n_fft; h->hop = hop; h->win = win;
  hipStream_t st = (hipStream_t)stream;
  auto fail = [&](hipError_t e, const char* what) {
    set_error("wavden_create: %s -> %s", what, hipGetErrorString(e));
    bsg_wavden_destroy(h);
    return e == hipErrorOutOfMemory ? BSG_ENOMEM : BSG_EHIP;
  };
  const size_t nb = (size_t)N * N * sizeof(float);
  hipError_t e;
  if ((e = hipMalloc((void**)&h->fwd, nb)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&h->inv, nb)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&h->wsq, N * sizeof(float))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMemcpyAsync(h->fwd, fwd.data(), nb, hipMemcpyHostToDevice, st)) != hipSuccess) return fail(e, "hipMemcpyAsync");
  if ((e = hipMemcpyAsync(h->inv, inv.data(), nb, hipMemcpyHostToDevice, st)) != hipSuccess) return fail(e, "hipMemcpyAsync");
  if ((e = hipMemcpyAsync(h->wsq, wsq.data(), N * sizeof(float), hipMemcpyHostToDevice, st)) != hipSuccess) return fail(e, "hipMemcpyAsync");
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(e, "hipStreamSynchronize");
  const int lds = FR * N * (int)sizeof(float);
  e = N == 512 ? hipFuncSetAttribute((const void*)wavden_kernel<512>, hipFuncAttributeMaxDynamicSharedMemorySize, lds)
               : hipFuncSetAttribute((const void*)wavden_kernel<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return fail(e, "hipFuncSetAttribute");
  *out = h;
  return BSG_OK;
}

extern "C" int bsg_wavden_forward(bsg_wavden* h, const float* wav, float* out, const int32_t* n_host, int32_t B, int32_t stride, float v,
                                  void* stream) {
  // the arguments first, the handle after them: these refusals need no device
  BSG_REQUIRE(B >= 1 && stride >= 1, "wavden_forward: B=%d rows of stride=%d samples: both must be >= 1", B, stride);
  BSG_REQUIRE(v >= 0.f && v <= FLT_MAX, "wavden_forward: v=%g must be a finite number >= 0", (double)v);
  if (n_host)
    for (int b = 0; b < B; ++b)
      BSG_REQUIRE(n_host[b] >= 0 && n_host[b] <= stride, "wavden_forward: n[%d]=%d outside 0 .. stride=%d", b, n_host[b], stride);
  BSG_REQUIRE(h && wav && out, "wavden_forward: null argument");
  const long long total = (long long)B * stride;
  BSG_REQUIRE(out + total <= wav || wav + total <= out, "wavden_forward: out overlaps wav (a workgroup reads samples its neighbours write)");
  hipStream_t st = (hipStream_t)stream;
  WavdenArgs a{};
  a.fwd = h->fwd; a.inv = h->inv; a.wsq = h->wsq; a.stride = stride; a.v = v;
  for (int b0 = 0; b0 < B; b0 += MAXB) {      // one launch for up to 64 rows
    const int rows = B - b0 < MAXB ? B - b0 : MAXB;
    a.wav = wav + (long long)b0 * stride;
    a.out = out + (long long)b0 * stride;
    for (int b = 0; b < rows; ++b) a.n[b] = n_host ? n_host[b0 + b] : stride;
    const int rc = h->n_fft == 512 ? wavden_launch<512>(a, rows, st) : wavden_launch<1024>(a, rows, st);
    if (rc != BSG_OK) return rc;
  }
  return BSG_OK;
}
