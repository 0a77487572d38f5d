// Workspace tables and owned allocations of the handles (bsg_ws.h): host code, and the one kernel that fills a handle's lengths row.
#include "bsg_ws.h"

namespace bsg {

bool is_capturing(hipStream_t st) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (st) (void)hipStreamIsCapturing(st, &cap);
  return cap != hipStreamCaptureStatusNone;
}

int ws_grow(const std::vector<WsBuf>& table, const char* kind, size_t* cap, size_t need, hipStream_t st, GrowHow how) {
  if (need <= *cap) return BSG_OK;
  const WsBuf* first = nullptr;
  for (const WsBuf& w : table)
    if (w.cap == cap) { first = &w; break; }
  BSG_REQUIRE(first, "%s: grow() of a capacity word that ws_table does not list", kind);
  if (is_capturing(st)) {
    if (how == GROW_LAZY && first->lazy) set_error("%s", first->lazy);
    else set_error("%s: a workspace has to grow for this shape, which a capturing stream cannot do; run the shape once eagerly before capturing", kind);
    return BSG_EINVAL;
  }
  BSG_HIP(hipStreamSynchronize(st));
  *cap = 0;
  for (const WsBuf& w : table)
    if (w.cap == cap) { if (*w.p) (void)hipFree(*w.p); *w.p = nullptr; }
  for (const WsBuf& w : table) {
    if (w.cap != cap) continue;
    const size_t bytes = need * w.unit + w.extra;
    const hipError_t e = hipMalloc(w.p, bytes);
    if (e != hipSuccess && how == GROW_SOFT) {
      (void)hipGetLastError();
      *w.p = nullptr;
      return BSG_OK;
    }
    BSG_HIP(e);
    if (w.flags & WS_ZERO) BSG_HIP(hipMemsetAsync(*w.p, 0, bytes, st));
  }
  *cap = need;
  return BSG_OK;
}

void ws_free(const std::vector<WsBuf>& table) {
  for (const WsBuf& w : table)
    if (*w.p) { (void)hipFree(*w.p); *w.p = nullptr; }
}

int ws_poison(const std::vector<WsBuf>& table, hipStream_t st) {
  for (const WsBuf& w : table)
    if ((w.flags & WS_POISON) && *w.p && *w.cap) BSG_HIP(hipMemsetAsync(*w.p, 0xFF, *w.cap * w.unit, st));
  return BSG_OK;
}

// Up to 256 counts travel in the ARGUMENTS of each launch, so a captured forward replays the same counts and no host memory is read after
// the call returns.
namespace {
struct LensChunk { int n[256]; };
__global__ void set_lens_kernel(LensChunk c, int* __restrict__ dst, int rows) {
  if ((int)threadIdx.x < rows) dst[threadIdx.x] = c.n[threadIdx.x];
}
}  // namespace

int lens_check(const int32_t* lengths_host, int B, int T, const char* who) {
  BSG_REQUIRE(lengths_host, "%s: lengths_host is null", who);
  BSG_REQUIRE(B > 0 && B <= 65535 && T > 0, "%s: bad argument (B=%d T=%d)", who, B, T);
  for (int b = 0; b < B; ++b)
    BSG_REQUIRE(lengths_host[b] >= 1 && lengths_host[b] <= T, "%s: lengths[%d]=%d outside 1..T=%d", who, b, lengths_host[b], T);
  return BSG_OK;
}

int lens_fill(int* dst, const int32_t* lengths_host, int B, hipStream_t st) {
  for (int b0 = 0; b0 < B; b0 += 256) {
    LensChunk c{};
    const int rows = B - b0 < 256 ? B - b0 : 256;
    for (int r = 0; r < rows; ++r) c.n[r] = lengths_host[b0 + r];
    hipLaunchKernelGGL(set_lens_kernel, dim3(1), dim3(256), 0, st, c, dst + b0, rows);
    BSG_LAUNCH_CHECK();
  }
  return BSG_OK;
}

int DevOwned::alloc(void** p, size_t bytes) {
  BSG_HIP(hipMalloc(p, bytes));
  ptrs.push_back(*p);
  return BSG_OK;
}

void DevOwned::free_all() {
  for (void* p : ptrs) (void)hipFree(p);
  ptrs.clear();
}

}  // namespace bsg
