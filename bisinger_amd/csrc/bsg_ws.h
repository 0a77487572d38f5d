// Device memory of a handle (host code only): the table of its shape-sized workspaces with the one way they grow, are freed and are
// poisoned, and the owner of the allocations that live as long as the handle.  DESIGN.md §4 "Workspaces".
#pragma once
#include <vector>

#include "bsg_common.h"

namespace bsg {

// One shape-sized buffer.  Buffers with the same capacity word form a group and are replaced together; a buffer holds `unit` bytes per
// capacity unit plus `extra`.  WS_ZERO: zeroed when (re)allocated (flag words, arrival counters).  WS_POISON: the handle's test hook
// fills it.  `lazy`: the group is (also) grown from a compute call — the refusal a GROW_LAZY site gets on a capturing stream.
enum : unsigned { WS_ZERO = 1, WS_POISON = 2 };
struct WsBuf {
  size_t* cap;
  void** p;
  size_t unit, extra = 0;
  unsigned flags = 0;
  const char* lazy = nullptr;
};

// How a call site grows a group.  GROW_BOUND: a failure is the call's.  GROW_LAZY: where a compute call may be the one that grows a group
// a prepare usually sized: under capture the refusal is the group's own `lazy` sentence.  GROW_SOFT: for a layout the caller can do
// without (a group of one buffer): out of device memory leaves the group empty (capacity 0), clears the HIP error and returns BSG_OK.
enum GrowHow { GROW_BOUND, GROW_LAZY, GROW_SOFT };

bool is_capturing(hipStream_t st);

// The group of `table` with capacity word `cap`, grown to `need` units; nothing happens while need <= *cap.  (Call sites whose table is
// built per call test that themselves first, so the common path builds no table.)  `kind` names the handle in the messages.
//   On a capturing stream: BSG_EINVAL before anything is touched — nothing is freed, the capture stays valid, the handle usable.
//   Otherwise, in this order: the stream is waited for before anything is freed (launches in flight may read the old buffers); the
//   capacity is 0 while the pointers are replaced, so a failed hipMalloc leaves the group empty, not dangling; the zeroing memsets go to
//   `st`, ahead of the launches that read the words; the capacity is set last.
int ws_grow(const std::vector<WsBuf>& table, const char* kind, size_t* cap, size_t need, hipStream_t st, GrowHow how = GROW_BOUND);
// destroy: every buffer of the table freed
void ws_free(const std::vector<WsBuf>& table);
// test hooks: 0xFF bytes (a NaN as fp16 and as fp32) over capacity x unit of every WS_POISON buffer
int ws_poison(const std::vector<WsBuf>& table, hipStream_t st);

// Ragged forwards (bsg_hifigan_forward_ragged, bsg_pitchext_forward_ragged): the rows' counts reach the kernels through a handle-owned
// device array — one more row of the handle's table, not poisoned — that the call itself fills.
//   lens_check: lengths_host non-null and every count in 1 .. T, else BSG_EINVAL naming the row; touches nothing on the device.
//   lens_fill:  launches of set_lens_kernel on `st` that carry the counts in their arguments and store them at dst[0 .. B).
int lens_check(const int32_t* lengths_host, int B, int T, const char* who);
int lens_fill(int* dst, const int32_t* lengths_host, int B, hipStream_t st);

// The allocations that live as long as a handle (packed weights, tables, once-only device words): allocated and remembered, freed
// together by destroy.
struct DevOwned {
  std::vector<void*> ptrs;
  int alloc(void** p, size_t bytes);
  void free_all();
};
template <class P>
static int own_alloc(DevOwned& o, P** p, size_t n) { return o.alloc((void**)p, n * sizeof(P)); }

}  // namespace bsg
