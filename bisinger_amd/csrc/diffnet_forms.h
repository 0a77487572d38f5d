// The launch forms of the denoiser in one place: which __global__ function a form is, its block size, the dynamic LDS it is launched with and
// the LDS the device has to grant it, what bsg_diffnet_last_path calls it, and — per handle — whether the grant was made and how many of its
// workgroups a CU holds.  Every kernel file names its forms through a getter (below); diffnet.hip plans with them and launches them.  Host
// side only.
#pragma once
#include "diffnet_res.h"

namespace bsg {

// what runs the L residual layers of an evaluation
enum StackForm {
  STACK_NONE,   // no stack launch: one launch per layer (launch_layer); also the family of every form that is no stack launch
  STACK_F43,    // Winograd F(4,3) on the fp32 matrix pipe (diffnet_f43.hip)
  STACK_H2,     // split-fp16, 32-row matrix tiles (residual_stack_h2_kernel, diffnet_h2.hip)
  STACK_H2Q,    // split-fp16, 16-row matrix tiles (residual_stack_q_kernel, diffnet_h2q.hip)
  STACK_PART,   // split-fp16 part form: several workgroups per tile (residual_part_h2_kernel, diffnet_h2.hip)
  STACK_BF16,   // bf16-operand configuration (diffnet_bf16.hip)
};

enum FormVariant { FORM_PLAIN, FORM_RAGGED, FORM_TOKEN };   // how a 16-row stack launch finds its rows and its conditioner term

enum LayerForm {   // the per-layer launches (bsg_diffnet_last_path)
  LAYER_PLAIN,    // "layer": residual_layer_kernel, one workgroup per 32-frame tile
  LAYER_SPLIT2,   // "split2": residual_split_kernel<false, 2>, a pair of workgroups per tile, each half of the channels
  LAYER_SPLIT4,   // "split4": residual_split_kernel<false, 4>
  LAYER_WIDE,     // "wide": residual_split_kernel<true, 1>, one 16-wave workgroup per tile
  LAYER_BF16,     // "bf16": bf16-operand configuration (residual_layer_bf16_kernel)
};

// One id per form: the index of its entry in a handle's FormMemo.
enum FormId {
  // diffnet_h2q.hip: residual_stack_q_kernel on 32- / 64-frame tiles; _UNFAIR: BSG_H2Q_FAIR=0; _DIAG1 .. 6: BSG_H2Q_DIAG (consecutive)
  FORM_Q32, FORM_Q64, FORM_Q32_UNFAIR, FORM_Q64_UNFAIR, FORM_Q64_RAGGED, FORM_Q64_TOKEN,
  FORM_Q64_DIAG1, FORM_Q64_DIAG2, FORM_Q64_DIAG3, FORM_Q64_DIAG4, FORM_Q64_DIAG5, FORM_Q64_DIAG6,
  // diffnet_h2.hip
  FORM_H2_32, FORM_H2_64, FORM_PART_QUAD32, FORM_PART_QUAD64, FORM_PART_PAIR64, FORM_TAIL_H2, FORM_IN_PROJ_H2,
  // diffnet_f43.hip
  FORM_F43,
  // diffnet_bf16.hip
  FORM_BF16_STACK, FORM_BF16_STACK_RAGGED, FORM_BF16_LAYER, FORM_BF16_LAYER_STAMPS,
  FORM_BF16_TAIL, FORM_BF16_TAIL_PLMS, FORM_BF16_TAIL_RAGGED, FORM_BF16_TAIL_RAGGED_PLMS,
  // diffnet.hip
  FORM_LAYER_DIRECT, FORM_LAYER_DIRECT_STAMPS, FORM_LAYER_WINO, FORM_LAYER_WINO_STAMPS,
  FORM_SPLIT2, FORM_SPLIT2_SMALL, FORM_SPLIT4, FORM_SPLIT4_SMALL, FORM_WIDE,
  FORM_TAIL_F32_80, FORM_TAIL_F32_96, FORM_TAIL_F32_80_PLMS, FORM_TAIL_F32_96_PLMS,
  FORM_COUNT
};

struct KernelForm {
  FormId id;
  const void* fn;         // the __global__ function (launched through hipLaunchKernel)
  const void* fn_tail;    // its instantiation with the sampler step's tail in the same launch (same arguments), or null
  int block;              // threads per workgroup
  size_t lds;             // dynamic LDS it is launched with
  size_t lds_grant;       // ... and asks the device for (residual_split_kernel: launched at two sizes, granted the larger)
  const char* name;       // bsg_diffnet_last_path
  const char* name_tail;  // ... with the tail inside the launch, or null
  StackForm family = STACK_NONE;
  int nct = 0;            // stack launches: column tiles of 32 frames per workgroup: tiles of 32 * nct frames
  int parts = 0;          // STACK_PART: workgroups per tile (4: quads, 2: pairs)
  FormVariant variant = FORM_PLAIN;
};

// the getters: every combination that has a kernel; null where there is none
const KernelForm* h2q_form(int nct, FormVariant variant, bool fair, int diag);   // diffnet_h2q.hip; diag: BSG_H2Q_DIAG 1 .. 6, else 0
const KernelForm* h2_form(int nct);                                              // diffnet_h2.hip: the 32-row stack launch
const KernelForm* part_form(int parts, int nct);                                 // ... (4, 1) quad of 32 frames, (4, 2) quad of 64, (2, 2) pair of 64
const KernelForm* h2_step_form(bool in_proj);                                    // ... step_tail_h2_kernel / in_proj_h2_kernel
const KernelForm* f43_form();                                                    // diffnet_f43.hip
const KernelForm* bf16_stack_form(bool ragged);                                  // diffnet_bf16.hip
const KernelForm* bf16_layer_form(bool stamps);
const KernelForm* bf16_tail_form(bool ragged, bool plms);
const KernelForm* layer_form(LayerForm layer, bool small_lds, bool stamps, bool wino);   // diffnet.hip: the fp32 per-layer launches
const KernelForm* tail_f32_form(int mp, bool plms);                                      // ... step_tail_kernel<mp, plms>, mp = 80 | 96

// Per handle, and so per device (a handle lives on one): the LDS grants made and the residencies asked.  Both are memos of what the device
// answers, not state of a call: const on a mutable store, so that planning reads a const handle.
class FormMemo {
 public:
  // the grant (hipFuncAttributeMaxDynamicSharedMemorySize on the form's functions), made once; every launch passes here: one array read
  int ready(const KernelForm& f) const {
    Entry& e = entry_[f.id];
    if (e.granted) return BSG_OK;
    for (const void* fn : {f.fn, f.fn_tail})
      if (fn) BSG_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds_grant));
    e.granted = true;
    return BSG_OK;
  }
  // resident workgroups per CU at the LDS size launched, as the runtime reports it (of the tail instantiation where there is one: the
  // larger kernel); asked once, behind the grant; 0 where either is refused
  int resident(const KernelForm& f) const {
    Entry& e = entry_[f.id];
    if (e.resident < 0) {
      int o = 0;
      e.resident = ready(f) == BSG_OK && hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, f.fn_tail ? f.fn_tail : f.fn, f.block, f.lds) == hipSuccess ? o : 0;
    }
    return e.resident;
  }

 private:
  struct Entry {
    bool granted = false;
    int resident = -1;   // -1: not asked
  };
  mutable Entry entry_[FORM_COUNT];
};

// one launch of `f` (with the step tail inside when `tail`) on `grid` workgroups; args: a pointer to every kernel argument, in order
inline int launch_form(const FormMemo& memo, const KernelForm& f, bool tail, dim3 grid, void** args, hipStream_t st) {
  const int rc = memo.ready(f);
  if (rc != BSG_OK) return rc;
  BSG_HIP(hipLaunchKernel(tail ? f.fn_tail : f.fn, grid, dim3(f.block), args, f.lds, st));
  return BSG_OK;
}

}  // namespace bsg
