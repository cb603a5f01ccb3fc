// Gradient reduction over the batch + torch.optim.AdamW / Adamax: the launch
// of reduce_adam.hip with another update rule.
//
// Replaces optimizer.step() of Trainer._epoch (deeprank2/trainer.py:690) for
// the optimizers a user hands to Trainer.configure_optimizers
// (trainer.py:401-428; the reference's README configures torch.optim.Adamax).
// The fixed-order partial sums and everything around the update (device step
// counter, fault flag, grad_div, packed-weight mirror, fault_clear / ticket,
// enabled == 0) are reduce_common.h's reduce_block, the code the Adam kernel
// runs; the rule is its compile-time OPT, one kernel instantiation per kind
// chosen on the host, so no kind pays a branch for another and the Adam
// kernel of dr_reduce_update stays as it is (DR_OPT_ADAM forwards to it).

#include <hip/hip_runtime.h>

#undef DR_STAMPS  // the stamps build's reduce timeline (drr::g_reduce_stamps) is reduce_adam.hip's alone
#include "reduce_common.h"

namespace {

using drr::RP;
using drr::RT;
#define DR_REDUCE_MAX_BLOCKS 512  // as reduce_adam.hip: 32 K parameter elements

struct alignas(64) ReduceArgs {
  drr::ReduceHdr h;
  drr::ParamRec rec[DR_MAX_PARAMS];
  // 1-D grid: block -> (parameter, first element); blocks never straddle two parameters
  uint8_t blk_param[DR_REDUCE_MAX_BLOCKS];
  uint16_t blk_elem[DR_REDUCE_MAX_BLOCKS];  // first element / RP
};

// Block j reduces RP consecutive elements of parameter blk_param[j] and
// applies rule OPT to them (reduce_adam_kernel's layout).
template <int OPT>
__global__ void __launch_bounds__(RT) reduce_optim_kernel(ReduceArgs a) {
  __shared__ float part[drr::RC][RP];
  const int pi = a.blk_param[blockIdx.x];
  const drr::ParamRec r = a.rec[pi];
  // every kernel-argument line this block uses in one scalar round trip
  {
    const float *slab = a.h.slab, *head = a.h.head;
    const int32_t B = a.h.B, ss = a.h.slab_stride, hs = a.h.head_stride, en = a.h.adam_enabled;
    asm volatile("" ::"s"(slab), "s"(head), "s"(B), "s"(ss), "s"(hs), "s"(en), "s"(r.param), "s"(r.grad), "s"(r.m),
                 "s"(r.v), "s"(r.numel), "s"(r.kind), "s"(r.off1), "s"(r.off2), "s"(r.cols));
  }
  const int64_t tstep = (a.h.step_counter && a.h.adam_enabled) ? a.h.step_counter[1] + 1 : 0;
  drr::reduce_block<0, false, false, OPT>(a.h, r, a.blk_elem[blockIdx.x], blockIdx.x == 0, threadIdx.x, part, tstep);
}

}  // namespace

extern "C" int dr_reduce_update_opt(const dr_param_table* t, const float* slab, const float* head, int32_t n_batch,
                                    const dr_optim* opt, const float* loss_per_graph, float loss_scale,
                                    float* loss_out, void* stream) {
  if (!opt) return DR_E_ARG;
  if (opt->kind == DR_OPT_ADAM)
    return dr_reduce_update(t, slab, head, n_batch, &opt->adam, loss_per_graph, loss_scale, loss_out, stream);
  if (opt->kind != DR_OPT_ADAMW && opt->kind != DR_OPT_ADAMAX) return DR_E_ARG;
  ReduceArgs a;
  std::memset(&a, 0, sizeof(a));
  const int blocks =
      drr::build_reduce(t, slab, head, n_batch, &opt->adam, loss_per_graph, loss_scale, loss_out, a.h, a.rec);
  if (blocks < 0) return blocks;
  if (blocks > DR_REDUCE_MAX_BLOCKS) return DR_E_UNSUPPORTED;
  a.h.om_beta1 = opt->om_beta1 != 0.f ? opt->om_beta1 : 1.f - opt->adam.beta1;
  a.h.om_beta2 = opt->om_beta2 != 0.f ? opt->om_beta2 : 1.f - opt->adam.beta2;
  int j = 0;
  for (int i = 0; i < t->n_params; ++i)
    for (int x = 0; x * RP < t->numel[i]; ++x, ++j) {
      a.blk_param[j] = (uint8_t)i;
      a.blk_elem[j] = (uint16_t)x;
    }
  if (blocks == 0) return DR_OK;
  if (opt->kind == DR_OPT_ADAMW)
    hipLaunchKernelGGL(reduce_optim_kernel<DR_OPT_ADAMW>, dim3(blocks), dim3(RT), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(reduce_optim_kernel<DR_OPT_ADAMAX>, dim3(blocks), dim3(RT), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
