// Gradient reduction over the batch + the optimizer update, the second launch
// of every fused model's training step (dr_reduce_update: torch.optim.Adam;
// dr_reduce_update_opt: Adam, AdamW or Adamax by dr_optim.kind;
// dr_reduce_update_multi: the same for up to DR_MAX_MEMBERS models at once).
//
// Replaces loss_.backward()'s accumulation over the batch and
// optimizer.step() of Trainer._epoch (deeprank2/trainer.py:689-690) for the
// optimizers a user hands to Trainer.configure_optimizers (trainer.py:401-428;
// Adam by default, the reference's README configures torch.optim.Adamax).
// Each parameter element's gradient is a sum over the per-graph partials the
// graph pass wrote (slab rows, or outer products of per-graph head vectors),
// taken in a fixed order: deterministic, no float atomics.  HBM-bound on the
// partials (~0.6 MB per GINet step at B=64).  The update rule is the kernel's
// compile-time OPT, one instantiation per kind chosen on the host, so no kind
// pays a branch for another.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/deeprank2_amd.h"
#include "dr_common.h"

#ifndef DR_RP
#define DR_RP 64
#endif
#ifndef DR_RC
#define DR_RC 8
#endif
#define DR_REDUCE_MAX_BLOCKS 512  // 32 K parameter elements (GINet at F=64: ~11.5 K)

// Diagnostic timeline (stamps build only, dr_debug_reduce_stamps): thread 0
// of block j writes s_memrealtime (100 MHz chip clock) at point i to
// g_reduce_stamps[j * 8 + i]: 0 entry, 5 kernel-argument record in, 1 its
// partials summed, 2 past the barrier, 3 stores issued, 4 stores done.
#ifdef DR_STAMPS
namespace drr {
__device__ int64_t g_reduce_stamps[4096 * 8];
}
static_assert(DR_REDUCE_MAX_BLOCKS <= 4096, "one stamp row per block of the largest grid");
#define RDSTAMP(i)                                                                                      \
  do {                                                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                                  \
    if (threadIdx.x == 0) drr::g_reduce_stamps[(int64_t)blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); \
    __builtin_amdgcn_sched_barrier(0);                                                                  \
  } while (0)
#else
#define RDSTAMP(i) \
  do {             \
  } while (0)
#endif

namespace {

constexpr int RP = DR_RP;  // parameter elements per block
constexpr int RC = DR_RC;  // batch chunks per block
constexpr int RU = 8;   // batch rows per chunk issued together (predicated)
constexpr int RU2 = 24; // then the rest of a chunk, this many at a time
constexpr int RT = RP * RC;  // threads per block

// One 64-byte kernel-argument line per parameter: a block fetches everything
// it needs about its parameter with one scalar load.
struct alignas(64) ParamRec {
  float* param;
  float* grad;
  float* m;
  float* v;
  int32_t numel, kind, off1, off2;
  int32_t cols, mbase, pad1, pad2;  // mbase: flat index of element 0 (dr_adam.mirror_idx)
};

struct alignas(64) ReduceHdr {
  const float* slab;
  const float* head;
  const float* lpg;
  float* loss_out;
  int64_t* step_counter;
  const float* grad_div;
  const uint32_t* fault;  // dr_adam.fault: nonzero -> NaN loss / gradients, no update
  int32_t B, slab_stride, head_stride, adam_enabled;
  float loss_scale, pad0;
  // pad0, n_params, blk0: read by no kernel, left zero.  They stay because
  // taking them out moves every later field and the block map, and hipcc then
  // schedules the kernels differently (not only other scalar-load offsets).
  float lr, beta1, beta2, eps, weight_decay, bias_c1, bias_c2_sqrt;
  float wd_mul;  // 1 - lr * weight_decay (AdamW's decoupled decay factor)
  float log2_beta1, log2_beta2;  // beta^t = exp2(t log2 beta): one v_exp_f32, not powf
  int32_t n_params, n_blocks;  // n_blocks: the grid, sum of ceil(numel / RP) (the fault_clear ticket counts to it)
  int16_t blk0[DR_MAX_PARAMS + 1];
  int32_t slab_rows;  // slab rows per graph (>= 1): a slab-kind gradient sums B * slab_rows rows
  float* mirror;            // dr_adam.mirror / mirror_idx: packed copies of updated elements
  const int4* mirror_idx;
  uint32_t* fault_clear;    // dr_adam.fault_clear / ticket
  uint32_t* ticket;
  // dr_optim.om_beta1 / om_beta2 (AdamW, Adamax; the Adam instantiation forms
  // 1.f - beta itself)
  float om_beta1, om_beta2;
};

struct alignas(64) ReduceArgs {
  ReduceHdr h;
  ParamRec rec[DR_MAX_PARAMS];
  // 1-D grid: block -> (parameter, first element); blocks never straddle two parameters
  uint8_t blk_param[DR_REDUCE_MAX_BLOCKS];
  uint16_t blk_elem[DR_REDUCE_MAX_BLOCKS];  // first element / RP
};

// One block = RP consecutive elements (from elem_block * RP) of parameter r,
// RC batch chunks per element; t = thread index within the block's RT
// threads, part = the block's [RC][RP] LDS scratch.  first: the block that
// also sums the loss and advances the step counter.  tstep: the optimizer
// step (counter[1] + 1) when h.step_counter is set.  The partials were
// written by an earlier launch (plain loads).  Every load of the block is
// issued in one straight-line group (clamped indices, zero weights past the
// batch), so one wait covers the partials and the optimizer state.
// OPT: the update rule (DR_OPT_*).
template <int OPT>
__device__ __forceinline__ void reduce_block(const ReduceHdr& h, const ParamRec& r, int elem_block, bool first, int t,
                                             float (*part)[RP], int64_t tstep) {
  const int lp = t % RP, ch = t / RP;
  const int e = elem_block * RP + lp;
  const bool live = e < r.numel;
  // a graph pass whose in-launch hand-off gave up (dr_pass.fault): its
  // partials are wrong, so the step reports NaN and changes no state
  const uint32_t fv = h.fault ? *h.fault : 0u;
  const bool bad = fv != 0u;
  if (first && t < 64 && h.lpg && h.loss_out) {
    float acc = 0.f;  // lane-strided partial sums, then a fixed-order wave reduction
    for (int b = t; b < h.B; b += 64) acc += h.lpg[b];
    acc = dr_wave_sum(acc);
    if (t == 0) h.loss_out[0] = bad ? __builtin_nanf("") : acc * h.loss_scale;
  } else if (bad && first && t == 0 && h.loss_out) {
    h.loss_out[0] = __builtin_nanf("");
  }
  const int ec = live ? e : 0;
  const bool slab_kind = r.kind == DR_GRAD_SLAB, outer = r.kind == DR_GRAD_OUTER;
  const bool has_src = h.slab && (slab_kind || outer || r.kind == DR_GRAD_HEAD);
  const int64_t st = slab_kind ? h.slab_stride : h.head_stride;
  const float* base = slab_kind ? h.slab : h.head;
  const int col1 = outer ? r.off1 + ec / r.cols : r.off1 + ec;
  const int col2 = outer ? r.off2 + ec % r.cols : 0;
  const int nb = slab_kind ? h.B * h.slab_rows : h.B;  // rows of this gradient's partials
  const int b0 = (nb * ch) / RC, b1 = (nb * (ch + 1)) / RC;
  float u[RU], w[RU];
  if (has_src && b0 < b1) {
#pragma unroll
    for (int k = 0; k < RU; ++k) {
      const int64_t row = min(b0 + k, b1 - 1);
      u[k] = base[row * st + col1];
      w[k] = outer ? base[row * st + col2] : 1.f;
    }
  }
  const bool upd = live && ch == 0 && h.adam_enabled && !bad;
  float p0 = 0.f, m0 = 0.f, v0 = 0.f, gin = 0.f;
  int4 mi = make_int4(-1, -1, -1, -1);  // dr_adam.mirror slots of this element, loaded with the state
  if (ch == 0 && h.adam_enabled && r.numel > 0) {  // numel 0: an empty record (no pointers)
    p0 = r.param[ec];
    m0 = r.m[ec];
    v0 = r.v[ec];
    if (h.mirror) mi = h.mirror_idx[r.mbase + ec];
  }
  float div = 1.f;
  if (ch == 0 && !h.slab && r.grad) {
    gin = r.grad[ec];
    if (h.grad_div) div = *h.grad_div;
  }
  if (h.slab) {
    float acc = 0.f;
    if (has_src && b0 < b1) {
#pragma unroll
      for (int k = 0; k < RU; ++k)
        if (b0 + k < b1) acc = outer ? fmaf(u[k], w[k], acc) : acc + u[k];
      // more than RU rows per chunk (e.g. split partial rows): the rest, RU2
      // rows' loads in flight at a time (same rows, same order)
      for (int bb = b0 + RU; bb < b1; bb += RU2) {
        float u2[RU2], w2[RU2];
#pragma unroll
        for (int k = 0; k < RU2; ++k) {
          const int64_t row = min(bb + k, b1 - 1);
          u2[k] = base[row * st + col1];
          w2[k] = outer ? base[row * st + col2] : 1.f;
        }
#pragma unroll
        for (int k = 0; k < RU2; ++k)
          if (bb + k < b1) acc = outer ? fmaf(u2[k], w2[k], acc) : acc + u2[k];
      }
    }
    part[ch][lp] = acc;
  }
  RDSTAMP(1);
  __syncthreads();
  RDSTAMP(2);
  if (ch != 0 || !live) return;
  // dr_adam.fault_clear: lane 0 of each block takes a ticket once its read of
  // the flag has returned; the last block's lane 0 clears the flag (every
  // block has read it by then) for the next graph pass
  const bool tick = h.fault_clear && lp == 0;
  uint32_t tk = 0u;
  if (tick) {
    asm volatile("" ::"v"(fv) : "memory");
    tk = __hip_atomic_fetch_add(h.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  float gsum;
  if (h.slab) {
    gsum = 0.f;
#pragma unroll
    for (int k = 0; k < RC; ++k) gsum += part[k][lp];
    if (bad) gsum = __builtin_nanf("");
    if (r.grad) r.grad[e] = gsum;
  } else {  // gradients supplied (e.g. after an RCCL all-reduce): the update only
    gsum = gin;
    if (h.grad_div) {
      gsum = gin / div;
      r.grad[e] = gsum;
      if (first && lp == 0 && h.loss_out) h.loss_out[0] = h.loss_out[0] / div;
    }
    if (bad) r.grad[e] = __builtin_nanf("");
  }
  if (upd) {
    float bc1 = h.bias_c1, bc2s = h.bias_c2_sqrt;
    if (h.step_counter) {  // step and bias corrections from the device counter
      bc1 = 1.f - exp2f((float)tstep * h.log2_beta1);
      bc2s = sqrtf(1.f - exp2f((float)tstep * h.log2_beta2));
      if (first && lp == 0) h.step_counter[0] = tstep;
    }
    // every product-sum spelled out (fmaf / __fmul_rn / __fadd_rn): no
    // contraction is left to the compiler
    float gr = gsum, pb = p0;  // the gradient and the parameter the rule starts from
    if constexpr (OPT == DR_OPT_ADAMW) {
      // torch.optim.AdamW (_single_tensor_adam, decoupled_weight_decay):
      // param.mul_(1 - lr*wd), the factor formed on the host in double as
      // Python forms it; the moments then see the raw gradient
      pb = __fmul_rn(p0, h.wd_mul);
    } else {
      if (h.weight_decay != 0.f) gr = fmaf(h.weight_decay, p0, gr);
    }
    // 1 - beta: Adam's own fp32 complement, or the caller's (dr_optim)
    const float ob1 = OPT == DR_OPT_ADAM ? 1.f - h.beta1 : h.om_beta1;
    const float ob2 = OPT == DR_OPT_ADAM ? 1.f - h.beta2 : h.om_beta2;
    // exp_avg.lerp_(g, 1-b1)
    const float mv = fmaf(ob1, __fsub_rn(gr, m0), m0);
    r.m[e] = mv;
    float pn;
    if constexpr (OPT == DR_OPT_ADAMAX) {
      // torch.optim.Adamax (_single_tensor_adamax): exp_inf = maximum(exp_inf*b2,
      // |g| + eps), NaN propagating (fmaxf alone would drop it);
      // param.addcdiv_(exp_avg, exp_inf, -lr / (1 - b1^t)).  r.v is the
      // table's exp_avg_sq slot, carrying exp_inf.
      const float ua = __fmul_rn(v0, h.beta2), ub = __fadd_rn(fabsf(gr), h.eps);
      const float uv = (ua != ua || ub != ub) ? __builtin_nanf("") : fmaxf(ua, ub);
      r.v[e] = uv;
      pn = fmaf(-(h.lr / bc1), __fdiv_rn(mv, uv), pb);
    } else {
      // torch.optim.Adam / AdamW: exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2)
      static_assert(OPT == DR_OPT_ADAM || OPT == DR_OPT_ADAMW, "unknown update rule");
      const float vv = fmaf(__fmul_rn(ob2, gr), gr, __fmul_rn(v0, h.beta2));
      r.v[e] = vv;
      const float denom = __fadd_rn(__fdiv_rn(sqrtf(vv), bc2s), h.eps);
      pn = fmaf(-(h.lr / bc1), __fdiv_rn(mv, denom), pb);
    }
    r.param[e] = pn;
    if (h.mirror) {
      if (mi.x >= 0) h.mirror[mi.x] = pn;
      if (mi.y >= 0) h.mirror[mi.y] = pn;
      if (mi.z >= 0) h.mirror[mi.z] = pn;
      if (mi.w >= 0) h.mirror[mi.w] = pn;
    }
  }
  if (tick && tk == (uint32_t)h.n_blocks - 1u) {
    *h.fault_clear = 0u;
    *h.ticket = 0u;
  }
  RDSTAMP(3);
#ifdef DR_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  RDSTAMP(4);
}

// 1-D grid over sum_p ceil(numel_p / RP) blocks: block j reduces RP
// consecutive elements of parameter blk_param[j] and applies rule OPT to
// them.  Its record and the header are scalar loads from the kernel arguments.
template <int OPT>
__global__ void __launch_bounds__(RT) reduce_kernel(ReduceArgs a) {
  __shared__ float part[RC][RP];
  RDSTAMP(0);
  const int pi = a.blk_param[blockIdx.x];
  const ParamRec r = a.rec[pi];
  // Pull every kernel-argument line this block uses in one scalar round trip
  // (hipcc would otherwise issue them lazily, one wait each).
  {
    const float *slab = a.h.slab, *head = a.h.head;
    const int32_t B = a.h.B, ss = a.h.slab_stride, hs = a.h.head_stride, en = a.h.adam_enabled;
    asm volatile("" ::"s"(slab), "s"(head), "s"(B), "s"(ss), "s"(hs), "s"(en), "s"(r.param), "s"(r.grad), "s"(r.m),
                 "s"(r.v), "s"(r.numel), "s"(r.kind), "s"(r.off1), "s"(r.off2), "s"(r.cols));
  }
  RDSTAMP(5);  // (stamps build: the block's kernel-argument record is in)
  const int64_t tstep = (a.h.step_counter && a.h.adam_enabled) ? a.h.step_counter[1] + 1 : 0;
  reduce_block<OPT>(a.h, r, a.blk_elem[blockIdx.x], blockIdx.x == 0, threadIdx.x, part, tstep);
}

// Host: header + records from the C-ABI table and optimizer settings; returns
// the number of RP-element blocks, or a negative DR_E_* code.
int build_reduce(const dr_param_table* t, const float* slab, const float* head, int32_t n_batch, const dr_adam* adam,
                 const float* loss_per_graph, float loss_scale, float* loss_out, ReduceHdr& h, ParamRec* rec) {
  if (!t || !adam || n_batch < 0) return DR_E_ARG;
  if ((slab == nullptr) != (head == nullptr)) return DR_E_ARG;
  if (t->n_params < 1 || t->n_params > DR_MAX_PARAMS) return DR_E_ARG;
  std::memset(&h, 0, sizeof(h));
  h.slab = slab;
  h.head = head;
  h.lpg = loss_per_graph;
  h.loss_out = loss_out;
  h.step_counter = adam->step_counter;
  h.grad_div = adam->grad_div;
  h.fault = adam->fault;
  h.B = n_batch;
  h.slab_stride = t->slab_stride;
  h.head_stride = t->head_stride;
  h.adam_enabled = adam->enabled;
  h.loss_scale = loss_scale;
  h.lr = adam->lr;
  h.beta1 = adam->beta1;
  h.beta2 = adam->beta2;
  h.eps = adam->eps;
  h.weight_decay = adam->weight_decay;
  h.bias_c1 = adam->bias_c1;
  h.bias_c2_sqrt = adam->bias_c2_sqrt;
  h.wd_mul = (float)(1.0 - (double)adam->lr * (double)adam->weight_decay);
  h.log2_beta1 = (float)std::log2((double)adam->beta1);
  h.log2_beta2 = (float)std::log2((double)adam->beta2);
  if ((adam->mirror == nullptr) != (adam->mirror_idx == nullptr)) return DR_E_ARG;
  if (adam->mirror_idx && (reinterpret_cast<uintptr_t>(adam->mirror_idx) & 15)) return DR_E_ARG;
  if (adam->fault_clear && !adam->ticket) return DR_E_ARG;
  h.mirror = adam->mirror;
  h.mirror_idx = reinterpret_cast<const int4*>(adam->mirror_idx);
  h.fault_clear = adam->fault_clear;
  h.ticket = adam->ticket;
  int blocks = 0, mbase = 0;
  for (int i = 0; i < t->n_params; ++i) {
    if (t->numel[i] < 0 || !t->param[i]) return DR_E_ARG;
    if (adam->enabled && (!t->exp_avg[i] || !t->exp_avg_sq[i])) return DR_E_ARG;
    if (!slab && !t->grad[i]) return DR_E_ARG;
    const dr_grad_recipe r = t->recipe[i];
    if (r.kind < DR_GRAD_ZERO || r.kind > DR_GRAD_HEAD || (r.kind == DR_GRAD_OUTER && r.cols <= 0)) return DR_E_ARG;
    ParamRec& pr = rec[i];
    std::memset(&pr, 0, sizeof(pr));
    pr.param = t->param[i];
    pr.grad = t->grad[i];
    pr.m = t->exp_avg[i];
    pr.v = t->exp_avg_sq[i];
    pr.numel = t->numel[i];
    pr.kind = r.kind;
    pr.off1 = r.off1;
    pr.off2 = r.off2;
    pr.cols = r.cols;
    pr.mbase = mbase;
    mbase += t->numel[i];
    blocks += (t->numel[i] + RP - 1) / RP;
  }
  if (blocks > 32767) return DR_E_UNSUPPORTED;
  h.n_blocks = blocks;
  if (t->slab_rows < 0 || t->slab_rows > 64) return DR_E_ARG;
  h.slab_rows = t->slab_rows > 0 ? t->slab_rows : 1;
  return blocks;
}

// Everything up to the launch, for a rule already validated by the caller.
// om_beta*: 0 = 1.f - beta (the Adam kernel does not read them).
int reduce_launch(int kind, const dr_param_table* t, const float* slab, const float* head, int32_t n_batch,
                  const dr_adam* adam, float om_beta1, float om_beta2, const float* loss_per_graph, float loss_scale,
                  float* loss_out, void* stream) {
  ReduceArgs a;
  std::memset(&a, 0, sizeof(a));
  const int blocks = build_reduce(t, slab, head, n_batch, adam, loss_per_graph, loss_scale, loss_out, a.h, a.rec);
  if (blocks < 0) return blocks;
  if (blocks > DR_REDUCE_MAX_BLOCKS) return DR_E_UNSUPPORTED;
  a.h.om_beta1 = om_beta1 != 0.f ? om_beta1 : 1.f - adam->beta1;
  a.h.om_beta2 = om_beta2 != 0.f ? om_beta2 : 1.f - adam->beta2;
  int j = 0;
  for (int i = 0; i < t->n_params; ++i)
    for (int x = 0; x * RP < t->numel[i]; ++x, ++j) {
      a.blk_param[j] = (uint8_t)i;
      a.blk_elem[j] = (uint16_t)x;
    }
  if (blocks == 0) return DR_OK;
  auto kernel = kind == DR_OPT_ADAMW    ? reduce_kernel<DR_OPT_ADAMW>
                : kind == DR_OPT_ADAMAX ? reduce_kernel<DR_OPT_ADAMAX>
                                        : reduce_kernel<DR_OPT_ADAM>;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(RT), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

// ---- several members in one launch (dr_reduce_update_multi) ---------------
// The argument buffer, in device memory: the block map the members share, then
// one header + record array per member.  (K ReduceArgs are ~3.3 KB each: past
// the kernel-argument segment.)
struct alignas(64) MultiHead {
  int32_t n_members, n_blocks, kind, pad[13];
  uint8_t blk_param[DR_REDUCE_MAX_BLOCKS];
  uint16_t blk_elem[DR_REDUCE_MAX_BLOCKS];
};
struct alignas(64) MultiMember {
  ReduceHdr h;
  ParamRec rec[DR_MAX_PARAMS];
};
static_assert(sizeof(MultiHead) % 64 == 0 && sizeof(MultiMember) % 64 == 0, "members start on 64-byte lines");

// Grid (n_blocks, K): block (j, k) is block j of member k's reduce_kernel<OPT>.
// The buffer is read-only for the launch: its map, header and record are read
// through the constant address space (scalar loads, as the kernel arguments
// of reduce_kernel are).
template <int OPT>
__global__ void __launch_bounds__(RT) reduce_multi_kernel(const void* args) {
  __shared__ float part[RC][RP];
  typedef const __attribute__((address_space(4))) MultiHead* CHead;
  typedef const __attribute__((address_space(4))) MultiMember* CMember;
  const CHead hd = (CHead)args;
  const int j = blockIdx.x, k = blockIdx.y;
  if (j >= hd->n_blocks || k >= hd->n_members) return;
  const CMember m = (CMember)((const __attribute__((address_space(4))) char*)args + sizeof(MultiHead)) + k;
  if (m->h.B == 0) return;  // the member sits this step out
  const int pi = hd->blk_param[j];
  const int eb = hd->blk_elem[j];
  const ReduceHdr& h = *(const ReduceHdr*)&m->h;
  const ParamRec& r = *(const ParamRec*)&m->rec[pi];
  // (every line of the header and the record the block uses, in one scalar round trip: as reduce_kernel)
  asm volatile("" ::"s"(h.slab), "s"(h.head), "s"(h.B), "s"(h.slab_stride), "s"(h.head_stride), "s"(h.adam_enabled),
               "s"(r.param), "s"(r.grad), "s"(r.m), "s"(r.v), "s"(r.numel), "s"(r.kind), "s"(r.off1), "s"(r.off2), "s"(r.cols));
  const int64_t tstep = (h.step_counter && h.adam_enabled) ? h.step_counter[1] + 1 : 0;
  reduce_block<OPT>(h, r, eb, j == 0, threadIdx.x, part, tstep);
}

}  // namespace

extern "C" int64_t dr_reduce_multi_args_bytes(int32_t n_members) {
  if (n_members < 1 || n_members > DR_MAX_MEMBERS) return -1;
  return (int64_t)sizeof(MultiHead) + (int64_t)n_members * (int64_t)sizeof(MultiMember);
}

extern "C" int dr_reduce_multi_build(const dr_reduce_member* members, int32_t n_members, void* host_buf, int64_t bytes) {
  if (!members || !host_buf || n_members < 1 || n_members > DR_MAX_MEMBERS) return DR_E_ARG;
  if (bytes < dr_reduce_multi_args_bytes(n_members)) return DR_E_ARG;
  // (built aside, so host_buf needs no alignment; it is left untouched on an error)
  MultiHead hd;
  std::memset(&hd, 0, sizeof(hd));
  MultiMember mm[DR_MAX_MEMBERS];
  const dr_param_table* t0 = members[0].t;
  const int kind = members[0].opt.kind;
  if (kind != DR_OPT_ADAM && kind != DR_OPT_ADAMW && kind != DR_OPT_ADAMAX) return DR_E_ARG;
  int blocks = 0;
  for (int k = 0; k < n_members; ++k) {
    const dr_reduce_member& m = members[k];
    if (m.opt.kind != kind) return DR_E_ARG;
    std::memset(&mm[k], 0, sizeof(MultiMember));
    const int b = build_reduce(m.t, m.slab, m.head, m.n_batch, &m.opt.adam, m.loss_per_graph, m.loss_scale, m.loss_out,
                               mm[k].h, mm[k].rec);
    if (b < 0) return b;
    if (b > DR_REDUCE_MAX_BLOCKS) return DR_E_UNSUPPORTED;
    // one block map: the members' parameters have the same sizes
    if (m.t->n_params != t0->n_params) return DR_E_ARG;
    for (int i = 0; i < t0->n_params; ++i)
      if (m.t->numel[i] != t0->numel[i]) return DR_E_ARG;
    mm[k].h.om_beta1 = m.opt.om_beta1 != 0.f ? m.opt.om_beta1 : 1.f - m.opt.adam.beta1;
    mm[k].h.om_beta2 = m.opt.om_beta2 != 0.f ? m.opt.om_beta2 : 1.f - m.opt.adam.beta2;
    blocks = b;
  }
  int j = 0;
  for (int i = 0; i < t0->n_params; ++i)
    for (int x = 0; x * RP < t0->numel[i]; ++x, ++j) {
      hd.blk_param[j] = (uint8_t)i;
      hd.blk_elem[j] = (uint16_t)x;
    }
  hd.n_members = n_members;
  hd.n_blocks = blocks;
  hd.kind = kind;
  std::memcpy(host_buf, &hd, sizeof(hd));
  std::memcpy(static_cast<char*>(host_buf) + sizeof(hd), mm, (size_t)n_members * sizeof(MultiMember));
  return blocks;
}

extern "C" int dr_reduce_update_multi(const void* dev_args, int32_t n_members, int32_t n_blocks, int32_t opt_kind,
                                      void* stream) {
  if (!dev_args || (reinterpret_cast<uintptr_t>(dev_args) & 63)) return DR_E_ARG;
  if (n_members < 1 || n_members > DR_MAX_MEMBERS || n_blocks < 0 || n_blocks > DR_REDUCE_MAX_BLOCKS) return DR_E_ARG;
  if (opt_kind != DR_OPT_ADAM && opt_kind != DR_OPT_ADAMW && opt_kind != DR_OPT_ADAMAX) return DR_E_ARG;
  if (n_blocks == 0) return DR_OK;
  auto kernel = opt_kind == DR_OPT_ADAMW    ? reduce_multi_kernel<DR_OPT_ADAMW>
                : opt_kind == DR_OPT_ADAMAX ? reduce_multi_kernel<DR_OPT_ADAMAX>
                                            : reduce_multi_kernel<DR_OPT_ADAM>;
  hipLaunchKernelGGL(kernel, dim3(n_blocks, n_members), dim3(RT), 0, (hipStream_t)stream, dev_args);
  return (int)hipGetLastError();
}

extern "C" int dr_reduce_update(const dr_param_table* t, const float* slab, const float* head, int32_t n_batch,
                                const dr_adam* adam, const float* loss_per_graph, float loss_scale, float* loss_out,
                                void* stream) {
  return reduce_launch(DR_OPT_ADAM, t, slab, head, n_batch, adam, 0.f, 0.f, loss_per_graph, loss_scale, loss_out, stream);
}

extern "C" int dr_reduce_update_opt(const dr_param_table* t, const float* slab, const float* head, int32_t n_batch,
                                    const dr_optim* opt, const float* loss_per_graph, float loss_scale,
                                    float* loss_out, void* stream) {
  if (!opt) return DR_E_ARG;
  if (opt->kind != DR_OPT_ADAM && opt->kind != DR_OPT_ADAMW && opt->kind != DR_OPT_ADAMAX) return DR_E_ARG;
  return reduce_launch(opt->kind, t, slab, head, n_batch, &opt->adam, opt->om_beta1, opt->om_beta2, loss_per_graph,
                       loss_scale, loss_out, stream);
}

#ifdef DR_STAMPS
// stamps build only: the reduce kernel's timeline stamps (of whichever kind ran last)
extern "C" int dr_debug_reduce_stamps(int64_t* host, int32_t n) {
  if (!host || n < 0 || n > 4096 * 8) return DR_E_ARG;
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(drr::g_reduce_stamps), (size_t)n * sizeof(int64_t), 0, hipMemcpyDeviceToHost);
}
#endif
