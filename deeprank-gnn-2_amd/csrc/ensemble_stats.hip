// The ensemble's answer from its members' predictions (dr_ensemble_stats):
// per graph the members' mean and their spread (regression: the unbiased
// standard deviation; classification: the mean of the members' softmax
// probabilities, its entropy and its arg-max label).
//
// One thread per graph; a thread walks the members in the order k = 0 .. K-1
// in registers.  No atomics and no cross-thread reduction: the result is a
// pure function of the inputs, whatever the launch shape.  K <= 8 members of
// <= 16 floats per graph: the kernel reads K n out_dim floats once and is
// launch-bound at every size this project meets (1 024 graphs x 8 members x
// 16 classes = 512 KB).

#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/deeprank2_amd.h"
#include "dr_common.h"

namespace dre {

constexpr int ENS_NT = 256;

struct EnsArgs {
  const float* out;
  int64_t member_stride;
  int32_t n_members, n, out_dim, pad;
  float* mean;
  float* spread;
  int32_t* label;
};

// mean = (o_0 + o_1 + ... + o_{K-1}) / (float)K, the adds in member order and
// the divide a separate, correctly rounded operation (never a multiply by a
// reciprocal, never fused into the last add)
__device__ __forceinline__ float member_mean(const float* p, int64_t stride, int K) {
  float s = p[0];
  for (int k = 1; k < K; ++k) s = __fadd_rn(s, p[k * stride]);
  return __fdiv_rn(s, (float)K);
}

__global__ void __launch_bounds__(ENS_NT) ensemble_regress_kernel(EnsArgs a) {
  const int64_t i = (int64_t)blockIdx.x * ENS_NT + threadIdx.x;
  if (i >= a.n) return;
  const int K = a.n_members;
  const float dof = (float)(K - 1);  // 0 for one member: 0 / 0 = NaN, as torch.std gives
  for (int c = 0; c < a.out_dim; ++c) {
    const int64_t e = i * a.out_dim + c;
    const float* p = a.out + e;
    const float m = member_mean(p, a.member_stride, K);
    float ss = 0.f;
    for (int k = 0; k < K; ++k) {
      const float d = p[k * a.member_stride] - m;
      ss += d * d;
    }
    a.mean[e] = m;
    a.spread[e] = sqrtf(ss / dof);
  }
}

__global__ void __launch_bounds__(ENS_NT) ensemble_classif_kernel(EnsArgs a) {
  const int64_t i = (int64_t)blockIdx.x * ENS_NT + threadIdx.x;
  if (i >= a.n) return;
  const int K = a.n_members, C = a.out_dim;
  float pbar[DR_MAX_OUT];  // every index below is a compile-time constant (the loops are unrolled): registers
#pragma unroll
  for (int c = 0; c < DR_MAX_OUT; ++c) pbar[c] = 0.f;
  for (int k = 0; k < K; ++k) {
    const float* o = a.out + k * a.member_stride + i * C;
    float v[DR_MAX_OUT];
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < DR_MAX_OUT; ++c) {
      v[c] = c < C ? o[c] : -INFINITY;
      mx = fmaxf(mx, v[c]);  // (a NaN logit is skipped here and turns the whole row NaN through the sum below)
    }
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < DR_MAX_OUT; ++c) {
      if (c < C) {
        v[c] = expf(v[c] - mx);
        sum += v[c];
      }
    }
#pragma unroll
    for (int c = 0; c < DR_MAX_OUT; ++c) {
      if (c < C) {
        const float p = v[c] / sum;
        pbar[c] = k == 0 ? p : __fadd_rn(pbar[c], p);
      }
    }
  }
  float h = 0.f;
  int best = 0;
  float best_p = 0.f;
  bool nan = false;
#pragma unroll
  for (int c = 0; c < DR_MAX_OUT; ++c) {
    if (c < C) {
      const float p = __fdiv_rn(pbar[c], (float)K);
      a.mean[i * C + c] = p;
      if (p != 0.f) h -= p * logf(p);  // (NaN: h becomes NaN)
      nan = nan || p != p;
      if (c == 0 || p > best_p) {  // strict: the lowest index among equals
        best = c;
        best_p = p;
      }
    }
  }
  a.spread[i] = h;
  a.label[i] = nan ? -1 : best;
}

}  // namespace dre
using namespace dre;

extern "C" int dr_ensemble_stats(const float* out, int64_t member_stride, int32_t n_members, int32_t n,
                                 int32_t out_dim, int32_t kind, float* mean, float* spread, int32_t* label,
                                 void* stream) {
  if (!out || !mean || !spread) return DR_E_ARG;
  if (kind != DR_ENS_REGRESS && kind != DR_ENS_CLASSIF) return DR_E_ARG;
  if (kind == DR_ENS_CLASSIF && !label) return DR_E_ARG;
  if (n_members < 1 || n_members > DR_MAX_MEMBERS) return DR_E_ARG;
  if (out_dim < 1 || out_dim > DR_MAX_OUT || n < 0) return DR_E_ARG;
  if (n_members > 1 && member_stride < (int64_t)n * out_dim) return DR_E_ARG;
  if (n == 0) return DR_OK;
  EnsArgs a;
  a.out = out;
  a.member_stride = n_members > 1 ? member_stride : 0;
  a.n_members = n_members;
  a.n = n;
  a.out_dim = out_dim;
  a.pad = 0;
  a.mean = mean;
  a.spread = spread;
  a.label = label;
  const dim3 grid((unsigned)(((int64_t)n + ENS_NT - 1) / ENS_NT));
  if (kind == DR_ENS_REGRESS)
    hipLaunchKernelGGL(ensemble_regress_kernel, grid, dim3(ENS_NT), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(ensemble_classif_kernel, grid, dim3(ENS_NT), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
