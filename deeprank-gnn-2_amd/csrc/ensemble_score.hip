// The members' validation losses and metric sums, formed on the device
// (dr_ensemble_score): per member the loss the training pass forms, over the
// whole held-out set, and the sums RMSE / MAE / Pearson r / R^2 (regression) or
// accuracy and the confusion matrix (classification) are made of.
//
// One 256-thread workgroup per member.  Thread t walks rows t, t + 256, ... in
// ascending order and adds into its own doubles; the 256 partials are combined
// through LDS by the tree v[t] += v[t + s], s = 128 .. 1.  No floating-point
// atomics: the result is a pure function of the inputs.  The confusion counts
// are integers, gathered by LDS atomics.  K <= 8 members of up to ~1e5 rows of
// <= 16 floats: the kernel is launch-bound at every size this project meets.
//
// A row whose graph id lies outside the store, or (classification) whose target
// is no class index, is counted and otherwise left out: the guard comes before
// the value indexes y, class_w or the confusion matrix.

#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/deeprank2_amd.h"
#include "dr_common.h"

namespace drs {

constexpr int SC_NT = 256;
constexpr int SC_ACC = 11;  // accumulated slots; slot 11 of DR_SCORE_SUMS is written as zero

struct ScoreArgs {
  const float* out;
  int64_t member_stride;
  const int64_t* gids;
  int64_t gid_stride;
  const float* y;
  int64_t n_graphs;
  const float* class_w;
  double* sums;
  int64_t* confusion;
  int32_t n[DR_MAX_MEMBERS];
  int32_t out_dim, loss_kind, flags;
  float loss_param;
};

// the graph row i of member k scores against, or -1 when it lies outside the store
__device__ __forceinline__ int64_t score_gid(const ScoreArgs& a, int k, int64_t i) {
  const int64_t g = a.gids ? a.gids[k * a.gid_stride + i] : i;
  return (g >= 0 && g < a.n_graphs) ? g : -1;
}

// the fixed tree over the threads' partials, then the member's row of sums
__device__ __forceinline__ void score_reduce(const double (&acc)[SC_ACC], double (*red)[SC_NT], double* sums, int t) {
#pragma unroll
  for (int j = 0; j < SC_ACC; ++j) red[j][t] = acc[j];
  __syncthreads();
  for (int s = SC_NT / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int j = 0; j < SC_ACC; ++j) red[j][t] += red[j][t + s];
    }
    __syncthreads();
  }
  if (t < DR_SCORE_SUMS) sums[t] = t < SC_ACC ? red[t][0] : 0.0;
}

__global__ void __launch_bounds__(SC_NT) ensemble_score_regress_kernel(ScoreArgs a) {
  __shared__ double red[SC_ACC][SC_NT];
  const int k = blockIdx.x, t = threadIdx.x;
  const int64_t n = a.n[k];
  const float* out = a.out + k * a.member_stride;
  double acc[SC_ACC];
#pragma unroll
  for (int j = 0; j < SC_ACC; ++j) acc[j] = 0.0;
  for (int64_t i = t; i < n; i += SC_NT) {
    const int64_t g = score_gid(a, k, i);
    if (g < 0) {
      acc[3] += 1.0;
      continue;
    }
    const float o = out[i * a.out_dim];  // column 0, as the training loss reads it
    const float yv = a.y[g];
    const float d = o - yv;
    float term, gd;
    if (a.loss_kind == DR_LOSS_MSE) term = d * d;
    else dr_regress_loss(a.loss_kind, a.loss_param, d, &term, &gd);
    const double dd = (double)d, od = (double)o, yd = (double)yv;
    acc[0] += (double)term;
    acc[1] += 1.0;
    if (term != term) acc[2] += 1.0;
    acc[4] += dd * dd;
    acc[5] += fabs(dd);
    acc[6] += od;
    acc[7] += yd;
    acc[8] += od * od;
    acc[9] += yd * yd;
    acc[10] += od * yd;
  }
  score_reduce(acc, red, a.sums + (int64_t)k * DR_SCORE_SUMS, t);
}

__global__ void __launch_bounds__(SC_NT) ensemble_score_classif_kernel(ScoreArgs a) {
  __shared__ double red[SC_ACC][SC_NT];
  __shared__ unsigned int conf[DR_MAX_OUT * DR_MAX_OUT];
  const int k = blockIdx.x, t = threadIdx.x, C = a.out_dim;
  const int64_t n = a.n[k];
  const float* out = a.out + k * a.member_stride;
  const bool probs = (a.flags & DR_SCORE_PROBS) != 0;
  conf[t] = 0u;  // (SC_NT == DR_MAX_OUT * DR_MAX_OUT)
  __syncthreads();
  double acc[SC_ACC];
#pragma unroll
  for (int j = 0; j < SC_ACC; ++j) acc[j] = 0.0;
  for (int64_t i = t; i < n; i += SC_NT) {
    const int64_t g = score_gid(a, k, i);
    if (g < 0) {
      acc[3] += 1.0;
      continue;
    }
    const float yv = a.y[g];
    if (!(yv >= 0.f && yv < (float)C)) {  // (NaN fails both)
      acc[3] += 1.0;
      continue;
    }
    const int yi = (int)yv;
    if ((float)yi != yv) {
      acc[3] += 1.0;
      continue;
    }
    const float* o = out + i * C;
    float v[DR_MAX_OUT];  // every index below is a compile-time constant (the loops are unrolled): registers
    float mx = 0.f, oy = 0.f, best_v = 0.f;
    int best = 0;
    bool nan = false;
#pragma unroll
    for (int c = 0; c < DR_MAX_OUT; ++c) {
      if (c < C) {
        v[c] = o[c];
        nan = nan || v[c] != v[c];
        mx = c == 0 ? v[c] : fmaxf(mx, v[c]);
        if (c == yi) oy = v[c];
        if (c == 0 || v[c] > best_v) {  // strict: the lowest index among equals
          best = c;
          best_v = v[c];
        }
      }
    }
    float term;
    if (probs) {
      term = -logf(oy);
    } else {
      float se = 0.f;
#pragma unroll
      for (int c = 0; c < DR_MAX_OUT; ++c)
        if (c < C) se += expf(v[c] - mx);
      const float lse = mx + logf(se);
      term = lse - oy;
    }
    const float wy = a.class_w ? a.class_w[yi] : 1.f;
    acc[0] += (double)(wy * term);
    acc[1] += (double)wy;
    acc[5] += 1.0;  // rows scored: the accuracy's denominator (slot 1 is a sum of weights)
    if (nan) {
      acc[2] += 1.0;
    } else {
      if (best == yi) acc[4] += 1.0;
      if (a.confusion) atomicAdd(&conf[yi * C + best], 1u);
    }
  }
  score_reduce(acc, red, a.sums + (int64_t)k * DR_SCORE_SUMS, t);  // (its barriers order the LDS atomics before the reads below)
  if (a.confusion && t < C * C) a.confusion[(int64_t)k * C * C + t] = (int64_t)conf[t];
}

}  // namespace drs
using namespace drs;

static_assert(SC_NT == DR_MAX_OUT * DR_MAX_OUT, "one thread per confusion entry");
static_assert(SC_ACC <= DR_SCORE_SUMS, "the accumulated slots fit a row of sums");

extern "C" int dr_ensemble_score(const float* out, int64_t member_stride, const int64_t* gids, int64_t gid_stride,
                                 const float* y, int64_t n_graphs, const int32_t* n, int32_t n_members, int32_t out_dim,
                                 int32_t loss_kind, float loss_param, const float* class_w, int32_t flags, double* sums,
                                 int64_t* confusion, void* stream) {
  if (!out || !y || !sums || !n) return DR_E_ARG;
  if (n_members < 1 || n_members > DR_MAX_MEMBERS) return DR_E_ARG;
  if (out_dim < 1 || out_dim > DR_MAX_OUT) return DR_E_ARG;
  if (n_graphs < 0 || gid_stride < 0 || (flags & ~DR_SCORE_PROBS)) return DR_E_ARG;
  int32_t n_max = 0;
  for (int k = 0; k < n_members; ++k) {
    if (n[k] < 0) return DR_E_ARG;
    n_max = n[k] > n_max ? n[k] : n_max;
  }
  if (n_members > 1 && member_stride < (int64_t)n_max * out_dim) return DR_E_ARG;
  dr_pass p{};
  p.loss_kind = loss_kind;
  p.loss_param = loss_param;
  if (loss_kind == DR_LOSS_NONE || dr_check_loss(&p) != DR_OK) return DR_E_ARG;
  const bool classif = loss_kind == DR_LOSS_CE;
  if (classif && out_dim < 2) return DR_E_ARG;
  if (!classif && ((flags & DR_SCORE_PROBS) || confusion)) return DR_E_ARG;
  ScoreArgs a;
  a.out = out;
  a.member_stride = n_members > 1 ? member_stride : 0;
  a.gids = gids;
  a.gid_stride = gid_stride;
  a.y = y;
  a.n_graphs = n_graphs;
  a.class_w = classif ? class_w : nullptr;
  a.sums = sums;
  a.confusion = confusion;
  for (int k = 0; k < DR_MAX_MEMBERS; ++k) a.n[k] = k < n_members ? n[k] : 0;
  a.out_dim = out_dim;
  a.loss_kind = loss_kind;
  a.flags = flags;
  a.loss_param = loss_param;
  // (a member without rows writes zeros: the launch is made whatever the counts are)
  if (classif)
    hipLaunchKernelGGL(ensemble_score_classif_kernel, dim3(n_members), dim3(SC_NT), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(ensemble_score_regress_kernel, dim3(n_members), dim3(SC_NT), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
