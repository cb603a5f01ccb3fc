// GINet training step, one workgroup per graph, everything resident in LDS.
//
// Replaces (deeprank2 v3.1.0):
//   GINetConvLayer.forward        deeprank2/neuralnets/gnn/ginet.py:40-60
//   GINet.forward                 ginet.py:90-125
//   get_preloaded_cluster         deeprank2/utils/community_pooling.py:23-27
//   community_pooling             community_pooling.py:165-242
//   max_pool_x / scatter_mean     ginet.py:103,114,117-118
//   autograd backward + loss      deeprank2/trainer.py:686-689
//
// Algebra used (all exact):
//   * the attention of ginet.py:48-55 is softmax over a size-1 dim, i.e. 1 for
//     every finite logit, so conv(x) = A·(x Wᵀ) with A[i,j] = #edges (i→j);
//     its parameters get exact-zero gradients (done by the reduce kernel);
//   * both branches see the same graph (data.clone(), ginet.py:92), so conv1
//     and conv1_ext are one GEMM with W = [W1; W1e] (32 outputs);
//   * per-batch cluster offsetting + consecutive_cluster is, graph by graph, a
//     dense relabelling of that graph's ids (precomputed into the store), and
//     pool_edge's coalesced pooled graph is precomputed as a CSR too.
//
// Execution: 1024 threads (16 waves) per graph; the graph and the weights are
// staged by global->LDS DMA (16-byte lanes where the store layout allows);
// conv1 aggregates first, Z = A·X, then H = relu(Z·Wᵀ) on the f32 MFMA
// (v_mfma_f32_16x16x4_f32: an exact k-ordered fmaf chain).  Because the
// depth-0 max pool routes each channel's gradient to one member per cluster,
// the conv1 weight gradient is sum_k v_k·Z[arg_k] and the backward needs no
// gather over the edges at all.
// Z depends only on the store's x and CSR, so by default it is built once per
// store (dr_aggregate_x) and the Z-input kernels (graph_body<..., ZIN>) DMA each
// graph's block into LDS instead of staging x / col / rowptr and gathering; the
// gather kernels stay as the fallback (no array yet, DR_GINET_AGGX=0).  The
// record kernels (graph_body<..., ZIN, REC>) go one step further: every input
// region of a graph but y is laid out once per store as the carve holds it
// (dr_graph_records), and one linear copy stages the graph.
// Roofline: HBM-bound on the compulsory inputs (x, CSR, clusters) and the
// per-graph partial writes — see DESIGN.md §Roofline.

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "../../include/deeprank2_amd.h"
#include "dr_common.h"
#include "graph_common.h"
#include "ginet_head.h"
#include "large_tile.h"

namespace {

using namespace drk;

constexpr int NT = 1024;     // 16 waves
constexpr int NW = NT / 64;
constexpr int HEADW = 672;   // G64 hpre128 hh128 hd128 dh128 dG64 dout16 spare16

struct Carve {
  int KP, LDW, XS;
  int w1, w2, fc2, x, z, rp, col, cl0, key, p1, a1, dp1, y2, h2, p1rp, p1c, p1trp, p1tc, m1p, m1i, p2, nt, cl1,
      head, dgp, keep, total;
};

// A walk over LDS in 4-byte words: each region starts 16-byte aligned.
struct LdsWalk {
  int o = 0;
  __host__ __device__ __forceinline__ void take(int& field, int words) {
    field = o;
    o += r4(words);
  }
};

// The regions every GINet carve lists, each written once (C: Carve or TailCarve).
template <class C>
__host__ __device__ __forceinline__ void take_head_weights(C& c, LdsWalk& w, int OUT) {
  w.take(c.w2, 1024);             // [W2 | W2e] (conv2 / conv2_ext .fc.weight)
  w.take(c.fc2, OUT * 128 + OUT); // fc2.weight rows, then fc2.bias
}
// the pooled graph and its transpose (one copy where the store aliases them), then the depth-1 members
template <class C>
__host__ __device__ __forceinline__ void take_pooled_inputs(C& c, LdsWalk& w, int K0, int P1, int K1, int alias) {
  w.take(c.p1rp, K0 + 1);
  w.take(c.p1c, P1);
  if (alias) {
    c.p1trp = c.p1rp;
    c.p1tc = c.p1c;
  } else {
    w.take(c.p1trp, K0 + 1);
    w.take(c.p1tc, P1);
  }
  w.take(c.m1p, K1 + 1);
  w.take(c.m1i, K0);
}
template <class C>
__host__ __device__ __forceinline__ void take_pool0(C& c, LdsWalk& w, int K0) {
  w.take(c.p1, K0 * 32);
  w.take(c.a1, K0 * 32);
  w.take(c.dp1, K0 * 32);
  w.take(c.y2, K0 * 64);
  w.take(c.h2, K0 * 64);
}
template <class C>
__host__ __device__ __forceinline__ void take_pool1_head(C& c, LdsWalk& w, int K0, int K1) {
  w.take(c.p2, K1 * 64);
  w.take(c.nt, K1 * 64);
  w.take(c.cl1, K0);  // depth-1 cluster of each depth-0 cluster
  w.take(c.head, HEADW);
  w.take(c.dgp, NW * 64);
}
// A graph's record (dr_graph_records), which is the Z-input carves' input
// regions as they lie in LDS: Z (rows of c.LDW words), the depth-0 cluster of
// each node, the pooled graph and the depth-1 members.
template <class C>
__host__ __device__ __forceinline__ void take_record_regions(C& c, LdsWalk& w, int N, int K0, int P1, int K1, int alias) {
  w.take(c.z, N * c.LDW);
  w.take(c.cl0, N);
  take_pooled_inputs(c, w, K0, P1, K1, alias);
}
// The sixteen regions from p1 to dgp, in the order carve() and tail_carve()
// share (everything the tail works in but the conv2 / head weights).
template <class C>
__host__ __device__ __forceinline__ void take_tail_regions(C& c, LdsWalk& w, int K0, int P1, int K1, int alias) {
  take_pool0(c, w, K0);
  take_pooled_inputs(c, w, K0, P1, K1, alias);
  take_pool1_head(c, w, K0, K1);
}

// K padded to the kernel's KPT (32 for F <= 32, else 64: the MFMA steps it
// runs; zeros past F).  (Until r05 KP was r16(F), shorter than KPT for F <= 16
// and 33..48: the padding zeroed to KPT then ran 14 words past Z into the
// row pointers being DMA'd beside it, and the last k steps read other
// waves' rows.)
__host__ __device__ __forceinline__ void carve_strides(Carve& c, int F, int zs) {
  c.KP = F <= 32 ? 32 : 64;
  c.LDW = zs > 0 ? zs : c.KP + 2;  // rows 2 words apart: lanes (row li, k+kq) hit 32 distinct banks
  c.XS = r4(F);
  c.x = c.rp = c.col = 0;
}

// LDS carve (4-byte words, every region 16-byte aligned).  X keeps the HBM
// row stride XS = r4(F) (16-byte rows for the DMA and the float4 gather);
// Z = A·X uses the stride KP+2 so the MFMA column reads are bank-conflict
// free.
// zs > 0: the Z-input form (dr_ginet_graph_pass_z): Z = A·X arrives from the
// store's array with rows of zs words, the stride it keeps in LDS, and the X,
// row pointer and column regions go.
__host__ __device__ __forceinline__ Carve carve(int N, int E, int F, int K0, int P1, int K1, int alias, int OUT, int zs = 0) {
  Carve c;
  carve_strides(c, F, zs);
  LdsWalk w;
  w.take(c.w1, 32 * F);  // [W1; W1e] (conv1 / conv1_ext .fc.weight), rows of F
  take_head_weights(c, w, OUT);
  if (zs > 0) {
    // every input region directly after z, in the order of the graph's record
    // (dr_graph_records): one linear copy stages them all
    take_record_regions(c, w, N, K0, P1, K1, alias);
    w.take(c.key, 2 * K0 * 32);
    take_pool0(c, w, K0);
    take_pool1_head(c, w, K0, K1);
  } else {
    w.take(c.x, N * c.XS);
    w.take(c.z, N * c.LDW);
    w.take(c.rp, N + 1);
    w.take(c.col, (E + 1) / 2);  // uint16 column ids
    w.take(c.cl0, N);            // depth-0 cluster of each node
    w.take(c.key, 2 * K0 * 32);  // depth-0 pooling keys (uint64)
    take_tail_regions(c, w, K0, P1, K1, alias);
  }
  w.take(c.keep, 32);  // 128 dropout keep bytes
  c.total = w.o;
  return c;
}

// The accumulating pass's prefetch layout (dr_ginet_acc_pass with the batch's
// maximum sizes): the weights stay put across a workgroup's graphs, and the
// inputs of graph k+1 are DMA'd by the waves that have no tile in graph k's
// front half (N <= 240), into the other of two input buffers:
//   [W1 | W2 | fc2] [inputs, parity 0: x rp col cl0 p1rp p1c p1trp p1tc m1p
//   m1i] [inputs, parity 1] [scratch: z key p1 a1 dp1 y2 h2 p2 nt cl1 head
//   dgp keep]
// (word offsets from the carve base; each region sized for the batch maxima).
// Three segments, each a walk of its own: a graph's carve (carve_acc) places
// them at the layout's segment starts, and the layout (acc_layout) is the
// same walks run on the batch maxima.
struct AccLayout {
  int in0, in1, scr, total;
};

__host__ __device__ __forceinline__ void acc_take_weights(Carve& c, LdsWalk& w, int F, int OUT) {
  w.take(c.w1, 32 * F);
  take_head_weights(c, w, OUT);
}
__host__ __device__ __forceinline__ void acc_take_inputs(Carve& c, LdsWalk& w, int N, int E, int K0, int P1, int K1, int alias,
                                                int zs) {
  if (zs > 0) {  // Z is an input: one copy per parity, the next graph's DMA'd under this graph's tail
    take_record_regions(c, w, N, K0, P1, K1, alias);
    return;
  }
  w.take(c.x, N * c.XS);
  w.take(c.rp, N + 1);
  w.take(c.col, (E + 1) / 2);
  w.take(c.cl0, N);
  take_pooled_inputs(c, w, K0, P1, K1, alias);
}
__host__ __device__ __forceinline__ void acc_take_scratch(Carve& c, LdsWalk& w, int N, int K0, int K1, int zs) {
  if (zs <= 0) w.take(c.z, N * c.LDW);
  w.take(c.key, 2 * K0 * 32);
  take_pool0(c, w, K0);
  take_pool1_head(c, w, K0, K1);
  w.take(c.keep, 32);
}

__host__ __device__ __forceinline__ Carve carve_acc(int N, int E, int F, int K0, int P1, int K1, int alias, int OUT,
                                           const AccLayout& L, int par, int zs = 0) {
  Carve c;
  carve_strides(c, F, zs);
  LdsWalk w;
  acc_take_weights(c, w, F, OUT);
  w.o = par ? L.in1 : L.in0;
  acc_take_inputs(c, w, N, E, K0, P1, K1, alias, zs);
  w.o = L.scr;
  acc_take_scratch(c, w, N, K0, K1, zs);
  c.total = w.o;
  return c;
}

// the layout for the batch maxima: the segments' starts and the total
__host__ __device__ __forceinline__ AccLayout acc_layout(int Nm, int Em, int F, int K0m, int P1m, int K1m, int alias, int OUT,
                                                int zs = 0) {
  AccLayout L;
  Carve c;
  carve_strides(c, F, zs);
  LdsWalk w;
  acc_take_weights(c, w, F, OUT);
  L.in0 = w.o;
  acc_take_inputs(c, w, Nm, Em, K0m, P1m, K1m, alias, zs);
  L.in1 = w.o;
  L.scr = L.in1 + (L.in1 - L.in0);
  w.o = L.scr;
  acc_take_scratch(c, w, Nm, K0m, K1m, zs);
  L.total = w.o;
  return L;
}

// A record on its own: section offsets from its first word, and its length
__host__ __device__ __forceinline__ Carve rec_layout(int N, int K0, int P1, int K1, int alias, int zs) {
  Carve c;
  c.LDW = zs;
  LdsWalk w;
  take_record_regions(c, w, N, K0, P1, K1, alias);
  c.total = w.o;
  return c;
}
// the words of a carve's record regions (z .. the end of m1i, the last of them)
__host__ __device__ __forceinline__ int rec_words(const Carve& c, int K0) { return c.m1i + r4(K0) - c.z; }

struct GinetArgs {
  dr_graph_store s;
  dr_ginet_weights w;
  dr_pass p;
  const dr_graph_desc* descs;
  int32_t B;
  // the Z-input kernels (dr_ginet_graph_pass_z / dr_ginet_acc_pass_z): the
  // store-wide Z = A·X of dr_aggregate_x, node i of the store at z + i * z_stride
  int32_t z_stride = 0;
  const float* z = nullptr;
  // the record kernels (dr_ginet_graph_pass_rec / dr_ginet_acc_pass_rec): the
  // buffer of dr_graph_records; descs then points at dr_graph_rec_desc
  // records (the sizes where dr_graph_desc has them, rec0 in the place of node0)
  const float* rec = nullptr;
};
static_assert(sizeof(dr_graph_rec_desc) == sizeof(dr_graph_desc) && offsetof(dr_graph_rec_desc, rec0) == offsetof(dr_graph_desc, node0) &&
                  offsetof(dr_graph_rec_desc, n_nodes) == offsetof(dr_graph_desc, n_nodes) &&
                  offsetof(dr_graph_rec_desc, gid) == offsetof(dr_graph_desc, gid),
              "the record kernels read dr_graph_rec_desc through dr_graph_desc");

// ---- the head's fc1.weight [128, 64] in the two register layouts ginet_head reads ----
//   row layout:    thread t holds W[t >> 3][8 * (t & 7) .. + 7]   (wave w: rows 8w .. 8w + 7, whole)
//   column layout: thread t holds W[8 * (t >> 6) + j][t & 63], j = 0 .. 7
// and the bias of row t >> 3.  (Wave w's two layouts are the same 8 x 64 tile,
// fetched twice.  Fetching it once and transposing it in LDS was measured and
// not kept: DESIGN.md §5, "weights once".)
__device__ __forceinline__ void fc1_load(const dr_ginet_weights& w, int tid, int wave, float (&row)[8], float (&col)[8],
                                         float& bias) {
  const int r = tid >> 3, part = tid & 7;
  const float4 u0 = *reinterpret_cast<const float4*>(w.fc1w + r * 64 + part * 8);
  const float4 u1 = *reinterpret_cast<const float4*>(w.fc1w + r * 64 + part * 8 + 4);
  row[0] = u0.x; row[1] = u0.y; row[2] = u0.z; row[3] = u0.w;
  row[4] = u1.x; row[5] = u1.y; row[6] = u1.z; row[7] = u1.w;
  bias = w.fc1b[r];
  const int o = tid & 63;
#pragma unroll
  for (int j = 0; j < 8; ++j) col[j] = w.fc1w[(wave * 8 + j) * 64 + o];
}

// ---- conv1's B operands of v_mfma_f32_16x16x4_f32, KPT = 32 ----
// Lane (li, kq) = (lane & 15, lane >> 4) holds, in register r of its 16 (wa[r]
// for r < 8: conv1, row li of W1; wb[r - 8]: conv1_ext, row li of W1e), the
// element at k = 16 * ((r & 7) >> 2) + 4 * (r & 3) + kq, zero past F.  The
// image is those 1 024 words in the order the lanes read them: four planes of
// 64 lanes x 4 words, lane l's registers 4p .. 4p + 3 at plane p, words 4l ..
// 4l + 3 — one 16-byte read per plane, consecutive lanes on consecutive 16-byte
// slots (conflict-free).  w1_image_src: image word -> its element of the packed
// [W1; W1e] (32 rows of F), or -1: zero.  The staging DMA (per-lane source
// address, linear LDS destination), the reads and the host test share it.
__host__ __device__ inline int w1_image_word(int lane, int r) { return (r >> 2) * 256 + lane * 4 + (r & 3); }
__host__ __device__ inline int w1_image_src(int F, int word) {
  const int p = word >> 8, l = (word >> 2) & 63, q = word & 3;
  const int li = l & 15, kq = l >> 4;
  const int kk = 16 * (p & 1) + 4 * q + kq;
  return kk < F ? ((p >> 1) * 16 + li) * F + kk : -1;
}

// Stage conv1's weights: the image (IMG; NT threads, one word each: one DMA
// instruction per wave, lanes of zero words masked off) or the packed rows.
template <bool IMG>
__device__ __forceinline__ void w1_stage(float* sW1, float* img, const dr_ginet_weights& w, int F, int tid) {
  if (IMG) {
    static_assert(NT == 1024, "one image word per thread");
    const int src = w1_image_src(F, tid);
    const int base = __builtin_amdgcn_readfirstlane(tid & ~63);
    if (src >= 0) {
      const float* g = tid < 512 ? w.w1 + src : w.w1e + (src - 16 * F);  // (planes 0, 1: W1; 2, 3: W1e)
      __builtin_amdgcn_global_load_lds(DRK_AS1(g), DRK_AS3(img + base), 4, 0, 0);
    }
  } else {
    dma_copy<NT, 4>(sW1, w.w1, 16 * F, tid);  // [W1; W1e] rows of F, packed
    dma_copy<NT, 4>(sW1 + 16 * F, w.w1e, 16 * F, tid);
  }
}
// the image's zero words (k >= F), by plain stores beside the DMA
template <bool IMG>
__device__ __forceinline__ void w1_zero_pad(float* img, int F, int tid) {
  if (IMG && w1_image_src(F, tid) < 0) img[tid] = 0.f;
}
// after the staging barrier: the lane's operands
template <int KPT, bool IMG>
__device__ __forceinline__ void w1_operands(const float* sW1, const float* img, int F, int lane, float (&wa)[KPT / 4],
                                            float (&wb)[KPT / 4]) {
  if constexpr (IMG) {
    static_assert(KPT == 32, "the image holds 8 + 8 registers per lane");
    const float4 a0 = *reinterpret_cast<const float4*>(img + w1_image_word(lane, 0));
    const float4 a1 = *reinterpret_cast<const float4*>(img + w1_image_word(lane, 4));
    const float4 b0 = *reinterpret_cast<const float4*>(img + w1_image_word(lane, 8));
    const float4 b1 = *reinterpret_cast<const float4*>(img + w1_image_word(lane, 12));
    wa[0] = a0.x; wa[1] = a0.y; wa[2] = a0.z; wa[3] = a0.w;
    wa[4] = a1.x; wa[5] = a1.y; wa[6] = a1.z; wa[7] = a1.w;
    wb[0] = b0.x; wb[1] = b0.y; wb[2] = b0.z; wb[3] = b0.w;
    wb[4] = b1.x; wb[5] = b1.y; wb[6] = b1.z; wb[7] = b1.w;
  } else {
    const int li = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int j = 0; j < KPT / 4; ++j) {
      const int kk = 16 * (j >> 2) + 4 * (j & 3) + kq;
      wa[j] = kk < F ? sW1[li * F + kk] : 0.f;
      wb[j] = kk < F ? sW1[(16 + li) * F + kk] : 0.f;
    }
  }
}

#ifdef DR_STAMPS
#define STAMP(i)                                                                                  \
  do {                                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                            \
    if (tid == 0 && a.p.stamps) a.p.stamps[(int64_t)b * 32 + (i)] = __builtin_amdgcn_s_memtime(); \
    __builtin_amdgcn_sched_barrier(0);                                                            \
  } while (0)
#define SSTAMP(i)                                                                                   \
  do {                                                                                              \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    if (tid == 0 && ga.p.stamps) ga.p.stamps[(int64_t)b * 32 + (i)] = __builtin_amdgcn_s_memtime(); \
    __builtin_amdgcn_sched_barrier(0);                                                              \
  } while (0)
// cross-workgroup timeline (s_memrealtime: one 100 MHz clock for the whole chip)
#define RSTAMP(row, i)                                                                                  \
  do {                                                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                                  \
    if (threadIdx.x == 0 && a.g.p.stamps) a.g.p.stamps[(int64_t)(row) * 32 + (i)] = __builtin_amdgcn_s_memrealtime(); \
    __builtin_amdgcn_sched_barrier(0);                                                                  \
  } while (0)
#else
#define RSTAMP(row, i) \
  do {                 \
  } while (0)
#define STAMP(i) \
  do {           \
  } while (0)
#define SSTAMP(i) \
  do {            \
  } while (0)
#endif
// -DDR_STAMPS=2: marks inside three tail phases as well (stamps 15-19, 28).
// Each waits for wave 0's LDS reads first, which ends the overlap the phase
// has without it: read these apart from the phase table of -DDR_STAMPS.
#if defined(DR_STAMPS) && DR_STAMPS >= 2
// (SUBSTAMP: in a `for (p = tid; ...)` loop, the first item only)
#define SUBSTAMP0(i)                                                                              \
  do {                                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                            \
    if (tid < 64 && a.p.stamps) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                \
    if (tid == 0 && a.p.stamps) a.p.stamps[(int64_t)b * 32 + (i)] = __builtin_amdgcn_s_memtime(); \
    __builtin_amdgcn_sched_barrier(0);                                                            \
  } while (0)
#define SUBSTAMP(i)          \
  do {                       \
    if (p < NT) SUBSTAMP0(i); \
  } while (0)
#else
#define SUBSTAMP0(i) \
  do {               \
  } while (0)
#define SUBSTAMP(i) \
  do {              \
  } while (0)
#endif

// f(integral_constant<int, M>) with M = min(n, G) for a wave-uniform n >= 1
// (n <= 0: nothing): a group of exactly M items, every slot of it live
template <int G, class F>
__device__ __forceinline__ void uniform_group(int n, F&& f) {
  if constexpr (G > 1) {
    if (n >= G) f(std::integral_constant<int, G>());
    else uniform_group<G - 1>(n, f);
  } else {
    if (n >= 1) f(std::integral_constant<int, 1>());
  }
}

// sum over a pooled CSR row [eb, ee) of v[col[e] * 64 + o], in edge order;
// four index reads, then four value reads in flight per step (same sum order
// as the plain loop).
__device__ __forceinline__ float pooled_row_sum(const int* col, int eb, int ee, const float* v, int o) {
  float acc = 0.f;
  int e = eb;
  for (; e + 4 <= ee; e += 4) {
    const int c0 = col[e], c1 = col[e + 1], c2 = col[e + 2], c3 = col[e + 3];
    const float v0 = v[c0 * 64 + o], v1 = v[c1 * 64 + o], v2 = v[c2 * 64 + o], v3 = v[c3 * 64 + o];
    acc = (((acc + v0) + v1) + v2) + v3;
  }
  for (; e < ee; ++e) acc += v[col[e] * 64 + o];
  return acc;
}

// Everything after the depth-0 pooling (P1 / A1 in LDS): conv2 on the pooled
// graph, depth-1 pooling, mean, head, loss and the whole backward.  Shared by
// the single-workgroup kernel and the large-graph tail kernel; zat(i, kk)
// reads Z = A·X at node i (LDS or the large path's HBM workspace).
struct TailLds {
  float *w2, *fc2, *p1, *dp1, *y2, *h2, *p2, *nt, *dgp;
  float *g, *hpre, *hh, *hd, *dh, *dg, *dout;
  int *a1, *p1rp, *p1c, *p1trp, *p1tc, *m1p, *m1i, *cl1;
  const uint8_t* keep = nullptr;  // prefetched dropout keep flags, or null (hash in the head)
  // accumulating pass (dr_ginet_acc_pass): the workgroup's running sums
  // [dW1cat 32F | dW2cat 1024 | the head's, GinetHeadLds::acc], or null
  float* acc = nullptr;
  float* accf = nullptr;  // GinetHeadLds::accf
  // p2's first row zeroed by the caller before its last barrier: with one
  // depth-1 cluster (K1 = 1, K0 < 16) conv2 folds the depth-1 max into it by
  // LDS atomic max, and the pooling and mean steps go
  bool p2_zeroed = false;
};

template <class C>
__device__ __forceinline__ TailLds tail_lds(const C& c, float* lds) {
  TailLds t;
  t.w2 = lds + c.w2;
  t.fc2 = lds + c.fc2;
  t.p1 = lds + c.p1;
  t.a1 = reinterpret_cast<int*>(lds + c.a1);
  t.dp1 = lds + c.dp1;
  t.y2 = lds + c.y2;
  t.h2 = lds + c.h2;
  t.p1rp = reinterpret_cast<int*>(lds + c.p1rp);
  t.p1c = reinterpret_cast<int*>(lds + c.p1c);
  t.p1trp = reinterpret_cast<int*>(lds + c.p1trp);
  t.p1tc = reinterpret_cast<int*>(lds + c.p1tc);
  t.m1p = reinterpret_cast<int*>(lds + c.m1p);
  t.m1i = reinterpret_cast<int*>(lds + c.m1i);
  t.p2 = lds + c.p2;
  t.nt = lds + c.nt;
  t.cl1 = reinterpret_cast<int*>(lds + c.cl1);
  t.g = lds + c.head;
  t.hpre = t.g + 64;
  t.hh = t.hpre + 128;
  t.hd = t.hh + 128;
  t.dh = t.hd + 128;
  t.dg = t.dh + 128;
  t.dout = t.dg + 64;
  t.dgp = lds + c.dgp;
  return t;
}

template <class ZAt, bool ACC = false>
__device__ __forceinline__ void ginet_tail(const GinetArgs& a, const TailLds& t, const float (&fc1_row)[8],
                                           const float (&fc1_col)[8], float fc1_bias, int b, int N, int K0, int K1,
                                           int F, int OUT, float y_g, uint64_t drop_offset, ZAt zat, int pb) {
  if (pb < 0) pb = b;  // the partials' row (slab, head vectors, loss term)
  const int tid = dr_tid<ACC>();
  STAMP(4);
  // one depth-1 cluster: its max over the K0 pooled rows per channel by LDS
  // atomic max on the bits as conv2 produces the rows (H2 >= +0 or NaN, so
  // the unsigned order of the bits is the value order; NaN wins, as the
  // reference's NaN-propagating amax), the tie counts in the pooling backward
  const bool one_cl = t.p2_zeroed && K1 == 1 && K0 < 16;
  // ---------------- conv2 on the pooled graph (ginet.py:101,112) ------------
  // H2[k][o] = relu(sum over pooled row k, in edge order, of Y2[j][o]) with
  // Y2[j][o] = P1[j] . W2[o] (16-term fmaf chain) formed per neighbour in
  // registers: no Y2 array and no barrier between the GEMM and the sum
  for (int p = tid; p < K0 * 64; p += NT) {
    const int k = p >> 6, o = p & 63, br = o >> 5;
    float wr[16];  // rows 0..31 = W2, 32..63 = W2e
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(t.w2 + o * 16 + 4 * q);
      wr[4 * q] = v.x;
      wr[4 * q + 1] = v.y;
      wr[4 * q + 2] = v.z;
      wr[4 * q + 3] = v.w;
    }
    float acc = 0.f;
    SUBSTAMP(15);
    // the row's neighbours two at a time and a last one alone: the group's
    // column ids, then its half-rows of P1 in flight, one chain per neighbour,
    // and the sums added in edge order.  (Groups of four hold 64 row values:
    // 113-127 VGPRs and scratch in three accumulating kernels.)
    // (k = p >> 6 is the same for a wave's 64 lanes: the row's bounds in
    // SGPRs, the group size a scalar branch.  A group never has an idle slot:
    // these phases are bound by the instructions one wave issues, and a
    // predicated group of fixed width ran its idle slots' instructions too)
    constexpr int G2 = 2;
    const int eb = __builtin_amdgcn_readfirstlane(t.p1rp[k]), ee = __builtin_amdgcn_readfirstlane(t.p1rp[k + 1]);
    for (int e0 = eb; e0 < ee; e0 += G2) {
      uniform_group<G2>(ee - e0, [&](auto m_t) {
        constexpr int M = decltype(m_t)::value;
        int c[M];
#pragma unroll
        for (int u = 0; u < M; ++u) c[u] = t.p1c[e0 + u];
        float4 v[M][4];
#pragma unroll
        for (int u = 0; u < M; ++u) {
          const float* pr = t.p1 + c[u] * 32 + br * 16;
#pragma unroll
          for (int q = 0; q < 4; ++q) v[u][q] = *reinterpret_cast<const float4*>(pr + 4 * q);
        }
        float y[M];
#pragma unroll
        for (int u = 0; u < M; ++u) {
          y[u] = 0.f;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            y[u] = fmaf(v[u][q].x, wr[4 * q], y[u]);
            y[u] = fmaf(v[u][q].y, wr[4 * q + 1], y[u]);
            y[u] = fmaf(v[u][q].z, wr[4 * q + 2], y[u]);
            y[u] = fmaf(v[u][q].w, wr[4 * q + 3], y[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < M; ++u) acc += y[u];
      });
    }
    SUBSTAMP(16);
    const float h2v = relu_keepnan(acc);
    t.h2[p] = h2v;
    if (one_cl) __hip_atomic_fetch_max(reinterpret_cast<uint32_t*>(t.p2) + o, __float_as_uint(h2v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();

  if (one_cl) {
    STAMP(5);  // (no pooling or mean step: stamps 5, 6 mark the same point)
    STAMP(6);
  } else {
    STAMP(5);
    // ---------------- depth-1 max_pool_x: scatter_reduce amax (ginet.py:103) --
    // NaN propagates; remember the tie count for the even-split backward.
    // Members are split into S slices per (cluster, channel): each slice's
    // max (NaN-propagating) and its count of members equal to it, combined per
    // pair (max is order-free here: H2 >= +0 or NaN).  Also record each
    // depth-0 cluster's depth-1 cluster for the backward.
    // (by the last wave, idle here unless K1 >= 15: the pooling pairs start at
    // wave 0; m counts the member offsets at or below q, all reads in flight)
    for (int q = tid - (NT - 64); q >= 0 && q < K0; q += 64) {
      int m = 0;
      if (K1 <= 16) {
#pragma unroll
        for (int j = 1; j < 16; ++j) m += (j < K1 && t.m1p[j < K1 ? j : 0] <= q) ? 1 : 0;
      } else {
        while (q >= t.m1p[m + 1]) ++m;
      }
      t.cl1[t.m1i[q]] = m;
    }
    if (K0 < 16) {  // few members per pair: one pass
      for (int p = tid; p < K1 * 64; p += NT) {
        const int m = p >> 6, o = p & 63;
        const int mb = t.m1p[m], me = t.m1p[m + 1];
        // members' values gathered once (<= 15): all index reads, then all
        // value reads in flight (predicated); max and tie count are order-free
        float v[16];
        int q[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) q[u] = t.m1i[(mb + u < me) ? mb + u : mb];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = t.h2[q[u] * 64 + o];
        float mx = v[0];
#pragma unroll
        for (int u = 1; u < 16; ++u)
          if (mb + u < me) mx = (mx != mx || v[u] != v[u]) ? __int_as_float(0x7fc00000) : fmaxf(mx, v[u]);
        float ties = 0.f;
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (mb + u < me) ties += (v[u] == mx) ? 1.f : 0.f;
        t.p2[p] = mx;
        t.nt[p] = ties;
        if (K1 == 1) t.g[o] = (0.f + mx) / (float)K1;  // the mean below, for one cluster (same ops)
      }
    } else {
      const int pairs = K1 * 64;
      const int LS = pairs <= 32 ? 4 : pairs <= 64 ? 3 : pairs <= 128 ? 2 : pairs <= 256 ? 1 : 0;  // pairs*S <= 512
      const int S = 1 << LS;
      float* smx = t.dgp;            // [pairs*S] (dgp is free until the head)
      float* scnt = t.dgp + 512;
      const float NEG = -__builtin_inff();
      for (int p = tid; p < pairs * S; p += NT) {
        const int sl = p & (S - 1), pr = p >> LS, m = pr >> 6, o = pr & 63;
        const int mb = t.m1p[m], cnt = t.m1p[m + 1] - mb;
        const int qb = mb + ((cnt * sl) >> LS), qe = mb + ((cnt * (sl + 1)) >> LS);
        float mx = NEG;
        for (int q = qb; q < qe; ++q) {
          const float v = t.h2[t.m1i[q] * 64 + o];
          mx = (mx != mx || v != v) ? __int_as_float(0x7fc00000) : fmaxf(mx, v);
        }
        float ties = 0.f;
        for (int q = qb; q < qe; ++q) ties += (t.h2[t.m1i[q] * 64 + o] == mx) ? 1.f : 0.f;
        smx[p] = mx;
        scnt[p] = ties;
      }
      __syncthreads();
      for (int p = tid; p < pairs; p += NT) {
        float mx = NEG;
        bool nan = false;
        for (int sl = 0; sl < S; ++sl) {
          const float v = smx[(p << LS) + sl];
          if (v != v) nan = true;
          else mx = fmaxf(mx, v);
        }
        float ties = 0.f;
        if (nan) mx = __int_as_float(0x7fc00000);
        else
          for (int sl = 0; sl < S; ++sl) ties += (smx[(p << LS) + sl] == mx) ? scnt[(p << LS) + sl] : 0.f;
        t.p2[p] = mx;
        t.nt[p] = ties;
      }
    }
    __syncthreads();

    STAMP(6);
    // ---------------- per-graph mean (scatter_mean, ginet.py:117-118) ----------
    // (K1 = 1 with K0 < 16: written by the pooling above)
    if (!(K1 == 1 && K0 < 16)) {
      if (tid < 64) {
        float acc = 0.f;
        for (int m = 0; m < K1; ++m) acc += t.p2[m * 64 + tid];
        t.g[tid] = acc / (float)K1;
      }
      __syncthreads();
    }
  }

  STAMP(7);
  {
    drk::GinetHeadLds hl;
    hl.fc2 = t.fc2;
    hl.g = one_cl ? t.p2 : t.g;  // (one cluster: the mean (0 + max) / 1 is the max itself)
    hl.hpre = t.hpre;
    hl.hh = t.hh;
    hl.hd = t.hd;
    hl.dh = t.dh;
    hl.dg = t.dg;
    hl.dout = t.dout;
    hl.dgp = t.dgp;
    hl.keep = t.keep;
    hl.acc = ACC ? t.acc + 32 * F + 1024 : nullptr;
    hl.accf = ACC ? t.accf : nullptr;
    hl.dg_deferred = true;  // summed from dgp by the pooling backward below
    if (!drk::ginet_head<NT, ACC>(a.p, hl, fc1_row, fc1_col, fc1_bias, b, OUT, y_g, drop_offset, 8, pb)) return;
  }  // stamps 8 (forward head done) and 9 (loss gradient done) are taken inside

  STAMP(10);
  // ---------------- depth-1 pooling + mean backward -------------------------
  // scatter_mean: grad/count; scatter_reduce amax: grad split evenly over the
  // members equal to the max ((src==max) * grad/ties, so NaN stays NaN).
  // dS2[k][o] (the gradient at H2's pre-activation) is formed per neighbour
  // inside dY2 = A1^T dS2 (pooled graph, transposed CSR, edge order): no dS2
  // array and no barrier between the two
  for (int p = tid; p < K0 * 64; p += NT) {
    const int j = p >> 6, o = p & 63;
    float dgs = 0.f;  // dG[o]: the head's 16 per-wave partials in order (ginet_head, dg_deferred)
#pragma unroll
    for (int rc = 0; rc < NW; ++rc) dgs += t.dgp[rc * 64 + o];
    const float dgo = dgs / (float)K1;
    float acc = 0.f;
    // every loop below goes four items at a time and the rest (1-3) as a
    // group of exactly that size, a group's reads in flight together (index
    // reads, then the gathers); the sums keep their terms and their order.
    // (j = p >> 6 is wave-uniform: the transposed row's bounds in SGPRs)
    const int eb = __builtin_amdgcn_readfirstlane(t.p1trp[j]), ee = __builtin_amdgcn_readfirstlane(t.p1trp[j + 1]);
    SUBSTAMP(17);
    if (one_cl) {  // the one cluster's tie count per channel, here instead of in the pooling step
      const float mx = t.p2[o];
      float ties = 0.f;
      for (int q0 = 0; q0 < K0; q0 += 4) {
        uniform_group<4>(K0 - q0, [&](auto m_t) {
          constexpr int M = decltype(m_t)::value;
          float hv[M];
#pragma unroll
          for (int u = 0; u < M; ++u) hv[u] = t.h2[(q0 + u) * 64 + o];
#pragma unroll
          for (int u = 0; u < M; ++u) ties += (hv[u] == mx) ? 1.f : 0.f;
        });
      }
      SUBSTAMP(18);
      for (int e0 = eb; e0 < ee; e0 += 4) {
        uniform_group<4>(ee - e0, [&](auto m_t) {
          constexpr int M = decltype(m_t)::value;
          int c[M];
#pragma unroll
          for (int u = 0; u < M; ++u) c[u] = t.p1tc[e0 + u];
          float h[M];
#pragma unroll
          for (int u = 0; u < M; ++u) h[u] = t.h2[c[u] * 64 + o];
#pragma unroll
          for (int u = 0; u < M; ++u) acc += relu_bwd(h[u], (h[u] == mx ? 1.f : 0.f) * (dgo / ties));
        });
      }
    } else {
      SUBSTAMP(18);
      for (int e0 = eb; e0 < ee; e0 += 4) {
        uniform_group<4>(ee - e0, [&](auto m_t) {
          constexpr int M = decltype(m_t)::value;
          int c[M], mo[M];
#pragma unroll
          for (int u = 0; u < M; ++u) c[u] = t.p1tc[e0 + u];
          float h[M], pm[M], tn[M];
#pragma unroll
          for (int u = 0; u < M; ++u) {
            mo[u] = t.cl1[c[u]] * 64 + o;
            h[u] = t.h2[c[u] * 64 + o];
          }
#pragma unroll
          for (int u = 0; u < M; ++u) {
            pm[u] = t.p2[mo[u]];
            tn[u] = t.nt[mo[u]];
          }
#pragma unroll
          for (int u = 0; u < M; ++u) acc += relu_bwd(h[u], (h[u] == pm[u] ? 1.f : 0.f) * (dgo / tn[u]));
        });
      }
    }
    SUBSTAMP(19);
    t.y2[p] = acc;
  }
  __syncthreads();
  STAMP(11);
  STAMP(12);
  // conv2 weight-gradient partials, and the gradient reaching each depth-0
  // arg member through relu (v = relu'(H1[arg]) * dP1); with many clusters on MFMA:
  // dW2 = dY2^T P1 per branch (4 tiles of 16 x 16, K = K0) and
  // dP1 = dY2 W2 per branch (ceil(K0/16) row tiles, K = 32); one wave per tile
  if (K0 < 12) {  // few clusters: direct loops
    float* slab = a.p.slab + (int64_t)pb * DR_SLAB_STRIDE(F) + 32 * F;
    for (int p = tid; p < 1024; p += NT) {
      const int br = p >> 9, o = ((p >> 4) & 31) + br * 32, j = p & 15;
      float acc = 0.f;
      int k = 0;
      for (; k + 4 <= K0; k += 4) {  // 8 independent reads, then the fmaf chain in k order
        float yv[4], pv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          yv[u] = t.y2[(k + u) * 64 + o];
          pv[u] = t.p1[(k + u) * 32 + br * 16 + j];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = fmaf(yv[u], pv[u], acc);
      }
      for (; k < K0; ++k) acc = fmaf(t.y2[k * 64 + o], t.p1[k * 32 + br * 16 + j], acc);
      if (ACC) t.acc[32 * F + p] += acc;
      else drk::st_part(slab + p, acc);
    }
    SUBSTAMP0(28);
    for (int p = tid; p < K0 * 32; p += NT) {
      const int k = p >> 5, ch = p & 31, br = ch >> 4, j = ch & 15;
      const float* wb = t.w2 + br * 512;
      float acc = 0.f;
      // the 32 + 32 operands in flight at once (dY2's half-row as eight
      // 16-byte reads), then the same chain
      float4 yv[8];
      float wv[32];
#pragma unroll
      for (int q = 0; q < 8; ++q) yv[q] = *reinterpret_cast<const float4*>(t.y2 + k * 64 + br * 32 + 4 * q);
#pragma unroll
      for (int o = 0; o < 32; ++o) wv[o] = wb[o * 16 + j];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        acc = fmaf(yv[q].x, wv[4 * q], acc);
        acc = fmaf(yv[q].y, wv[4 * q + 1], acc);
        acc = fmaf(yv[q].z, wv[4 * q + 2], acc);
        acc = fmaf(yv[q].w, wv[4 * q + 3], acc);
      }
      const int i = t.a1[p];
      t.dp1[p] = (i < N) ? relu_bwd(t.p1[p], acc) : 0.f;  // P1 = H1[arg] exactly
    }
  } else
  {
    const int lane = tid & 63, wave = dr_wave<ACC>(tid), li = lane & 15, kq = lane >> 4;
    float* slab = a.p.slab + (int64_t)pb * DR_SLAB_STRIDE(F) + 32 * F;
    const int nrt = (K0 + 15) >> 4;
    for (int job = wave; job < 4 + 2 * nrt; job += NW) {
      if (job < 4) {
        const int br = job >> 1, ot = job & 1;
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < K0; k0 += 4) {
          const int k = k0 + kq;
          const float av = k < K0 ? t.y2[k * 64 + br * 32 + ot * 16 + li] : 0.f;
          const float bv = k < K0 ? t.p1[k * 32 + br * 16 + li] : 0.f;
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
        }
        if (ACC) {  // the four sums read first, then written (no read-after-write chain)
          float o[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = t.acc[32 * F + br * 512 + (ot * 16 + kq * 4 + r) * 16 + li];
#pragma unroll
          for (int r = 0; r < 4; ++r) t.acc[32 * F + br * 512 + (ot * 16 + kq * 4 + r) * 16 + li] = o[r] + acc[r];
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) drk::st_part(slab + br * 512 + (ot * 16 + kq * 4 + r) * 16 + li, acc[r]);
        }
      } else {
        const int q = job - 4, br = q & 1, r0 = (q >> 1) * 16;
        const int kr = min(r0 + li, K0 - 1);
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int o = 4 * u + kq;
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(t.y2[kr * 64 + br * 32 + o], t.w2[br * 512 + o * 16 + li], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = r0 + kq * 4 + r;
          if (k < K0) {
            const int p = k * 32 + br * 16 + li;
            const int i = t.a1[p];
            t.dp1[p] = (i < N) ? relu_bwd(t.p1[p], acc[r]) : 0.f;  // P1 = H1[arg] exactly
          }
        }
      }
    }
  }
  __syncthreads();

  STAMP(13);
  // ---------------- dW1cat[c, :] = sum_k v[k, c] * Z[arg(k, c), :] ---------
  // (dH1 is non-zero only at the depth-0 arg members, so dS1^T (A X) needs
  // K0 rows of Z per channel instead of a backward gather over all edges.)
  {
    const int SS = DR_SLAB_STRIDE(F);
    float* slab = a.p.slab + (int64_t)pb * SS;
    // G clusters at a time, the last group predicated (clusters past K0 and
    // empty ones contribute nothing): every Z read of a group in flight (HBM on
    // the large path: with many clusters, groups of 16 halve the round trips),
    // then accumulated in cluster order (same fmaf chain)
    auto dw1 = [&](auto g_t) {
      constexpr int G = decltype(g_t)::value;
      for (int p = tid; p < 32 * F; p += NT) {
        const int ch = p / F, kk = p - ch * F;
        float acc = 0.f;
        for (int k = 0; k < K0; k += G) {
          float zv[G], dv[G];
          bool ok[G];
#pragma unroll
          for (int u = 0; u < G; ++u) {
            const bool in = k + u < K0;
            const int i = in ? t.a1[(k + u) * 32 + ch] : N;
            ok[u] = i < N;
            dv[u] = in ? t.dp1[(k + u) * 32 + ch] : 0.f;
            zv[u] = zat(ok[u] ? i : 0, kk);
          }
#pragma unroll
          for (int u = 0; u < G; ++u)
            if (ok[u]) acc = fmaf(dv[u], zv[u], acc);
        }
        if (ACC) t.acc[p] += acc;
        else drk::st_part(slab + p, acc);
      }
    };
    if (K0 > 8) dw1(std::integral_constant<int, 16>());  // (all of K0 <= 32 in flight at once: +0.6 us atom, not kept)
    else dw1(std::integral_constant<int, 8>());
  }
  STAMP(14);
}

// A graph descriptor by one s_load_dwordx16 (the pointer is wave-uniform);
// `touch` (optional): one dword of another descriptor loaded beside it and
// dropped, so that line is in the scalar cache when its graph starts
__device__ __forceinline__ uint64_t uniform_ptr(const void* p) {
  const uint64_t u = reinterpret_cast<uint64_t>(p);
  return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(u >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)u);
}
__device__ __forceinline__ dr_graph_desc desc_scalar(const dr_graph_desc* p, const dr_graph_desc* touch = nullptr) {
  typedef int v16i __attribute__((ext_vector_type(16)));
  v16i r;
  if (touch) {
    int dropped;
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dword %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=s"(r), "=s"(dropped)
                 : "s"(uniform_ptr(p)), "s"(uniform_ptr(touch)));
  } else {
    asm volatile("s_load_dwordx16 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(uniform_ptr(p)));
  }
  dr_graph_desc d;
  __builtin_memcpy(&d, &r, sizeof(d));
  return d;
}

// Accumulating pass (dr_ginet_acc_pass): a workgroup runs graphs gi, gi + R,
// ... one after another and adds each graph's gradients to running sums (LDS
// region acc at the front of its LDS, fc1.weight's in the caller's registers)
// instead of writing per-graph partials; the graph carve starts acc_words in.
struct AccCtx {
  int gi = -1;           // the graph (batch position) this call runs
  float* acc = nullptr;  // [dW1cat 32F | dW2cat 1024 | GinetHeadLds::acc's block]
  float* accf = nullptr;  // fc1.weight's sums in the kernel's registers (null: in acc)
  int acc_words = 0;
  // prefetch layout (graph_body<..., PF = true>): this graph's tail-input
  // buffer (parity), whether its inputs and W1 still need staging (the
  // workgroup's first graph), and the next graph's batch position (-1: none)
  AccLayout lay;
  int par = 0, next = -1;
  bool first = true;
  int64_t step = 0;  // dr_pass.step_counter[0] (constant for the launch)
  // PF: LDS word set to 1 by the graph whose idle waves staged the next
  // graph's inputs (read by that next graph before its staging)
  uint32_t* staged = nullptr;
  // graph_body<..., IG = true> (ginet_integrated_grad_kernel): the step's
  // point alpha of the path from the baseline, and the baseline's store-wide
  // Zb = A xb in the layout of a.z (null: a zero baseline)
  float ig_alpha = 1.f;
  const float* ig_zb = nullptr;
};

// KPT: conv1's K (F) padded to whole 16-deep MFMA steps, 32 (F <= 32) or 64.
// ACC / PF: the accumulating pass (AccCtx) and its prefetch layout.  Returns
// the step counter value the pass used (its dropout offset).
// ZIN: Z = A·X comes from the store-wide array of dr_aggregate_x (a.z, rows of
// a.z_stride words, the LDS row stride too): the graph's block is DMA'd into
// sZ in the place of x, the column ids and the row pointers, and the gather
// and the zeroing of Z's K padding are compiled out (the array holds the same
// bits the gather would write, zeros past F).  From the MFMA on, the same code.
// REC (with ZIN): the graph's record (dr_graph_records) is that Z block with
// every other input region behind it as the carve lists them: one copy in
// 16-byte lanes, spread over the sixteen waves, stages the whole graph.
// IG (with ZIN, 16-byte Z rows): the pass runs at the point ac.ig_alpha of the
// straight path from a baseline to x.  Z is linear in x, so each wave rescales
// the staged rows of its own tile in place before its MFMA reads them, to
// alpha * Z (zero baseline) or Zb + alpha * (Z - Zb); the tail then sees that Z.
template <int KPT, bool ACC = false, bool PF = false, bool ZIN = false, bool REC = false, bool IG = false>
__device__ __forceinline__ uint64_t graph_body(const GinetArgs& a, const AccCtx& ac) {
  static_assert(ZIN || !REC, "a record holds Z");
  static_assert(!IG || (ZIN && !REC && !ACC && !PF), "the path's points are formed on the per-graph Z-input form");
  extern __shared__ __attribute__((aligned(16))) float lds_raw[];
  float* lds = lds_raw + (ACC ? ac.acc_words : 0);
  // (ACC, IG: the body runs in a loop; an opaque tid keeps what derives from it out of registers held over the loop)
  const int tid = dr_tid<ACC || IG>();
  const int lane = tid & 63;
  const int wave = dr_wave<ACC || IG>(tid);
  const int b = ACC ? ac.gi : (int)blockIdx.x;
  const dr_graph_store& s = a.s;
  // one 64-byte scalar load (ACC: spelled out — in the accumulating kernel's
  // loop hipcc cannot prove the descriptors unwritten and reads them with
  // vector loads and readfirstlanes, ~1 K cycles)
  const dr_graph_desc d = ACC ? desc_scalar(a.descs + b, ac.next >= 0 ? a.descs + ac.next : nullptr) : a.descs[b];
  const int g = d.gid;
  const int64_t n0 = d.node0, ec0 = d.col0, k00 = d.k0, q0 = d.p1, k10 = d.k1;
  const int N = d.n_nodes, E = d.n_edges, K0 = d.n_k0, P1 = d.n_p1, K1 = d.n_k1;
  const int F = s.n_feat;
  const int alias = s.transpose_aliased;
  const int OUT = a.p.out_dim;
  // Fetch every kernel-argument field the staging needs, and the descriptor,
  // in one scalar round trip each (hipcc would otherwise load them lazily
  // with a wait before each DMA).
  if (REC)  // (n0: the record's first word)
    asm volatile("" ::"s"(a.rec), "s"(s.y), "s"(F), "s"(alias), "s"(OUT), "s"(n0), "s"(N), "s"(E), "s"(K0), "s"(P1), "s"(K1), "s"(g));
  else
    asm volatile("" ::"s"(s.x), "s"(s.col), "s"(s.rowptr), "s"(s.cl0), "s"(s.p1_rowptr), "s"(s.p1_col),
                 "s"(s.p1t_rowptr), "s"(s.p1t_col), "s"(s.m1_ptr), "s"(s.m1_idx), "s"(s.y), "s"(F), "s"(alias),
                 "s"(OUT), "s"(n0), "s"(ec0), "s"(k00), "s"(q0), "s"(k10), "s"(N), "s"(E), "s"(K0), "s"(P1), "s"(K1),
                 "s"(g));
  STAMP(23);  // (descriptor and kernel arguments in)
  const int zs = ZIN ? a.z_stride : 0;
  const Carve c = PF ? carve_acc(N, E, F, K0, P1, K1, alias, OUT, ac.lay, ac.par, zs) : carve(N, E, F, K0, P1, K1, alias, OUT, zs);
  const int LDW = c.LDW, XS = c.XS;

  float* sW1 = lds + c.w1;
  float* sW2 = lds + c.w2;
  float* sFc2 = lds + c.fc2;
  float* sX = lds + c.x;
  float* sZ = lds + c.z;
  int* srp = reinterpret_cast<int*>(lds + c.rp);
  uint16_t* scol = reinterpret_cast<uint16_t*>(lds + c.col);
  int* scl0 = reinterpret_cast<int*>(lds + c.cl0);
  unsigned long long* skey = reinterpret_cast<unsigned long long*>(lds + c.key);
  float* sP1 = lds + c.p1;
  int* sA1 = reinterpret_cast<int*>(lds + c.a1);
  int* sp1rp = reinterpret_cast<int*>(lds + c.p1rp);
  int* sp1c = reinterpret_cast<int*>(lds + c.p1c);
  int* sp1trp = reinterpret_cast<int*>(lds + c.p1trp);
  int* sp1tc = reinterpret_cast<int*>(lds + c.p1tc);
  int* sm1p = reinterpret_cast<int*>(lds + c.m1p);
  int* sm1i = reinterpret_cast<int*>(lds + c.m1i);
  uint8_t* skeep = reinterpret_cast<uint8_t*>(lds + c.keep);

  STAMP(0);
  // ---------------- stage the graph into LDS --------------------------------
  // Only the graph and conv1's weights are staged (DMA'd straight into LDS):
  // one CU pulls ~11-30 B/cycle, so the staging time is its bytes, and the
  // head's 64 KB of fc1 registers (row and column layouts, fc1_load) are loaded
  // after the staging barrier instead, under the LDS-bound front half.
  float fc1_row[8], fc1_col[8], fc1_bias;
  // conv1's B operands as a lane-ordered image in dgp (free until the head;
  // PF stages the weights once per workgroup and reuses dgp per graph: packed rows)
  constexpr bool IMG = KPT == 32 && !PF;
  float* sImg = lds + c.dgp;
  float wv2, wfc[3];
  auto load_head_weights = [&]() {
    wv2 = (tid < 512) ? a.w.w2[tid] : a.w.w2e[tid - 512];
    const int nf = OUT * 128;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int p = tid + u * NT;
      wfc[u] = 0.f;
      if (p < nf) wfc[u] = a.w.fc2w[p];
      else if (p < nf + OUT) wfc[u] = a.w.fc2b[p - nf];
    }
    // fc1 last: the wait for W2 / fc2 before their LDS stores (end of the
    // front half) then leaves these 11 loads in flight (vmcnt counts in order)
    fc1_load(a.w, tid, wave, fc1_row, fc1_col, fc1_bias);
  };
  // (ACC: scalar loads through the constant address space — read-only for the
  // launch; hipcc cannot prove that in the accumulating loop and would use a
  // vector load, waited for by the staging's vmcnt(0))
  typedef const __attribute__((address_space(4))) float* CF32;
  const float y_g = ACC ? *(CF32)(s.y + g) : s.y[g];
  uint64_t drop_offset = a.p.drop_offset;
  // the graph's inputs (PF: graph k+1's are DMA'd during graph k's tail)
  // (asm-issued: waited for by the s_waitcnt vmcnt(0) before the staging barrier)
  // (The three stagings below stay written out: driven from one list of the
  // inputs they cost ginet_multi_kernel 0.15 us per step,
  // profiles/dead_variants/staging_variants.txt.)
  auto stage_inputs = [&](const dr_graph_desc& dd, const Carve& cc) {
    const int64_t dn0 = dd.node0, dk00 = dd.k0;
    const int dg = dd.gid, dN = dd.n_nodes, dK0 = dd.n_k0;
    if (REC) {  // the whole record, as it lies in HBM (dd.node0: its first word)
      dma_copy<NT, 16, DMA_ASM>(lds + cc.z, a.rec + dn0, rec_words(cc, dK0) / 4, tid);
      return;
    }
    if (ZIN) {  // the graph's Z block as it lies in HBM (16-byte lanes where the stride gives 16-byte rows)
      if ((LDW & 3) == 0) dma_copy<NT, 16, DMA_ASM>(lds + cc.z, a.z + dn0 * (int64_t)LDW, dN * LDW / 4, tid);
      else dma_copy<NT, 4, DMA_ASM>(lds + cc.z, a.z + dn0 * (int64_t)LDW, dN * LDW, tid);
    } else {
      dma_copy<NT, 16, DMA_ASM>(lds + cc.x, s.x + dn0 * (int64_t)XS, dN * XS / 4, tid);
      dma_copy<NT, 16, DMA_ASM>(lds + cc.col, s.col + dd.col0, (dd.n_edges + 7) / 8, tid, 7);
      dma_copy<NT, 4, DMA_ASM>(lds + cc.rp, s.rowptr + dn0 + dg, dN + 1, tid, 13);
    }
    dma_copy<NT, 4, DMA_ASM>(lds + cc.cl0, s.cl0 + dn0, dN, tid, 3);
    dma_copy<NT, 4, DMA_ASM>(lds + cc.p1rp, s.p1_rowptr + dk00 + dg, dK0 + 1, tid, 10);
    dma_copy<NT, 4, DMA_ASM>(lds + cc.p1c, s.p1_col + dd.p1, dd.n_p1, tid, 11);
    if (!alias) {
      dma_copy<NT, 4, DMA_ASM>(lds + cc.p1trp, s.p1t_rowptr + dk00 + dg, dK0 + 1, tid, 12);
      dma_copy<NT, 4, DMA_ASM>(lds + cc.p1tc, s.p1t_col + dd.p1, dd.n_p1, tid, 9);
    }
    dma_copy<NT, 4, DMA_ASM>(lds + cc.m1p, s.m1_ptr + dd.k1 + dg, dd.n_k1 + 1, tid, 8);
    dma_copy<NT, 4, DMA_ASM>(lds + cc.m1i, s.m1_idx + dk00, dK0, tid, 1);
  };
  if (!PF && REC) {
    dma_copy<NT, 16>(sZ, a.rec + n0, rec_words(c, K0) / 4, tid);
  } else if (!PF) {  // (every copy from wave 0: starting waves spread over the copies measured slower)
    if (ZIN) {
      if ((LDW & 3) == 0) dma_copy<NT, 16>(sZ, a.z + n0 * (int64_t)LDW, N * LDW / 4, tid);
      else dma_copy<NT, 4>(sZ, a.z + n0 * (int64_t)LDW, N * LDW, tid);
    } else {
      dma_copy<NT, 16>(sX, s.x + n0 * (int64_t)XS, N * XS / 4, tid);
      dma_copy<NT, 16>(scol, s.col + ec0, (E + 7) / 8, tid);
      dma_copy<NT, 4>(srp, s.rowptr + n0 + g, N + 1, tid);
    }
    dma_copy<NT, 4>(scl0, s.cl0 + n0, N, tid);
    dma_copy<NT, 4>(sp1rp, s.p1_rowptr + k00 + g, K0 + 1, tid);
    dma_copy<NT, 4>(sp1c, s.p1_col + q0, P1, tid);
    if (!alias) {
      dma_copy<NT, 4>(sp1trp, s.p1t_rowptr + k00 + g, K0 + 1, tid);
      dma_copy<NT, 4>(sp1tc, s.p1t_col + q0, P1, tid);
    }
    dma_copy<NT, 4>(sm1p, s.m1_ptr + k10 + g, K1 + 1, tid);
    dma_copy<NT, 4>(sm1i, s.m1_idx + k00, K0, tid);
  } else if (ac.first || *ac.staged == 0u) {
    stage_inputs(d, c);
  }
  STAMP(24);  // (wave 0: the graph's last copy issued)
  if (!PF || ac.first) w1_stage<IMG>(sW1, sImg, a.w, F, tid);  // (last: ahead of the graph's copies it was 0.3 us slower)
  STAMP(25);  // (conv1's weights issued)
  // ZIN: the front half is too short to cover the head weights' latency (it
  // showed as a wait before W2's and fc2's LDS stores), so they are requested
  // here, beside the staging DMA, and arrive with it: 10.50 -> 10.25 us per
  // pass.  (Only W2 / fc2 here and fc1's 64 KB of registers after the barrier:
  // 10.6 us, profiles/r07.)
  if (ZIN) load_head_weights();
  {  // zero Z's K padding (cols XS..KPT; X's own pad is zero) and the pooling keys
    const int padz = KPT - XS;  // (rows are KP = KPT wide, carve; ZIN: the array's rows arrive whole)
    if (!ZIN)
      for (int p = tid; p < N * padz; p += NT) {
        const int i = p / padz;
        sZ[i * LDW + XS + (p - i * padz)] = 0.f;
      }
    for (int p = tid; p < K0 * 32; p += NT) skey[p] = 0ull;
    if (tid < 64) lds[c.p2 + tid] = 0.f;  // (TailLds::p2_zeroed)
    w1_zero_pad<IMG>(sImg, F, tid);
  }
  // loaded late: no early wait (ACC: read once per launch by the kernel)
  if (a.p.step_counter) drop_offset = ACC ? (uint64_t)ac.step : (uint64_t)a.p.step_counter[0];
  STAMP(26);  // (head weights requested, zeroing stores issued)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  STAMP(27);  // (wave 0's copies and loads landed)
  // snapshot for dr_reduce_update, stored only now so that no wait for the
  // counter load sits between the descriptor and the graph DMA
  if (a.p.step_counter && b == 0 && tid == 0) a.p.step_counter[1] = (int64_t)drop_offset;
  __syncthreads();

  STAMP(1);
  // The conv2 / head weights are not needed before the tail: load them into
  // VGPRs now and store them to LDS after the front half, so their latency
  // overlaps it.  (An LDS DMA here would make hipcc wait for it before every
  // LDS read.)
  if (!ZIN) load_head_weights();
  // ---------------- conv1 + depth-0 pooling, one 16-row tile per wave -------
  // Each wave runs its rows through the whole front half with no workgroup
  // barrier in between:
  //   Z = A X  (ginet.py:45,58 aggregated first: A (X W^T) = (A X) W^T), 8
  //     lanes per row, edges in CSR order (torch_scatter's scatter_add_ order),
  //     two rows per lane in flight;
  //   H = relu(Z [W1;W1e]^T) on v_mfma_f32_16x16x4_f32 (exact k-ordered fmaf
  //     chain), B operands in registers;
  //   depth-0 max pool (torch_scatter scatter_max, community_pooling.py:209):
  //     a 64-bit LDS atomic max of (H bits << 32 | ~node) per (cluster,
  //     channel): H >= +0 after relu so the bit order is the value order, and
  //     among equal values the smallest node wins — the first max of the
  //     reference's node-ordered strict '>' scan; NaN never enters; an empty
  //     (cluster, channel) keeps key 0 -> value 0, no arg.  H itself is never
  //     stored: the backward needs only P1 = H[arg] and Z[arg].
  {
    const int li = lane & 15, kq = lane >> 4;
    // gather lanes -> (row slot, 16-byte chunk): ds_read_b128 serves a wave in
    // four 16-lane groups ({0-3,12-15,20-27}, {4-11,16-19,28-31}, and the same
    // +32; MI355X_MICROARCH.md §LDS), so each group takes both halves of two
    // slots' rows: with 128-byte rows it then waits an extra cycle only when
    // those two rows share a bank half, not when either of two half-row pairs does
    const int q4 = (lane & 31) >> 2;
    const int slot = ((lane >> 5) << 2) + ((0x31130220u >> (4 * q4)) & 3);
    const int sub = (((0xCCu >> q4) & 1) << 2) | (lane & 3), nch = XS >> 2;
    // conv1 B operand of v_mfma_f32_16x16x4_f32: lane (li, kq) holds
    // W[li][k + 4u + kq] (wa: conv1 rows, wb: conv1_ext rows), zero past F
    constexpr int NKV = KPT / 4;
    float wa[NKV], wb[NKV];
    w1_operands<KPT, IMG>(sW1, sImg, F, lane, wa, wb);
    if (PF && !ZIN) {  // the waves with no tile stage the next graph's inputs into the other buffer
      const int busy = (N + 15) >> 4;
      if (ac.next >= 0 && busy < NW && wave >= busy) {
        const dr_graph_desc dn = desc_scalar(a.descs + ac.next);
        const Carve cn = carve_acc(dn.n_nodes, dn.n_edges, F, dn.n_k0, dn.n_p1, dn.n_k1, alias, OUT, ac.lay, ac.par ^ 1);
        const int nw = NW - busy;
        const int64_t dn0 = dn.node0, dk00 = dn.k0;
        const int dg = dn.gid, dN = dn.n_nodes, dK0 = dn.n_k0;
        dma_copy<NT, 16, DMA_ASM>(lds + cn.x, s.x + dn0 * (int64_t)XS, dN * XS / 4, tid, busy, nw);
        dma_copy<NT, 16, DMA_ASM>(lds + cn.col, s.col + dn.col0, (dn.n_edges + 7) / 8, tid, busy, nw);
        dma_copy<NT, 4, DMA_ASM>(lds + cn.rp, s.rowptr + dn0 + dg, dN + 1, tid, busy, nw);
        dma_copy<NT, 4, DMA_ASM>(lds + cn.cl0, s.cl0 + dn0, dN, tid, busy, nw);
        dma_copy<NT, 4, DMA_ASM>(lds + cn.p1rp, s.p1_rowptr + dk00 + dg, dK0 + 1, tid, busy, nw);
        dma_copy<NT, 4, DMA_ASM>(lds + cn.p1c, s.p1_col + dn.p1, dn.n_p1, tid, busy, nw);
        if (!alias) {
          dma_copy<NT, 4, DMA_ASM>(lds + cn.p1trp, s.p1t_rowptr + dk00 + dg, dK0 + 1, tid, busy, nw);
          dma_copy<NT, 4, DMA_ASM>(lds + cn.p1tc, s.p1t_col + dn.p1, dn.n_p1, tid, busy, nw);
        }
        dma_copy<NT, 4, DMA_ASM>(lds + cn.m1p, s.m1_ptr + dn.k1 + dg, dn.n_k1 + 1, tid, busy, nw);
        dma_copy<NT, 4, DMA_ASM>(lds + cn.m1i, s.m1_idx + dk00, dK0, tid, busy, nw);
      }
      if (tid == 0) *ac.staged = (ac.next >= 0 && busy < NW) ? 1u : 0u;
    }
    for (int tt = wave; tt * 16 < N; tt += NW) {
      const int r0 = tt * 16;
      if (!ZIN) {
      if (nch <= 8) {  // one row per lane (r0 + lane/4), chunks q and q ^ 4 (q = lane%4, or +4 on odd rows)
        const int i = r0 + (lane >> 2);
        const int ca = (lane & 3) | ((lane & 4)), cb = ca ^ 4;
        const int eb = i < N ? srp[i] : 0, ee = i < N ? srp[i + 1] : 0;
        float4 za, zb;
        drk::gather_row_two_chunks_imm(scol, eb, ee, reinterpret_cast<const char*>(sX + ca * 4), (cb - ca) * 16, XS * 4, za, zb);
        if (i < N) {
          // (rows LDW = KP + 2 words apart: 8-byte aligned, two 64-bit stores per chunk)
          if (ca < nch) {
            float2* zr = reinterpret_cast<float2*>(sZ + i * LDW + ca * 4);
            zr[0] = make_float2(za.x, za.y);
            zr[1] = make_float2(za.z, za.w);
          }
          if (cb < nch) {
            float2* zr = reinterpret_cast<float2*>(sZ + i * LDW + cb * 4);
            zr[0] = make_float2(zb.x, zb.y);
            zr[1] = make_float2(zb.z, zb.w);
          }
        }
      } else {  // rows r0+slot and r0+8+slot together: two independent edge chains per lane
        const int i0 = r0 + slot, i1 = r0 + 8 + slot;
        const int eb0 = i0 < N ? srp[i0] : 0, ee0 = i0 < N ? srp[i0 + 1] : 0;
        const int eb1 = i1 < N ? srp[i1] : 0, ee1 = i1 < N ? srp[i1 + 1] : 0;
        for (int ch = sub; ch < nch; ch += 8) {
          float4 z0, z1;
          drk::gather_two_row_chunks(scol, eb0, ee0, eb1, ee1, sX, XS, ch * 4, z0, z1);
          if (i0 < N) {
            float* zr = sZ + i0 * LDW + ch * 4;
            zr[0] = z0.x;
            zr[1] = z0.y;
            zr[2] = z0.z;
            zr[3] = z0.w;
          }
          if (i1 < N) {
            float* zr = sZ + i1 * LDW + ch * 4;
            zr[0] = z1.x;
            zr[1] = z1.y;
            zr[2] = z1.z;
            zr[3] = z1.w;
          }
        }
      }
      // this wave's Z rows are complete in LDS before its own MFMA reads them
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }  // (ZIN: Z was staged whole, before the barrier)
      if (IG) {
        // columns 0 .. KPT - 1 (all the MFMA and the tail read), one 16-byte chunk
        // per lane and round; Zb straight from the array (L2-resident, read once per step)
        constexpr int CH = KPT / 4;
        const float al = ac.ig_alpha;
        for (int p = lane; p < 16 * CH; p += 64) {
          const int row = r0 + p / CH, ch = p % CH;
          if (row < N) {
            float4* zp = reinterpret_cast<float4*>(sZ + row * LDW + ch * 4);
            float4 v = *zp;
            if (ac.ig_zb) {
              const float4 zb = *reinterpret_cast<const float4*>(ac.ig_zb + (n0 + row) * (int64_t)LDW + ch * 4);
              v.x = fmaf(al, v.x - zb.x, zb.x);
              v.y = fmaf(al, v.y - zb.y, zb.y);
              v.z = fmaf(al, v.z - zb.z, zb.z);
              v.w = fmaf(al, v.w - zb.w, zb.w);
            } else {
              v.x *= al;
              v.y *= al;
              v.z *= al;
              v.w *= al;
            }
            *zp = v;
          }
        }
      }
      if (tt == 0) STAMP(20);  // (wave 0's first tile: gather done)
      const int ar = min(r0 + li, N - 1);  // rows past N compute garbage that is never pooled
      floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KPT / 16; ++ks) {
        float av[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) av[u] = sZ[ar * LDW + ks * 16 + 4 * u + kq];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], wa[4 * ks + u], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], wb[4 * ks + u], acc1, 0, 0, 0);
        }
      }
      if (tt == 0) STAMP(21);  // (MFMA issued)
      // the four rows' clusters in one 16-byte read (rows past N: unused)
      const int4 kk4 = *reinterpret_cast<const int4*>(scl0 + r0 + kq * 4);
      const int kk[4] = {kk4.x, kk4.y, kk4.z, kk4.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + kq * 4 + r;
        if (row < N) {
          const int k = kk[r];
          const unsigned long long low = 0xffffffffull - (unsigned long long)(uint32_t)row;
          const float v0 = relu_keepnan(acc0[r]), v1 = relu_keepnan(acc1[r]);
          if (v0 == v0)
            __hip_atomic_fetch_max(skey + k * 32 + li, ((unsigned long long)__float_as_uint(v0) << 32) | low,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (v1 == v1)
            __hip_atomic_fetch_max(skey + k * 32 + 16 + li, ((unsigned long long)__float_as_uint(v1) << 32) | low,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
      if (tt == 0) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        STAMP(22);  // (pool atomics done)
      }
    }
  }
  // the head's dropout keep flags, by the last two waves (idle in the front
  // half up to N = 224): off the tail's critical path
  if (tid >= NT - 128) {
    const int r = tid - (NT - 128);
    if (a.p.use_dropout) skeep[r] = drk::keep_unit(a.p, drop_offset, a.p.slot ? a.p.slot[b] : b, r) ? 1 : 0;
  }
  sW2[tid] = wv2;
  {
    const int nf = OUT * 128 + OUT;
#pragma unroll
    for (int u = 0; u < 3; ++u)
      if (tid + u * NT < nf) sFc2[tid + u * NT] = wfc[u];
  }
  if (PF && ZIN) {
    // With no gather the front half is a few hundred cycles per wave and no
    // wave idles through it, so every wave issues its share of the next
    // graph's inputs, after its own tile and the weight stores above (whose
    // wait for their loads would otherwise take these copies in): the copies
    // land under this graph's tail.
    if (ac.next >= 0) {
      const dr_graph_desc dn = desc_scalar(a.descs + ac.next);
      stage_inputs(dn, carve_acc(dn.n_nodes, dn.n_edges, F, dn.n_k0, dn.n_p1, dn.n_k1, alias, OUT, ac.lay, ac.par ^ 1, zs));
    }
    if (tid == 0) *ac.staged = ac.next >= 0 ? 1u : 0u;
  }
  STAMP(2);
  __syncthreads();
  STAMP(3);
  for (int p = tid; p < K0 * 32; p += NT) {
    const unsigned long long key = skey[p];
    sP1[p] = key ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
    sA1[p] = key ? (int)(0xffffffffu - (uint32_t)key) : N;
  }
  __syncthreads();  // (conv2 reading the pooled rows from the keys, with no barrier here, measured 0.1 us slower)

  TailLds t = tail_lds(c, lds);
  t.p2_zeroed = true;
  t.keep = skeep;
  t.acc = ACC ? ac.acc : nullptr;
  t.accf = ACC ? ac.accf : nullptr;
  auto zat = [&](int i, int kk) { return sZ[i * LDW + kk]; };
  // (dr_pass.slot: the graph's rows of the batch when it is split over launches)
  const int orow = a.p.slot ? a.p.slot[b] : b;
  ginet_tail<decltype(zat), ACC>(a, t, fc1_row, fc1_col, fc1_bias, orow, N, K0, K1, F, OUT, y_g, drop_offset, zat, orow);
  return drop_offset;
}

template <int KPT, bool ZIN = false, bool REC = false>
__global__ void __launch_bounds__(NT) ginet_graph_kernel(GinetArgs a) {
#ifdef DR_STAMPS  // cross-kernel timeline (s_memrealtime, 100 MHz chip clock): slots 30 / 31 = entry / exit
  if (threadIdx.x == 0 && a.p.stamps) a.p.stamps[(int64_t)blockIdx.x * 32 + 30] = __builtin_amdgcn_s_memrealtime();
#endif
  graph_body<KPT, false, false, ZIN, REC>(a, AccCtx{});
#ifdef DR_STAMPS
  if (threadIdx.x == 0 && a.p.stamps) a.p.stamps[(int64_t)blockIdx.x * 32 + 31] = __builtin_amdgcn_s_memrealtime();
#endif
}

// ---------------------------------------------------------------------------
// Input gradients (dr_ginet_input_grad_pass): the training pass of
// ginet_graph_kernel, then dX = d(out . dout) / dx from the LDS state its
// backward leaves.  Conv1 is H = relu((A X) [W1; W1e]^T) and the depth-0 max
// pool routes each (cluster, channel)'s gradient to its one winning node, so
//   dZ[i, :] = sum over (k, ch) with a1[k, ch] = i of dp1[k, ch] * Wcat[ch, :F]
// has at most 32 K0 non-zero rows (a node belongs to one cluster: rows of
// different clusters never collide), and dX = A^T dZ is the front half's CSR
// gather over the store's transposed CSR (t_rowptr, t_col: stable, so each row
// sums its in-edges in the original edge order).
// The transposed CSR in LDS: the gather form reuses its rp / col regions (same
// sizes, dead after the front half); the Z-input form has none and appends
// them after the carve.
// ---------------------------------------------------------------------------
struct IgLds {
  int trp, tcol, total;
};
__host__ __device__ inline IgLds ig_lds(const Carve& c, int N, int E, int zs) {
  IgLds g;
  if (zs > 0) {
    g.trp = c.total;
    g.tcol = g.trp + r4(N + 1);
    g.total = g.tcol + r4((E + 1) / 2);
  } else {
    g.trp = c.rp;
    g.tcol = c.col;
    g.total = c.total;
  }
  return g;
}

template <int KPT, bool ZIN>
__global__ void __launch_bounds__(NT) ginet_input_grad_kernel(GinetArgs a, dr_input_grad ig) {
  extern __shared__ __attribute__((aligned(16))) float lds_raw[];
  graph_body<KPT, false, false, ZIN>(a, AccCtx{});
  __syncthreads();  // the tail's last step (dW1) has read Z; dp1 / a1 are complete
  float* lds = lds_raw;
  const int tid = threadIdx.x, b = blockIdx.x;
  const dr_graph_desc d = a.descs[b];
  const int N = d.n_nodes, E = d.n_edges, K0 = d.n_k0, F = a.s.n_feat;
  const int zs = ZIN ? a.z_stride : 0;
  const Carve c = carve(N, E, F, K0, d.n_p1, d.n_k1, a.s.transpose_aliased, a.p.out_dim, zs);
  const IgLds g = ig_lds(c, N, E, zs);
  // dZ in the Z region, rows of DS = r4(F) words (16-byte rows for the gather's
  // reads, DS <= LDW in both forms; columns F .. DS - 1 stay zero)
  float* dZ = lds + c.z;
  const int DS = c.XS;
  int* trp = reinterpret_cast<int*>(lds + g.trp);
  uint16_t* tcol = reinterpret_cast<uint16_t*>(lds + g.tcol);
  const float* dp1 = lds + c.dp1;
  const int* a1 = reinterpret_cast<const int*>(lds + c.a1);
  for (int p = tid; p < N * c.LDW; p += NT) dZ[p] = 0.f;
  dma_copy<NT, 4>(trp, a.s.t_rowptr + d.node0 + d.gid, N + 1, tid);
  dma_copy<NT, 16>(tcol, a.s.t_col + d.col0, (E + 7) / 8, tid, 7);
  const int64_t row0 = ig.row_off[b];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // one thread per (cluster k, feature f), channels in ascending order: no two
  // threads touch one word (k fixes the node's cluster, f the column), and the
  // order of the fmaf chain into a word is fixed
  for (int p = tid; p < K0 * F; p += NT) {
    const int k = p / F, f = p - k * F;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const float* wsrc = (hf ? a.w.w1e : a.w.w1) + f;
      float w[16], v[16];
      int i[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) w[u] = wsrc[u * F];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int4 iv = *reinterpret_cast<const int4*>(a1 + k * 32 + hf * 16 + 4 * q);
        const float4 vv = *reinterpret_cast<const float4*>(dp1 + k * 32 + hf * 16 + 4 * q);
        i[4 * q] = iv.x; i[4 * q + 1] = iv.y; i[4 * q + 2] = iv.z; i[4 * q + 3] = iv.w;
        v[4 * q] = vv.x; v[4 * q + 1] = vv.y; v[4 * q + 2] = vv.z; v[4 * q + 3] = vv.w;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (i[u] < N) dZ[i[u] * DS + f] = fmaf(v[u], w[u], dZ[i[u] * DS + f]);
    }
  }
  __syncthreads();
  // dX[m, :] = sum over transposed row m, in slot order from +0, of dZ[t_col[s], :]
  // (8 lanes per row, one 16-byte chunk each); zeros past r4(F)
  const int sub = tid & 7, nchd = DS >> 2, ncho = ig.dx_stride >> 2;
  for (int m = tid >> 3; m < N; m += NT / 8) {
    const int eb = trp[m], ee = trp[m + 1];
    float* row = ig.dx + (row0 + m) * (int64_t)ig.dx_stride;
    for (int ch = sub; ch < ncho; ch += 8) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ch < nchd) acc = drk::gather_row_chunk_lds(tcol, eb, ee, dZ, DS, ch * 4);
      *reinterpret_cast<float4*>(row + ch * 4) = acc;
    }
  }
}

// ---------------------------------------------------------------------------
// Integrated gradients (dr_ginet_integrated_grad_pass):
//   attr = (x - xb) . sum_s w_s g_s,  g_s = d(out . dout) / dx at xb + alpha_s (x - xb).
// Z = A x is linear in x, so step s is the Z-input pass on the graph's Z block
// rescaled to Zb + alpha_s (Z - Zb) (graph_body<..., IG>), followed by
// ginet_input_grad_kernel's dZ chain with dp1 weighted by w_s; dX = A^T dZ is
// linear too, so the steps' dZ are summed in LDS (dZacc) and the transposed
// gather runs once.  Workgroup (b, g) runs graph b over the steps
// [g S / G, (g + 1) S / G) in ascending order and writes its sum to its own
// rows of part[g]; ig_finish_kernel adds the groups' rows.  The training
// pass's slab / head / out writes go to group g's own scratch rows: no word is
// written by two workgroups.  LDS: the Z-form input-gradient layout (the
// transposed CSR behind the carve), then dZacc, N rows of r4(F) words.
// ---------------------------------------------------------------------------
struct IntGradLds {
  int trp, tcol, dz, total;
};
__host__ __device__ inline IntGradLds intgrad_lds(const Carve& c, int N, int E, int zs) {
  const IgLds g = ig_lds(c, N, E, zs);
  IntGradLds t;
  t.trp = g.trp;
  t.tcol = g.tcol;
  t.dz = g.total;
  t.total = t.dz + r4(N * c.XS);
  return t;
}

struct IntGradArgs {
  GinetArgs a;
  dr_integrated_grad ig;
};
// What the kernel's own phases need of a graph's LDS, re-derived from the
// descriptor around every pass instead of being held in registers over it
struct IntGradView {
  int N, E, K0, DS;
  float* dZ;
  int* trp;
  uint16_t* tcol;
  const float* dp1;
  const int* a1;
};
__device__ __forceinline__ IntGradView intgrad_view(const GinetArgs& a, const dr_graph_desc& d, float* lds) {
  const Carve c = carve(d.n_nodes, d.n_edges, a.s.n_feat, d.n_k0, d.n_p1, d.n_k1, a.s.transpose_aliased, a.p.out_dim, a.z_stride);
  const IntGradLds g = intgrad_lds(c, d.n_nodes, d.n_edges, a.z_stride);
  IntGradView v;
  v.N = d.n_nodes;
  v.E = d.n_edges;
  v.K0 = d.n_k0;
  v.DS = c.XS;
  v.dZ = lds + g.dz;
  v.trp = reinterpret_cast<int*>(lds + g.trp);
  v.tcol = reinterpret_cast<uint16_t*>(lds + g.tcol);
  v.dp1 = lds + c.dp1;
  v.a1 = reinterpret_cast<const int*>(lds + c.a1);
  return v;
}

template <int KPT>
__global__ void __launch_bounds__(NT) ginet_integrated_grad_kernel(IntGradArgs ia) {
  extern __shared__ __attribute__((aligned(16))) float lds_raw[];
  float* lds = lds_raw;
  // every phase reads the arguments from the kernarg segment through a pointer
  // the optimiser cannot follow (as ginet_acc_kernel's loop does): scalar
  // loads of what the phase uses, nothing held in SGPRs over the passes
  auto kargs = []() {
    typedef const __attribute__((address_space(4))) IntGradArgs* KArgs;
    KArgs ka = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("; dr_kargs" : "+s"(ka));
    return (const IntGradArgs*)ka;
  };
  const int b = blockIdx.x, grp = blockIdx.y;
  {
    const IntGradArgs* ka = kargs();
    const int tid = dr_tid<true>();
    const dr_graph_desc d = desc_scalar(ka->a.descs + b);
    const IntGradView v = intgrad_view(ka->a, d, lds);
    // behind the carve, so no pass touches them: zeroed / copied once (the first
    // pass's staging wait and barrier cover both)
    for (int p = tid; p < v.N * v.DS; p += NT) v.dZ[p] = 0.f;
    dma_copy<NT, 4>(v.trp, ka->a.s.t_rowptr + d.node0 + d.gid, v.N + 1, tid);
    dma_copy<NT, 16>(v.tcol, ka->a.s.t_col + d.col0, (v.E + 7) / 8, tid, 7);
  }
  const int s0 = (int)((int64_t)grp * ia.ig.n_steps / ia.ig.n_groups);
  const int s1 = (int)((int64_t)(grp + 1) * ia.ig.n_steps / ia.ig.n_groups);
  for (int s = s0; s < s1; ++s) {
    {
      const IntGradArgs* ka = kargs();
      GinetArgs a = ka->a;
      const int F = a.s.n_feat, OUT = a.p.out_dim;
      // this group's rows of the training pass's outputs
      a.p.slab = ka->ig.slab + (int64_t)grp * a.B * DR_SLAB_STRIDE(F);
      a.p.head = ka->ig.head + (int64_t)grp * a.B * DR_HEAD_STRIDE(OUT);
      a.p.out = ka->ig.out + (int64_t)grp * a.B * OUT;
      AccCtx ac;
      typedef const __attribute__((address_space(4))) float* CF32;
      ac.ig_alpha = *(CF32)(ka->ig.alpha + s);
      ac.ig_zb = ka->ig.zb;
      graph_body<KPT, false, false, true, false, true>(a, ac);
    }
    __syncthreads();  // the tail's last step (dW1) has read Z; dp1 / a1 are complete
    {
      // ginet_input_grad_kernel's chain, dp1 weighted by w_s, into the running
      // dZacc: one thread per (cluster, feature), channels ascending.  (Written
      // out here and in that kernel: called from one helper, with the gather,
      // that kernel's VGPR and SGPR-spill figures moved: 91 -> 89, 42 -> 43.)
      const IntGradArgs* ka = kargs();
      const int tid = dr_tid<true>();
      const IntGradView v = intgrad_view(ka->a, desc_scalar(ka->a.descs + b), lds);
      const int F = ka->a.s.n_feat, N = v.N, DS = v.DS;
      typedef const __attribute__((address_space(4))) float* CF32;
      const float ws = *(CF32)(ka->ig.weight + s);
      for (int p = tid; p < v.K0 * F; p += NT) {
        const int k = p / F, f = p - k * F;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const float* wsrc = (hf ? ka->a.w.w1e : ka->a.w.w1) + f;
          float w[16], dv[16];
          int i[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) w[u] = wsrc[u * F];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int4 iv = *reinterpret_cast<const int4*>(v.a1 + k * 32 + hf * 16 + 4 * q);
            const float4 vv = *reinterpret_cast<const float4*>(v.dp1 + k * 32 + hf * 16 + 4 * q);
            i[4 * q] = iv.x; i[4 * q + 1] = iv.y; i[4 * q + 2] = iv.z; i[4 * q + 3] = iv.w;
            dv[4 * q] = ws * vv.x; dv[4 * q + 1] = ws * vv.y; dv[4 * q + 2] = ws * vv.z; dv[4 * q + 3] = ws * vv.w;
          }
#pragma unroll
          for (int u = 0; u < 16; ++u)
            if (i[u] < N) v.dZ[i[u] * DS + f] = fmaf(dv[u], w[u], v.dZ[i[u] * DS + f]);
        }
      }
    }
    __syncthreads();  // the chain has read dp1 / a1 before the next step's staging and zeroing
  }
  // part[g][m, :] = sum over transposed row m, in slot order from +0, of dZacc[t_col[s], :]
  const IntGradArgs* ka = kargs();
  const int tid = dr_tid<true>();
  const IntGradView v = intgrad_view(ka->a, desc_scalar(ka->a.descs + b), lds);
  const int DXS = ka->ig.dx_stride;
  const int sub = tid & 7, nchd = v.DS >> 2, ncho = DXS >> 2;
  typedef const __attribute__((address_space(4))) int64_t* CI64;
  float* prow0 = ka->ig.part + ((int64_t)grp * ka->ig.part_rows + *(CI64)(ka->ig.part_off + b)) * (int64_t)DXS;
  for (int m = tid >> 3; m < v.N; m += NT / 8) {
    const int eb = v.trp[m], ee = v.trp[m + 1];
    float* row = prow0 + m * (int64_t)DXS;
    for (int ch = sub; ch < ncho; ch += 8) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ch < nchd) acc = drk::gather_row_chunk_lds(v.tcol, eb, ee, v.dZ, v.DS, ch * 4);
      *reinterpret_cast<float4*>(row + ch * 4) = acc;
    }
  }
}

// attr = (x - xb) . (part[0] + part[1] + ... + part[G - 1]), the groups summed
// ascending from +0, zeros in columns F .. dx_stride - 1, and attr_sum[b] =
// the graph's sum of attr in fp64: each thread sums its elements in ascending
// order, then a fixed tree over the 256 threads (no atomics: equal bits on
// every call).  One workgroup per graph.
constexpr int NTF = 256;
__global__ void __launch_bounds__(NTF) ig_finish_kernel(dr_graph_store s, const dr_graph_desc* descs, dr_integrated_grad ig) {
  __shared__ double red[NTF];
  const int tid = threadIdx.x, b = blockIdx.x;
  const dr_graph_desc d = descs[b];
  const int N = d.n_nodes, F = s.n_feat, DXS = ig.dx_stride;
  const int64_t arow0 = ig.row_off[b], prow0 = ig.part_off[b], gstride = ig.part_rows * (int64_t)DXS;
  double acc = 0.0;
  for (int p = tid; p < N * DXS; p += NTF) {
    const int m = p / DXS, f = p - m * DXS;
    float v = 0.f;
    if (f < F) {
      const float* pp = ig.part + (prow0 + m) * (int64_t)DXS + f;
      float sum = 0.f;
      for (int g = 0; g < ig.n_groups; ++g) sum += pp[g * gstride];
      float dxv = s.x[(d.node0 + m) * (int64_t)s.x_stride + f];
      if (ig.xb) dxv -= ig.xb[(d.node0 + m) * (int64_t)s.x_stride + f];
      v = dxv * sum;
      acc += (double)v;
    }
    ig.attr[(arow0 + m) * (int64_t)DXS + f] = v;
  }
  red[tid] = acc;
  __syncthreads();
  for (int h = NTF / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) ig.attr_sum[b] = red[0];
}

// ---------------------------------------------------------------------------
// Several members in one launch (dr_ginet_multi_pass): a batch of 64 graphs
// occupies 64 of the 256 CUs for the length of one graph's chain of phases, so
// up to DR_MAX_MEMBERS independent models (an ensemble, the folds of a
// cross-validation, a sweep) run side by side on a grid (max B_k, K).  Row
// blockIdx.y is member y: its weights, its whole dr_pass and its batch; the
// store and Z are shared.  The body is graph_body as ginet_graph_kernel calls
// it (the graph from blockIdx.x, everything else from GinetArgs), so a member
// computes what its own launch computes.
// ---------------------------------------------------------------------------
struct MultiMemberArgs {
  dr_ginet_weights w;
  dr_pass p;
  const dr_graph_desc* descs;
  int32_t B, pad;
};
struct MultiArgs {
  dr_graph_store s;
  const float* z;
  int32_t z_stride, n_members;
  MultiMemberArgs m[DR_MAX_MEMBERS];
};
// the kernel-argument segment: 4 KB, of which the runtime's hidden arguments take up to 256 bytes
static_assert(sizeof(MultiArgs) <= 4096 - 256, "DR_MAX_MEMBERS members by value must fit the kernel arguments");

template <int KPT, bool ZIN>
__global__ void __launch_bounds__(NT) ginet_multi_kernel(MultiArgs ma) {
  // the member's record is read with scalar loads through a kernarg pointer
  // the optimiser cannot follow (as ginet_acc_kernel's): indexing the by-value
  // array with blockIdx.y would put it in scratch or in spilled SGPRs
  typedef const __attribute__((address_space(4))) MultiArgs* KArgs;
  KArgs kp = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("; dr_kargs" : "+s"(kp));
  const MultiArgs* ka = (const MultiArgs*)kp;
  const int k = blockIdx.y;
  if ((int)blockIdx.x >= ka->m[k].B) return;  // past this member's batch (before the first barrier)
  GinetArgs a;
  a.s = ka->s;
  a.w = ka->m[k].w;
  a.p = ka->m[k].p;
  a.descs = ka->m[k].descs;
  a.B = ka->m[k].B;
  a.z = ka->z;
  a.z_stride = ka->z_stride;
  graph_body<KPT, false, false, ZIN>(a, AccCtx{});
}

// ---------------------------------------------------------------------------
// Accumulating pass (dr_ginet_acc_pass; batches past the CU count): R
// workgroups, workgroup w runs graphs w, w + R, w + 2R, ... in that order and
// sums their gradients on chip — the conv weights' and the head's in an LDS
// region ahead of the graph carve, fc1.weight's (dh (x) g, 128 x 64) in
// registers — then writes ONE row [dW1cat | dW2cat | fc1.weight | fc1.bias |
// fc2.weight | fc2.bias] (dr_ginet_acc_row_floats) and its loss sum to
// loss_per_graph[w].  The reduce then sums R rows instead of B per-graph
// partials (and no outer products): the per-graph slab, B x (32F + 1024 +
// 320) floats written and read back per step, becomes R x ~10 K.  The graph
// -> workgroup map and each workgroup's order are fixed, so the sums are
// deterministic (another fp32 association than the per-graph partials: the
// tests compare the two at fp32 tolerance).
// ---------------------------------------------------------------------------
// The accumulators (LDS, ahead of the graph carve): [dW1cat 32F | dW2cat 1024
// | fc1.bias 128 | fc2.weight OUT x 128 | fc2.bias OUT | loss | pad | fc1.weight
// 128 x 64 unless it is summed in registers (F <= 32)].  The row written per
// workgroup: [dW1cat | dW2cat | fc1.weight | fc1.bias | fc2.weight | fc2.bias].
__host__ __device__ inline int acc_row_floats(int F, int OUT) { return r4(32 * F + 1024 + 128 * 64 + 128 + 128 * OUT + OUT); }
__host__ __device__ inline int acc_head_words(int OUT) { return r4(128 + 128 * OUT + OUT + 1); }
__host__ __device__ inline int acc_words(int F, int OUT, bool fc1_in_lds) {
  return 32 * F + 1024 + acc_head_words(OUT) + (fc1_in_lds ? 128 * 64 : 0);
}

template <int KPT, bool PF, bool ZIN = false, bool REC = false>
__global__ void __launch_bounds__(NT) ginet_acc_kernel(GinetArgs a, const int32_t* plan, AccLayout lay) {
  extern __shared__ __attribute__((aligned(16))) float lds_raw[];
  const int F = a.s.n_feat, OUT = a.p.out_dim, tid = threadIdx.x;
  constexpr bool REG = KPT == 32;  // fc1.weight's sums in registers where the kernel has them to spare
  AccCtx ac;
  ac.acc = lds_raw;
  ac.acc_words = acc_words(F, OUT, !REG) + 4;  // + the staged flag (16 bytes)
  ac.staged = reinterpret_cast<uint32_t*>(lds_raw + ac.acc_words - 4);
  ac.lay = lay;
  typedef const __attribute__((address_space(4))) int64_t* CI64K;
  ac.step = a.p.step_counter ? *(CI64K)a.p.step_counter : 0;
  float accf[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  ac.accf = REG ? accf : nullptr;
  for (int p = tid; p < ac.acc_words; p += NT) lds_raw[p] = 0.f;
  __syncthreads();
  // plan: [R + 1 starts | the batch positions, workgroup by workgroup], or
  // null: every R-th position from blockIdx.x
  const int R = gridDim.x, w = blockIdx.x;
  typedef const __attribute__((address_space(4))) int32_t* CPlan;  // scalar loads (read-only for the launch)
  const CPlan cp = (CPlan)plan;
  const int k0 = plan ? cp[w] : 0, k1 = plan ? cp[w + 1] : (a.B - w + R - 1) / R;
  for (int k = k0; k < k1; ++k) {
    ac.gi = plan ? cp[R + 1 + k] : w + k * R;
    ac.first = k == k0;
    ac.par = (k - k0) & 1;
    ac.next = k + 1 < k1 ? (plan ? cp[R + 2 + k] : w + (k + 1) * R) : -1;
    // the body reads the arguments from the kernarg segment through a pointer
    // the optimiser cannot follow across iterations: each graph reloads what it
    // uses (scalar loads) instead of every argument being held in SGPRs over the
    // whole loop (spilled to VGPR lanes: ~650 readlane/writelane)
    typedef const __attribute__((address_space(4))) GinetArgs* KArgs;
    KArgs ka = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("; dr_kargs" : "+s"(ka));
    graph_body<KPT, true, PF, ZIN, REC>(*(const GinetArgs*)ka, ac);
    __syncthreads();  // the graph carve is restaged by the next graph
  }
  // the workgroup's row, then its loss sum
  const int c0 = 32 * F + 1024, HW = 128 + 128 * OUT + OUT;
  float* row = a.p.slab + (int64_t)blockIdx.x * acc_row_floats(F, OUT);
  for (int p = tid; p < c0 / 4; p += NT) reinterpret_cast<float4*>(row)[p] = reinterpret_cast<const float4*>(lds_raw)[p];
  float4* rw = reinterpret_cast<float4*>(row + c0 + tid * 8);
  if (REG) {
    rw[0] = make_float4(accf[0], accf[1], accf[2], accf[3]);
    rw[1] = make_float4(accf[4], accf[5], accf[6], accf[7]);
  } else {
    const float4* src = reinterpret_cast<const float4*>(lds_raw + c0 + acc_head_words(OUT) + tid * 8);
    rw[0] = src[0];
    rw[1] = src[1];
  }
  for (int p = tid; p < HW; p += NT) row[c0 + 128 * 64 + p] = lds_raw[c0 + p];
  if (tid == 0) a.p.loss_per_graph[blockIdx.x] = lds_raw[c0 + HW];
}

// =========================================================================
// Graphs larger than one workgroup's LDS (atom-level: N ~ 3e3, E ~ 5e4).
// =========================================================================

struct LargeArgs {
  GinetArgs g;
  dr_large_plan plan;
};

struct ConvCarve {
  int KP, LDW, XS, w1, z, h, m0i, m0p, rng, flg, xh, hid, lcol, trp, total;
};

// HM / EM: halo rows and edges of the largest tile (0: no halo staging)
__host__ __device__ inline ConvCarve conv_carve(int N, int F, int K0, int HM, int EM) {
  ConvCarve c;
  c.KP = r16(F);
  c.LDW = c.KP + 2;
  c.XS = r4(F);
  int o = 0;
  c.w1 = o;
  o += r4(32 * c.LDW);
  c.z = o;
  o += r4(TR * c.LDW);
  // with halos (HM > 0): H lives in the halo-X region (dead after the
  // gather) and the tile's own member lists replace the graph's
  c.h = o;
  o += HM ? 0 : TR * 32;
  c.m0i = o;
  o += r4(HM ? TR : N);
  c.m0p = o;
  o += r4(K0 + 1);
  c.rng = o;
  o += r4(2 * K0);
  c.flg = o;  // per tile row: a depth-0 pooling arg candidate (its Z row is stored)
  o += r4(TR);
  c.xh = o;  // halo X rows (XS stride, 16-byte rows), then H
  o += HM ? r4(drk::imax(HM * c.XS, TR * 32)) : 0;
  if (HM) c.h = c.xh;
  c.hid = o;
  o += r4(HM);
  c.trp = o;  // the tile's rowptr slice
  o += HM ? r4(TR + 1) : 0;
  c.lcol = o;  // the tile's edges as halo indices (uint16); last, so its size moves nothing
  o += HM ? r4((EM + 8) / 2) : 0;
  c.total = o;
  return c;
}

// The tile's partial depth-0 max per (cluster, channel) of H (LDS, stride 32,
// rows r0..r0+nrows-1), see tile_run_max.  Published by 64-bit atomic max keys
// or, without plan->part_key, as per-tile partials the tail combines in tile
// order.  Ends with the row flags visible to the workgroup.
__device__ __forceinline__ void tile_partial_max(const dr_large_plan& pl, const TileCtx& x, const float* sH,
                                                 const int* sm0i, const int* sm0p, int* srng, bool compact, int* sflag) {
  const int tid = threadIdx.x;
  // each cluster's members inside this tile: a sub-run of its ascending list
  for (int k = tid; k < x.K0; k += NTA) {
    const int mb = sm0p[k], me = sm0p[k + 1];
    srng[2 * k] = compact ? mb : lower_bound_lds(sm0i, mb, me, x.r0);
    srng[2 * k + 1] = compact ? me : lower_bound_lds(sm0i, mb, me, x.r0 + x.nrows);
  }
  __syncthreads();
  for (int p = tid; p < x.K0 * 32; p += NTA) {
    const int k = p >> 5, ch = p & 31;
    const RunMax m = tile_run_max<32>(pl, x, sH, sm0i, srng[2 * k], srng[2 * k + 1], k, ch, sflag);
    if (!pl.part_key) {
      const int64_t o = ((int64_t)x.tile * pl.k0_max + k) * 32 + ch;
      pl.part_val[o] = m.best;
      pl.part_arg[o] = m.arg;
    }
  }
  __syncthreads();
}

// One tile of TR nodes: Z rows (CSR gather over HBM/L2), H = relu(Z W^T) on
// MFMA, and the tile's partial depth-0 max per (cluster, channel).
// IG (dr_ginet_large_integrated_grad_pass): every gathered chunk is rescaled to
// Zb + alpha (Z - Zb) before it is stored to sZ, with graph_body<..., IG>'s
// expressions (zb: the store-wide A xb, rows of zb_stride words, or NULL: alpha Z),
// over columns 0 .. r4(F) - 1: all the MFMA and the tail read but zeros.
template <bool IG = false>
__device__ __forceinline__ void conv_tile_f32(const LargeArgs& la, float* lds, float ig_alpha = 0.f,
                                              const float* ig_zb = nullptr, int ig_zb_stride = 0) {
  const GinetArgs& a = la.g;
  const dr_large_plan& pl = la.plan;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const TileCtx x = tile_ctx(a.descs, pl);
  const dr_graph_store& s = a.s;
  const int64_t n0 = x.d.node0;
  const int F = s.n_feat, TRr = pl.tile_rows, r0 = x.r0, nrows = x.nrows;
  const ConvCarve c = conv_carve(x.N, F, x.K0, pl.halo_max, 0);
  const int KP = c.KP, LDW = c.LDW, XS = c.XS;
  float* sW1 = lds + c.w1;
  float* sZ = lds + c.z;
  float* sH = lds + c.h;
  int* sm0i = reinterpret_cast<int*>(lds + c.m0i);
  int* sm0p = reinterpret_cast<int*>(lds + c.m0p);
  int* srng = reinterpret_cast<int*>(lds + c.rng);
  int* sflag = reinterpret_cast<int*>(lds + c.flg);
  const float* X = s.x + n0 * (int64_t)XS;

  const bool compact = stage_pool_lists(s, pl, x, sm0i, sm0p, sflag);
  for (int p = tid; p < 32 * KP; p += NTA) {  // [W1; W1e] zero-padded to KP
    const int r = p / KP, k = p - r * KP;
    float v = 0.f;
    if (k < F) v = (r < 16) ? a.w.w1[r * F + k] : a.w.w1e[(r - 16) * F + k];
    sW1[r * LDW + k] = v;
  }
  for (int p = tid; p < TRr * (KP - XS); p += NTA) {  // Z pad columns
    const int r = p / (KP - XS);
    sZ[r * LDW + XS + (p - r * (KP - XS))] = 0.f;
  }
  // Z = A X for the tile's rows: 8 lanes per row, 16-byte chunks of X rows
  // summed in CSR order
  auto gather_rows = [&](const uint16_t* col, const float* Xs, const int* rowp, int ebase) {
    const int nch = XS >> 2, sub = tid & 7;
    for (int r = tid >> 3; r < nrows; r += NTA / 8) {
      const int eb = rowp[r] - ebase, ee = rowp[r + 1] - ebase;
      for (int ch = sub; ch < nch; ch += 8) {
        const int c4 = ch * 4;
        float4 acc = gather_row_chunk(col, eb, ee, Xs, XS, c4);  // (the _imm form measured +0.4 us on the halo path)
        if (IG) {
          if (ig_zb) {
            const float4 zb = *reinterpret_cast<const float4*>(ig_zb + (n0 + r0 + r) * (int64_t)ig_zb_stride + c4);
            acc.x = fmaf(ig_alpha, acc.x - zb.x, zb.x);
            acc.y = fmaf(ig_alpha, acc.y - zb.y, zb.y);
            acc.z = fmaf(ig_alpha, acc.z - zb.z, zb.z);
            acc.w = fmaf(ig_alpha, acc.w - zb.w, zb.w);
          } else {
            acc.x *= ig_alpha;
            acc.y *= ig_alpha;
            acc.z *= ig_alpha;
            acc.w *= ig_alpha;
          }
        }
        float* zr = sZ + r * LDW + c4;
        zr[0] = acc.x;
        zr[1] = acc.y;
        zr[2] = acc.z;
        zr[3] = acc.w;
      }
    }
  };
  if (pl.halo_ids) {  // halo path: the tile's rowptr slice, neighbour X rows and edges (as halo indices) in LDS
    int* strp = reinterpret_cast<int*>(lds + c.trp);
    int* shid = reinterpret_cast<int*>(lds + c.hid);
    uint16_t* slcol = reinterpret_cast<uint16_t*>(lds + c.lcol);
    float* sXh = lds + c.xh;
    const TileHalo hl = stage_halo_index(s, pl, x, strp, shid);
    stage_halo_rows(pl, x, hl, shid, slcol, X, XS, sXh, [] {}, lane, wave);  // (lane, wave passed: see stage_halo_rows)
    gather_rows(slcol, sXh, strp, hl.ebase);
  } else {  // per-edge gather of X rows from HBM / L2
    gather_rows(s.col + x.d.col0, X, s.rowptr + n0 + x.d.gid + r0, 0);
  }
  __syncthreads();
  // H = relu(Z [W1; W1e]^T), one 16-row MFMA tile per wave
  {
    const int li = lane & 15, kq = lane >> 4;
    for (int tt = wave; tt * 16 < nrows; tt += NTA / 64) {
      const int q0 = tt * 16;
      const int ar = min(q0 + li, nrows - 1);
      floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < KP; k += 16) {
        float av[4], b0[4], b1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int kk = k + 4 * u + kq;
          av[u] = sZ[ar * LDW + kk];
          b0[u] = sW1[li * LDW + kk];
          b1[u] = sW1[(16 + li) * LDW + kk];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], b0[u], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], b1[u], acc1, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = q0 + kq * 4 + r;
        if (row < nrows) {
          sH[row * 32 + li] = relu_keepnan(acc0[r]);
          sH[row * 32 + 16 + li] = relu_keepnan(acc1[r]);
        }
      }
    }
  }
  tile_partial_max(pl, x, sH, sm0i, sm0p, srng, compact, sflag);
  float* zg = pl.z + (int64_t)pl.z_row0[x.b] * XS;
  const int nch = XS >> 2;
  for (int p = tid; p < nrows * nch; p += NTA) {
    const int r = p / nch, c4 = (p - r * nch) * 4;
    if (sflag[r]) {
      const float2* zr = reinterpret_cast<const float2*>(sZ + r * LDW + c4);  // (rows 8-byte aligned)
      const float2 lo = zr[0], hi = zr[1];
      *reinterpret_cast<float4*>(zg + (int64_t)(r0 + r) * XS + c4) = make_float4(lo.x, lo.y, hi.x, hi.y);
    }
  }
}

__global__ void __launch_bounds__(NTA) ginet_large_conv1_kernel(LargeArgs la) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  conv_tile_f32(la, lds);
}

// ---- bf16 compute (dr_pass.compute_dtype == DR_DTYPE_BF16, BASELINE configs[3]) ----
// Same tile as ginet_large_conv1_kernel with the node GEMM on bf16 operands:
// X rows come from the store's bf16 copy (half the bytes of the halo staging
// and of the gather's LDS reads), Z = A X is accumulated in fp32 and rounded
// to bf16 (its LDS operand copy and the HBM workspace the tail reads for
// dW1), W1 is rounded to bf16, and H = relu(Z W1^T) comes from
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation (one MFMA per 16x16 output
// tile and 32 of K).  H, the pooling and everything after it stay fp32.

typedef short bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
__device__ __forceinline__ uint16_t f2bf(float f) {  // round to nearest even (torch's .to(bfloat16))
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);  // quiet NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__device__ __forceinline__ uint2 pack4bf(float a, float b, float c, float d) {
  return make_uint2((uint32_t)f2bf(a) | ((uint32_t)f2bf(b) << 16), (uint32_t)f2bf(c) | ((uint32_t)f2bf(d) << 16));
}
__device__ __forceinline__ float4 unpack4bf(uint2 v) {
  return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
                     __uint_as_float(v.y & 0xffff0000u));
}

struct ConvCarveB {  // offsets in 4-byte words; bf16 row strides in bf16 elements
  int KPB, ZSB, XSB, w1, z, h, m0i, m0p, rng, flg, xh, hid, lcol, trp, total;
};

__host__ __device__ inline ConvCarveB conv_carve_bf16(int N, int F, int K0, int HM, int EM) {
  ConvCarveB c;
  c.KPB = (F + 31) & ~31;  // K padded to whole 32-deep MFMA steps (zeros)
  c.ZSB = c.KPB + 8;       // 16-byte row shift: the 16 rows of an operand read start on distinct bank quads
  c.XSB = (F + 7) & ~7;    // the store's x_bf16_stride (16-byte rows)
  int o = 0;
  c.w1 = o;
  o += r4(32 * c.ZSB / 2);
  c.z = o;
  o += r4(TR * c.ZSB / 2);
  c.h = o;
  o += TR * 32;  // fp32 H
  c.m0i = o;
  o += r4(HM ? TR : N);
  c.m0p = o;
  o += r4(K0 + 1);
  c.rng = o;
  o += r4(2 * K0);
  c.flg = o;  // per tile row: a depth-0 pooling arg candidate (as conv_carve)
  o += r4(TR);
  c.xh = o;  // halo X rows, bf16, XSB stride
  o += HM ? r4(HM * c.XSB / 2) : 0;
  c.hid = o;
  o += r4(HM);
  c.trp = o;
  o += HM ? r4(TR + 1) : 0;
  c.lcol = o;
  o += HM ? r4((EM + 8) / 2) : 0;
  c.total = o;
  return c;
}

__device__ __forceinline__ void conv_tile_bf16(const LargeArgs& la, float* lds) {
  const GinetArgs& a = la.g;
  const dr_large_plan& pl = la.plan;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const TileCtx x = tile_ctx(a.descs, pl);
  const dr_graph_store& s = a.s;
  const int64_t n0 = x.d.node0;
  const int F = s.n_feat, TRr = pl.tile_rows, r0 = x.r0, nrows = x.nrows;
  const ConvCarveB c = conv_carve_bf16(x.N, F, x.K0, pl.halo_max, 0);
  const int KPB = c.KPB, ZSB = c.ZSB, XSB = s.x_bf16_stride;
  uint16_t* sW = reinterpret_cast<uint16_t*>(lds + c.w1);
  uint16_t* sZ = reinterpret_cast<uint16_t*>(lds + c.z);
  float* sH = lds + c.h;
  int* sm0i = reinterpret_cast<int*>(lds + c.m0i);
  int* sm0p = reinterpret_cast<int*>(lds + c.m0p);
  int* srng = reinterpret_cast<int*>(lds + c.rng);
  int* sflag = reinterpret_cast<int*>(lds + c.flg);
  const uint16_t* X = s.x_bf16 + n0 * (int64_t)XSB;
  uint16_t* zg = reinterpret_cast<uint16_t*>(pl.z) + (int64_t)pl.z_row0[x.b] * XSB;

  const bool compact = stage_pool_lists(s, pl, x, sm0i, sm0p, sflag);
  for (int p = tid; p < 32 * KPB; p += NTA) {  // [W1; W1e] in bf16, K zero-padded to KPB
    const int r = p / KPB, k = p - r * KPB;
    float v = 0.f;
    if (k < F) v = (r < 16) ? a.w.w1[r * F + k] : a.w.w1e[(r - 16) * F + k];
    sW[r * ZSB + k] = f2bf(v);
  }
  for (int p = tid; p < TRr * (KPB - XSB); p += NTA) {  // Z pad columns (X's own pad is zero)
    const int r = p / (KPB - XSB);
    sZ[r * ZSB + XSB + (p - r * (KPB - XSB))] = 0;
  }
  // Z = A X for the tile's rows: 8 lanes per row, 4 bf16 (8 bytes) per lane
  // and edge, summed in fp32 in CSR order; rounded to bf16 once per row.
  const int nch = XSB >> 2, sub = tid & 7;
  if (pl.halo_ids) {
    int* strp = reinterpret_cast<int*>(lds + c.trp);
    int* shid = reinterpret_cast<int*>(lds + c.hid);
    uint16_t* slcol = reinterpret_cast<uint16_t*>(lds + c.lcol);
    uint16_t* sXh = reinterpret_cast<uint16_t*>(lds + c.xh);
    const TileHalo hl = stage_halo_index(s, pl, x, strp, shid);
    stage_halo_rows(pl, x, hl, shid, slcol, X, XSB, sXh);
    const int ebase = hl.ebase;
    for (int r = tid >> 3; r < nrows; r += NTA / 8) {
      const int eb = strp[r] - ebase, ee = strp[r + 1] - ebase;
      for (int ch = sub; ch < nch; ch += 8) {
        const int c4 = ch * 4;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        int e = eb;
        for (; e + 4 <= ee; e += 4) {
          int e1 = e + 1, e2 = e + 2, e3 = e + 3;
          asm volatile("" : "+v"(e1), "+v"(e2), "+v"(e3));
          const int j0 = slcol[e], j1 = slcol[e1], j2 = slcol[e2], j3 = slcol[e3];
          const uint2 v0 = *reinterpret_cast<const uint2*>(&sXh[__umul24(j0, XSB) + c4]);
          const uint2 v1 = *reinterpret_cast<const uint2*>(&sXh[__umul24(j1, XSB) + c4]);
          const uint2 v2 = *reinterpret_cast<const uint2*>(&sXh[__umul24(j2, XSB) + c4]);
          const uint2 v3 = *reinterpret_cast<const uint2*>(&sXh[__umul24(j3, XSB) + c4]);
          acc = f4add(f4add(f4add(f4add(acc, unpack4bf(v0)), unpack4bf(v1)), unpack4bf(v2)), unpack4bf(v3));
        }
        for (; e < ee; ++e) acc = f4add(acc, unpack4bf(*reinterpret_cast<const uint2*>(&sXh[__umul24((int)slcol[e], XSB) + c4])));
        const uint2 zb = pack4bf(acc.x, acc.y, acc.z, acc.w);
        *reinterpret_cast<uint2*>(&sZ[r * ZSB + c4]) = zb;
      }
    }
  } else {
    const int* rp = s.rowptr + n0 + x.d.gid;
    const uint16_t* col = s.col + x.d.col0;
    for (int r = tid >> 3; r < nrows; r += NTA / 8) {
      const int i = r0 + r;
      const int eb = rp[i], ee = rp[i + 1];
      for (int ch = sub; ch < nch; ch += 8) {
        const int c4 = ch * 4;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        int e = eb;
        for (; e + 4 <= ee; e += 4) {
          const int j0 = col[e], j1 = col[e + 1], j2 = col[e + 2], j3 = col[e + 3];
          const uint2 v0 = *reinterpret_cast<const uint2*>(X + (int64_t)j0 * XSB + c4);
          const uint2 v1 = *reinterpret_cast<const uint2*>(X + (int64_t)j1 * XSB + c4);
          const uint2 v2 = *reinterpret_cast<const uint2*>(X + (int64_t)j2 * XSB + c4);
          const uint2 v3 = *reinterpret_cast<const uint2*>(X + (int64_t)j3 * XSB + c4);
          acc = f4add(f4add(f4add(f4add(acc, unpack4bf(v0)), unpack4bf(v1)), unpack4bf(v2)), unpack4bf(v3));
        }
        for (; e < ee; ++e) acc = f4add(acc, unpack4bf(*reinterpret_cast<const uint2*>(X + (int64_t)col[e] * XSB + c4)));
        const uint2 zb = pack4bf(acc.x, acc.y, acc.z, acc.w);
        *reinterpret_cast<uint2*>(&sZ[r * ZSB + c4]) = zb;
      }
    }
  }
  __syncthreads();
  // H = relu(Z [W1; W1e]^T): lane l holds Z[row l&15][k 8(l>>4)..+7] and
  // W[col l&15][same k] (16-byte LDS reads); C row (l>>4)*4+r, col l&15.
  {
    const int li = lane & 15, kq = lane >> 4;
    for (int tt = wave; tt * 16 < nrows; tt += NTA / 64) {
      const int q0 = tt * 16;
      const int ar = min(q0 + li, nrows - 1);
      floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < KPB; k += 32) {
        const bf16x8 av = *reinterpret_cast<const bf16x8*>(&sZ[ar * ZSB + k + 8 * kq]);
        const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(&sW[li * ZSB + k + 8 * kq]);
        const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(&sW[(16 + li) * ZSB + k + 8 * kq]);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b1, acc1, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = q0 + kq * 4 + r;
        if (row < nrows) {
          sH[row * 32 + li] = relu_keepnan(acc0[r]);
          sH[row * 32 + 16 + li] = relu_keepnan(acc1[r]);
        }
      }
    }
  }
  tile_partial_max(pl, x, sH, sm0i, sm0p, srng, compact, sflag);
  for (int p = tid; p < nrows * nch; p += NTA) {
    const int r = p / nch, c4 = (p - r * nch) * 4;
    if (sflag[r]) *reinterpret_cast<uint2*>(zg + (int64_t)(r0 + r) * XSB + c4) = *reinterpret_cast<const uint2*>(&sZ[r * ZSB + c4]);
  }
}

__global__ void __launch_bounds__(NTA) ginet_large_conv1_bf16_kernel(LargeArgs la) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  conv_tile_bf16(la, lds);
}

struct TailCarve {
  int w2, fc2, p1, a1, dp1, y2, h2, p1rp, p1c, p1trp, p1tc, m1p, m1i, p2, nt, cl1, head, dgp, total;
};

__host__ __device__ inline TailCarve tail_carve(int K0, int P1, int K1, int alias, int OUT) {
  TailCarve c;
  LdsWalk w;
  take_head_weights(c, w, OUT);
  take_tail_regions(c, w, K0, P1, K1, alias);
  c.total = w.o;
  return c;
}

// The per-graph tail of the large path, one workgroup per graph: combine the
// tiles' partial maxima, then ginet_tail.
__device__ __forceinline__ void tail_body(const LargeArgs& la, int b, float* lds) {
  const GinetArgs& a = la.g;
  const dr_large_plan& pl = la.plan;
  const int tid = threadIdx.x;
  const dr_graph_store& s = a.s;
  const dr_graph_desc d = a.descs[b];
  const int g = d.gid;
  const int64_t k00 = d.k0, q0 = d.p1, k10 = d.k1;
  const int N = d.n_nodes, K0 = d.n_k0, P1 = d.n_p1, K1 = d.n_k1;
  const int F = s.n_feat, alias = s.transpose_aliased, OUT = a.p.out_dim;
  const TailCarve c = tail_carve(K0, P1, K1, alias, OUT);
  const TailLds t = tail_lds(c, lds);
  const int row = a.p.slot ? a.p.slot[b] : b;  // the graph's rows of the batch (dr_pass.slot)
  STAMP(0);

  float fc1_row[8], fc1_col[8], fc1_bias;
  fc1_load(a.w, tid, tid >> 6, fc1_row, fc1_col, fc1_bias);
  const float y_g = s.y[g];
  uint64_t drop_offset = a.p.drop_offset;
  dma_copy<NT, 4>(t.p1rp, s.p1_rowptr + k00 + g, K0 + 1);
  dma_copy<NT, 4>(t.p1c, s.p1_col + q0, P1);
  if (!alias) {
    dma_copy<NT, 4>(t.p1trp, s.p1t_rowptr + k00 + g, K0 + 1);
    dma_copy<NT, 4>(t.p1tc, s.p1t_col + q0, P1);
  }
  dma_copy<NT, 4>(t.m1p, s.m1_ptr + k10 + g, K1 + 1);
  dma_copy<NT, 4>(t.m1i, s.m1_idx + k00, K0);
  t.w2[tid] = (tid < 512) ? a.w.w2[tid] : a.w.w2e[tid - 512];
  for (int p = tid; p < OUT * 129; p += NT) t.fc2[p] = (p < OUT * 128) ? a.w.fc2w[p] : a.w.fc2b[p - OUT * 128];
  STAMP(1);
  // tiles in node order, strict '>': the first maximum over the whole graph
  const int tb = pl.tile_first[b], te = pl.tile_first[b + 1];
  if (pl.part_key) decode_keys<32, NT>(pl, b, K0, N, t.p1, t.a1);
  else
  for (int p = tid; p < K0 * 32; p += NT) {
    float best = LOWEST;
    int arg = N;
    int tl = tb;
    for (; tl + 8 <= te; tl += 8) {  // 8 tiles' partials loaded together, combined in tile order
      float v[8];
      int ag[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t o = ((int64_t)(tl + u) * pl.k0_max) * 32 + p;
        v[u] = pl.part_val[o];
        ag[u] = pl.part_arg[o];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (v[u] > best) {
          best = v[u];
          arg = ag[u];
        }
    }
    for (; tl < te; ++tl) {
      const int64_t o = ((int64_t)tl * pl.k0_max) * 32 + p;
      const float v = pl.part_val[o];
      if (v > best) {
        best = v;
        arg = pl.part_arg[o];
      }
    }
    t.p1[p] = (best == LOWEST) ? 0.f : best;
    t.a1[p] = arg;
  }
  if (a.p.step_counter) drop_offset = (uint64_t)a.p.step_counter[0];  // loaded late: no early wait
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // snapshot for dr_reduce_update, stored only now so that no wait for the
  // counter load sits between the descriptor and the graph DMA
  if (a.p.step_counter && b == 0 && tid == 0) a.p.step_counter[1] = (int64_t)drop_offset;
  __syncthreads();
  STAMP(2);
  STAMP(3);
  if (a.p.compute_dtype == DR_DTYPE_BF16) {  // the bf16 Z the conv1 GEMM consumed
    const int XSB = s.x_bf16_stride;
    const uint16_t* zb = reinterpret_cast<const uint16_t*>(pl.z) + (int64_t)pl.z_row0[b] * XSB;
    ginet_tail(a, t, fc1_row, fc1_col, fc1_bias, row, N, K0, K1, F, OUT, y_g, drop_offset,
               [&](int i, int kk) { return bf2f(zb[(int64_t)i * XSB + kk]); }, -1);
    return;
  }
  const float* z = pl.z + (int64_t)pl.z_row0[b] * r4(F);
  const int XS = r4(F);
  ginet_tail(a, t, fc1_row, fc1_col, fc1_bias, row, N, K0, K1, F, OUT, y_g, drop_offset,
             [&](int i, int kk) { return z[(int64_t)i * XS + kk]; }, -1);
}

__global__ void __launch_bounds__(NT) ginet_large_tail_kernel(LargeArgs la) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  tail_body(la, blockIdx.x, lds);
}

// ---- input gradients on the large path (dr_ginet_large_input_grad_pass) ----
// ginet_input_grad_kernel's epilogue cut at its barrier: the tail forms dZ in
// a global workspace (dz: graph b's rows of DS = r4(F) words from row
// plan.z_row0[b]), and a tile kernel gathers dX = A^T dZ from it.
//
// Tail: tail_body as it is, then ginet_input_grad_kernel's loop on the global
// rows: one thread per (cluster k, feature f) runs
//   dZ[a1[k, ch], f] = fmaf(dp1[k, ch], [W1; W1e][ch, f], dZ[a1[k, ch], f]),  ch = 0 .. 31,
// as 32 read-modify-writes in channel order (the loads hit the words this
// thread stored, or the workgroup's zeros).  No two threads touch one word (k
// fixes the node's cluster, f the column), and the loop runs over all K0 F
// items (K0 <= 64: up to four per thread).  The graph's dz rows are zeroed by
// the workgroup before tail_body.  A form that sorted each cluster's
// (node, channel) pairs and stored every touched word once from a register
// measured level with this one and was not kept.
__global__ void __launch_bounds__(NT) ginet_large_input_grad_tail_kernel(LargeArgs la, float* dz) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int F = la.g.s.n_feat, DS = r4(F);
  float* dzg = dz + (int64_t)la.plan.z_row0[b] * DS;
  {  // early: nothing reads dz before the loop below
    const int n4 = la.g.descs[b].n_nodes * (DS >> 2);
    float4* z4 = reinterpret_cast<float4*>(dzg);
    for (int p = tid; p < n4; p += NT) z4[p] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  tail_body(la, b, lds);
  __syncthreads();  // the tail's last step (dW1) has read Z; dp1 / a1 are complete, the zeros above are stored
  const dr_graph_desc d = la.g.descs[b];
  const int N = d.n_nodes, K0 = d.n_k0;
  const TailCarve c = tail_carve(K0, d.n_p1, d.n_k1, la.g.s.transpose_aliased, la.g.p.out_dim);
  const float* dp1 = lds + c.dp1;
  const int* a1 = reinterpret_cast<const int*>(lds + c.a1);
  for (int p = tid; p < K0 * F; p += NT) {
    const int k = p / F, f = p - k * F;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const float* wsrc = (hf ? la.g.w.w1e : la.g.w.w1) + f;
      float w[16], v[16];
      int i[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) w[u] = wsrc[u * F];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int4 iv = *reinterpret_cast<const int4*>(a1 + k * 32 + hf * 16 + 4 * q);
        const float4 vv = *reinterpret_cast<const float4*>(dp1 + k * 32 + hf * 16 + 4 * q);
        i[4 * q] = iv.x; i[4 * q + 1] = iv.y; i[4 * q + 2] = iv.z; i[4 * q + 3] = iv.w;
        v[4 * q] = vv.x; v[4 * q + 1] = vv.y; v[4 * q + 2] = vv.z; v[4 * q + 3] = vv.w;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (i[u] < N) dzg[i[u] * DS + f] = fmaf(v[u], w[u], dzg[i[u] * DS + f]);
    }
  }
}

// dX[m, :] = sum over transposed CSR row m, in slot order from +0, of dZ[t_col[s], :]
// for the rows of one tile: 8 lanes per row, one 16-byte chunk each, dz read
// from global memory (a graph's block stays in its tiles' L2: tile_ctx);
// zeros past r4(F).
// (dz: the first dz row of the tile's graph; out: the tile's first output row, rows of dx_stride words)
__device__ __forceinline__ void dx_tile_rows(const dr_graph_store& s, const TileCtx& x, const float* dzg, float* out,
                                             int dx_stride) {
  const int tid = threadIdx.x, DS = r4(s.n_feat);
  const int* trp = s.t_rowptr + x.d.node0 + x.d.gid + x.r0;
  const uint16_t* tcol = s.t_col + x.d.col0;
  const int sub = tid & 7, nchd = DS >> 2, ncho = dx_stride >> 2;
  for (int r = tid >> 3; r < x.nrows; r += NTA / 8) {
    const int eb = trp[r], ee = trp[r + 1];
    float* row = out + r * (int64_t)dx_stride;
    for (int ch = sub; ch < ncho; ch += 8) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ch < nchd) acc = drk::gather_row_chunk(tcol, eb, ee, dzg, DS, ch * 4);
      *reinterpret_cast<float4*>(row + ch * 4) = acc;
    }
  }
}

__global__ void __launch_bounds__(NTA) ginet_large_dx_kernel(LargeArgs la, dr_input_grad ig, const float* dz) {
  const TileCtx x = tile_ctx(la.g.descs, la.plan);
  dx_tile_rows(la.g.s, x, dz + (int64_t)la.plan.z_row0[x.b] * r4(la.g.s.n_feat),
               ig.dx + (ig.row_off[x.b] + x.r0) * (int64_t)ig.dx_stride, ig.dx_stride);
}

// ---- integrated gradients on the large path (dr_ginet_large_integrated_grad_pass) ----
// ginet_integrated_grad_kernel cut at its barriers into launches: group g's
// step s0_g + j is round j of a (tile, tail) launch pair with grid.y = G, on
// group g's own Z rows, pooling partials / keys, dz rows and slab / head / out
// rows (no word is written by two workgroups of a launch, and nothing of the
// plan's own workspaces is touched); the steps' weighted dZ add up in dz[g]
// over the rounds, in step order, and one gather launch forms part[g] = A^T
// dz[g] for ig_finish_kernel.  Stream order is the only ordering between
// launches.  A workgroup whose group has no step in this round returns before
// any barrier or store.
struct IgTileArgs {
  dr_integrated_grad ig;
  dr_ig_tiles ws;
  int round;
};

// group grp's step of this round, or -1
__device__ __forceinline__ int ig_tile_step(const IgTileArgs& ia, int grp) {
  const int s = (int)((int64_t)grp * ia.ig.n_steps / ia.ig.n_groups) + ia.round;
  return s < (int)((int64_t)(grp + 1) * ia.ig.n_steps / ia.ig.n_groups) ? s : -1;
}

// la as group grp sees it: the plan's workspaces and the pass's outputs are the group's own
__device__ __forceinline__ void ig_tile_view(LargeArgs& la, const IgTileArgs& ia, int grp) {
  const int F = la.g.s.n_feat, OUT = la.g.p.out_dim;
  const int64_t keys = (int64_t)la.plan.k0_max * 32;
  la.plan.z = ia.ws.z + (int64_t)grp * ia.ws.rows * r4(F);  // (rows of r4(F) words, as the tile kernel and the tail index plan->z)
  if (la.plan.part_key) la.plan.part_key = ia.ws.part_key + (int64_t)grp * la.g.B * keys;
  else {
    la.plan.part_val = ia.ws.part_val + (int64_t)grp * la.plan.n_tiles * keys;
    la.plan.part_arg = ia.ws.part_arg + (int64_t)grp * la.plan.n_tiles * keys;
  }
  la.g.p.slab = ia.ig.slab + (int64_t)grp * la.g.B * DR_SLAB_STRIDE(F);
  la.g.p.head = ia.ig.head + (int64_t)grp * la.g.B * DR_HEAD_STRIDE(OUT);
  la.g.p.out = ia.ig.out + (int64_t)grp * la.g.B * OUT;
}

__global__ void __launch_bounds__(NTA) ginet_large_ig_conv1_kernel(LargeArgs la, IgTileArgs ia) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int grp = blockIdx.y, s = ig_tile_step(ia, grp);
  if (s < 0) return;
  ig_tile_view(la, ia, grp);
  conv_tile_f32<true>(la, lds, ia.ig.alpha[s], ia.ig.zb, ia.ws.zb_stride);
}

// Tail: on the group's first step the graph's rows of dz[g] are zeroed; then
// tail_body as it is, on the group's view; then ginet_integrated_grad_kernel's
// weighted chain on the global rows (dv = w_s dp1, one fmaf per channel in
// ascending order), over all K0 F items as ginet_large_input_grad_tail_kernel.
__global__ void __launch_bounds__(NT) ginet_large_ig_tail_kernel(LargeArgs la, IgTileArgs ia) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, b = blockIdx.x, grp = blockIdx.y, s = ig_tile_step(ia, grp);
  if (s < 0) return;
  ig_tile_view(la, ia, grp);
  const int F = la.g.s.n_feat, DS = r4(F);
  float* dzg = ia.ws.dz + ((int64_t)grp * ia.ws.rows + la.plan.z_row0[b]) * DS;
  if (ia.round == 0) {  // early: nothing reads dz before the loop below
    const int n4 = la.g.descs[b].n_nodes * (DS >> 2);
    float4* z4 = reinterpret_cast<float4*>(dzg);
    for (int p = tid; p < n4; p += NT) z4[p] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  tail_body(la, b, lds);
  __syncthreads();  // the tail's last step (dW1) has read Z; dp1 / a1 are complete, the zeros above are stored
  const dr_graph_desc d = la.g.descs[b];
  const int N = d.n_nodes, K0 = d.n_k0;
  const TailCarve c = tail_carve(K0, d.n_p1, d.n_k1, la.g.s.transpose_aliased, la.g.p.out_dim);
  const float* dp1 = lds + c.dp1;
  const int* a1 = reinterpret_cast<const int*>(lds + c.a1);
  const float ws = ia.ig.weight[s];
  for (int p = tid; p < K0 * F; p += NT) {
    const int k = p / F, f = p - k * F;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const float* wsrc = (hf ? la.g.w.w1e : la.g.w.w1) + f;
      float w[16], dv[16];
      int i[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) w[u] = wsrc[u * F];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int4 iv = *reinterpret_cast<const int4*>(a1 + k * 32 + hf * 16 + 4 * q);
        const float4 vv = *reinterpret_cast<const float4*>(dp1 + k * 32 + hf * 16 + 4 * q);
        i[4 * q] = iv.x; i[4 * q + 1] = iv.y; i[4 * q + 2] = iv.z; i[4 * q + 3] = iv.w;
        dv[4 * q] = ws * vv.x; dv[4 * q + 1] = ws * vv.y; dv[4 * q + 2] = ws * vv.z; dv[4 * q + 3] = ws * vv.w;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (i[u] < N) dzg[i[u] * DS + f] = fmaf(dv[u], w[u], dzg[i[u] * DS + f]);
    }
  }
}

// part[g][part_off[b] + m, :] = ginet_large_dx_kernel's gather of dz[g], grid (n_tiles, G)
__global__ void __launch_bounds__(NTA) ginet_large_ig_dx_kernel(LargeArgs la, IgTileArgs ia) {
  const TileCtx x = tile_ctx(la.g.descs, la.plan);
  const int grp = blockIdx.y, DXS = ia.ig.dx_stride;
  dx_tile_rows(la.g.s, x, ia.ws.dz + ((int64_t)grp * ia.ws.rows + la.plan.z_row0[x.b]) * r4(la.g.s.n_feat),
               ia.ig.part + ((int64_t)grp * ia.ig.part_rows + ia.ig.part_off[x.b] + x.r0) * (int64_t)DXS, DXS);
}

}  // namespace

extern "C" int64_t dr_ginet_lds_bytes(int32_t n_nodes, int32_t n_edges, int32_t n_feat, int32_t k0, int32_t p1_edges,
                                      int32_t k1, int32_t transpose_aliased, int32_t out_dim) {
  return 4LL * carve(n_nodes, n_edges, n_feat, k0, p1_edges, k1, transpose_aliased, out_dim).total;
}

// What dr_ginet_graph_pass, dr_ginet_graph_pass_z and (per member)
// dr_ginet_multi_pass check before anything is launched
static int graph_pass_check(const dr_graph_store* store, const dr_graph_desc* descs, int32_t n_batch,
                            const dr_ginet_weights* w, const dr_pass* pass, int32_t lds_bytes) {
  if (!store || !descs || !w || !pass || n_batch < 0) return DR_E_ARG;
  DR_CHECK(dr_check_loss(pass));
  if (pass->out_dim < 1 || pass->out_dim > DR_MAX_OUT) return DR_E_UNSUPPORTED;
  if (store->n_feat < 1 || 32 * store->n_feat > 2 * NT) return DR_E_UNSUPPORTED;  // F <= 64
  if (lds_bytes > 160 * 1024) return DR_E_LDS;
  if (pass->compute_dtype != DR_DTYPE_F32) return DR_E_UNSUPPORTED;  // bf16 runs dr_ginet_large_pass
  DR_CHECK(dr_check_pass_args(pass, true));
  return DR_OK;
}

// The per-graph kernels are instantiated for KPT = 32 (F <= 32) or 64 and for
// the gather or the Z-input form: launch(KPT, ZIN) gets the two as
// std::integral_constant values and returns the entry's result.
template <class Launch>
static int dispatch_kpt_zin(int F, bool zin, Launch launch) {
  using K32 = std::integral_constant<int, 32>;
  using K64 = std::integral_constant<int, 64>;
  if (F <= 32) return zin ? launch(K32(), std::true_type()) : launch(K32(), std::false_type());
  return zin ? launch(K64(), std::true_type()) : launch(K64(), std::false_type());
}

// dr_ginet_graph_pass (z = null) and dr_ginet_graph_pass_z
static int graph_pass_launch(const dr_graph_store* store, const dr_graph_desc* descs, int32_t n_batch,
                             const dr_ginet_weights* w, const dr_pass* pass, int32_t lds_bytes, const float* z,
                             int32_t z_stride, void* stream, const float* rec = nullptr) {
  DR_CHECK(graph_pass_check(store, descs, n_batch, w, pass, lds_bytes));
  if (n_batch == 0) return DR_OK;
  if (!store->cl0) return DR_E_ARG;
  GinetArgs args;
  args.s = *store;
  args.w = *w;
  args.p = *pass;
  args.descs = descs;
  args.B = n_batch;
  args.z = z;
  args.z_stride = z_stride;
  args.rec = rec;
  return dispatch_kpt_zin(store->n_feat, z != nullptr || rec != nullptr, [&](auto kpt, auto zin) {
    constexpr int KPT = decltype(kpt)::value;
    constexpr bool ZIN = decltype(zin)::value;
    const auto kernel = ZIN && rec ? &ginet_graph_kernel<KPT, ZIN, ZIN> : &ginet_graph_kernel<KPT, ZIN>;
    DR_CHECK(dr_allow_big_lds(reinterpret_cast<const void*>(kernel)));
    hipLaunchKernelGGL(kernel, dim3(n_batch), dim3(NT), lds_bytes, (hipStream_t)stream, args);
    return (int)hipGetLastError();
  });
}

extern "C" int dr_ginet_graph_pass(const dr_graph_store* store, const dr_graph_desc* descs, int32_t n_batch,
                                   const dr_ginet_weights* w, const dr_pass* pass, int32_t lds_bytes,
                                   void* stream) {
  return graph_pass_launch(store, descs, n_batch, w, pass, lds_bytes, nullptr, 0, stream);
}

// a usable Z array: rows at least the kernel's K wide, and 8-byte aligned (stride even)
static bool z_args_ok(const dr_graph_store* store, const float* z, int32_t z_stride) {
  if (!z || !store) return false;
  const int kpt = store->n_feat <= 32 ? 32 : 64;
  return z_stride >= kpt && z_stride % 2 == 0;
}

extern "C" int64_t dr_ginet_z_lds_bytes(int32_t n_nodes, int32_t n_edges, int32_t n_feat, int32_t k0, int32_t p1_edges,
                                        int32_t k1, int32_t transpose_aliased, int32_t out_dim, int32_t z_stride) {
  if (z_stride < (n_feat <= 32 ? 32 : 64)) return -1;
  return 4LL * carve(n_nodes, n_edges, n_feat, k0, p1_edges, k1, transpose_aliased, out_dim, z_stride).total;
}

extern "C" int dr_ginet_graph_pass_z(const dr_graph_store* store, const dr_graph_desc* descs, int32_t n_batch,
                                     const dr_ginet_weights* w, const dr_pass* pass, int32_t lds_bytes, const float* z,
                                     int32_t z_stride, void* stream) {
  if (!z_args_ok(store, z, z_stride)) return DR_E_ARG;
  return graph_pass_launch(store, descs, n_batch, w, pass, lds_bytes, z, z_stride, stream);
}

// the records' buffer: 16-byte aligned, for a usable stride
static bool rec_args_ok(const dr_graph_store* store, const void* rdescs, const float* rec, int32_t z_stride) {
  return rdescs && rec && reinterpret_cast<uintptr_t>(rec) % 16 == 0 && z_args_ok(store, rec, z_stride);
}

extern "C" int dr_ginet_graph_pass_rec(const dr_graph_store* store, const dr_graph_rec_desc* rdescs, int32_t n_batch,
                                       const dr_ginet_weights* w, const dr_pass* pass, int32_t lds_bytes,
                                       const float* rec, int32_t z_stride, void* stream) {
  if (!rec_args_ok(store, rdescs, rec, z_stride)) return DR_E_ARG;
  return graph_pass_launch(store, reinterpret_cast<const dr_graph_desc*>(rdescs), n_batch, w, pass, lds_bytes, nullptr,
                           z_stride, stream, rec);
}

extern "C" int64_t dr_ginet_input_grad_lds_bytes(int32_t n_nodes, int32_t n_edges, int32_t n_feat, int32_t k0,
                                                 int32_t p1_edges, int32_t k1, int32_t transpose_aliased, int32_t out_dim,
                                                 int32_t z_stride) {
  if (z_stride > 0 && z_stride < (n_feat <= 32 ? 32 : 64)) return -1;
  const int zs = z_stride > 0 ? z_stride : 0;
  const Carve c = carve(n_nodes, n_edges, n_feat, k0, p1_edges, k1, transpose_aliased, out_dim, zs);
  return 4LL * ig_lds(c, n_nodes, n_edges, zs).total;
}

extern "C" int dr_ginet_input_grad_pass(const dr_graph_store* store, const dr_graph_desc* descs, int32_t n_batch,
                                        const dr_ginet_weights* w, const dr_pass* pass, const dr_input_grad* ig,
                                        const float* z, int32_t z_stride, int32_t lds_bytes, void* stream) {
  DR_CHECK(graph_pass_check(store, descs, n_batch, w, pass, lds_bytes));
  if (!(pass->flags & DR_PASS_BACKWARD)) return DR_E_ARG;
  if (pass->slot || pass->step_counter) return DR_E_ARG;
  if (!ig || !ig->dx || !ig->row_off) return DR_E_ARG;
  if (ig->dx_stride < store->n_feat || ig->dx_stride % 4 != 0) return DR_E_ARG;
  if (reinterpret_cast<uintptr_t>(ig->dx) % 16 != 0) return DR_E_ARG;
  if (z && !z_args_ok(store, z, z_stride)) return DR_E_ARG;
  if (n_batch == 0) return DR_OK;
  if (!store->cl0 || !store->t_rowptr || !store->t_col) return DR_E_ARG;
  GinetArgs args;
  args.s = *store;
  args.w = *w;
  args.p = *pass;
  args.descs = descs;
  args.B = n_batch;
  args.z = z;
  args.z_stride = z ? z_stride : 0;
  const dr_input_grad iga = *ig;
  return dispatch_kpt_zin(store->n_feat, z != nullptr, [&](auto kpt, auto zin) {
    const auto kernel = &ginet_input_grad_kernel<decltype(kpt)::value, decltype(zin)::value>;
    DR_CHECK(dr_allow_big_lds(reinterpret_cast<const void*>(kernel)));
    hipLaunchKernelGGL(kernel, dim3(n_batch), dim3(NT), lds_bytes, (hipStream_t)stream, args, iga);
    return (int)hipGetLastError();
  });
}

extern "C" int64_t dr_ginet_integrated_grad_lds_bytes(int32_t n_nodes, int32_t n_edges, int32_t n_feat, int32_t k0,
                                                      int32_t p1_edges, int32_t k1, int32_t transpose_aliased,
                                                      int32_t out_dim, int32_t z_stride) {
  if (z_stride < (n_feat <= 32 ? 32 : 64)) return -1;  // (no gather form: a Z stride is required)
  const Carve c = carve(n_nodes, n_edges, n_feat, k0, p1_edges, k1, transpose_aliased, out_dim, z_stride);
  return 4LL * intgrad_lds(c, n_nodes, n_edges, z_stride).total;
}

extern "C" int dr_ginet_integrated_grad_pass(const dr_graph_store* store, const dr_graph_desc* descs, int32_t n_batch,
                                             const dr_ginet_weights* w, const dr_pass* pass, const dr_integrated_grad* ig,
                                             const float* z, int32_t z_stride, int32_t lds_bytes, void* stream) {
  if (!pass || !ig) return DR_E_ARG;
  dr_pass gp = *pass;  // the pass as the steps run it: its partials go to the groups' scratch rows
  gp.slab = ig->slab;
  gp.head = ig->head;
  gp.out = ig->out;
  gp.loss_per_graph = nullptr;  // (one word per graph, which the groups would all write)
  gp.stamps = nullptr;
  DR_CHECK(graph_pass_check(store, descs, n_batch, w, &gp, lds_bytes));
  if (!(pass->flags & DR_PASS_BACKWARD)) return DR_E_ARG;
  if (pass->slot || pass->step_counter) return DR_E_ARG;
  if (!ig->attr || !ig->row_off || !ig->alpha || !ig->weight || !ig->part || !ig->part_off || !ig->attr_sum ||
      !ig->slab || !ig->head || !ig->out)
    return DR_E_ARG;
  if (ig->n_steps < 1 || ig->n_groups < 1 || ig->n_groups > ig->n_steps) return DR_E_ARG;
  if (ig->dx_stride < store->n_feat || ig->dx_stride % 4 != 0) return DR_E_ARG;
  if (reinterpret_cast<uintptr_t>(ig->attr) % 16 != 0 || reinterpret_cast<uintptr_t>(ig->part) % 16 != 0) return DR_E_ARG;
  if (ig->part_rows < 0) return DR_E_ARG;
  if ((ig->zb != nullptr) != (ig->xb != nullptr)) return DR_E_ARG;
  // no gather form; the steps rescale Z in 16-byte chunks (rows of z and zb a multiple of 4 words, 16-byte aligned)
  if (!z_args_ok(store, z, z_stride) || z_stride % 4 != 0) return DR_E_ARG;
  if (reinterpret_cast<uintptr_t>(z) % 16 != 0 || reinterpret_cast<uintptr_t>(ig->zb) % 16 != 0) return DR_E_ARG;
  if (n_batch == 0) return DR_OK;
  if (!store->cl0 || !store->t_rowptr || !store->t_col || !store->x) return DR_E_ARG;
  IntGradArgs ia;
  GinetArgs& args = ia.a;
  args.s = *store;
  args.w = *w;
  args.p = gp;
  args.descs = descs;
  args.B = n_batch;
  args.z = z;
  args.z_stride = z_stride;
  ia.ig = *ig;
  const auto launch = [&](auto kpt) {
    const auto kernel = &ginet_integrated_grad_kernel<decltype(kpt)::value>;
    DR_CHECK(dr_allow_big_lds(reinterpret_cast<const void*>(kernel)));
    hipLaunchKernelGGL(kernel, dim3(n_batch, ia.ig.n_groups), dim3(NT), lds_bytes, (hipStream_t)stream, ia);
    return (int)hipGetLastError();
  };
  DR_CHECK(store->n_feat <= 32 ? launch(std::integral_constant<int, 32>()) : launch(std::integral_constant<int, 64>()));
  hipLaunchKernelGGL(ig_finish_kernel, dim3(n_batch), dim3(NTF), 0, (hipStream_t)stream, args.s, descs, ia.ig);
  return (int)hipGetLastError();
}

extern "C" int dr_ginet_multi_pass(const dr_graph_store* store, const dr_ginet_member* members, int32_t n_members,
                                   int32_t lds_bytes, const float* z, int32_t z_stride, void* stream) {
  if (!store || !members || n_members < 1 || n_members > DR_MAX_MEMBERS) return DR_E_ARG;
  if (z && !z_args_ok(store, z, z_stride)) return DR_E_ARG;
  int max_b = 0;
  for (int k = 0; k < n_members; ++k) {
    const dr_ginet_member& m = members[k];
    DR_CHECK(graph_pass_check(store, m.descs, m.n_batch, m.w, m.pass, lds_bytes));
    if (m.pass->slot) return DR_E_UNSUPPORTED;  // (a batch split over launches runs the members' own passes)
    if (m.pass->out_dim != members[0].pass->out_dim) return DR_E_UNSUPPORTED;
    max_b = m.n_batch > max_b ? m.n_batch : max_b;
  }
  if (max_b == 0) return DR_OK;
  if (!store->cl0) return DR_E_ARG;
  MultiArgs args;
  std::memset(&args, 0, sizeof(args));
  args.s = *store;
  args.z = z;
  args.z_stride = z ? z_stride : 0;
  args.n_members = n_members;
  for (int k = 0; k < n_members; ++k) {
    args.m[k].w = *members[k].w;
    args.m[k].p = *members[k].pass;
    args.m[k].descs = members[k].descs;
    args.m[k].B = members[k].n_batch;
  }
  return dispatch_kpt_zin(store->n_feat, z != nullptr, [&](auto kpt, auto zin) {
    const auto kernel = &ginet_multi_kernel<decltype(kpt)::value, decltype(zin)::value>;
    DR_CHECK(dr_allow_big_lds(reinterpret_cast<const void*>(kernel)));
    hipLaunchKernelGGL(kernel, dim3(max_b, n_members), dim3(NT), lds_bytes, (hipStream_t)stream, args);
    return (int)hipGetLastError();
  });
}

// Accumulating pass: n_groups workgroups, graph gi on workgroup gi % n_groups
// (or as plan lists them); each writes one row of dr_ginet_acc_row_floats
// floats to pass->slab and its loss sum to pass->loss_per_graph[w].
// max_sizes (host, optional): the batch's largest N, E, K0, P1, K1 — the
// prefetch layout when it fits, else lds_bytes (the largest graph's carve, as
// for dr_ginet_graph_pass) plus the accumulators.
extern "C" int32_t dr_ginet_acc_row_floats(int32_t n_feat, int32_t out_dim) { return acc_row_floats(n_feat, out_dim); }

// The accumulating kernels' dynamic LDS: the accumulators and the staged flag
// (acc_front_bytes), then a graph carve or (acc_prefetch_bytes) the prefetch
// layout L of the batch maxima, Z-input form for zs > 0.
static int64_t acc_front_bytes(int F, int OUT) { return 4LL * (acc_words(F, OUT, F > 32) + 4); }
static int64_t acc_prefetch_bytes(const int32_t* max_sizes, int F, int alias, int OUT, int zs, AccLayout* L) {
  *L = acc_layout(max_sizes[0], max_sizes[1], F, max_sizes[2], max_sizes[3], max_sizes[4], alias, OUT, zs);
  return acc_front_bytes(F, OUT) + 4LL * L->total;
}

extern "C" int64_t dr_ginet_acc_lds_bytes(const int32_t* max_sizes, int32_t n_feat, int32_t transpose_aliased, int32_t out_dim) {
  if (!max_sizes) return -1;
  AccLayout L;
  return acc_prefetch_bytes(max_sizes, n_feat, transpose_aliased, out_dim, 0, &L);
}

// dr_ginet_acc_pass (z = null) and dr_ginet_acc_pass_z.  Whether the pass can
// run at all is decided by the gather form's sizes either way.  The Z-input
// form's per-graph carve (lds_z_bytes: its largest graph's) is smaller than the
// gather form's, but its prefetch layout is not always: it holds Z once per
// parity, 2 (KPT + 4) N words against 2 (r4(F) N + N + E / 2) + (KPT + 2) N, so
// for small F (F <= 8 at E ~ 15 N) it is the larger one.  Where the gather
// prefetch layout fits and the Z one does not, the Z kernel without prefetch
// runs (same results); where that does not fit either, the gather kernels.
static int acc_pass_launch(const dr_graph_store* store, const dr_graph_desc* descs, int32_t n_batch,
                           const dr_ginet_weights* w, const dr_pass* pass, int32_t lds_bytes, int32_t n_groups,
                           const int32_t* plan, const int32_t* max_sizes, const float* z, int32_t z_stride,
                           int32_t lds_z_bytes, void* stream, const dr_graph_rec_desc* rdescs = nullptr) {
  // (rdescs: z is the buffer of dr_graph_records, the record kernels run where the Z kernels would)
  if (!store || !descs || !w || !pass || n_batch < 0 || n_groups < 1) return DR_E_ARG;
  DR_CHECK(dr_check_loss(pass));
  if (pass->out_dim < 1 || pass->out_dim > DR_MAX_OUT) return DR_E_UNSUPPORTED;
  if (store->n_feat < 1 || 32 * store->n_feat > 2 * NT) return DR_E_UNSUPPORTED;  // F <= 64
  if (pass->compute_dtype != DR_DTYPE_F32) return DR_E_UNSUPPORTED;
  // training passes only (the sums are gradients), with the fused loss
  if (!(pass->flags & DR_PASS_BACKWARD) || !pass->slab || !pass->loss_per_graph) return DR_E_ARG;
  if (pass->loss_kind == DR_LOSS_NONE || pass->slot) return DR_E_UNSUPPORTED;
  if ((pass->flags & DR_PASS_FORWARD) && !pass->out) return DR_E_ARG;
  if (pass->use_dropout == DR_DROPOUT_MASK && !pass->mask) return DR_E_ARG;
  if (pass->use_dropout < DR_DROPOUT_OFF || pass->use_dropout > DR_DROPOUT_HASH) return DR_E_ARG;
  const int F = store->n_feat, OUT = pass->out_dim;
  const int64_t lds = (int64_t)lds_bytes + acc_front_bytes(F, OUT);
  AccLayout L{};
  const int64_t lds_pf = max_sizes ? acc_prefetch_bytes(max_sizes, F, store->transpose_aliased, OUT, 0, &L) : -1;
  const bool pf = lds_pf > 0 && lds_pf <= 160 * 1024;
  if (!pf && lds > 160 * 1024) return DR_E_LDS;
  int64_t lds_z = 0, lds_pf_z = 0;
  bool pf_z = false;
  if (z) {
    lds_z = (int64_t)lds_z_bytes + acc_front_bytes(F, OUT);
    if (pf) {
      AccLayout Lz;
      lds_pf_z = acc_prefetch_bytes(max_sizes, F, store->transpose_aliased, OUT, z_stride, &Lz);
      pf_z = lds_pf_z <= 160 * 1024;
      if (pf_z) L = Lz;
    }
    if (!pf_z && lds_z > 160 * 1024) z = nullptr;  // neither Z layout fits: the gather kernels, as dr_ginet_acc_pass
  }
  if (n_batch == 0) return DR_OK;
  if (!store->cl0) return DR_E_ARG;
  if (n_groups > n_batch && !plan) n_groups = n_batch;
  GinetArgs args;
  args.s = *store;
  args.w = *w;
  args.p = *pass;
  args.descs = descs;
  args.B = n_batch;
  const bool rec = z && rdescs;
  args.z = rec ? nullptr : z;
  args.z_stride = z ? z_stride : 0;
  if (rec) {
    args.rec = z;
    args.descs = reinterpret_cast<const dr_graph_desc*>(rdescs);
  }
  return dispatch_kpt_zin(F, z != nullptr, [&](auto kpt, auto zin) {
    constexpr int KPT = decltype(kpt)::value;
    constexpr bool ZIN = decltype(zin)::value;
    const bool prefetch = ZIN ? pf_z : pf;
    const int64_t bytes = ZIN ? (pf_z ? lds_pf_z : lds_z) : (pf ? lds_pf : lds);
    const auto kernel = ZIN && rec ? (prefetch ? &ginet_acc_kernel<KPT, true, ZIN, ZIN> : &ginet_acc_kernel<KPT, false, ZIN, ZIN>)
                                   : (prefetch ? &ginet_acc_kernel<KPT, true, ZIN> : &ginet_acc_kernel<KPT, false, ZIN>);
    DR_CHECK(dr_allow_big_lds(reinterpret_cast<const void*>(kernel)));
    hipLaunchKernelGGL(kernel, dim3(n_groups), dim3(NT), (int)bytes, (hipStream_t)stream, args, plan, L);
    return (int)hipGetLastError();
  });
}

extern "C" int dr_ginet_acc_pass(const dr_graph_store* store, const dr_graph_desc* descs, int32_t n_batch,
                                 const dr_ginet_weights* w, const dr_pass* pass, int32_t lds_bytes, int32_t n_groups,
                                 const int32_t* plan, const int32_t* max_sizes, void* stream) {
  return acc_pass_launch(store, descs, n_batch, w, pass, lds_bytes, n_groups, plan, max_sizes, nullptr, 0, 0, stream);
}

extern "C" int dr_ginet_acc_pass_z(const dr_graph_store* store, const dr_graph_desc* descs, int32_t n_batch,
                                   const dr_ginet_weights* w, const dr_pass* pass, int32_t lds_bytes, int32_t lds_z_bytes,
                                   int32_t n_groups, const int32_t* plan, const int32_t* max_sizes, const float* z,
                                   int32_t z_stride, void* stream) {
  if (!z_args_ok(store, z, z_stride) || lds_z_bytes < 0) return DR_E_ARG;
  return acc_pass_launch(store, descs, n_batch, w, pass, lds_bytes, n_groups, plan, max_sizes, z, z_stride, lds_z_bytes, stream);
}

extern "C" int dr_ginet_acc_pass_rec(const dr_graph_store* store, const dr_graph_desc* descs, const dr_graph_rec_desc* rdescs,
                                     int32_t n_batch, const dr_ginet_weights* w, const dr_pass* pass, int32_t lds_bytes,
                                     int32_t lds_z_bytes, int32_t n_groups, const int32_t* plan, const int32_t* max_sizes,
                                     const float* rec, int32_t z_stride, void* stream) {
  if (!rec_args_ok(store, rdescs, rec, z_stride) || lds_z_bytes < 0) return DR_E_ARG;
  return acc_pass_launch(store, descs, n_batch, w, pass, lds_bytes, n_groups, plan, max_sizes, rec, z_stride, lds_z_bytes, stream,
                         rdescs);
}

// ---------------------------------------------------------------------------
// Z = A·X for whole graphs of the store (dr_aggregate_x): what conv1's gather
// computes in every pass, once.  One workgroup per graph, one thread per
// (row, column): the CSR row's x values added one at a time in CSR order from
// +0.f — the chain of drk::gather_row_two_chunks*, so the same bits.  Columns
// past F and the stride padding are written as zeros.  Not on the hot path.
// ---------------------------------------------------------------------------
namespace {
__global__ void __launch_bounds__(256) aggregate_x_kernel(dr_graph_store s, float* z, int32_t z_stride, int32_t g0) {
  const int g = g0 + blockIdx.x;
  const int64_t n0 = s.node_off[g];
  const int N = (int)(s.node_off[g + 1] - n0);
  const int32_t* rp = s.rowptr + n0 + g;
  const uint16_t* col = s.col + s.col_off[g];
  const float* x = s.x + n0 * (int64_t)s.x_stride;
  float* zg = z + n0 * (int64_t)z_stride;
  for (int p = threadIdx.x; p < N * z_stride; p += blockDim.x) {
    const int i = p / z_stride, c = p - i * z_stride;
    float acc = 0.f;
    if (c < s.n_feat)
      for (int e = rp[i]; e < rp[i + 1]; ++e) acc = acc + x[(int64_t)col[e] * s.x_stride + c];
    zg[p] = acc;
  }
}
}  // namespace

extern "C" int dr_aggregate_x(const dr_graph_store* store, float* z, int32_t z_stride, int32_t g0, int32_t n_graphs,
                              void* stream) {
  if (!store || !z || g0 < 0 || n_graphs < 0) return DR_E_ARG;
  if (z_stride < store->n_feat || g0 + (int64_t)n_graphs > store->n_graphs) return DR_E_ARG;
  if (n_graphs == 0) return DR_OK;
  hipLaunchKernelGGL(aggregate_x_kernel, dim3(n_graphs), dim3(256), 0, (hipStream_t)stream, *store, z, z_stride, g0);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// One record per graph (dr_graph_records): rec_layout's regions, the Z block
// by aggregate_x_kernel's sum chain (from +0, one fp32 add per edge in CSR
// order: the same bits), the index regions copied from the store's arrays,
// every region's padding zero.  One workgroup per graph; not on the hot path.
// ---------------------------------------------------------------------------
namespace {
__global__ void __launch_bounds__(256) graph_records_kernel(dr_graph_store s, float* out, int32_t z_stride, const int64_t* rec_off,
                                                            int32_t g0) {
  const int g = g0 + blockIdx.x;
  const int64_t n0 = s.node_off[g], k00 = s.k0_off[g], q0 = s.p1_off[g], k10 = s.k1_off[g];
  const int N = (int)(s.node_off[g + 1] - n0), K0 = (int)(s.k0_off[g + 1] - k00), P1 = (int)(s.p1_off[g + 1] - q0),
            K1 = (int)(s.k1_off[g + 1] - k10);
  const Carve c = rec_layout(N, K0, P1, K1, s.transpose_aliased, z_stride);
  float* r = out + rec_off[g];
  int32_t* ri = reinterpret_cast<int32_t*>(r);
  const int32_t* rp = s.rowptr + n0 + g;
  const uint16_t* col = s.col + s.col_off[g];
  const float* x = s.x + n0 * (int64_t)s.x_stride;
  for (int p = threadIdx.x; p < c.cl0; p += blockDim.x) {  // (c.cl0: the Z block's padded length; c.z = 0)
    const int i = p / z_stride, k = p - i * z_stride;
    float acc = 0.f;
    if (i < N && k < s.n_feat)
      for (int e = rp[i]; e < rp[i + 1]; ++e) acc = acc + x[(int64_t)col[e] * s.x_stride + k];
    r[p] = acc;
  }
  auto put = [&](int at, const int32_t* src, int n) {
    for (int p = threadIdx.x; p < r4(n); p += blockDim.x) ri[at + p] = p < n ? src[p] : 0;
  };
  put(c.cl0, s.cl0 + n0, N);
  put(c.p1rp, s.p1_rowptr + k00 + g, K0 + 1);
  put(c.p1c, s.p1_col + q0, P1);
  if (!s.transpose_aliased) {
    put(c.p1trp, s.p1t_rowptr + k00 + g, K0 + 1);
    put(c.p1tc, s.p1t_col + q0, P1);
  }
  put(c.m1p, s.m1_ptr + k10 + g, K1 + 1);
  put(c.m1i, s.m1_idx + k00, K0);
}
}  // namespace

extern "C" int64_t dr_graph_record_words(int32_t n_nodes, int32_t k0, int32_t p1_edges, int32_t k1, int32_t transpose_aliased,
                                         int32_t z_stride) {
  if (n_nodes < 0 || k0 < 0 || p1_edges < 0 || k1 < 0 || z_stride < 1) return -1;
  return rec_layout(n_nodes, k0, p1_edges, k1, transpose_aliased, z_stride).total;
}

extern "C" int dr_graph_records(const dr_graph_store* store, float* out, int32_t z_stride, const int64_t* rec_off, int32_t g0,
                                int32_t n_graphs, void* stream) {
  if (!store || !out || !rec_off || g0 < 0 || n_graphs < 0) return DR_E_ARG;
  if (z_stride < store->n_feat || g0 + (int64_t)n_graphs > store->n_graphs) return DR_E_ARG;
  if (reinterpret_cast<uintptr_t>(out) % 16 != 0) return DR_E_ARG;
  if (n_graphs == 0) return DR_OK;
  if (!store->cl0) return DR_E_ARG;
  hipLaunchKernelGGL(graph_records_kernel, dim3(n_graphs), dim3(256), 0, (hipStream_t)stream, *store, out, z_stride, rec_off, g0);
  return (int)hipGetLastError();
}

extern "C" int dr_debug_graph_record(const int32_t* q, int32_t* offs) {
  if (!q || !offs) return DR_E_ARG;
  const Carve c = rec_layout(q[0], q[1], q[2], q[3], q[4], q[5]);
  const int v[9] = {c.z, c.cl0, c.p1rp, c.p1c, c.p1trp, c.p1tc, c.m1p, c.m1i, c.total};
  for (int i = 0; i < 9; ++i) offs[i] = v[i];
  return DR_OK;
}

extern "C" int64_t dr_ginet_large_conv_lds_bytes(int32_t n_nodes, int32_t n_feat, int32_t k0, int32_t halo_max,
                                                 int32_t tile_edges_max) {
  return 4LL * conv_carve(n_nodes, n_feat, k0, halo_max, tile_edges_max).total;
}

extern "C" int64_t dr_ginet_large_conv_lds_bytes_bf16(int32_t n_nodes, int32_t n_feat, int32_t k0, int32_t halo_max,
                                                      int32_t tile_edges_max) {
  return 4LL * conv_carve_bf16(n_nodes, n_feat, k0, halo_max, tile_edges_max).total;
}

extern "C" int64_t dr_ginet_tail_lds_bytes(int32_t k0, int32_t p1_edges, int32_t k1, int32_t transpose_aliased,
                                           int32_t out_dim) {
  return 4LL * tail_carve(k0, p1_edges, k1, transpose_aliased, out_dim).total;
}

// What dr_ginet_large_pass and dr_ginet_large_input_grad_pass check before anything is launched
static int large_pass_check(const dr_graph_store* store, const dr_graph_desc* descs, int32_t n_batch,
                            const dr_large_plan* plan, const dr_ginet_weights* w, const dr_pass* pass,
                            int32_t conv_lds_bytes, int32_t tail_lds_bytes, bool f32_only) {
  if (!store || !descs || !w || !pass || !plan || n_batch < 0) return DR_E_ARG;
  DR_CHECK(dr_check_loss(pass));
  if (pass->out_dim < 1 || pass->out_dim > DR_MAX_OUT) return DR_E_UNSUPPORTED;
  if (store->n_feat < 1 || store->n_feat > 64) return DR_E_UNSUPPORTED;
  if (conv_lds_bytes > 160 * 1024 || tail_lds_bytes > 160 * 1024) return DR_E_LDS;
  DR_CHECK(dr_check_large_plan(plan, n_batch, true));
  DR_CHECK(dr_check_pass_args(pass, true));
  const bool bf16 = pass->compute_dtype == DR_DTYPE_BF16;
  if (f32_only && pass->compute_dtype != DR_DTYPE_F32) return DR_E_UNSUPPORTED;
  if (pass->compute_dtype != DR_DTYPE_F32 && !bf16) return DR_E_ARG;
  if (bf16 && (!store->x_bf16 || store->x_bf16_stride < store->n_feat || store->x_bf16_stride % 8)) return DR_E_ARG;
  return DR_OK;
}

extern "C" int dr_ginet_large_pass(const dr_graph_store* store, const dr_graph_desc* descs, int32_t n_batch,
                                   const dr_large_plan* plan, const dr_ginet_weights* w, const dr_pass* pass,
                                   int32_t conv_lds_bytes, int32_t tail_lds_bytes, void* stream) {
  DR_CHECK(large_pass_check(store, descs, n_batch, plan, w, pass, conv_lds_bytes, tail_lds_bytes, false));
  const bool bf16 = pass->compute_dtype == DR_DTYPE_BF16;
  if (n_batch == 0) return DR_OK;
  DR_CHECK(dr_allow_big_lds(reinterpret_cast<const void*>(&ginet_large_conv1_kernel)));
  DR_CHECK(dr_allow_big_lds(reinterpret_cast<const void*>(&ginet_large_conv1_bf16_kernel)));
  DR_CHECK(dr_allow_big_lds(reinterpret_cast<const void*>(&ginet_large_tail_kernel)));
  LargeArgs la;
  la.g.s = *store;
  la.g.w = *w;
  la.g.p = *pass;
  la.g.descs = descs;
  la.g.B = n_batch;
  la.plan = *plan;
  hipStream_t st = (hipStream_t)stream;
  if (bf16)
    hipLaunchKernelGGL(ginet_large_conv1_bf16_kernel, dim3(plan->n_tiles), dim3(NTA), conv_lds_bytes, st, la);
  else
    hipLaunchKernelGGL(ginet_large_conv1_kernel, dim3(plan->n_tiles), dim3(NTA), conv_lds_bytes, st, la);
  hipLaunchKernelGGL(ginet_large_tail_kernel, dim3(n_batch), dim3(NT), tail_lds_bytes, st, la);
  return (int)hipGetLastError();
}

extern "C" int dr_ginet_large_input_grad_pass(const dr_graph_store* store, const dr_graph_desc* descs, int32_t n_batch,
                                              const dr_large_plan* plan, const dr_ginet_weights* w, const dr_pass* pass,
                                              const dr_input_grad* ig, float* dz, int32_t conv_lds_bytes,
                                              int32_t tail_lds_bytes, void* stream) {
  DR_CHECK(large_pass_check(store, descs, n_batch, plan, w, pass, conv_lds_bytes, tail_lds_bytes, true));
  if (!(pass->flags & DR_PASS_BACKWARD)) return DR_E_ARG;
  if (pass->slot || pass->step_counter) return DR_E_ARG;
  if (!ig || !ig->dx || !ig->row_off || !dz) return DR_E_ARG;
  if (ig->dx_stride < store->n_feat || ig->dx_stride % 4 != 0) return DR_E_ARG;
  if (reinterpret_cast<uintptr_t>(ig->dx) % 16 != 0 || reinterpret_cast<uintptr_t>(dz) % 16 != 0) return DR_E_ARG;
  if (!store->cl0 || !store->t_rowptr || !store->t_col) return DR_E_ARG;
  if (n_batch == 0) return DR_OK;
  DR_CHECK(dr_allow_big_lds(reinterpret_cast<const void*>(&ginet_large_conv1_kernel)));
  DR_CHECK(dr_allow_big_lds(reinterpret_cast<const void*>(&ginet_large_input_grad_tail_kernel)));
  LargeArgs la;
  la.g.s = *store;
  la.g.w = *w;
  la.g.p = *pass;
  la.g.descs = descs;
  la.g.B = n_batch;
  la.plan = *plan;
  const dr_input_grad iga = *ig;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ginet_large_conv1_kernel, dim3(plan->n_tiles), dim3(NTA), conv_lds_bytes, st, la);
  hipLaunchKernelGGL(ginet_large_input_grad_tail_kernel, dim3(n_batch), dim3(NT), tail_lds_bytes, st, la, dz);
  hipLaunchKernelGGL(ginet_large_dx_kernel, dim3(plan->n_tiles), dim3(NTA), 0, st, la, iga, static_cast<const float*>(dz));
  return (int)hipGetLastError();
}

extern "C" int dr_ginet_large_integrated_grad_pass(const dr_graph_store* store, const dr_graph_desc* descs, int32_t n_batch,
                                                   const dr_large_plan* plan, const dr_ginet_weights* w, const dr_pass* pass,
                                                   const dr_integrated_grad* ig, const dr_ig_tiles* ws,
                                                   int32_t conv_lds_bytes, int32_t tail_lds_bytes, void* stream) {
  if (!pass || !ig || !ws) return DR_E_ARG;
  dr_pass gp = *pass;  // the pass as the steps run it: its partials go to the groups' scratch rows
  gp.slab = ig->slab;
  gp.head = ig->head;
  gp.out = ig->out;
  gp.loss_per_graph = nullptr;  // (one word per graph, which the groups would all write)
  gp.stamps = nullptr;
  DR_CHECK(large_pass_check(store, descs, n_batch, plan, w, &gp, conv_lds_bytes, tail_lds_bytes, true));
  if (!(pass->flags & DR_PASS_BACKWARD)) return DR_E_ARG;
  if (pass->slot || pass->step_counter) return DR_E_ARG;
  if (!ig->attr || !ig->row_off || !ig->alpha || !ig->weight || !ig->part || !ig->part_off || !ig->attr_sum ||
      !ig->slab || !ig->head || !ig->out)
    return DR_E_ARG;
  if (ig->n_steps < 1 || ig->n_groups < 1 || ig->n_groups > ig->n_steps) return DR_E_ARG;
  if (ig->dx_stride < store->n_feat || ig->dx_stride % 4 != 0) return DR_E_ARG;
  if (reinterpret_cast<uintptr_t>(ig->attr) % 16 != 0 || reinterpret_cast<uintptr_t>(ig->part) % 16 != 0) return DR_E_ARG;
  if (ig->part_rows < 0) return DR_E_ARG;
  if ((ig->zb != nullptr) != (ig->xb != nullptr)) return DR_E_ARG;
  // the tile kernel reads zb rows in 16-byte chunks over r4(F) columns
  if (ig->zb && (ws->zb_stride < r4(store->n_feat) || ws->zb_stride % 4 != 0 || reinterpret_cast<uintptr_t>(ig->zb) % 16 != 0))
    return DR_E_ARG;
  if (!ws->dz || !ws->z || ws->rows < 0) return DR_E_ARG;
  if (plan->part_key ? !ws->part_key : (!ws->part_val || !ws->part_arg)) return DR_E_ARG;
  if (reinterpret_cast<uintptr_t>(ws->dz) % 16 != 0 || reinterpret_cast<uintptr_t>(ws->z) % 16 != 0) return DR_E_ARG;
  if (!store->cl0 || !store->t_rowptr || !store->t_col) return DR_E_ARG;
  if (n_batch == 0) return DR_OK;
  if (!store->x) return DR_E_ARG;
  DR_CHECK(dr_allow_big_lds(reinterpret_cast<const void*>(&ginet_large_ig_conv1_kernel)));
  DR_CHECK(dr_allow_big_lds(reinterpret_cast<const void*>(&ginet_large_ig_tail_kernel)));
  LargeArgs la;
  la.g.s = *store;
  la.g.w = *w;
  la.g.p = gp;
  la.g.descs = descs;
  la.g.B = n_batch;
  la.plan = *plan;
  IgTileArgs ia;
  ia.ig = *ig;
  ia.ws = *ws;
  hipStream_t st = (hipStream_t)stream;
  const int G = ig->n_groups, R = (ig->n_steps + G - 1) / G;  // the longest range of steps
  for (ia.round = 0; ia.round < R; ++ia.round) {
    hipLaunchKernelGGL(ginet_large_ig_conv1_kernel, dim3(plan->n_tiles, G), dim3(NTA), conv_lds_bytes, st, la, ia);
    hipLaunchKernelGGL(ginet_large_ig_tail_kernel, dim3(n_batch, G), dim3(NT), tail_lds_bytes, st, la, ia);
  }
  ia.round = 0;
  hipLaunchKernelGGL(ginet_large_ig_dx_kernel, dim3(plan->n_tiles, G), dim3(NTA), 0, st, la, ia);
  DR_CHECK((int)hipGetLastError());
  hipLaunchKernelGGL(ig_finish_kernel, dim3(n_batch), dim3(NTF), 0, st, la.g.s, descs, ia.ig);
  return (int)hipGetLastError();
}

extern "C" int dr_dropout_mask(uint64_t seed, uint64_t offset, int32_t n, float p, uint8_t* keep_host) {
  if (n < 0 || (n > 0 && !keep_host)) return DR_E_ARG;
  for (int i = 0; i < n; ++i) keep_host[i] = dr_uniform(seed, offset, (uint32_t)i) >= p ? 1 : 0;
  return DR_OK;
}

// ---- carve descriptions for the host-side carve tests (tests/test_lds_carves.py)
static void describe_carve(DrCarveDesc& d, const Carve& c) {
  DR_DESC_P(d, c, KP);
  DR_DESC_P(d, c, LDW);
  DR_DESC_P(d, c, XS);
  DR_DESC(d, c, w1);
  DR_DESC(d, c, w2);
  DR_DESC(d, c, fc2);
  DR_DESC(d, c, x);
  DR_DESC(d, c, z);
  DR_DESC(d, c, rp);
  DR_DESC(d, c, col);
  DR_DESC(d, c, cl0);
  DR_DESC(d, c, key);
  DR_DESC(d, c, p1);
  DR_DESC(d, c, a1);
  DR_DESC(d, c, dp1);
  DR_DESC(d, c, y2);
  DR_DESC(d, c, h2);
  DR_DESC(d, c, p1rp);
  DR_DESC(d, c, p1c);
  DR_DESC(d, c, p1trp);
  DR_DESC(d, c, p1tc);
  DR_DESC(d, c, m1p);
  DR_DESC(d, c, m1i);
  DR_DESC(d, c, p2);
  DR_DESC(d, c, nt);
  DR_DESC(d, c, cl1);
  DR_DESC(d, c, head);
  DR_DESC(d, c, dgp);
  DR_DESC(d, c, keep);
}

// q: N, E, F, K0, P1, K1, alias, OUT
extern "C" int dr_debug_carve_ginet(const int32_t* q, char* buf, int32_t len) {
  const Carve c = carve(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]);
  DrCarveDesc d{buf, len, 0};
  describe_carve(d, c);
  DR_DESC(d, c, total);
  return d.pos;
}

// the Z-input form; q: N, E, F, K0, P1, K1, alias, OUT, zs (> 0)
extern "C" int dr_debug_carve_ginet_z(const int32_t* q, char* buf, int32_t len) {
  const Carve c = carve(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]);
  DrCarveDesc d{buf, len, 0};
  describe_carve(d, c);
  DR_DESC(d, c, total);
  return d.pos;
}

// The prefetch layout of the batch maxima and one graph's carve inside it.
// q: N, E, F, K0, P1, K1, alias, OUT, then the maxima Nm, Em, K0m, P1m, K1m,
// the parity and zs (0: gather form).  "total": the layout's; "$end": where
// the graph's own walk of the scratch segment ends.
extern "C" int dr_debug_carve_ginet_acc(const int32_t* q, char* buf, int32_t len) {
  const AccLayout L = acc_layout(q[8], q[9], q[2], q[10], q[11], q[12], q[6], q[7], q[14]);
  const Carve c = carve_acc(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], L, q[13], q[14]);
  DrCarveDesc d{buf, len, 0};
  describe_carve(d, c);
  dr_carve_put(d, "$in0", L.in0);
  dr_carve_put(d, "$in1", L.in1);
  dr_carve_put(d, "$scr", L.scr);
  dr_carve_put(d, "$end", c.total);
  dr_carve_put(d, "$acc_words", acc_words(q[2], q[7], q[2] > 32));
  DR_DESC(d, L, total);
  return d.pos;
}

// the input-gradient kernel's LDS: the per-graph carve and the transposed CSR;
// q: N, E, F, K0, P1, K1, alias, OUT, zs (0: gather form)
extern "C" int dr_debug_carve_ginet_ig(const int32_t* q, char* buf, int32_t len) {
  const Carve c = carve(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]);
  const IgLds g = ig_lds(c, q[0], q[1], q[8]);
  DrCarveDesc d{buf, len, 0};
  describe_carve(d, c);
  DR_DESC(d, g, trp);
  DR_DESC(d, g, tcol);
  dr_carve_put(d, "$carve_total", c.total);
  DR_DESC(d, g, total);
  return d.pos;
}

// the integrated-gradient kernel's LDS: the Z-form carve, the transposed CSR
// and the running dZ sum; q: N, E, F, K0, P1, K1, alias, OUT, zs (> 0)
extern "C" int dr_debug_carve_ginet_intgrad(const int32_t* q, char* buf, int32_t len) {
  const Carve c = carve(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]);
  const IntGradLds g = intgrad_lds(c, q[0], q[1], q[8]);
  DrCarveDesc d{buf, len, 0};
  describe_carve(d, c);
  DR_DESC(d, g, trp);
  DR_DESC(d, g, tcol);
  DR_DESC(d, g, dz);
  dr_carve_put(d, "$carve_total", c.total);
  DR_DESC(d, g, total);
  return d.pos;
}

extern "C" int dr_debug_xcd_tile(int32_t n_blocks, int32_t* tiles) {
  if (n_blocks < 0 || (n_blocks > 0 && !tiles)) return DR_E_ARG;
  for (int b = 0; b < n_blocks; ++b) tiles[b] = drk::xcd_tile_of(b, n_blocks);
  return DR_OK;
}

extern "C" int dr_debug_carve_ginet_conv(const int32_t* q, char* buf, int32_t len) {
  const ConvCarve c = conv_carve(q[0], q[1], q[2], q[3], q[4]);
  DrCarveDesc d{buf, len, 0};
  DR_DESC_P(d, c, KP);
  DR_DESC_P(d, c, LDW);
  DR_DESC_P(d, c, XS);
  DR_DESC(d, c, w1);
  DR_DESC(d, c, z);
  DR_DESC(d, c, h);
  DR_DESC(d, c, m0i);
  DR_DESC(d, c, m0p);
  DR_DESC(d, c, rng);
  DR_DESC(d, c, flg);
  DR_DESC(d, c, xh);
  DR_DESC(d, c, hid);
  DR_DESC(d, c, lcol);
  DR_DESC(d, c, trp);
  DR_DESC(d, c, total);
  return d.pos;
}

extern "C" int dr_debug_carve_ginet_conv_bf16(const int32_t* q, char* buf, int32_t len) {
  const ConvCarveB c = conv_carve_bf16(q[0], q[1], q[2], q[3], q[4]);
  DrCarveDesc d{buf, len, 0};
  DR_DESC_P(d, c, KPB);
  DR_DESC_P(d, c, ZSB);
  DR_DESC_P(d, c, XSB);
  DR_DESC(d, c, w1);
  DR_DESC(d, c, z);
  DR_DESC(d, c, h);
  DR_DESC(d, c, m0i);
  DR_DESC(d, c, m0p);
  DR_DESC(d, c, rng);
  DR_DESC(d, c, flg);
  DR_DESC(d, c, xh);
  DR_DESC(d, c, hid);
  DR_DESC(d, c, lcol);
  DR_DESC(d, c, trp);
  DR_DESC(d, c, total);
  return d.pos;
}

extern "C" int dr_debug_carve_ginet_tail(const int32_t* q, char* buf, int32_t len) {
  const TailCarve c = tail_carve(q[0], q[1], q[2], q[3], q[4]);
  DrCarveDesc d{buf, len, 0};
  DR_DESC(d, c, w2);
  DR_DESC(d, c, fc2);
  DR_DESC(d, c, p1);
  DR_DESC(d, c, a1);
  DR_DESC(d, c, dp1);
  DR_DESC(d, c, y2);
  DR_DESC(d, c, h2);
  DR_DESC(d, c, p1rp);
  DR_DESC(d, c, p1c);
  DR_DESC(d, c, p1trp);
  DR_DESC(d, c, p1tc);
  DR_DESC(d, c, m1p);
  DR_DESC(d, c, m1i);
  DR_DESC(d, c, p2);
  DR_DESC(d, c, nt);
  DR_DESC(d, c, cl1);
  DR_DESC(d, c, head);
  DR_DESC(d, c, dgp);
  DR_DESC(d, c, total);
  return d.pos;
}

// ---- the weight registers of the graph kernels (tests/test_ginet_weight_image_host.py,
// tests/test_gpu_ginet_weight_regs.py); debug entries, not part of the public header
namespace {

constexpr int WEIGHT_REGS_STRIDE = 49;  // per thread: fc1_row 8 | fc1_col 8 | fc1_bias | wa 16 | wb 16 (KPT = 32: 8 + 8 used)

// One workgroup runs the staging and loader helpers in graph_body's order
// (stage, request fc1, zero the pad, staging barrier, operands) and stores
// every thread's registers.  LDS: [w1 32F | image 1 024].
template <int KPT>
__global__ void __launch_bounds__(NT) ginet_weight_regs_kernel(dr_ginet_weights w, int F, float* out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr bool IMG = KPT == 32;
  constexpr int NKV = KPT / 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* sW1 = lds;
  float* sImg = lds + r4(32 * F);
  float fc1_row[8], fc1_col[8], fc1_bias;
  w1_stage<IMG>(sW1, sImg, w, F, tid);
  fc1_load(w, tid, wave, fc1_row, fc1_col, fc1_bias);
  w1_zero_pad<IMG>(sImg, F, tid);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  float wa[NKV], wb[NKV];
  w1_operands<KPT, IMG>(sW1, sImg, F, lane, wa, wb);
  float* o = out + (int64_t)tid * WEIGHT_REGS_STRIDE;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    o[j] = fc1_row[j];
    o[8 + j] = fc1_col[j];
  }
  o[16] = fc1_bias;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    o[17 + j] = j < NKV ? wa[j < NKV ? j : 0] : 0.f;
    o[33 + j] = j < NKV ? wb[j < NKV ? j : 0] : 0.f;
  }
}

}  // namespace

// out[word] = the element of the packed [W1; W1e] (32 rows of F) that image
// word `word` holds, or -1: zero (w1_image_src); n = 1 024 words.  Host only.
extern "C" int dr_debug_ginet_w1_image(int32_t F, int32_t* out, int32_t n) {
  if (F < 1 || F > 32 || !out || n != NT) return DR_E_ARG;
  for (int wd = 0; wd < n; ++wd) out[wd] = w1_image_src(F, wd);
  return DR_OK;
}

// out (device, NT x 49 floats; row t = thread t: fc1_row[8] | fc1_col[8] |
// fc1_bias | wa[16] | wb[16], the KPT / 4 registers of F's kernel, then zeros)
extern "C" int dr_debug_ginet_weight_regs(const dr_ginet_weights* w, int32_t F, float* out, int64_t n_out, void* stream) {
  if (!w || !out || F < 1 || F > 64 || n_out < (int64_t)NT * WEIGHT_REGS_STRIDE) return DR_E_ARG;
  const int lds_bytes = 4 * (r4(32 * F) + NT);
  if (F <= 32) hipLaunchKernelGGL((ginet_weight_regs_kernel<32>), dim3(1), dim3(NT), lds_bytes, (hipStream_t)stream, *w, F, out);
  else hipLaunchKernelGGL((ginet_weight_regs_kernel<64>), dim3(1), dim3(NT), lds_bytes, (hipStream_t)stream, *w, F, out);
  return (int)hipGetLastError();
}
