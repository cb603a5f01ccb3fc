// The tile scaffold of the large-graph path (dr_large_plan): what the conv1
// tile kernels of GINet, bf16 GINet and FoutNet / SGAT and their per-graph
// tails do alike.  A tile kernel is, in order: tile_ctx, stage_pool_lists, its
// own weight staging, stage_halo_index + stage_halo_rows (with halos), its own
// gather and MFMA, tile_run_max over each cluster's member run, and its own
// store of the flagged rows to plan->z; a tail starts from decode_keys.
#pragma once

#include "graph_common.h"

namespace drk {

constexpr int NTA = 512;           // threads of a tile kernel: 8 waves
constexpr int TR = DR_LARGE_TILE;  // most rows of a tile (the LDS carves reserve this many)

typedef __attribute__((address_space(1))) unsigned long long gu64;

// Which tile this workgroup runs, and of which graph
struct TileCtx {
  int tile, b, t;   // the tile (XCD order), its graph's batch slot, its index within the graph
  dr_graph_desc d;  // the graph
  int N, K0;        // the graph's nodes and depth-0 clusters
  int r0, nrows;    // the tile's first row and its rows (< tile_rows in a graph's last tile)
};

__device__ __forceinline__ TileCtx tile_ctx(const dr_graph_desc* descs, const dr_large_plan& pl) {
  TileCtx x;
  x.tile = xcd_tile();
  x.b = pl.tile_slot[x.tile];
  x.t = x.tile - pl.tile_first[x.b];
  x.d = descs[x.b];
  x.N = x.d.n_nodes;
  x.K0 = x.d.n_k0;
  x.r0 = x.t * pl.tile_rows;
  x.nrows = min(pl.tile_rows, x.N - x.r0);
  return x;
}

// What the partial max reads besides H: the cluster member lists (DMA, no
// wait here) and the row flags, cleared.  With halos the plan holds this
// tile's members by cluster (host-built, runs from tile_mptr: "compact",
// returned); without, the whole graph's lists are staged and each cluster's
// run inside the tile is found by lower_bound_lds.
// Rows go to plan->z only at the tile's depth-0 pooling arg candidates, which
// sflag marks: the tail reads plan->z at the final args, and those are tile
// args.
__device__ __forceinline__ bool stage_pool_lists(const dr_graph_store& s, const dr_large_plan& pl, const TileCtx& x,
                                                 int* sm0i, int* sm0p, int* sflag) {
  for (int p = threadIdx.x; p < pl.tile_rows; p += NTA) sflag[p] = 0;
  const bool compact = pl.tile_members != nullptr;
  if (compact) {
    dma_copy<NTA, 4>(sm0i, pl.tile_members + (int64_t)x.tile * pl.tile_rows, x.nrows);
    dma_copy<NTA, 4>(sm0p, pl.tile_mptr + (int64_t)x.tile * (pl.k0_max + 1), x.K0 + 1);
  } else {
    dma_copy<NTA, 4>(sm0i, s.m0_idx + x.d.node0, x.N);
    dma_copy<NTA, 4>(sm0p, s.m0_ptr + x.d.k0 + x.d.gid, x.K0 + 1);
  }
  return compact;
}

// Halo staging, step (a): the tile's rowptr slice and its halo ids into LDS,
// waited for (with every DMA issued before) and visible to the workgroup.
struct TileHalo {
  int H;          // halo rows
  int ebase, ne;  // the tile's first CSR edge and its edge count
};

__device__ __forceinline__ TileHalo stage_halo_index(const dr_graph_store& s, const dr_large_plan& pl, const TileCtx& x,
                                                     int* strp, int* shid) {
  TileHalo h;
  const int h0 = pl.halo_off[x.tile];
  h.H = pl.halo_off[x.tile + 1] - h0;
  dma_copy<NTA, 4>(strp, s.rowptr + x.d.node0 + x.d.gid + x.r0, x.nrows + 1);
  dma_copy<NTA, 4>(shid, pl.halo_ids + h0, h.H);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  h.ebase = strp[0];
  h.ne = strp[x.nrows] - h.ebase;
  return h;
}

// Step (b): the tile's edges as halo indices and the halo's rows of X (the
// graph's rows of T, `stride` elements each, a multiple of 16 bytes) into LDS
// in 16-byte DMA lanes -- stride * sizeof(T) / 16 per row, fp32 or bf16 alike
// -- waited for and visible.  more_dma(): a kernel's own per-edge DMA (SGAT's
// edge weights), issued after the edges' and before the rows': the DMA issue
// order the kernel has always had.  lane, wave: threadIdx.x & 63 and >> 6.
// Whether a kernel hands in its own two or has them recomputed (the overload
// below) changes nothing but its register allocation, and these kernels are
// sensitive to that: with the SGAT gather's operands two registers lower its
// v_pk_fma reads all three from one VGPR bank (tile kernel 90.6 vs 88.2 us).
// Each caller uses the form in which it measured level with the code before
// the extraction (profiles/large_tile_refactor/bench_summary.txt): FoutNet,
// SGAT and fp32 GINet pass theirs, bf16 GINet does not.
template <class T, class MoreDma>
__device__ __forceinline__ void stage_halo_rows(const dr_large_plan& pl, const TileCtx& x, const TileHalo& h,
                                                const int* shid, uint16_t* slcol, const T* X, int stride, T* sXh,
                                                MoreDma more_dma, int lane, int wave) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 2, "fp32 or bf16 rows");
  constexpr int SH = sizeof(T) == 4 ? 2 : 3, PER = 1 << SH;  // elements per lane
  dma_copy<NTA, 16>(slcol, pl.lcol + pl.lcol_off[x.tile], (h.ne + 7) / 8);
  more_dma();
  {
    const int n16 = stride >> SH, tot = h.H * n16;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    for (int base = wv * 64; base < tot; base += NTA)
      if (base + lane < tot) {
        const int hr = (base + lane) / n16, q = base + lane - hr * n16;
        __builtin_amdgcn_global_load_lds(DRK_AS1(X + (int64_t)shid[hr] * stride + q * PER), DRK_AS3(sXh + base * PER), 16, 0, 0);
      }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}
template <class T>
__device__ __forceinline__ void stage_halo_rows(const dr_large_plan& pl, const TileCtx& x, const TileHalo& h,
                                                const int* shid, uint16_t* slcol, const T* X, int stride, T* sXh) {
  stage_halo_rows(pl, x, h, shid, slcol, X, stride, sXh, [] {}, threadIdx.x & 63, threadIdx.x >> 6);
}

// first position in the ascending run v[lo, hi) whose value is >= key
__device__ __forceinline__ int lower_bound_lds(const int* v, int lo, int hi, int key) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The tile's partial depth-0 max of channel ch of cluster k, over the
// cluster's members inside the tile, sm0i[mb, me) (ascending nodes; sH: the
// tile's H rows, CH channels each): strict '>' in node order, so the first
// max wins and NaN never enters (torch_scatter scatter_max,
// community_pooling.py:209).  The arg's row is flagged for the Z store.  With
// plan->part_key the result joins the graph's other tiles' by a 64-bit atomic
// max (order-free, see dr_large_plan.part_key; keys are 32 apart per cluster
// for every CH); without, the caller publishes the returned partial.
struct RunMax {
  float best;  // LOWEST: no member, or none that compares greater
  int arg;     // N then
};

template <int CH>
__device__ __forceinline__ RunMax tile_run_max(const dr_large_plan& pl, const TileCtx& x, const float* sH,
                                               const int* sm0i, int mb, int me, int k, int ch, int* sflag) {
  RunMax m = {LOWEST, x.N};
  for (int i_m = mb; i_m < me; ++i_m) {
    const int i = sm0i[i_m];
    const float v = sH[(i - x.r0) * CH + ch];
    if (v > m.best) {
      m.best = v;
      m.arg = i;
    }
  }
  if (m.arg < x.N) sflag[m.arg - x.r0] = 1;  // (benign race: every writer stores 1)
  if (pl.part_key && m.best > LOWEST)
    __hip_atomic_fetch_max((gu64*)(pl.part_key) + ((int64_t)x.b * pl.k0_max + k) * 32 + ch,
                           ((unsigned long long)__float_as_uint(m.best) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)m.arg),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return m;
}

// Tail, by its NTH threads: graph slot b's depth-0 pool from the tiles' keys
// (P1 / A1, K0 x CH; a key no tile raised: 0 and N), and the keys back to zero
// for the next pass.
template <int CH, int NTH>
__device__ __forceinline__ void decode_keys(const dr_large_plan& pl, int b, int K0, int N, float* P1, int* A1) {
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(pl.part_key) + (int64_t)b * pl.k0_max * 32;
  for (int p = threadIdx.x; p < K0 * CH; p += NTH) {
    unsigned long long* kp = keys + (p / CH) * 32 + p % CH;
    const unsigned long long key = *kp;
    *kp = 0ull;
    P1[p] = key ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
    A1[p] = key ? (int)(0xffffffffu - (uint32_t)key) : N;
  }
}

}  // namespace drk
