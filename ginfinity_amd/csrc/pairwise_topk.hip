// Exact top-k nearest rows over 128-d fp16 embeddings: the k best b-rows of every a-row, ordered
// by (key, b-row index), without ever writing the n x m matrix (semantics: include/gfy.h).
//
// The sweep is that of k_pairwise<false, ...> (pairwise.hip): a-fragments resident in registers,
// b in 128-row tiles by LDS-DMA into a ring of four buffers, the product taken as
// (B-tile) x (A-block)^T so the a-row sits on the MFMA lane, two tiles per barrier with the next
// pair requested behind the first multiply.  A k-deep list per a-row does not fit beside 128
// a-rows per wave (pairwise.hip is at the 256-register ceiling), so the block shape is its own:
//   * a workgroup (8 waves, 2 x 4) owns 128 a-rows; a wave holds 64 of them (64 fragment
//     registers, 32 accumulators) against 32 b-rows of every tile;
//   * per lane and a-row slot a list of D = 4 / 8 / 16 (g, index) pairs sorted by g descending
//     lives in registers; k is rounded up to a depth, the surplus columns are never stored.
// The pair's key is computed exactly as the nearest-row kernel computes it, so that column 0 IS
// its answer bit for bit:  L2  g = a.b - |b|^2 / 2  out of the MFMAs (the chain starts from
// -|b|^2 / 2 in the C operand),  cosine  g = -fma(a.b, -1/|b|, 0).  g is maximised; the key that
// leaves the kernel is -2 g (L2) or -g (cosine), both exact.
// A lane sees its b-rows in ascending index order, so "strictly greater" keeps the lowest index
// among equal keys at every insertion; every later merge compares (key, index).
// The cheap test stays in front of the list: v_max3 over the lane's 16 values against the
// lane's D-th best, then __ballot; the extract-and-insert loop runs only when a lane beats it.
// After the sweep the ring is free: 128 rows x 8 holders (2 lane halves x 4 b-waves) x D x 8 B
// (128 KB at D = 16) go there and one thread per a-row merges them.  The per-chunk lists go to
// the workspace as [chunks][n][k]; k_topk_finish merges the chunks and applies the value formulas
// of k_nearest_finish.
//
// Ranges (gfy_pairwise_topk_ranges; instantiated in pairwise_topk_ranges.hip from the same
// pairwise_topk.inc): every a-row skips a half-open range of b-rows, its own record in a
// record-sorted self-search.  The 128 ranges of a block are clipped to [0, m) at block set-up
// and stay in 1 KB of LDS behind the rings; their union is two SGPRs.  A tile that does not meet
// the union takes exactly the path above (one scalar comparison more); a tile that does sets, per
// a-row slot, the lane's values whose b-row lies in that a-row's range to -inf in front of
// max16 — two LDS words, 16 x (subtract, compare, select).  For record-sorted self-search that
// is the few tiles under the block's own records; for arbitrary ranges it may be every tile,
// which is correct and is not meant to be fast.
//
// One hit per record of b (gfy_pairwise_topk_distinct): the kDistinct instantiations and their
// finish kernel, told at the head of pairwise_topk_distinct.hip.
#include "gfy_common.h"
#include "pairwise_topk.inc"

namespace gfy {
namespace {

// one thread per a-row: the chunks' lists (each sorted by (key, index), chunks in ascending
// index order) into one, then the values of k_nearest_finish
__global__ __launch_bounds__(256) void k_topk_finish(const float* __restrict__ part_key,
                                                     const int32_t* __restrict__ part_idx,
                                                     const float* __restrict__ a_term, int64_t n,
                                                     int chunks, int k, int metric,
                                                     float* __restrict__ top_val,
                                                     int32_t* __restrict__ top_idx) {
  constexpr int D = GFY_PAIRWISE_TOPK_MAX;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float lk[D];   // -key, descending
  int li[D];
#pragma unroll
  for (int q = 0; q < D; ++q) {
    lk[q] = -__builtin_inff();
    li[q] = kNoIndex;
  }
  for (int c = 0; c < chunks; ++c) {
    const float* keys = part_key + ((int64_t)c * n + i) * k;
    const int32_t* idx = part_idx + ((int64_t)c * n + i) * k;
    for (int q = 0; q < k; ++q) {
      const float g = -keys[q];
      if (!(g > lk[D - 1])) break;   // sorted: nothing behind it gets in either
      list_insert<D>(lk, li, g, idx[q]);
    }
  }
  const float at = a_term[i];
#pragma unroll
  for (int q = 0; q < D; ++q) {
    if (q < k) {
      const float v = -lk[q];
      float out;
      if (metric == GFY_L2) {
        const float d2 = at + v;
        out = __builtin_sqrtf(d2 > 0.f ? d2 : 0.f);
      } else {
        out = -v * at;
      }
      top_val[i * k + q] = out;
      top_idx[i * k + q] = li[q] == kNoIndex ? -1 : li[q];
    }
  }
}

struct TopkWorkspace {
  float *s, *t, *a_term, *part_key;
  int32_t* part_idx;
  int blocks_a, chunks;
  int64_t chunk_rows;
  size_t bytes;
};

// Layout: s and t (tiles_b * 128 floats each), a_term (n floats), part_key and part_idx
// ([chunks][n][k] each), every array rounded up to 256 bytes.  chunks: enough workgroups for
// four per CU, and of the next few counts the one whose grid ends in the fewest sweeps (the
// reasoning of carve() in pairwise.hip, for 128-row a-blocks); it does not depend on k.
TopkWorkspace carve_topk(void* base, int64_t n, int64_t m, int k) {
  TopkWorkspace w;
  w.blocks_a = (int)((n + kBlockA - 1) / kBlockA);
  const int64_t tiles_b = (m + kTileB - 1) / kTileB;
  int64_t chunks = (1024 + w.blocks_a - 1) / w.blocks_a;
  {
    constexpr int64_t kCus = 256;   // MI355X; another part only loses the fit
    const int64_t least = chunks;
    double best = 1e300;
    for (int64_t c = least; c < least + 6; ++c) {
      const double sweeps = (double)((w.blocks_a * c + kCus - 1) / kCus) / (double)c;
      if (sweeps < best * 0.99) best = sweeps, chunks = c;   // a later count only for a real gain
    }
  }
  if (chunks > tiles_b) chunks = tiles_b;
  if (chunks < 1) chunks = 1;
  const int64_t tiles_per_chunk = (tiles_b + chunks - 1) / chunks;
  w.chunk_rows = tiles_per_chunk * kTileB;
  w.chunks = (int)((tiles_b + tiles_per_chunk - 1) / tiles_per_chunk);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    void* ptr = base ? (char*)base + off : nullptr;
    off += align_up(bytes, 256);
    return ptr;
  };
  w.s = (float*)take((size_t)tiles_b * kTileB * 4);   // padded to whole tiles
  w.t = (float*)take((size_t)tiles_b * kTileB * 4);
  w.a_term = (float*)take((size_t)n * 4);
  w.part_key = (float*)take((size_t)w.chunks * n * k * 4);
  w.part_idx = (int32_t*)take((size_t)w.chunks * n * k * 4);
  w.bytes = off;
  return w;
}

}  // namespace

size_t pairwise_topk_workspace_bytes(int64_t n, int64_t m, int k) {
  return carve_topk(nullptr, n, m, k).bytes;
}

int launch_pairwise_topk(const void* a, int64_t n, const void* b, int64_t m, int metric, int k,
                         int64_t exclude_offset, int exclude_on, const int32_t* skip_lo,
                         const int32_t* skip_hi, const int32_t* group_lo, const int32_t* group_hi,
                         float* top_val, int32_t* top_idx, void* ws, size_t ws_bytes,
                         hipStream_t s) {
  const TopkWorkspace w = carve_topk(ws, n, m, k);
  GFY_REQUIRE(ws_bytes >= w.bytes, GFY_ERR_WORKSPACE,
              "gfy_pairwise_topk: workspace %zu < required %zu", ws_bytes, w.bytes);
  const int64_t padded_m = (m + kTileB - 1) / kTileB * kTileB;
  const bool fold = metric == GFY_L2;
  if (const int rc = launch_pairwise_row_terms(b, m, padded_m, metric, fold, w.s, w.t, nullptr, s))
    return rc;
  if (const int rc = launch_pairwise_row_terms(a, n, n, metric, 0, nullptr, nullptr, w.a_term, s))
    return rc;
  TopkArgs p{};
  p.a = (const f16*)a;
  p.b = (const f16*)b;
  p.s = w.s;
  p.t = w.t;
  p.n = n;
  p.m = m;
  p.exclude_offset = exclude_offset;
  p.exclude_on = exclude_on;
  p.blocks_a = w.blocks_a;
  p.chunks = w.chunks;
  p.chunk_rows = w.chunk_rows;
  p.k = k;
  p.part_key = w.part_key;
  p.part_idx = w.part_idx;
  p.skip_lo = skip_lo;
  p.skip_hi = skip_hi;
  p.group_lo = group_lo;
  p.group_hi = group_hi;
  if (group_lo) {   // one hit per record of b: sweep and finish of pairwise_topk_distinct.hip
    if (const int rc = launch_topk_sweep_distinct(p, fold, s)) return rc;
    return launch_topk_finish_distinct(p, w.a_term, metric, top_val, top_idx, s);
  }
  int rc;
  if (skip_lo) rc = launch_topk_sweep_ranges(p, fold, s);   // per-row ranges: pairwise_topk_ranges.hip
  else if (k <= 4) rc = fold ? launch_sweep<4, true, false>(p, s) : launch_sweep<4, false, false>(p, s);
  else if (k <= 8) rc = fold ? launch_sweep<8, true, false>(p, s) : launch_sweep<8, false, false>(p, s);
  else rc = fold ? launch_sweep<16, true, false>(p, s) : launch_sweep<16, false, false>(p, s);
  if (rc) return rc;
  k_topk_finish<<<(int)((n + 255) / 256), 256, 0, s>>>(w.part_key, w.part_idx, w.a_term, n,
                                                        w.chunks, k, metric, top_val, top_idx);
  GFY_CHECK_HIP(hipGetLastError());
  return GFY_OK;
}

}  // namespace gfy
