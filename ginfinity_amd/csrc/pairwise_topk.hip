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
// the workspace as [chunks][n][k]; k_topk_finish merges the chunks and applies pair_value, the
// value formula of k_nearest_finish.
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

// topk_finish (pairwise_topk.inc) for the plain lists
__global__ __launch_bounds__(256) void k_topk_finish(const float* __restrict__ part_key,
                                                     const int32_t* __restrict__ part_idx,
                                                     const float* __restrict__ a_term, int64_t n,
                                                     int chunks, int k, int metric,
                                                     float* __restrict__ top_val,
                                                     int32_t* __restrict__ top_idx) {
  topk_finish<false>(part_key, part_idx, a_term, nullptr, nullptr, n, chunks, k, metric, top_val,
                     top_idx);
}

struct TopkWorkspace : SweepWorkspace {
  float* part_key;
  int32_t* part_idx;
};

// Layout: the terms (pairwise_sweep.inc), then part_key and part_idx ([chunks][n][k] each); the
// split of b does not depend on k
TopkWorkspace carve_topk(void* base, int64_t n, int64_t m, int k) {
  TopkWorkspace w;
  Carver carver{base};
  w.split = split_b(n, m, kFrameA);
  carver.terms(n, m, w.s, w.t, w.a_term);
  w.part_key = (float*)carver.take((size_t)w.split.chunks * n * k * 4);
  w.part_idx = (int32_t*)carver.take((size_t)w.split.chunks * n * k * 4);
  w.bytes = carver.bytes;
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
  TopkArgs p{};
  if (const int rc = begin_sweep("gfy_pairwise_topk", w, ws_bytes, a, n, b, m, metric, s, p))
    return rc;
  const bool fold = metric == GFY_L2;
  p.exclude_offset = exclude_offset;
  p.exclude_on = exclude_on;
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
  // per-row ranges: the instantiations of pairwise_topk_ranges.hip
  if (const int rc = skip_lo ? launch_topk_sweep_ranges(p, fold, s)
                             : launch_topk_sweep<false>(p, fold, s))
    return rc;
  k_topk_finish<<<(int)((n + 255) / 256), 256, 0, s>>>(w.part_key, w.part_idx, w.a_term, n,
                                                        p.chunks, k, metric, top_val, top_idx);
  GFY_CHECK_HIP(hipGetLastError());
  return GFY_OK;
}

}  // namespace gfy
