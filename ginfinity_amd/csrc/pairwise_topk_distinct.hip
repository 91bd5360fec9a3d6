// The top-k sweep with at most one hit per record of b (gfy_pairwise_topk_distinct; semantics:
// include/gfy.h): the kDistinct = true instantiations of k_pairwise_topk (pairwise_topk.inc; the sweep
// itself is told at the head of pairwise_topk.hip) and the merge of the chunks' lists that goes
// with them.  A translation unit of its own, so that pairwise_topk.hip and
// pairwise_topk_ranges.hip hold the kernels they held before, unchanged.
//
// b's rows lie in contiguous records; the record of b-row j is [group_lo[j], group_hi[j]).  A
// record's representative for an a-row is its first non-excluded row in the order (key, index);
// the result is the k best representatives.  Every list of the search — a lane's, a holder's, a
// chunk's, the final one — holds at most one entry per record, the best row of that record among
// the b-rows the list has seen:
//   * a list entry stays (g, index), two registers: an entry e lies in the candidate's record iff
//     (unsigned)(e.index - lo) < (unsigned)(hi - lo), lo and hi being the candidate's;
//   * (group_lo, group_hi) of a tile's 128 b-rows travel by LDS-DMA into a ring of four 1 KB
//     slots behind the ranges (LDS: 128 KB rows + 4 KB terms + 1 KB ranges + 4 KB = 137 KB of
//     160), and a lane reads a pair only for a candidate that has passed the cheap test (max16
//     against the lane's D-th best, then __ballot).  That test stays necessary: a row that is not
//     better than the D-th of D records' rows is none of the D best representatives;
//   * list_insert_distinct drops the candidate when its record has an entry at least as good, and
//     otherwise lets it take that entry's place in the order — one pass over the D positions.
//     Ties still go to the lowest index by strict comparison alone: inside a tile the maximum is
//     taken at its lowest position, across tiles a lane meets rows in ascending order;
//   * the merge of an a-row's eight holders and the merge of the chunks take the best head and
//     skip it when a column already holds a row of its record.  There the record of an index is
//     read from group_lo / group_hi in global memory: a record may straddle lanes, waves, tiles
//     and chunks.
// Exclusions are always ranges (the single-pair forms are ranges of one row); an empty range
// costs one uniform comparison per tile, as in pairwise_topk_ranges.hip.
//
// Depth D >= k per list is enough for an exact result.  Let x be the representative of record R
// and one of the k best representatives, and S any subset of b's rows that holds x.  A record
// whose best row in S beats x has a representative that beats x, so fewer than k records do: x
// is among the k <= D entries of S's list, and it is R's entry there (it is R's best row
// anywhere).  So every merge sees all k answers; a worse row of R out of another list comes
// behind x and is skipped.  And a column never holds a non-representative y of a record Q in
// front of Q's representative z: if z is one of the k best it is in a list and in front of y;
// if it is not, k representatives beat z and so y, all of them in the lists, and y is not among
// the first k.
//
// The group arrays are only ever compared (and indexed by row numbers the kernel made itself),
// never used as addresses: arrays that are no partition of [0, m) give unspecified columns and
// no access outside the caller's buffers.
#include "gfy_common.h"
#include "pairwise_topk.inc"

namespace gfy {
namespace {

// topk_finish (pairwise_topk.inc) for lists with one entry per record
__global__ __launch_bounds__(256) void k_topk_finish_distinct(
    const float* __restrict__ part_key, const int32_t* __restrict__ part_idx,
    const float* __restrict__ a_term, const int32_t* __restrict__ group_lo,
    const int32_t* __restrict__ group_hi, int64_t n, int chunks, int k, int metric,
    float* __restrict__ top_val, int32_t* __restrict__ top_idx) {
  topk_finish<true>(part_key, part_idx, a_term, group_lo, group_hi, n, chunks, k, metric, top_val,
                    top_idx);
}

}  // namespace

int launch_topk_sweep_distinct(const TopkArgs& p, bool fold, hipStream_t s) {
  return launch_topk_sweep<true, true>(p, fold, s);
}

int launch_topk_finish_distinct(const TopkArgs& p, const float* a_term, int metric, float* top_val,
                                int32_t* top_idx, hipStream_t s) {
  k_topk_finish_distinct<<<(int)((p.n + 255) / 256), 256, 0, s>>>(
      p.part_key, p.part_idx, a_term, p.group_lo, p.group_hi, p.n, p.chunks, p.k, metric, top_val,
      top_idx);
  GFY_CHECK_HIP(hipGetLastError());
  return GFY_OK;
}

}  // namespace gfy
