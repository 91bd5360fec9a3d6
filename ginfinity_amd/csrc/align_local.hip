// Batched local alignment of record pairs (gfy_align_local; semantics: include/gfy.h): Smith-
// Waterman with affine gaps (Gotoh) over the cosine of the records' rows, the Lq x Lr matrix of a
// pair never written to memory.  Our own definition, as the whole distance path's is: not the
// external aligner of the reference, whose scoring formula is nowhere in its tree.
//
// The kernel's body, and how a wave walks a pair, is align_local.inc; this file instantiates it
// without origins (kSpan = false: score and end), align_span.hip with them.
#include "align_local.inc"

namespace gfy {
namespace {

__global__ __launch_bounds__(kAlignThreads) void k_align_local(const AlignArgs p) {
  align_pairs<false>(p, nullptr);
}

}  // namespace

// two carry buffers of max_rows_b (H, F) pairs per wave of the grid
size_t align_workspace_bytes(int64_t pairs, int64_t max_rows_b) {
  return align_carry_bytes<false>(pairs, max_rows_b);
}

int launch_align_local(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                       const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                       const int32_t* pairs, int64_t P, float match_scale, float match_shift,
                       float gap_open, float gap_extend, float* out_score, int32_t* out_end,
                       void* ws, size_t ws_bytes, hipStream_t s) {
  return align_launch<false>(
      "gfy_align_local", reinterpret_cast<const void*>(k_align_local), a, n, ptr_a, records_a, b,
      m, ptr_b, records_b, pairs, P, match_scale, match_shift, gap_open, gap_extend, out_score,
      out_end, ws, ws_bytes, [s](int groups, const AlignArgs& p) {
        k_align_local<<<groups, kAlignThreads, kAlignLds, s>>>(p);
      });
}

}  // namespace gfy
