// Batched local alignment of record pairs (gfy_align_local; semantics: include/gfy.h): Smith-
// Waterman with affine gaps (Gotoh) over the cosine of the records' rows, the Lq x Lr matrix of a
// pair never written to memory.  Our own definition, as the whole distance path's is: not the
// external aligner of the reference, whose scoring formula is nowhere in its tree.
//
// The kernel's body, and how a wave walks a pair, is align_local.inc; this file instantiates it
// without origins (mode 0: score and end), align_span.hip with them.
#include "align_local.inc"

namespace gfy {
namespace {

__global__ __launch_bounds__(kAlignThreads) void k_align_local(const AlignArgs p) {
  align_pairs<0>(p, nullptr);
}

}  // namespace

// two carry buffers of max_rows_b (H, F) pairs per wave of the grid
size_t align_workspace_bytes(int64_t pairs, int64_t max_rows_b) {
  return align_carry_bytes<false>(pairs, max_rows_b);
}

int launch_align_local(const AlignArgs& call, void* ws, size_t ws_bytes, hipStream_t s) {
  AlignArgs p = call;
  if (const int rc = align_take_carry<false>("gfy_align_local", &p, ws, ws_bytes)) return rc;
  return align_launch<k_align_local>(p, align_groups(p.P), s);
}

}  // namespace gfy
