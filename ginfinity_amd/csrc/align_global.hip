// Global and query-in-target alignment of record pairs (gfy_align_global; semantics:
// include/gfy.h): the loop of align_local.inc in mode kGlobal.  The recurrences, the strips,
// the skew and the carry are the local aligner's; what differs is what lies outside the matrix
// (charged borders, iterated, and with `within` a free top border), that 0 is no candidate of the
// max, and where the score is read (the last cell, or the best of the last row).  The workspace
// is gfy_align_local's.
#include "align_local.inc"

namespace gfy {
namespace {

struct GlobalArgs {
  AlignArgs align;
  int within;
};

__global__ __launch_bounds__(kAlignThreads) void k_align_global(const GlobalArgs p) {
  align_pairs<kGlobal>(p.align, nullptr, nullptr, p.within != 0);
}

}  // namespace

int launch_align_global(const AlignArgs& call, int within, void* ws, size_t ws_bytes,
                        hipStream_t s) {
  GlobalArgs p{call, within};
  if (const int rc = align_take_carry<false>("gfy_align_global", &p.align, ws, ws_bytes)) return rc;
  return align_launch<k_align_global>(p, align_groups(call.P), s);
}

}  // namespace gfy
