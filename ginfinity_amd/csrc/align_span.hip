// Local alignment with start cells (gfy_align_local_span; semantics: include/gfy.h): the loop of
// align_local.inc in mode kSpan.  Next to H, E and F every lane carries the origin of each,
// the first matched cell of the path behind it, so a pair's (start, end) box comes out of the
// same sweep and the Lq x Lr matrix is still never written.  The workspace holds 16-byte carry
// entries (H, F and their origins), twice that of gfy_align_local.
#include "align_local.inc"

namespace gfy {
namespace {

struct SpanArgs {
  AlignArgs align;
  int32_t* out_start;   // [P][2]
};

__global__ __launch_bounds__(kAlignThreads) void k_align_span(const SpanArgs p) {
  align_pairs<kSpan>(p.align, p.out_start);
}

}  // namespace

size_t align_span_workspace_bytes(int64_t pairs, int64_t max_rows_b) {
  return align_carry_bytes<true>(pairs, max_rows_b);
}

int launch_align_local_span(const AlignArgs& call, int32_t* out_start, void* ws, size_t ws_bytes,
                            hipStream_t s) {
  SpanArgs p{call, out_start};
  if (const int rc = align_take_carry<true>("gfy_align_local_span", &p.align, ws, ws_bytes))
    return rc;
  return align_launch<k_align_span>(p, align_groups(call.P), s);
}

}  // namespace gfy
