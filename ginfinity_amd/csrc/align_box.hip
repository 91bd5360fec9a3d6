// Local alignment inside a box of rows per pair (gfy_align_local_box, gfy_align_local_span_box;
// semantics: include/gfy.h): the loop of align_local.inc with the mode bits kBand | kBox, once
// for the score kernel and once for the span kernel.  The box is the matrix, as the band is: a
// cell outside rows i_lo .. i_hi of the a-record or j_lo .. j_hi of the b-record is outside it.
// resolve_pair puts the box in the records' place (a row is 256 bytes, so any row can start a
// strip or a b-tile) and shifts the band into it, the loop runs on the box as on two records of
// their own, and finish_pair puts the cells back into the records' coordinates.  A call without a
// band has the covering one (a null `bands`), which is the call without a band bit for bit and
// saves two more instantiations.  The path needs no kernel of its own: start..end lies inside
// the box, so gfy_align_trace / gfy_align_trace_band on start..end walk it (include/gfy.h has the
// argument).  The workspaces and their cut are those of the unbanded kernels; what a carry buffer
// has to hold is the widest box's columns.
#include "align_local.inc"

namespace gfy {
namespace {

struct SpanBoxArgs {
  AlignArgs align;
  int32_t* out_start;   // [P][2]
};

__global__ __launch_bounds__(kAlignThreads) void k_align_local_box(const AlignArgs p) {
  align_pairs<kBand | kBox>(p, nullptr);
}

__global__ __launch_bounds__(kAlignThreads) void k_align_span_box(const SpanBoxArgs p) {
  align_pairs<kSpan | kBand | kBox>(p.align, p.out_start);
}

}  // namespace

int launch_align_local_box(const AlignArgs& call, void* ws, size_t ws_bytes, hipStream_t s) {
  AlignArgs p = call;
  if (const int rc = align_take_carry<false>("gfy_align_local_box", &p, ws, ws_bytes)) return rc;
  return align_launch<k_align_local_box>(p, align_groups(p.P), s);
}

int launch_align_local_span_box(const AlignArgs& call, int32_t* out_start, void* ws,
                                size_t ws_bytes, hipStream_t s) {
  SpanBoxArgs p{call, out_start};
  if (const int rc = align_take_carry<true>("gfy_align_local_span_box", &p.align, ws, ws_bytes))
    return rc;
  return align_launch<k_align_span_box>(p, align_groups(call.P), s);
}

}  // namespace gfy
