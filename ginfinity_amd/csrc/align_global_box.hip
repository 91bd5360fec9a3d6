// Global and query-in-target alignment inside a box of rows per pair (gfy_align_global_box,
// gfy_align_global_trace_box; semantics: include/gfy.h): the loop of align_local.inc with the
// mode bits kGlobal | kBox, once for the score kernel and once, with kTrace, for the path.  The
// box is the matrix: row -1 and column -1 of the definition are the rows just outside it, so a
// boxed call is the call without a box on rows i_lo .. i_hi of A and j_lo .. j_hi of B taken as
// two records of their own.  resolve_pair puts the box in the records' place (a row is 256 bytes,
// so any row can start a strip or a b-tile), the loop, the borders and the walk run on it
// unchanged, and finish_pair and trace_walk put the cells back into the records' coordinates.
// There is no band on these modes.  The trace takes the same boxes as the score call: its own
// box, rows 0 .. box rows - 1 and columns 0 .. end_j of the caller's box, starts at that box's
// corner.  The workspaces and their cut are those of the kernels without a box; what they have to
// hold is the widest box's columns and the largest box.
#include "align_local.inc"

namespace gfy {
namespace {

struct GlobalBoxArgs {
  AlignArgs align;
  int within;
};

struct GlobalTraceBoxArgs {
  AlignArgs align;
  TraceArgs trace;
  int32_t* out_start;   // [P][2]
  int within;
};

__global__ __launch_bounds__(kAlignThreads) void k_align_global_box(const GlobalBoxArgs p) {
  align_pairs<kGlobal | kBox>(p.align, nullptr, nullptr, p.within != 0);
}

__global__ __launch_bounds__(kAlignThreads) void k_align_global_trace_box(
    const GlobalTraceBoxArgs p) {
  align_pairs<kTrace | kGlobal | kBox>(p.align, p.out_start, &p.trace, p.within != 0);
}

}  // namespace

int launch_align_global_box(const AlignArgs& call, int within, void* ws, size_t ws_bytes,
                            hipStream_t s) {
  GlobalBoxArgs p{call, within};
  if (const int rc = align_take_carry<false>("gfy_align_global_box", &p.align, ws, ws_bytes))
    return rc;
  return align_launch<k_align_global_box>(p, align_groups(call.P), s);
}

int launch_align_global_trace_box(const AlignArgs& call, const TraceArgs& trace,
                                  int32_t* out_start, int within, int64_t max_box_rows,
                                  int64_t max_box_cols, void* ws, size_t ws_bytes, hipStream_t s) {
  GlobalTraceBoxArgs p{call, trace, out_start, within};
  if (const int rc = trace_take_workspace("gfy_align_global_trace_box", &p.align, &p.trace,
                                          max_box_rows, max_box_cols, ws, ws_bytes))
    return rc;
  // whole workgroups of the waves that have a part; the rest of the last one returns at once
  return align_launch<k_align_global_trace_box>(
      p, (int)((p.trace.waves + kAlignWaves - 1) / kAlignWaves), s);
}

}  // namespace gfy
