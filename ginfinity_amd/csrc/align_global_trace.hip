// The aligned path of a global or query-in-target alignment (gfy_align_global_trace; semantics:
// include/gfy.h): the loop of align_local.inc in mode kTrace | kGlobal.  The box is
// rows 0 .. L_q - 1 and columns 0 .. end_j of the pair's records, whose top-left corner is the
// matrix's own, so every value in it is the full matrix's by construction; the walk leaves it
// over a border and the border's ops are added behind it.  The workspace is cut as
// gfy_align_trace's is: per wave two carry buffers of (H, F) entries, then the direction words.
#include "align_local.inc"

namespace gfy {
namespace {

struct GlobalTraceArgs {
  AlignArgs align;
  TraceArgs trace;
  int32_t* out_start;   // [P][2]
  int within;
};

__global__ __launch_bounds__(kAlignThreads) void k_align_global_trace(const GlobalTraceArgs p) {
  align_pairs<kTrace | kGlobal>(p.align, p.out_start, &p.trace, p.within != 0);
}

}  // namespace

size_t align_global_trace_workspace_bytes(int64_t pairs, int64_t max_rows_a, int64_t max_rows_b) {
  return (size_t)align_groups(pairs) * kAlignWaves * trace_wave_bytes(max_rows_a, max_rows_b);
}

int launch_align_global_trace(const AlignArgs& call, const TraceArgs& trace, int32_t* out_start,
                              int within, int64_t max_rows_a, int64_t max_rows_b, void* ws,
                              size_t ws_bytes, hipStream_t s) {
  GlobalTraceArgs p{call, trace, out_start, within};
  if (const int rc = trace_take_workspace("gfy_align_global_trace", &p.align, &p.trace, max_rows_a,
                                          max_rows_b, ws, ws_bytes))
    return rc;
  // whole workgroups of the waves that have a part; the rest of the last one returns at once
  return align_launch<k_align_global_trace>(
      p, (int)((p.trace.waves + kAlignWaves - 1) / kAlignWaves), s);
}

}  // namespace gfy
