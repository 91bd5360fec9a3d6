// The aligned path of each pair (gfy_align_trace; semantics: include/gfy.h): the loop of
// align_local.inc in mode kTrace, run on the box start..end that gfy_align_local_span named.
// The recurrences on the box alone take every cell of the chosen path to the value it has in the
// full matrix, so the walk back by the origin rules gives the same ops; the box's direction bits,
// 4 per cell, are the first thing proportional to L_q x L_r the library writes, per wave in
// flight and for the box only.  The workspace is cut into equal parts, one per wave: two carry
// buffers of (H, F) entries, then the direction words.
#include "align_local.inc"

namespace gfy {
namespace {

struct TraceKernelArgs {
  AlignArgs align;
  TraceArgs trace;
};

__global__ __launch_bounds__(kAlignThreads) void k_align_trace(const TraceKernelArgs p) {
  align_pairs<kTrace>(p.align, nullptr, &p.trace);
}

}  // namespace

size_t align_trace_workspace_bytes(int64_t pairs, int64_t max_box_rows, int64_t max_box_cols) {
  return (size_t)align_groups(pairs) * kAlignWaves * trace_wave_bytes(max_box_rows, max_box_cols);
}

int launch_align_trace(const AlignArgs& call, const TraceArgs& trace, int64_t max_box_rows,
                       int64_t max_box_cols, void* ws, size_t ws_bytes, hipStream_t s) {
  TraceKernelArgs p{call, trace};
  if (const int rc = trace_take_workspace("gfy_align_trace", &p.align, &p.trace, max_box_rows,
                                          max_box_cols, ws, ws_bytes))
    return rc;
  // whole workgroups of the waves that have a part; the rest of the last one returns at once
  return align_launch<k_align_trace>(p, (int)((p.trace.waves + kAlignWaves - 1) / kAlignWaves), s);
}

}  // namespace gfy
