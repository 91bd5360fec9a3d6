// The aligned path of each pair (gfy_align_trace; semantics: include/gfy.h): the loop of
// align_local.inc with kTrace = true, run on the box start..end that gfy_align_local_span named.
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
  align_pairs<false, true>(p.align, nullptr, &p.trace);
}

int64_t trace_region_words(int64_t max_box_rows, int64_t max_box_cols) {
  return max_box_rows * ((max_box_cols + 7) / 8);
}

// two carry buffers of max_box_cols (H, F) entries and the direction words of the largest box
size_t trace_wave_bytes(int64_t max_box_rows, int64_t max_box_cols) {
  return align_up((size_t)2 * max_box_cols * sizeof(AlignCarry<false>) +
                      (size_t)trace_region_words(max_box_rows, max_box_cols) * 4 + 1, 256);
}

}  // namespace

size_t align_trace_workspace_bytes(int64_t pairs, int64_t max_box_rows, int64_t max_box_cols) {
  return (size_t)align_groups(pairs) * kAlignWaves * trace_wave_bytes(max_box_rows, max_box_cols);
}

int launch_align_trace(const AlignArgs& call, const TraceArgs& trace, int64_t max_box_rows,
                       int64_t max_box_cols, void* ws, size_t ws_bytes, hipStream_t s) {
  const size_t wave_bytes = trace_wave_bytes(max_box_rows, max_box_cols);
  GFY_REQUIRE(ws_bytes >= wave_bytes, GFY_ERR_WORKSPACE,
              "gfy_align_trace: workspace %zu < the %zu of one wave", ws_bytes, wave_bytes);
  const size_t fit = ws_bytes / wave_bytes, waves = (size_t)align_groups(call.P) * kAlignWaves;
  TraceKernelArgs p{call, trace};
  p.align.carry = ws;
  p.align.cap = (int)max_box_cols;
  p.trace.waves = (int64_t)(fit < waves ? fit : waves);
  p.trace.wave_bytes = (int64_t)wave_bytes;
  p.trace.region_words = trace_region_words(max_box_rows, max_box_cols);
  // whole workgroups of the waves that have a part; the rest of the last one returns at once
  return align_launch<k_align_trace>(p, (int)((p.trace.waves + kAlignWaves - 1) / kAlignWaves), s);
}

}  // namespace gfy
