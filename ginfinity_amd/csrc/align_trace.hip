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

int launch_align_trace(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                       const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                       const int32_t* pairs, int64_t P, float match_scale, float match_shift,
                       float gap_open, float gap_extend, const int32_t* starts,
                       const int32_t* ends, const int64_t* op_ptr, uint8_t* out_ops,
                       int32_t* out_len, int64_t max_box_rows, int64_t max_box_cols, void* ws,
                       size_t ws_bytes, hipStream_t s) {
  const size_t wave_bytes = trace_wave_bytes(max_box_rows, max_box_cols);
  GFY_REQUIRE(ws_bytes >= wave_bytes, GFY_ERR_WORKSPACE,
              "gfy_align_trace: workspace %zu < the %zu of one wave", ws_bytes, wave_bytes);
  const int groups = align_groups(P);
  const size_t fit = ws_bytes / wave_bytes;
  static PerDeviceOnce opt_in;
  if (const int rc = opt_in.run([]() -> int {
        GFY_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_align_trace),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, kAlignLds));
        return GFY_OK;
      }))
    return rc;
  TraceKernelArgs p{};
  p.align.a = (const f16*)a;
  p.align.b = (const f16*)b;
  p.align.ptr_a = ptr_a;
  p.align.ptr_b = ptr_b;
  p.align.pairs = pairs;
  p.align.n = n;
  p.align.m = m;
  p.align.P = P;
  p.align.records_a = (int)records_a;
  p.align.records_b = (int)records_b;
  p.align.match_scale = match_scale;
  p.align.match_shift = match_shift;
  p.align.gap_open = gap_open;
  p.align.gap_extend = gap_extend;
  p.align.carry = ws;
  p.align.cap = (int)max_box_cols;
  p.trace.starts = starts;
  p.trace.ends = ends;
  p.trace.op_ptr = op_ptr;
  p.trace.out_ops = out_ops;
  p.trace.out_len = out_len;
  p.trace.waves = (int64_t)(fit < (size_t)groups * kAlignWaves ? fit : (size_t)groups * kAlignWaves);
  p.trace.wave_bytes = (int64_t)wave_bytes;
  p.trace.region_words = trace_region_words(max_box_rows, max_box_cols);
  // whole workgroups of the waves that have a part; the rest of the last one returns at once
  const int launched = (int)((p.trace.waves + kAlignWaves - 1) / kAlignWaves);
  k_align_trace<<<launched, kAlignThreads, kAlignLds, s>>>(p);
  GFY_CHECK_HIP(hipGetLastError());
  return GFY_OK;
}

}  // namespace gfy
