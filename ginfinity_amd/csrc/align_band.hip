// Local alignment inside a band of diagonals per pair (gfy_align_local_band,
// gfy_align_local_span_band, gfy_align_trace_band; semantics: include/gfy.h): the loop of
// align_local.inc with the mode bit kBand, once for each of the three local kernels.  The band is
// the matrix: a cell whose diagonal j - i lies outside (lo, hi) is outside it, and the columns of
// a strip that hold no band cell are neither staged, multiplied nor stepped over (the loop bounds
// and the places where a band could go wrong are said in align_local.inc at the statements that
// deal with them).  Arguments, workspaces and their cut are those of the unbanded kernels.
#include "align_local.inc"

namespace gfy {
namespace {

struct SpanBandArgs {
  AlignArgs align;
  int32_t* out_start;   // [P][2]
};

struct TraceBandArgs {
  AlignArgs align;
  TraceArgs trace;
};

__global__ __launch_bounds__(kAlignThreads) void k_align_local_band(const AlignArgs p) {
  align_pairs<kBand>(p, nullptr);
}

__global__ __launch_bounds__(kAlignThreads) void k_align_span_band(const SpanBandArgs p) {
  align_pairs<kSpan | kBand>(p.align, p.out_start);
}

__global__ __launch_bounds__(kAlignThreads) void k_align_trace_band(const TraceBandArgs p) {
  align_pairs<kTrace | kBand>(p.align, nullptr, &p.trace);
}

}  // namespace

int launch_align_local_band(const AlignArgs& call, void* ws, size_t ws_bytes, hipStream_t s) {
  AlignArgs p = call;
  if (const int rc = align_take_carry<false>("gfy_align_local_band", &p, ws, ws_bytes)) return rc;
  return align_launch<k_align_local_band>(p, align_groups(p.P), s);
}

int launch_align_local_span_band(const AlignArgs& call, int32_t* out_start, void* ws,
                                 size_t ws_bytes, hipStream_t s) {
  SpanBandArgs p{call, out_start};
  if (const int rc = align_take_carry<true>("gfy_align_local_span_band", &p.align, ws, ws_bytes))
    return rc;
  return align_launch<k_align_span_band>(p, align_groups(call.P), s);
}

int launch_align_trace_band(const AlignArgs& call, const TraceArgs& trace, int64_t max_box_rows,
                            int64_t max_box_cols, void* ws, size_t ws_bytes, hipStream_t s) {
  TraceBandArgs p{call, trace};
  if (const int rc = trace_take_workspace("gfy_align_trace_band", &p.align, &p.trace,
                                          max_box_rows, max_box_cols, ws, ws_bytes))
    return rc;
  // whole workgroups of the waves that have a part; the rest of the last one returns at once
  return align_launch<k_align_trace_band>(p, (int)((p.trace.waves + kAlignWaves - 1) / kAlignWaves),
                                          s);
}

}  // namespace gfy
