// Local alignment with start cells (gfy_align_local_span; semantics: include/gfy.h): the loop of
// align_local.inc with kSpan = true.  Next to H, E and F every lane carries the origin of each,
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
  align_pairs<true>(p.align, p.out_start);
}

}  // namespace

size_t align_span_workspace_bytes(int64_t pairs, int64_t max_rows_b) {
  return align_carry_bytes<true>(pairs, max_rows_b);
}

int launch_align_local_span(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                            const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                            const int32_t* pairs, int64_t P, float match_scale, float match_shift,
                            float gap_open, float gap_extend, float* out_score,
                            int32_t* out_start, int32_t* out_end, void* ws, size_t ws_bytes,
                            hipStream_t s) {
  return align_launch<true>(
      "gfy_align_local_span", reinterpret_cast<const void*>(k_align_span), a, n, ptr_a, records_a,
      b, m, ptr_b, records_b, pairs, P, match_scale, match_shift, gap_open, gap_extend, out_score,
      out_end, ws, ws_bytes, [s, out_start](int groups, const AlignArgs& p) {
        k_align_span<<<groups, kAlignThreads, kAlignLds, s>>>(SpanArgs{p, out_start});
      });
}

}  // namespace gfy
