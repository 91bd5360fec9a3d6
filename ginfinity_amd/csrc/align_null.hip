// Null scores of local alignment (gfy_align_local_null; semantics: include/gfy.h): the loop of
// align_local.inc with the mode bits kBand | kBox | kOrder, once, score only.  Every pair is
// aligned `shuffles` times, and in run k column j of its matrix holds row order[j] of its b-side
// (the b-record, or the b-rows of its box) under the k-th of the pair's orders: the shuffled
// target is never written, an order entry is 4 bytes where the row it names is 256.  The kernel
// runs over the virtual pairs v = p * shuffles + k as the boxed score kernel runs over pairs: one
// wave per virtual pair, the same strips, multiply, recurrences, band and box arithmetic and tie
// rules; only resolve_pair (which order is mine, and is it one) and load_b (which row a column
// holds) know the mode.  A null `bands` is the covering band and a null `boxes` the covering box,
// so band, box, both or neither need no further instantiation.  Grid and carry are those of the
// score kernels for P * shuffles pairs.
#include "align_local.inc"

namespace gfy {
namespace {

struct NullArgs {
  AlignArgs align;    // P counts the virtual pairs
  OrderArgs orders;
};

__global__ __launch_bounds__(kAlignThreads) void k_align_local_null(const NullArgs p) {
  align_pairs<kBand | kBox | kOrder>(p.align, nullptr, nullptr, false, &p.orders);
}

}  // namespace

int launch_align_local_null(const AlignArgs& call, const OrderArgs& orders, void* ws,
                            size_t ws_bytes, hipStream_t s) {
  NullArgs p{call, orders};
  p.align.P = call.P * orders.shuffles;   // the entry point has checked that it fits
  if (const int rc = align_take_carry<false>("gfy_align_local_null", &p.align, ws, ws_bytes))
    return rc;
  return align_launch<k_align_local_null>(p, align_groups(p.align.P), s);
}

}  // namespace gfy
