// The top-k sweep with an excluded range of b-rows per a-row (gfy_pairwise_topk_ranges): the
// kRanges = true instantiations of k_pairwise_topk (pairwise_topk.inc; the design and the cost of
// the range mode are told at the head of pairwise_topk.hip).  A translation unit of its own, so
// that pairwise_topk.hip holds the kernels it held before, unchanged.
#include "gfy_common.h"
#include "pairwise_topk.inc"

namespace gfy {

int launch_topk_sweep_ranges(const TopkArgs& p, bool fold, hipStream_t s) {
  return launch_topk_sweep<true>(p, fold, s);
}

}  // namespace gfy
