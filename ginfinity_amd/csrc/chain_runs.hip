// Chains of diagonal runs across neighbouring diagonals (gfy_chain_runs_link, gfy_chain_runs_emit;
// semantics: include/gfy.h): the step between gfy_hit_runs_emit and the gfy_align_*_band calls
// that turns the pieces an insertion or deletion cuts a shared region into back into one seed.
//
// The caller sorts the runs by record pair (a stable sort, so that a pair's runs keep their order)
// and names the groups: `order` [runs] and `bounds` [groups + 1].
//   * Link (k_chain_link): one wave per record pair.  The wave first copies what it needs of its
//     runs (head cell, length, run index) into arrays indexed by the position inside the group;
//     these arrays, the scores and the two choices live in LDS when the group has at most
//     kChainLdsRuns runs and in the workspace otherwise, behind the same generic pointers, so
//     there is one loop for both.  Forward pass: t serial and ascending, the 64 lanes stride over
//     the earlier runs, a wave-wide arg-max over the total order (C, -|dd|, s) fixes pred[t] and
//     C[t].  Backward pass: the same loop descending, for succ[s] and D[s] (in C's storage: C is
//     not read again).  Runs of a group ascend in i, so a lane stops at the first run that lies
//     too far in front of (behind) t to link; `plain` scans them all, and the result is the same.
//     Then one lane per run: a run whose pred does not choose it back is a chain head; it walks
//     its chain serially, writes its own run index at every member, and the aggregates (count,
//     hits, float64 weight, end, min / max diagonal) at itself.  marks[s] is the count at a head
//     and 0 at every other run.
//   * The caller turns (marks > 0) into running sums: slots.
//   * Emit (k_chain_emit): one lane per run.  A head writes its chain's row at slots - 1; every
//     run writes the chain of its head to members.
// Whatever the arrays hold, no access leaves them and no loop runs on: every index read from
// memory (order, bounds, pred, succ, the heads, slots) is clipped or checked against the sizes of
// the call in front of its use, a walk only ever moves forward, and what does not fit sets
// *status.  Every store is an ordinary vector store or a vector atomic.
#include "seed_launch.h"

namespace gfy {
namespace {

constexpr int kChainWave = 64;          // one wave per workgroup: its barrier orders its own stores
constexpr int kChainEmitThreads = 256;
constexpr int kChainLdsRuns = 1024;     // 32 bytes per run: 32 KB of LDS
constexpr int kStatusOrder = 1;   // order, bounds or the links read back contradict the call
constexpr int kStatusSlots = 2;   // heads or slots do not number the chains 1..chains

struct ChainArgs {
  const int32_t* pairs;     // [runs][2]
  const int32_t* cells;     // [runs][2]
  const int32_t* lengths;   // [runs]
  const float* weights;     // [runs]
  int64_t runs;
  const int64_t* order;     // [runs]: the runs sorted by record pair, stable
  const int64_t* bounds;    // [groups + 1]: group g is order[bounds[g] .. bounds[g + 1])
  int64_t groups;
  int64_t max_gap, max_shift;
  int plain;
  int32_t* marks;           // [runs]: link writes, emit reads
  int32_t* status;
  // the workspace; by position in `order` (groups beyond kChainLdsRuns alone):
  int64_t* score;           // [runs] C, then D
  int32_t *row, *col, *len, *run, *pred, *succ;   // [runs] each
  // by run, written and read at the heads alone (head: at every run):
  double* sum;              // [runs]
  int32_t *hits, *head;     // [runs] each
  int32_t *end, *diag;      // [runs][2] each
  // emit
  const int64_t* slots;     // [runs] running sums of (marks > 0)
  int64_t chains;
  int32_t *out_pairs, *out_starts, *out_ends, *out_diagonals;   // [chains][2]
  int32_t *out_counts, *out_lengths;                           // [chains]
  float* out_weights;                                          // [chains]
  int32_t* out_members;                                        // [runs]
};

// The best of the wave's candidates (c, dd, s), s < 0 for none, in every lane: c descending, then
// dd ascending, then s descending (`later`) or ascending.  The order is total, s being distinct.
__device__ __forceinline__ void wave_best(int64_t& c, int64_t& dd, int32_t& s, bool later) {
  for (int offset = kChainWave / 2; offset; offset >>= 1) {
    const int64_t oc = __shfl_xor((long long)c, offset);
    const int64_t odd = __shfl_xor((long long)dd, offset);
    const int32_t os = __shfl_xor(s, offset);
    const bool take = os >= 0 && (s < 0 || oc > c ||
        (oc == c && (odd < dd || (odd == dd && (later ? os > s : os < s)))));
    if (take) {
      c = oc;
      dd = odd;
      s = os;
    }
  }
}

// Whether the run (is, js, ls) may precede the one at (it, jt); dd = |d_t - d_s| where it may.
__device__ __forceinline__ bool links(int64_t is, int64_t js, int64_t ls, int64_t it, int64_t jt,
                                      int64_t max_gap, int64_t max_shift, int64_t& dd) {
  const int64_t gi = it - (is + ls), gj = jt - (js + ls);
  if (gi < 0 || gj < 0 || (gi > gj ? gi : gj) > max_gap) return false;
  dd = gj > gi ? gj - gi : gi - gj;
  return dd <= max_shift;
}

__global__ __launch_bounds__(kChainWave) void k_chain_link(const ChainArgs p) {
  __shared__ int64_t lds_score[kChainLdsRuns];
  __shared__ int32_t lds_words[6][kChainLdsRuns];
  const int lane = threadIdx.x;
  int64_t lo = p.bounds[blockIdx.x], hi = p.bounds[blockIdx.x + 1];
  if ((lo < 0 || hi < lo || hi > p.runs) && lane == 0) atomicOr(p.status, kStatusOrder);
  lo = lo < 0 ? 0 : lo > p.runs ? p.runs : lo;
  hi = hi < lo ? lo : hi > p.runs ? p.runs : hi;
  const int32_t count = (int32_t)(hi - lo);   // runs < 2^31
  if (count == 0) return;
  const bool fits = count <= kChainLdsRuns;
  int64_t* score = fits ? lds_score : p.score + lo;
  int32_t* row = fits ? lds_words[0] : p.row + lo;
  int32_t* col = fits ? lds_words[1] : p.col + lo;
  int32_t* len = fits ? lds_words[2] : p.len + lo;
  int32_t* run = fits ? lds_words[3] : p.run + lo;
  int32_t* pred = fits ? lds_words[4] : p.pred + lo;
  int32_t* succ = fits ? lds_words[5] : p.succ + lo;

  // the group's runs by position; a run of another pair than the first one's contradicts `order`
  int64_t first = p.order[lo];
  first = first < 0 ? 0 : first >= p.runs ? p.runs - 1 : first;
  const int32_t q = p.pairs[2 * first], r = p.pairs[2 * first + 1];
  int32_t longest = 0;
  bool sound = true;
  for (int32_t k = lane; k < count; k += kChainWave) {
    int64_t s = p.order[lo + k];
    sound = sound && s >= 0 && s < p.runs;
    s = s < 0 ? 0 : s >= p.runs ? p.runs - 1 : s;
    sound = sound && p.pairs[2 * s] == q && p.pairs[2 * s + 1] == r;
    run[k] = (int32_t)s;
    row[k] = p.cells[2 * s];
    col[k] = p.cells[2 * s + 1];
    len[k] = p.lengths[s];
    longest = len[k] > longest ? len[k] : longest;
  }
  if (!sound) atomicOr(p.status, kStatusOrder);
  for (int offset = kChainWave / 2; offset; offset >>= 1) {
    const int32_t other = __shfl_xor(longest, offset);
    longest = other > longest ? other : longest;
  }
  __syncthreads();

  // forward: C[t] = L_t + max(0, max over s -> t of C[s]); ties: smallest |dd|, then largest s
  for (int32_t t = 0; t < count; ++t) {
    const int64_t it = row[t], jt = col[t];
    const int64_t nearest = it - p.max_gap - longest;   // a run that starts in front cannot link
    int64_t best = 0, best_dd = 0;
    int32_t best_s = -1;
    for (int32_t s = t - 1 - lane; s >= 0; s -= kChainWave) {
      const int64_t is = row[s];
      if (!p.plain && is < nearest) break;   // the runs ascend in i: nor can any in front of it
      int64_t dd;
      if (!links(is, col[s], len[s], it, jt, p.max_gap, p.max_shift, dd)) continue;
      const int64_t c = score[s];
      if (best_s < 0 || c > best || (c == best && dd < best_dd)) {   // s descends: first wins
        best = c;
        best_dd = dd;
        best_s = s;
      }
    }
    wave_best(best, best_dd, best_s, true);
    if (lane == 0) {
      score[t] = (int64_t)len[t] + (best_s < 0 ? 0 : best);
      pred[t] = best_s;
    }
    __syncthreads();   // C[t] in front of the next step's reads
  }

  // backward, the mirror image: D[s] = L_s + max(0, max over s -> t of D[t]); ties: smallest
  // |dd|, then smallest t
  for (int32_t s = count - 1; s >= 0; --s) {
    const int64_t is = row[s], js = col[s], ls = len[s];
    const int64_t farthest = is + ls + p.max_gap;   // a run that starts behind cannot link
    int64_t best = 0, best_dd = 0;
    int32_t best_t = -1;
    for (int64_t t = (int64_t)s + 1 + lane; t < count; t += kChainWave) {
      const int64_t it = row[t];
      if (!p.plain && it > farthest) break;   // the runs ascend in i: nor can any behind it
      int64_t dd;
      if (!links(is, js, ls, it, col[t], p.max_gap, p.max_shift, dd)) continue;
      const int64_t d = score[t];
      if (best_t < 0 || d > best || (d == best && dd < best_dd)) {   // t ascends: first wins
        best = d;
        best_dd = dd;
        best_t = (int32_t)t;
      }
    }
    wave_best(best, best_dd, best_t, false);
    if (lane == 0) {
      score[s] = ls + (best_t < 0 ? 0 : best);
      succ[s] = best_t;
    }
    __syncthreads();   // D[s] in front of the next step's reads
  }

  // a link is kept where both ends choose each other; a run without a kept predecessor is a head
  for (int32_t k = lane; k < count; k += kChainWave) {
    const int32_t own = run[k], before = pred[k];
    if (before >= k || before < -1) atomicOr(p.status, kStatusOrder);
    if (before >= 0 && before < k && succ[before] == k) {
      p.marks[own] = 0;   // inside a chain: its head counts it
      continue;
    }
    int32_t at = k, members = 0, low = 0, high = 0;
    int64_t hits = 0;
    double sum = 0.0;
    for (;;) {
      const int32_t s = run[at], diagonal = col[at] - row[at];
      p.head[s] = own;
      const double weight = (double)p.weights[s];
      sum = members ? sum + weight : weight;   // chain order, one rounded float64 addition each
      low = members && low < diagonal ? low : diagonal;
      high = members && high > diagonal ? high : diagonal;
      hits += len[at];
      ++members;
      const int32_t next = succ[at];
      if (next < 0) break;
      if (next <= at || next >= count) {   // a walk only moves forward, inside the group
        atomicOr(p.status, kStatusOrder);
        break;
      }
      if (pred[next] != at) break;
      at = next;
    }
    p.marks[own] = members;
    p.sum[own] = sum;
    p.hits[own] = (int32_t)hits;
    p.end[2 * (int64_t)own] = row[at] + len[at] - 1;
    p.end[2 * (int64_t)own + 1] = col[at] + len[at] - 1;
    p.diag[2 * (int64_t)own] = low;
    p.diag[2 * (int64_t)own + 1] = high;
  }
}

__global__ __launch_bounds__(kChainEmitThreads) void k_chain_emit(const ChainArgs p) {
  const int64_t s = (int64_t)blockIdx.x * kChainEmitThreads + threadIdx.x;
  if (s >= p.runs) return;
  const int64_t h = p.head[s];
  if (h < 0 || h > s || p.marks[h] <= 0) {   // a chain's head is its first run
    atomicOr(p.status, kStatusSlots);
    return;
  }
  const int64_t chain = p.slots[h] - 1;
  if (chain < 0 || chain >= p.chains) {
    atomicOr(p.status, kStatusSlots);
    return;
  }
  p.out_members[s] = (int32_t)chain;
  if (h != s) return;
  p.out_pairs[2 * chain] = p.pairs[2 * s];
  p.out_pairs[2 * chain + 1] = p.pairs[2 * s + 1];
  p.out_starts[2 * chain] = p.cells[2 * s];
  p.out_starts[2 * chain + 1] = p.cells[2 * s + 1];
  p.out_ends[2 * chain] = p.end[2 * s];
  p.out_ends[2 * chain + 1] = p.end[2 * s + 1];
  p.out_diagonals[2 * chain] = p.diag[2 * s];
  p.out_diagonals[2 * chain + 1] = p.diag[2 * s + 1];
  p.out_counts[chain] = p.marks[s];
  p.out_lengths[chain] = p.hits[s];
  p.out_weights[chain] = (float)p.sum[s];   // rounded to float32 once
}

// What both calls check, without a device, and the arguments they share.
int checked_chain_runs(const char* who, const int32_t* pairs, const int32_t* cells,
                       const int32_t* lengths, const float* weights, int64_t runs,
                       const int32_t* marks, int32_t* status, void* ws, size_t ws_bytes,
                       ChainArgs& p) {
  GFY_REQUIRE(pairs && cells && lengths && weights && marks && status && ws, GFY_ERR_INVALID,
              "%s: a pointer is NULL", who);
  GFY_REQUIRE(runs > 0 && runs < INT32_MAX, GFY_ERR_INVALID, "%s: runs = %lld outside 1..2^31 - 2",
              who, (long long)runs);
  GFY_REQUIRE(ws_bytes >= gfy_chain_runs_workspace_bytes(runs), GFY_ERR_WORKSPACE,
              "%s: workspace of %zu bytes, %zu needed", who, ws_bytes,
              gfy_chain_runs_workspace_bytes(runs));
  p.pairs = pairs;
  p.cells = cells;
  p.lengths = lengths;
  p.weights = weights;
  p.runs = runs;
  p.marks = const_cast<int32_t*>(marks);
  p.status = status;
  p.score = (int64_t*)ws;
  p.sum = (double*)(p.score + runs);
  int32_t* words = (int32_t*)(p.sum + runs);
  int32_t** const arrays[] = {&p.row, &p.col, &p.len, &p.run, &p.pred, &p.succ, &p.hits, &p.head};
  for (int32_t** const array : arrays) {
    *array = words;
    words += runs;
  }
  p.end = words;
  p.diag = words + 2 * runs;
  return GFY_OK;
}

}  // namespace
}  // namespace gfy

using namespace gfy;

size_t gfy_chain_runs_workspace_bytes(int64_t runs) {
  // two 8-byte and twelve 4-byte entries per run
  return align_up((size_t)(runs < 1 ? 1 : runs) * 64, 256);
}

int gfy_chain_runs_link(const int32_t* pairs, const int32_t* cells, const int32_t* lengths,
                        const float* weights, int64_t runs, const int64_t* order,
                        const int64_t* bounds, int64_t groups, int64_t max_gap, int64_t max_shift,
                        int plain, int32_t* marks, int32_t* status, void* ws, size_t ws_bytes,
                        void* stream) {
  const char* who = "gfy_chain_runs_link";
  clear_error();
  ChainArgs p{};
  if (const int rc = checked_chain_runs(who, pairs, cells, lengths, weights, runs, marks, status,
                                        ws, ws_bytes, p))
    return rc;
  GFY_REQUIRE(order && bounds, GFY_ERR_INVALID, "%s: a pointer is NULL", who);
  GFY_REQUIRE(groups > 0 && groups <= runs, GFY_ERR_INVALID, "%s: groups = %lld outside 1..runs",
              who, (long long)groups);
  GFY_REQUIRE(max_gap >= 0 && max_gap <= INT32_MAX && max_shift >= 0 && max_shift <= INT32_MAX,
              GFY_ERR_INVALID, "%s: max_gap = %lld or max_shift = %lld outside 0..2^31 - 1", who,
              (long long)max_gap, (long long)max_shift);
  p.order = order;
  p.bounds = bounds;
  p.groups = groups;
  p.max_gap = max_gap;
  p.max_shift = max_shift;
  p.plain = plain != 0;
  return seed_launch<k_chain_link>(p, (unsigned)groups, kChainWave, stream);
}

int gfy_chain_runs_emit(const int32_t* pairs, const int32_t* cells, const int32_t* lengths,
                        const float* weights, int64_t runs, const int32_t* marks,
                        const int64_t* slots, int64_t chains, int32_t* out_pairs,
                        int32_t* out_starts, int32_t* out_ends, int32_t* out_diagonals,
                        int32_t* out_counts, int32_t* out_lengths, float* out_weights,
                        int32_t* out_members, int32_t* status, void* ws, size_t ws_bytes,
                        void* stream) {
  const char* who = "gfy_chain_runs_emit";
  clear_error();
  ChainArgs p{};
  if (const int rc = checked_chain_runs(who, pairs, cells, lengths, weights, runs, marks, status,
                                        ws, ws_bytes, p))
    return rc;
  GFY_REQUIRE(slots && out_pairs && out_starts && out_ends && out_diagonals && out_counts &&
                  out_lengths && out_weights && out_members,
              GFY_ERR_INVALID, "%s: a pointer is NULL", who);
  GFY_REQUIRE(chains > 0 && chains <= runs, GFY_ERR_INVALID, "%s: chains = %lld outside 1..runs",
              who, (long long)chains);
  p.slots = slots;
  p.chains = chains;
  p.out_pairs = out_pairs;
  p.out_starts = out_starts;
  p.out_ends = out_ends;
  p.out_diagonals = out_diagonals;
  p.out_counts = out_counts;
  p.out_lengths = out_lengths;
  p.out_weights = out_weights;
  p.out_members = out_members;
  const unsigned grid = (unsigned)((runs + kChainEmitThreads - 1) / kChainEmitThreads);
  return seed_launch<k_chain_emit>(p, grid, kChainEmitThreads, stream);
}
