// Maximal diagonal runs of radius-search hits (gfy_hit_runs_mark, gfy_hit_runs_emit; semantics:
// include/gfy.h): the seeding step between gfy_pairwise_within_fill and the banded alignment.
//
// One lane per hit.  The hits are sorted by a-row and, inside an a-row, by b-row, so everything a
// lane has to know is a binary search away:
//   * its a-row i: the segment of `offsets` that holds its position h;
//   * its records q, r: the first record that ends behind the row (a row at a boundary belongs to
//     the record that starts there, a record of zero rows owns nothing);
//   * whether a cell (i', j') is a hit, and where: j' in row i's segment of `indices`.
// No sort, no atomics on the results: a run is a fixed function of the hits and the counts.
//   * Mark (k_hit_runs_mark): a hit whose predecessor (i - 1, j - 1) is a hit inside the same two
//     records writes 0.  Any other hit is a head: it walks its diagonal forward, one binary search
//     per step, until a cell is no hit or either record ends, adds the values in float64 in that
//     order, and writes the length to marks[h] and the sum to the workspace.  The walk is serial:
//     a run of L hits is L steps of one lane.
//   * The caller turns (marks >= min_length) into running sums: slots.
//   * Emit (k_hit_runs_emit): a head with marks[h] >= min_length writes its record pair, its cell
//     inside the two records, its length and its sum rounded to float32 once at slots[h] - 1.
// Whatever the arrays hold, no access leaves them: every index read from memory is clipped or
// checked against the sizes of the call in front of its use, and what does not fit sets *status.
// Every store is an ordinary vector store or a vector atomic.
#include "seed_launch.h"

namespace gfy {
namespace {

constexpr int kRunThreads = 256;
constexpr int kStatusHits = 1;    // offsets, indices or the record pointers contradict the sizes
constexpr int kStatusSlots = 2;   // slots do not number the kept heads 1..runs

struct HitRunsArgs {
  const int64_t* offsets;   // [n + 1]
  const int32_t* indices;   // [hits]
  const float* values;      // [hits]
  const int32_t* ptr_a;     // [records_a + 1]
  const int32_t* ptr_b;     // [records_b + 1]
  int64_t n, m, hits;
  int records_a, records_b;
  int32_t* marks;           // [hits]: mark writes, emit reads
  double* sums;             // [hits], the workspace: written and read at the heads alone
  int32_t* status;
  const int64_t* slots;     // emit: [hits] running sums of (marks >= min_length)
  int64_t runs;
  int min_length;
  int32_t* out_pairs;       // [runs][2]
  int32_t* out_cells;       // [runs][2]
  int32_t* out_lengths;     // [runs]
  float* out_weights;       // [runs]
};

// The first record that ends behind `row`: records when there is none.
__device__ __forceinline__ int record_of_row(const int32_t* ptr, int records, int64_t row) {
  int lo = 0, hi = records;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)ptr[mid + 1] > row) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// Row `row`'s segment of the hits, clipped to [0, hits] and to ascending order; 0 <= row < n.
__device__ __forceinline__ void hit_segment(const HitRunsArgs& p, int64_t row, int64_t& lo,
                                            int64_t& hi) {
  lo = p.offsets[row];
  hi = p.offsets[row + 1];
  lo = lo < 0 ? 0 : lo > p.hits ? p.hits : lo;
  hi = hi < lo ? lo : hi > p.hits ? p.hits : hi;
}

// The position of the hit (row, col), -1 when the cell is none; 0 <= row < n.
__device__ __forceinline__ int64_t find_hit(const HitRunsArgs& p, int64_t row, int64_t col) {
  int64_t lo, end;
  hit_segment(p, row, lo, end);
  int64_t hi = end;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)p.indices[mid] < col) lo = mid + 1; else hi = mid;
  }
  return lo < end && (int64_t)p.indices[lo] == col ? lo : -1;
}

struct HitPlace {
  int64_t i, j;           // the rows of a and b
  int q, r;               // their records
  int64_t a_lo, a_hi;     // rows of record q: [a_lo, a_hi), clipped to [0, n]
  int64_t b_lo, b_hi;     // rows of record r: [b_lo, b_hi), clipped to [0, m]
};

// Where hit h lies; false (and *status) when the arrays contradict the sizes of the call.
__device__ __forceinline__ bool place_hit(const HitRunsArgs& p, int64_t h, HitPlace& at) {
  // the last row whose segment starts at or in front of h: offsets[i + 1] > h first holds at i
  int64_t lo = 0, hi = p.n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (p.offsets[mid + 1] > h) hi = mid; else lo = mid + 1;
  }
  bool ok = lo < p.n;
  if (ok) ok = p.offsets[lo] <= h && p.offsets[lo + 1] > h;
  at.i = lo;
  at.j = p.indices[h];
  ok = ok && at.j >= 0 && at.j < p.m;
  if (ok) {
    at.q = record_of_row(p.ptr_a, p.records_a, at.i);
    at.r = record_of_row(p.ptr_b, p.records_b, at.j);
    ok = at.q < p.records_a && at.r < p.records_b;
  }
  if (ok) {
    at.a_lo = p.ptr_a[at.q];
    at.a_hi = p.ptr_a[at.q + 1];
    at.b_lo = p.ptr_b[at.r];
    at.b_hi = p.ptr_b[at.r + 1];
    ok = at.a_lo >= 0 && at.a_lo <= at.i && at.b_lo >= 0 && at.b_lo <= at.j;
    at.a_hi = at.a_hi > p.n ? p.n : at.a_hi;
    at.b_hi = at.b_hi > p.m ? p.m : at.b_hi;
  }
  if (!ok) atomicOr(p.status, kStatusHits);
  return ok;
}

__global__ __launch_bounds__(kRunThreads) void k_hit_runs_mark(const HitRunsArgs p) {
  const int64_t h = (int64_t)blockIdx.x * kRunThreads + threadIdx.x;
  if (h >= p.hits) return;
  HitPlace at;
  if (!place_hit(p, h, at)) {
    p.marks[h] = 0;
    return;
  }
  if (at.i - 1 >= at.a_lo && at.j - 1 >= at.b_lo && find_hit(p, at.i - 1, at.j - 1) >= 0) {
    p.marks[h] = 0;   // inside a run: its head counts it
    return;
  }
  int32_t length = 1;
  double sum = (double)p.values[h];
  while (at.i + length < at.a_hi && at.j + length < at.b_hi) {
    const int64_t next = find_hit(p, at.i + length, at.j + length);
    if (next < 0) break;
    sum += (double)p.values[next];   // ascending t, one rounded float64 addition each
    ++length;
  }
  p.marks[h] = length;
  p.sums[h] = sum;
}

__global__ __launch_bounds__(kRunThreads) void k_hit_runs_emit(const HitRunsArgs p) {
  const int64_t h = (int64_t)blockIdx.x * kRunThreads + threadIdx.x;
  if (h >= p.hits) return;
  const int32_t length = p.marks[h];
  if (length < p.min_length) return;
  const int64_t s = p.slots[h] - 1;
  HitPlace at;
  if (s < 0 || s >= p.runs) {
    atomicOr(p.status, kStatusSlots);
    return;
  }
  if (!place_hit(p, h, at)) return;
  p.out_pairs[2 * s] = at.q;
  p.out_pairs[2 * s + 1] = at.r;
  p.out_cells[2 * s] = (int32_t)(at.i - at.a_lo);
  p.out_cells[2 * s + 1] = (int32_t)(at.j - at.b_lo);
  p.out_lengths[s] = length;
  p.out_weights[s] = (float)p.sums[h];   // rounded to float32 once
}

// What both calls check, without a device, and the arguments they share.
int checked_hit_runs(const char* who, const int64_t* offsets, int64_t n, const int32_t* indices,
                     const float* values, int64_t hits, const int32_t* ptr_a, int64_t records_a,
                     const int32_t* ptr_b, int64_t records_b, int64_t m, const int32_t* marks,
                     int32_t* status, void* ws, size_t ws_bytes, HitRunsArgs& p) {
  GFY_REQUIRE(offsets && indices && values && ptr_a && ptr_b && marks && status && ws,
              GFY_ERR_INVALID, "%s: a pointer is NULL", who);
  GFY_REQUIRE(n > 0 && n < INT32_MAX && m > 0 && m < INT32_MAX, GFY_ERR_INVALID,
              "%s: n = %lld or m = %lld outside 1..2^31 - 2", who, (long long)n, (long long)m);
  GFY_REQUIRE(hits > 0 && hits < INT32_MAX, GFY_ERR_INVALID, "%s: hits = %lld outside 1..2^31 - 2",
              who, (long long)hits);
  GFY_REQUIRE(records_a > 0 && records_a <= GFY_PAIRWISE_RECORDS_MAX && records_b > 0 &&
                  records_b <= GFY_PAIRWISE_RECORDS_MAX,
              GFY_ERR_INVALID, "%s: records_a = %lld or records_b = %lld outside 1..%d", who,
              (long long)records_a, (long long)records_b, GFY_PAIRWISE_RECORDS_MAX);
  GFY_REQUIRE(ws_bytes >= gfy_hit_runs_workspace_bytes(hits), GFY_ERR_WORKSPACE,
              "%s: workspace of %zu bytes, %zu needed", who, ws_bytes,
              gfy_hit_runs_workspace_bytes(hits));
  p.offsets = offsets;
  p.indices = indices;
  p.values = values;
  p.ptr_a = ptr_a;
  p.ptr_b = ptr_b;
  p.n = n;
  p.m = m;
  p.hits = hits;
  p.records_a = (int)records_a;
  p.records_b = (int)records_b;
  p.marks = const_cast<int32_t*>(marks);
  p.sums = (double*)ws;
  p.status = status;
  return GFY_OK;
}

}  // namespace
}  // namespace gfy

using namespace gfy;

size_t gfy_hit_runs_workspace_bytes(int64_t hits) {
  return align_up((size_t)(hits < 1 ? 1 : hits) * sizeof(double), 256);
}

int gfy_hit_runs_mark(const int64_t* offsets, int64_t n, const int32_t* indices,
                      const float* values, int64_t hits, const int32_t* ptr_a, int64_t records_a,
                      const int32_t* ptr_b, int64_t records_b, int64_t m, int32_t* marks,
                      int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  HitRunsArgs p{};
  if (const int rc = checked_hit_runs("gfy_hit_runs_mark", offsets, n, indices, values, hits,
                                      ptr_a, records_a, ptr_b, records_b, m, marks, status, ws,
                                      ws_bytes, p))
    return rc;
  const unsigned grid = (unsigned)((hits + kRunThreads - 1) / kRunThreads);
  return seed_launch<k_hit_runs_mark>(p, grid, kRunThreads, stream);
}

int gfy_hit_runs_emit(const int64_t* offsets, int64_t n, const int32_t* indices,
                      const float* values, int64_t hits, const int32_t* ptr_a, int64_t records_a,
                      const int32_t* ptr_b, int64_t records_b, int64_t m, const int32_t* marks,
                      const int64_t* slots, int min_length, int64_t runs, int32_t* out_pairs,
                      int32_t* out_cells, int32_t* out_lengths, float* out_weights,
                      int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "gfy_hit_runs_emit";
  clear_error();
  HitRunsArgs p{};
  if (const int rc = checked_hit_runs(who, offsets, n, indices, values, hits, ptr_a, records_a,
                                      ptr_b, records_b, m, marks, status, ws, ws_bytes, p))
    return rc;
  GFY_REQUIRE(slots && out_pairs && out_cells && out_lengths && out_weights, GFY_ERR_INVALID,
              "%s: a pointer is NULL", who);
  GFY_REQUIRE(min_length >= 1, GFY_ERR_INVALID, "%s: min_length = %d is not positive", who,
              min_length);
  GFY_REQUIRE(runs > 0 && runs <= hits, GFY_ERR_INVALID, "%s: runs = %lld outside 1..hits", who,
              (long long)runs);
  p.slots = slots;
  p.runs = runs;
  p.min_length = min_length;
  p.out_pairs = out_pairs;
  p.out_cells = out_cells;
  p.out_lengths = out_lengths;
  p.out_weights = out_weights;
  const unsigned grid = (unsigned)((hits + kRunThreads - 1) / kRunThreads);
  return seed_launch<k_hit_runs_emit>(p, grid, kRunThreads, stream);
}
