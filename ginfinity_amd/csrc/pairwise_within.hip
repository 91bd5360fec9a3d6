// Radius search over 128-d fp16 embeddings (gfy_pairwise_within_count, gfy_pairwise_within_fill;
// semantics: include/gfy.h): for every a-row EVERY b-row whose value passes a threshold, without
// ever writing the n x m matrix.  Two sweeps: one counts, the caller turns the counts into
// offsets, the other writes the hits into the segments the offsets describe.
//
// The sweep and the 128-row block are the shared ones of pairwise_sweep.inc (BlockFrame: 8
// waves, 2 x 4, a wave holds 64 a-rows against 32 b-rows of every tile), b in 128-row tiles by
// LDS-DMA into the ring of four, two tiles per barrier, the a-row on the MFMA lane with 16 values
// per lane and a-row slot.  The pair's g (maximised) is computed exactly as in top-k and the
// record scores:  L2  g = a.b - |b|^2 / 2  out of the MFMAs,  cosine  g = -fma(a.b, -1/|b|, 0)
// (cosine_key).  What is here is the epilogue.
//   * The predicate.  The value of a pair is value(g) = pair_value(-2 g or -g, a_term), and a
//     pair is a hit iff value <= threshold (L2) / value >= threshold (cosine).  value is
//     monotone in g for a fixed a-row — fp32 add, a product with a positive term and the
//     correctly rounded square root are — so  hit  <=>  g >= bound_i,  where bound_i is the
//     smallest fp32 g that passes.  k_within_bound finds it once per a-row by bisection over the
//     float's ordered bits, evaluating the very formula the fill writes values with; a row that
//     no g passes gets NaN, which no comparison satisfies.  g = -inf never passes a finite
//     threshold, so the padded rows of a ragged last tile (g = -inf, k_row_terms) and the zero
//     rows past n (bound NaN) are never hits.
//   * Count (k_within_count): per lane and a-row slot an integer count of the 16 values that
//     pass, kept in registers over the chunk; the lane halves are combined with one __shfl_xor
//     and ONE integer atomicAdd per wave goes to counts[a-row].  Integer sums do not depend on
//     order: no [chunks] partials, no merge.
//   * Fill (k_within_fill): a lane with c > 0 hits for an a-row in a tile reserves c slots with
//     one atomicAdd on the row's cursor and writes (b-row, value) for each into the row's
//     segment.  The segment is [offsets[i], offsets[i + 1]) clipped to [0, offsets[n]] and to
//     ascending order (row_segment); a hit whose slot lies past it is dropped and *status is
//     set, so no store ever leaves the segment whatever offsets holds.  The path is taken per
//     wave and tile only when a lane has a hit (one max16 and a ballot otherwise).
//   * Ranges (kRanges): the skip ranges of pairwise_sweep.inc — one unsigned comparison per
//     value, skipped wave-uniformly in the tiles that miss the union of the block's ranges.
//   * Order (k_within_order): the arrival order inside a segment is arbitrary, so one wave per
//     row sorts its segment by b-row, values moved along — up to 64 entries in registers, up to
//     kOrderLds in LDS, longer ones in place in global memory with the same network, which is
//     correct and not meant to be fast.  (a-row, b-row) pairs are unique, so the final bytes
//     are deterministic.  A row whose cursor differs from its segment's length (offsets that do
//     not come from this call's counts) sets *status as well.
// Every store is an ordinary vector store or a vector atomic.
#include "gfy_common.h"
#include "pairwise_sweep.inc"

namespace gfy {
namespace {

constexpr int kOrderLds = 2048;             // entries k_within_order sorts in LDS (16 KB)

struct WithinArgs : SweepArgs {
  const int32_t* skip_lo;   // kRanges: a-row i skips the b-rows [skip_lo[i], skip_hi[i]), [n] each
  const int32_t* skip_hi;
  const float* bound;   // [n]: the smallest g that is a hit (k_within_bound)
  const float* a_term;  // [n]
  int32_t* counts;      // count: [n], zeroed in front of the sweep
  const int64_t* offsets;   // fill: [n + 1]
  uint32_t* cursor;     // fill: [n] entries of the row's segment handed out, zeroed in front
  int32_t* indices;
  float* values;
  int32_t* status;
};

// what top-k reports for a pair whose sweep value is g: the key is -2 g (L2) or -g (cosine)
template <bool kFold>
__device__ __forceinline__ float value_of_g(float g, float a_term) {
  return pair_value(kFold ? -2.0f * g : -g, a_term, kFold ? GFY_L2 : GFY_COSINE);
}

template <bool kFold>
__device__ __forceinline__ bool passes(float g, float a_term, float threshold) {
  const float value = value_of_g<kFold>(g, a_term);
  return kFold ? value <= threshold : value >= threshold;
}

// bound[i]: the smallest g with passes(g), NaN when there is none.  passes(-inf) is false for
// every finite threshold and passes is monotone, so 32 steps over the ordered bits find it.
template <bool kFold>
__global__ __launch_bounds__(256) void k_within_bound(const float* __restrict__ a_term, int64_t n,
                                                      float threshold, float* __restrict__ bound) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float at = a_term[i];
  uint32_t lo = ordered(-__builtin_inff()), hi = ordered(__builtin_inff());
  if (!passes<kFold>(__builtin_inff(), at, threshold)) {
    bound[i] = __builtin_nanf("");
    return;
  }
  while (hi - lo > 1) {   // passes(lo) is false, passes(hi) true
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (passes<kFold>(unordered(mid), at, threshold)) hi = mid; else lo = mid;
  }
  bound[i] = unordered(hi);
}

// Row i's segment of the hit arrays as (first, length): [offsets[i], offsets[i + 1]) clipped to
// [0, offsets[n]] and to ascending order, so that whatever offsets holds, a segment lies inside
// the offsets[n] entries the caller says the arrays have.  The fill and the order kernel agree
// on it by calling this.
__device__ __forceinline__ void row_segment(const int64_t* offsets, int64_t n, int64_t i,
                                            int64_t& first, uint32_t& length) {
  int64_t total = offsets[n];
  total = total > 0 ? total : 0;
  int64_t lo = offsets[i], hi = offsets[i + 1];
  lo = lo < 0 ? 0 : lo > total ? total : lo;
  hi = hi < lo ? lo : hi > total ? total : hi;
  first = lo;
  length = hi - lo < 0x7fffffff ? (uint32_t)(hi - lo) : 0x7fffffffu;
}

template <bool kFold, bool kRanges, bool kFill>
__device__ __forceinline__ void within_sweep(const WithinArgs& p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  const BlockFrame f = block_frame(p);
  const int lane = f.lane, r = f.r, hq = f.hq, wa = f.wa, wb = f.wb;
  const int64_t a0 = f.a0, j_begin = f.j_begin;

  auto request = [&](int k) __attribute__((always_inline)) {
    sweep_request<kFold>(p, lds0, f.wave, j_begin, k);
  };

  stage_a_block<kFrameA>(smem, p.a, p.n, a0);
  int2* const ranges = skip_ranges(smem);
  if constexpr (kRanges) stage_skip_ranges(ranges, p.skip_lo, p.skip_hi, p, f);
  // the lane's two a-rows' bounds; a row past n gets NaN: never a hit
  float bound[2];
#pragma unroll
  for (int at = 0; at < 2; ++at) {
    const int64_t i = a0 + 64 * wa + 32 * at + r;
    bound[at] = i < p.n ? p.bound[i] : __builtin_nanf("");
  }
  f16x8 af[2][8];
  load_block_fragments(af, smem, f, request);
  SkipUnion skip;
  if constexpr (kRanges) skip = skip_union(ranges, lane);
  release_a_block(f, request);

  int hits[2] = {0, 0};   // count: per a-row slot, the lane's hits of the chunk
  bool dropped = false;   // fill: a hit of this lane did not fit its row's segment

  f32x16 acc[2];   // [at]
  const int jw = f.jw;   // first of this lane's b-rows inside a tile
  auto multiply = [&](int k) __attribute__((always_inline)) {
    sweep_multiply<2, kFold>(acc, af, smem, k, wb, r, hq);
  };

  // what happens to the products of tile k (still in acc)
  auto reduce = [&](int k) __attribute__((always_inline)) {
    const int64_t j0 = j_begin + (int64_t)k * kTileB;
    const bool may_skip = kRanges && skip.meets_tile(j0);
    const int jb = (int)(j0 + jw);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int at = 0; at < 2; ++at) {
      __builtin_amdgcn_sched_barrier(0);   // one a-row at a time: its terms are not read early
      f32x16& g = acc[at];   // in place: the products are spent
      if constexpr (!kFold) cosine_key(g, smem, k, jw);
      if (may_skip)   // block-uniform: the tiles under the block's own ranges
        mask_skip_range(g, ranges[64 * wa + 32 * at + r], jb);
      if constexpr (!kFill) {
        int c = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) c += g[q] >= bound[at] ? 1 : 0;
        hits[at] += c;
      } else {
        const bool any = max16(g) >= bound[at];
        if (__ballot(any)) {   // wave-uniform; rare at the thresholds a search is run with
          if (any) {           // bound is no NaN: the a-row lies in front of n
            const int64_t i = a0 + 64 * wa + 32 * at + r;
            int c = 0;
#pragma unroll
            for (int q = 0; q < 16; ++q) c += g[q] >= bound[at] ? 1 : 0;
            int64_t first;
            uint32_t length;
            row_segment(p.offsets, p.n, i, first, length);
            const float a_term = p.a_term[i];
            uint32_t slot = atomicAdd(p.cursor + i, (uint32_t)c);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              if (g[q] >= bound[at]) {
                if (slot < length) {
                  p.indices[first + slot] = jb + 8 * (q >> 2) + (q & 3);
                  p.values[first + slot] = value_of_g<kFold>(g[q], a_term);
                } else {
                  dropped = true;
                }
                ++slot;
              }
            }
          }
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  sweep_tile_pairs(f.tiles, multiply, request, reduce);

  if constexpr (!kFill) {
    // lane L ends up with the hits of a-row 64 wa + L (slot hq, row r)
    const int mine = hq ? hits[1] : hits[0];
    const int got = __shfl_xor(hq ? hits[0] : hits[1], 32, 64);
    const int64_t i = a0 + 64 * wa + lane;
    if (i < p.n && mine + got > 0) atomicAdd(p.counts + i, mine + got);
  } else {
    if (dropped) atomicOr(p.status, 1);
  }
}

template <bool kFold, bool kRanges>
__global__ __launch_bounds__(kThreads, 1) void k_within_count(const WithinArgs p) {
  within_sweep<kFold, kRanges, false>(p);
}

template <bool kFold, bool kRanges>
__global__ __launch_bounds__(kThreads, 1) void k_within_fill(const WithinArgs p) {
  within_sweep<kFold, kRanges, true>(p);
}

// The sorting network of k_within_order over `count` entries in memory, by one wave: a bitonic
// sort in the form whose every compare-exchange puts the smaller entry at the lower position
// (the first step of a merge mirrors, the others shift), so that the positions from `count` to
// the next power of two behave as entries that are larger than all and never move: a pair that
// reaches past `count` is left out.  key(i) is entry i's b-row, exchange(i, l) swaps two entries.
template <class Key, class Exchange>
__device__ __forceinline__ void order_in_memory(int count, int lane, Key&& key,
                                                Exchange&& exchange) {
  int padded = 2;
  while (padded < count) padded <<= 1;
  for (int width = 2; width <= padded; width <<= 1)
    for (int half = width >> 1; half > 0; half >>= 1) {
      const bool mirror = half == (width >> 1);
      for (int pair = lane; pair < (padded >> 1); pair += 64) {
        const int base = (pair / half) * 2 * half, off = pair % half;
        const int i = base + off;
        const int l = mirror ? base + 2 * half - 1 - off : i + half;
        if (l < count && key(i) > key(l)) exchange(i, l);
      }
      __syncthreads();   // one wave: the step's stores are seen by the next step's reads
    }
}

// One wave per a-row: its segment into ascending b-row order, values moved along.
__global__ __launch_bounds__(64) void k_within_order(const int64_t* offsets, const uint32_t* cursor,
                                                     int64_t n, int32_t* indices, float* values,
                                                     int32_t* status) {
  __shared__ uint64_t entries[kOrderLds];   // (b-row << 32) | the value's bits
  const int64_t i = blockIdx.x;
  const int lane = threadIdx.x;
  int64_t first;
  uint32_t length;
  row_segment(offsets, n, i, first, length);
  const uint32_t got = cursor[i];
  if (got != length && lane == 0) atomicOr(status, 1);   // offsets that are not this call's counts
  const int count = (int)(got < length ? got : length);
  if (count < 2) return;
  int32_t* idx = indices + first;
  float* val = values + first;
  if (count <= 64) {
    // in registers: an absent entry is larger than all
    uint64_t mine = ~0ull;
    if (lane < count) mine = ((uint64_t)(uint32_t)idx[lane] << 32) | __float_as_uint(val[lane]);
#pragma unroll
    for (int width = 2; width <= 64; width <<= 1)
#pragma unroll
      for (int half = width >> 1; half > 0; half >>= 1) {
        const int mask = half == (width >> 1) ? width - 1 : half;
        const uint64_t other = __shfl_xor((unsigned long long)mine, mask, 64);
        const bool low = (lane & half) == 0;   // the lower position of its pair: keeps the smaller
        mine = (other < mine) == low ? other : mine;
      }
    if (lane < count) {
      idx[lane] = (int32_t)(mine >> 32);
      val[lane] = __uint_as_float((uint32_t)mine);
    }
  } else if (count <= kOrderLds) {
    for (int e = lane; e < count; e += 64)
      entries[e] = ((uint64_t)(uint32_t)idx[e] << 32) | __float_as_uint(val[e]);
    __syncthreads();
    order_in_memory(
        count, lane, [&](int e) { return entries[e]; },
        [&](int e, int l) {
          const uint64_t keep = entries[e];
          entries[e] = entries[l];
          entries[l] = keep;
        });
    for (int e = lane; e < count; e += 64) {
      idx[e] = (int32_t)(entries[e] >> 32);
      val[e] = __uint_as_float((uint32_t)entries[e]);
    }
  } else {
    // longer than the LDS holds: the same network in place in global memory.  Correct and not
    // meant to be fast: about log2(count)^2 / 2 passes over the segment by one wave.
    volatile int32_t* vidx = idx;
    volatile float* vval = val;
    order_in_memory(
        count, lane, [&](int e) { return vidx[e]; },
        [&](int e, int l) {
          const int32_t keep_idx = vidx[e];
          const float keep_val = vval[e];
          vidx[e] = vidx[l];
          vval[e] = vval[l];
          vidx[l] = keep_idx;
          vval[l] = keep_val;
        });
  }
}

struct WithinWorkspace : SweepWorkspace {
  float* bound;
  uint32_t* cursor;
};

// Layout: the terms (pairwise_sweep.inc), then bound and cursor ([n] words each)
WithinWorkspace carve_within(void* base, int64_t n, int64_t m) {
  WithinWorkspace w;
  Carver carver{base};
  w.split = split_b(n, m, kFrameA);
  carver.terms(n, m, w.s, w.t, w.a_term);
  w.bound = (float*)carver.take((size_t)n * 4);
  w.cursor = (uint32_t*)carver.take((size_t)n * 4);
  w.bytes = carver.bytes;
  return w;
}

template <bool kFill>
int launch_within_sweep(const WithinArgs& p, bool fold, bool ranges, hipStream_t s) {
  const int grid = p.blocks_a * p.chunks;
  constexpr int kLds = kSweepLds + kRangeBytes;
  if constexpr (kFill) {
    if (ranges)
      return fold ? launch_sweep<&k_within_fill<true, true>, kLds>(p, grid, s)
                  : launch_sweep<&k_within_fill<false, true>, kLds>(p, grid, s);
    return fold ? launch_sweep<&k_within_fill<true, false>, kSweepLds>(p, grid, s)
                : launch_sweep<&k_within_fill<false, false>, kSweepLds>(p, grid, s);
  } else {
    if (ranges)
      return fold ? launch_sweep<&k_within_count<true, true>, kLds>(p, grid, s)
                  : launch_sweep<&k_within_count<false, true>, kLds>(p, grid, s);
    return fold ? launch_sweep<&k_within_count<true, false>, kSweepLds>(p, grid, s)
                : launch_sweep<&k_within_count<false, false>, kSweepLds>(p, grid, s);
  }
}

}  // namespace

size_t pairwise_within_workspace_bytes(int64_t n, int64_t m) {
  return carve_within(nullptr, n, m).bytes;
}

int pairwise_within_chunks(int64_t n, int64_t m) { return split_b(n, m, kFrameA).chunks; }

// counts != nullptr: the count; else the fill into (offsets, indices, values, status)
int launch_pairwise_within(const void* a, int64_t n, const void* b, int64_t m, int metric,
                           float threshold, const int32_t* skip_lo, const int32_t* skip_hi,
                           int32_t* counts, const int64_t* offsets, int32_t* indices,
                           float* values, int32_t* status, void* ws, size_t ws_bytes,
                           hipStream_t s) {
  const char* who = counts ? "gfy_pairwise_within_count" : "gfy_pairwise_within_fill";
  const WithinWorkspace w = carve_within(ws, n, m);
  WithinArgs p{};
  if (const int rc = begin_sweep(who, w, ws_bytes, a, n, b, m, metric, s, p)) return rc;
  const bool fold = metric == GFY_L2;
  const int bound_grid = (int)((n + 255) / 256);
  if (fold)
    k_within_bound<true><<<bound_grid, 256, 0, s>>>(w.a_term, n, threshold, w.bound);
  else
    k_within_bound<false><<<bound_grid, 256, 0, s>>>(w.a_term, n, threshold, w.bound);
  GFY_CHECK_HIP(hipGetLastError());
  p.skip_lo = skip_lo;
  p.skip_hi = skip_hi;
  p.bound = w.bound;
  p.a_term = w.a_term;
  p.counts = counts;
  p.offsets = offsets;
  p.cursor = w.cursor;
  p.indices = indices;
  p.values = values;
  p.status = status;
  if (counts) {
    GFY_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)n * 4, s));
    return launch_within_sweep<false>(p, fold, skip_lo != nullptr, s);
  }
  GFY_CHECK_HIP(hipMemsetAsync(w.cursor, 0, (size_t)n * 4, s));
  GFY_CHECK_HIP(hipMemsetAsync(status, 0, 4, s));
  if (const int rc = launch_within_sweep<true>(p, fold, skip_lo != nullptr, s)) return rc;
  k_within_order<<<(unsigned)n, 64, 0, s>>>(offsets, w.cursor, n, indices, values, status);
  GFY_CHECK_HIP(hipGetLastError());
  return GFY_OK;
}

}  // namespace gfy
