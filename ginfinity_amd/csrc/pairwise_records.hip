// Record-to-record best-match scores over 128-d fp16 embeddings (gfy_pairwise_record_best,
// gfy_pairwise_record_scores; semantics: include/gfy.h): for every a-row the best pair inside
// every record of b, and the mean of those over the rows of every record of a, without ever
// writing the n x m matrix.
//
// The sweep and the 128-row block are the shared ones of pairwise_sweep.inc (BlockFrame: 8
// waves, 2 x 4, a wave holds 64 a-rows against 32 b-rows of every tile), b in 128-row tiles by
// LDS-DMA into the ring of four, two tiles per barrier, the next pair requested behind the first
// multiply, the a-row on the MFMA lane with 16 values per lane and a-row slot.  The pair's value
// g (maximised) is computed exactly as in top-k and in the nearest-row kernel:  L2
// g = a.b - |b|^2 / 2  out of the MFMAs,  cosine  g = -fma(a.b, -1/|b|, 0) (cosine_key).
// What is here is the epilogue: instead of a k-deep list, ONE running maximum per lane and a-row
// slot, which belongs to the record of b the sweep is in.
//   * The records' boundaries (ptr_b, running sums) are the same for the whole workgroup: the
//     current record, its end and the next record's end are wave-uniform and live in SGPRs.
//   * A tile is cut at the record ends that fall into it.  Per segment a wave whose 32 b-rows lie
//     inside the segment takes max16 and one maximum per a-row slot; a wave that holds a
//     boundary masks its values outside the segment with one unsigned comparison each (the idiom
//     of the range exclusions); a wave whose rows miss the segment does nothing.
//   * At a record's end (and at the end of the workgroup's chunk) a wave that has seen rows of
//     the record flushes: the two lane halves are combined with one __shfl_xor so that lane L
//     holds the maximum of a-row 64 wa + L, g is mapped monotonically to a uint32, and ONE
//     integer atomic max per wave goes to bits[record][a-row] — 64 consecutive words.  The
//     maximum does not depend on the order of its operands, so the four b-waves, the chunks and
//     whatever order the hardware takes them in give the same bits; no [chunks] partials, no
//     merge in LDS and no barrier per record are needed.  bits is filled with the image of -inf
//     in front of the sweep, which is also what a record of zero rows keeps.
//   * Padded rows of the ragged last tile hold g = -inf (k_row_terms) and are masked besides
//     (every segment ends at m at the latest); their DMA re-reads the last row of b.
// ptr_b is only compared and used to step the record number, which stays inside [0, records_b):
// running sums that are none give unspecified values and no access outside the workspace.
//
// k_record_finish_best turns bits into the values of k_nearest_finish, transposed to [n][R];
// k_record_finish_scores sums them per (record of a, record of b) in float64 in ascending row
// order — one thread per pair, the values staged through LDS so that the reads of bits stay
// coalesced along the a-rows — divides by the record's rows and rounds to float32 once.
#include "gfy_common.h"
#include "pairwise_sweep.inc"

namespace gfy {
namespace {

constexpr uint32_t kBelowAll = 0x007fffffu;    // ordered(-inf)

struct RecordArgs : SweepArgs {
  const int32_t* ptr_b; // [records_b + 1] running sums
  int records_b;
  uint32_t* bits;       // [records_b][n]: ordered(max g)
};

// max16 over the lane's values whose b-row lies in [from, from + count): b-row of position q is
// jb + 8 (q >> 2) + (q & 3); one unsigned comparison since 0 <= from <= from + count < 2^31
__device__ __forceinline__ float max16_inside(const f32x16& g, int jb, int from, uint32_t count) {
  float high = -__builtin_inff();
#pragma unroll
  for (int q = 0; q < 16; ++q)
    high = __builtin_fmaxf(
        high, (uint32_t)(jb + 8 * (q >> 2) + (q & 3) - from) < count ? g[q] : -__builtin_inff());
  return high;
}

// the value of k_nearest_finish for the maximum g of an (a-row, record) pair: the key is -2 g (L2)
// or -g (cosine), both exact
__device__ __forceinline__ float value_of(uint32_t bits, float a_term, int metric) {
  const float g = unordered(bits);
  return pair_value(metric == GFY_L2 ? -2.0f * g : -g, a_term, metric);
}

template <bool kFold>
__global__ __launch_bounds__(kThreads, 1) void k_record_sweep(const RecordArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  const BlockFrame f = block_frame(p);
  const int lane = f.lane, r = f.r, hq = f.hq, wa = f.wa, wb = f.wb, tiles = f.tiles;
  const int64_t a0 = f.a0, j_begin = f.j_begin, j_end = f.j_end;

  auto request = [&](int k) __attribute__((always_inline)) {
    sweep_request<kFold>(p, lds0, f.wave, j_begin, k);
  };

  stage_a_block<kFrameA>(smem, p.a, p.n, a0);
  f16x8 af[2][8];
  load_block_fragments(af, smem, f, request);
  release_a_block(f, request);

  // The record the sweep is in: the first one that ends behind j_begin (records of zero rows in
  // front of it own nothing), found by bisection over the running sums; then its end and the
  // next record's end, one step ahead of their use.  All wave-uniform.
  // read through the constant address space: uniform addresses there are scalar loads, counted
  // by lgkmcnt — a vector load would be waited for with vmcnt(0), which drains the DMA look-ahead
  typedef const int32_t __attribute__((address_space(4))) * ConstantWords;
  const ConstantWords ptr_b = (ConstantWords)(uintptr_t)p.ptr_b;
  const int last_record = p.records_b - 1;
  int rec = 0, rec_end = 0x7fffffff, next_end = 0x7fffffff;
  if (tiles > 0) {
    int lo = 0, hi = last_record;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)ptr_b[mid + 1] > j_begin) hi = mid; else lo = mid + 1;
    }
    rec = __builtin_amdgcn_readfirstlane(lo);
    rec_end = rec < last_record ? ptr_b[rec + 1] : 0x7fffffff;
    next_end = rec + 1 < last_record ? ptr_b[rec + 2] : 0x7fffffff;
  }

  float cur[2] = {-__builtin_inff(), -__builtin_inff()};   // per a-row slot: best g of record `rec`
  bool dirty = false;   // wave-uniform: cur has seen rows of record `rec`

  // cur -> bits[record]: lane L ends up with the maximum of a-row 64 wa + L (slot hq, row r)
  auto flush = [&](int record) __attribute__((always_inline)) {
    const float mine = hq ? cur[1] : cur[0];
    const float got = __shfl_xor(hq ? cur[0] : cur[1], 32, 64);
    const int64_t i = a0 + 64 * wa + lane;
    if (i < p.n) atomicMax(p.bits + (int64_t)record * p.n + i, ordered(__builtin_fmaxf(mine, got)));
    cur[0] = cur[1] = -__builtin_inff();
  };

  f32x16 acc[2];   // [at]
  const int jw = f.jw;   // first of this lane's b-rows inside a tile
  auto multiply = [&](int k) __attribute__((always_inline)) {
    sweep_multiply<2, kFold>(acc, af, smem, k, wb, r, hq);
  };

  // what happens to the products of tile k (still in acc)
  auto reduce = [&](int k) __attribute__((always_inline)) {
    const int j0 = (int)(j_begin + (int64_t)k * kTileB);
    const int tile_end = j0 + kTileB < (int)j_end ? j0 + kTileB : (int)j_end;
    const int jb = j0 + jw;
    const int w_lo = j0 + 32 * wb, w_hi = w_lo + 32;   // this wave's b-rows
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!kFold) {   // both a-row slots ahead of the segments, which read either
#pragma unroll
      for (int at = 0; at < 2; ++at) cosine_key(acc[at], smem, k, jw);
    }
    int seg_lo = j0;
    for (;;) {   // the segments of the tile, wave-uniform
      const bool ends = rec_end <= tile_end;   // the record ends inside this tile or with it
      const int seg_hi = ends ? rec_end : tile_end;
      if (seg_lo < seg_hi && seg_lo < w_hi && seg_hi > w_lo) {
        dirty = true;
        if (seg_lo <= w_lo && seg_hi >= w_hi) {   // the wave's rows lie inside one record
#pragma unroll
          for (int at = 0; at < 2; ++at) cur[at] = __builtin_fmaxf(cur[at], max16(acc[at]));
        } else {
#pragma unroll
          for (int at = 0; at < 2; ++at)
            cur[at] = __builtin_fmaxf(
                cur[at], max16_inside(acc[at], jb, seg_lo, (uint32_t)(seg_hi - seg_lo)));
        }
      }
      if (!ends) break;
      if (dirty) flush(rec);
      dirty = false;
      seg_lo = seg_lo > rec_end ? seg_lo : rec_end;
      // rec < last_record here: the last record's end is held as 0x7fffffff and never reached
      rec = __builtin_amdgcn_readfirstlane(rec + 1);
      rec_end = next_end;
      next_end = rec + 1 < last_record ? ptr_b[rec + 2] : 0x7fffffff;
      if (seg_lo >= tile_end) break;
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  sweep_tile_pairs(tiles, multiply, request, reduce);
  if (dirty) flush(rec);   // the record that goes on behind the chunk, or the last one
}

// bits [R][n] -> best [n][R], the values of k_nearest_finish: 32 x 32 tiles through LDS so that
// both the reads (along the a-rows) and the stores (along the records) are coalesced
__global__ __launch_bounds__(256) void k_record_finish_best(const uint32_t* __restrict__ bits,
                                                            const float* __restrict__ a_term,
                                                            int64_t n, int records_b, int metric,
                                                            float* __restrict__ best) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t i0 = (int64_t)blockIdx.x * 32;
  const int r0 = blockIdx.y * 32;
  for (int rr = ty; rr < 32; rr += 8)
    if (r0 + rr < records_b && i0 + tx < n)
      tile[rr][tx] = value_of(bits[(int64_t)(r0 + rr) * n + i0 + tx], a_term[i0 + tx], metric);
  __syncthreads();
  for (int ii = ty; ii < 32; ii += 8)
    if (i0 + ii < n && r0 + tx < records_b)
      best[(i0 + ii) * records_b + r0 + tx] = tile[tx][ii];
}

// scores [Q][R]: workgroup (q, 64 records of b); the values of record q's rows go through LDS
// 64 rows at a time (read along the a-rows), thread r < 64 adds its record's in ascending row
// order in float64.  No atomics: the order is fixed.
__global__ __launch_bounds__(256) void k_record_finish_scores(
    const uint32_t* __restrict__ bits, const float* __restrict__ a_term,
    const int32_t* __restrict__ ptr_a, int64_t n, int records_b, int metric,
    float* __restrict__ scores) {
  __shared__ float tile[64][65];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t q = blockIdx.x;
  const int r0 = blockIdx.y * 64;
  int64_t lo = ptr_a[q], hi = ptr_a[q + 1];
  lo = lo < 0 ? 0 : lo > n ? n : lo;   // only running sums are promised; nothing is read outside bits
  hi = hi < lo ? lo : hi > n ? n : hi;
  double sum = 0.0;
  for (int64_t c = lo; c < hi; c += 64) {
    const int count = hi - c < 64 ? (int)(hi - c) : 64;
    if (lane < count) {
      const float at = a_term[c + lane];
      for (int rr = wave; rr < 64; rr += 4)
        if (r0 + rr < records_b)
          tile[rr][lane] = value_of(bits[(int64_t)(r0 + rr) * n + c + lane], at, metric);
    }
    __syncthreads();
    if (t < 64 && r0 + t < records_b)
      for (int x = 0; x < count; ++x) sum += (double)tile[t][x];
    __syncthreads();
  }
  if (t < 64 && r0 + t < records_b)
    scores[q * records_b + r0 + t] = (float)(sum / (double)(hi - lo));   // no rows: 0 / 0 = NaN
}

struct RecordWorkspace : SweepWorkspace {
  uint32_t* bits;
};

// Layout: the terms (pairwise_sweep.inc), then bits ([records_b][n] words)
RecordWorkspace carve_records(void* base, int64_t n, int64_t m, int64_t records_b) {
  RecordWorkspace w;
  Carver carver{base};
  w.split = split_b(n, m, kFrameA);
  carver.terms(n, m, w.s, w.t, w.a_term);
  w.bits = (uint32_t*)carver.take((size_t)records_b * (size_t)n * 4);
  w.bytes = carver.bytes;
  return w;
}

}  // namespace

size_t pairwise_record_workspace_bytes(int64_t n, int64_t m, int64_t records_b) {
  return carve_records(nullptr, n, m, records_b).bytes;
}

int pairwise_record_chunks(int64_t n, int64_t m) { return split_b(n, m, kFrameA).chunks; }

// ptr_a == nullptr: out is best [n][records_b]; else out is scores [records_a][records_b]
int launch_pairwise_records(const void* a, int64_t n, const void* b, int64_t m, int metric,
                            const int32_t* ptr_a, int64_t records_a, const int32_t* ptr_b,
                            int64_t records_b, float* out, void* ws, size_t ws_bytes,
                            hipStream_t s) {
  const char* who = ptr_a ? "gfy_pairwise_record_scores" : "gfy_pairwise_record_best";
  const RecordWorkspace w = carve_records(ws, n, m, records_b);
  RecordArgs p{};
  if (const int rc = begin_sweep(who, w, ws_bytes, a, n, b, m, metric, s, p)) return rc;
  const bool fold = metric == GFY_L2;
  GFY_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)w.bits, (int)kBelowAll,
                                  (size_t)records_b * (size_t)n, s));
  p.ptr_b = ptr_b;
  p.records_b = (int)records_b;
  p.bits = w.bits;
  const int grid = p.blocks_a * p.chunks;
  if (const int rc = fold ? launch_sweep<&k_record_sweep<true>, kSweepLds>(p, grid, s)
                          : launch_sweep<&k_record_sweep<false>, kSweepLds>(p, grid, s))
    return rc;
  if (ptr_a) {
    const dim3 grid((unsigned)records_a, (unsigned)((records_b + 63) / 64));
    k_record_finish_scores<<<grid, 256, 0, s>>>(w.bits, w.a_term, ptr_a, n, (int)records_b, metric,
                                                out);
  } else {
    const dim3 grid((unsigned)((n + 31) / 32), (unsigned)((records_b + 31) / 32));
    k_record_finish_best<<<grid, 256, 0, s>>>(w.bits, w.a_term, n, (int)records_b, metric, out);
  }
  GFY_CHECK_HIP(hipGetLastError());
  return GFY_OK;
}

}  // namespace gfy
