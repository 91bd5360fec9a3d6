// Record-to-record best-match scores over 128-d fp16 embeddings (gfy_pairwise_record_best,
// gfy_pairwise_record_scores; semantics: include/gfy.h): for every a-row the best pair inside
// every record of b, and the mean of those over the rows of every record of a, without ever
// writing the n x m matrix.
//
// The sweep is that of k_pairwise_topk (pairwise_topk.inc; told at the head of pairwise_topk.hip):
// 128 a-rows per workgroup (8 waves, 2 x 4, a wave holds 64 a-rows against 32 b-rows of every
// tile), b in 128-row tiles by LDS-DMA into the ring of four, two tiles per barrier, the next
// pair requested behind the first multiply, the a-row on the MFMA lane with 16 values per lane
// and a-row slot.  The pair's value g (maximised) is computed exactly as there and in the
// nearest-row kernel:  L2  g = a.b - |b|^2 / 2  out of the MFMAs,  cosine  g = -fma(a.b, -1/|b|, 0).
// What differs is the epilogue: instead of a k-deep list, ONE running maximum per lane and a-row
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

namespace gfy {
namespace {

constexpr int kBlockA = 128;  // a-rows per workgroup
constexpr int kTileB = 128;   // b-rows per LDS tile
constexpr int kThreads = 512;
constexpr int kBuffers = 4;   // b-tile ring: the pair being consumed and the pair in flight
constexpr int kRowBytes = kTileB * 256;        // one b-tile of rows
constexpr int kTermBytes = 2 * kTileB * 4;     // its (s, t)
constexpr int kTermSlots = 4;                  // (s, t) ring, like the rows
constexpr int kRecordLds = kBuffers * kRowBytes + kTermSlots * kTermBytes;
constexpr uint32_t kBelowAll = 0x007fffffu;    // ordered(-inf)

struct RecordArgs {
  const f16* a;
  const f16* b;
  const float* s;       // [m] padded to whole tiles (k_row_terms)
  const float* t;
  int64_t n, m;
  int blocks_a, chunks;
  int64_t chunk_rows;   // multiple of kTileB
  const int32_t* ptr_b; // [records_b + 1] running sums
  int records_b;
  uint32_t* bits;       // [records_b][n]: ordered(max g)
};

// COPIES of pairwise_topk.inc (which copies pairwise.hip), kept here so that the machine code of
// those kernels cannot move with this file: uniform_pointer, off256, the ring constants above,
// max16, and in the kernel the `request` and `multiply` lambdas and the loop around them.  A fix
// to the DMA addressing, to the swizzle or to the key forms there has to be made here too, and
// the other way round.
template <class T>
__device__ __forceinline__ const T* uniform_pointer(const T* pointer) {
  const uint64_t bits = (uint64_t)(uintptr_t)pointer;
  const uint32_t low = __builtin_amdgcn_readfirstlane((uint32_t)bits);
  const uint32_t high = __builtin_amdgcn_readfirstlane((uint32_t)(bits >> 32));
  return reinterpret_cast<const T*>(((uint64_t)high << 32) | low);
}

__device__ __forceinline__ int off256(int row, int chunk) {
  return row * 256 + ((chunk ^ (row & 15)) << 4);
}

__device__ __forceinline__ float max16(const f32x16& g) {
  float high = __builtin_fmaxf(g[0], g[1]);
#pragma unroll
  for (int q = 2; q < 16; q += 2)
    high = __builtin_fmaxf(__builtin_fmaxf(high, g[q]), g[q + 1]);   // v_max3_f32
  return high;
}

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

// fp32 -> uint32, monotone: x < y  <=>  ordered(x) < ordered(y) (no NaN comes out of the sweep)
__device__ __forceinline__ uint32_t ordered(float x) {
  const uint32_t u = __float_as_uint(x);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float unordered(uint32_t u) {
  return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xffffffffu));
}

// the value of k_nearest_finish for the maximum g of an (a-row, record) pair
__device__ __forceinline__ float value_of(uint32_t bits, float a_term, int metric) {
  const float g = unordered(bits);
  if (metric == GFY_L2) {
    const float d2 = a_term + -2.0f * g;   // -2 g: the key, exact
    return __builtin_sqrtf(d2 > 0.f ? d2 : 0.f);
  }
  return g * a_term;   // -key * a_term, key = -g
}

template <bool kFold>
__global__ __launch_bounds__(kThreads, 1) void k_record_sweep(const RecordArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int r = lane & 31, hq = lane >> 5;
  // wave owns a-rows [64wa, 64wa+64) and b-rows [32wb, 32wb+32) of each tile
  const int wa = wave & 1, wb = wave >> 1;
  const int chunk = blockIdx.x / p.blocks_a;
  const int block_a = blockIdx.x - chunk * p.blocks_a;
  const int64_t a0 = (int64_t)block_a * kBlockA;
  const int64_t j_begin = (int64_t)chunk * p.chunk_rows;
  const int64_t j_end = j_begin + p.chunk_rows < p.m ? j_begin + p.chunk_rows : p.m;

  // one b-tile -> its ring buffer, (s, t) -> the term ring.  A copy: see the note at
  // uniform_pointer — change all or none.
  auto request = [&](int k) __attribute__((always_inline)) {
    const int64_t j0 = j_begin + (int64_t)k * kTileB;
    const uint32_t base = lds0 + (uint32_t)(k & (kBuffers - 1)) * kRowBytes;
    const f16* rows = uniform_pointer(p.b + j0 * 128);
    uint32_t me = threadIdx.x;
    asm volatile("" : "+v"(me));
    const uint32_t sub = (me >> 4) & 3u, slot = me & 15u;
    const uint32_t at_home = ((uint32_t)(16 * wave) + sub) * 256u + ((slot ^ sub) << 4);
    if (j0 + kTileB <= p.m) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        dma16(rows, (at_home ^ (uint32_t)(q << 6)) + 1024u * q,
              base + (uint32_t)(wave * 4 + q) * 1024u);
    } else {   // ragged last tile: rows past the end re-read the last row (their t never wins)
      const int last = (int)(p.m - 1 - j0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t full = (at_home ^ (uint32_t)(q << 6)) + 1024u * q;
        const int row = (int)(full >> 8);   // 16 wave + 4 q + sub
        const int from = row < last ? row : last;
        dma16(rows, (uint32_t)from * 256u + (full & 255u),
              base + (uint32_t)(wave * 4 + q) * 1024u);
      }
    }
    if (wave < (kFold ? 1 : 2) && (me & 32u) == 0)   // 128 floats = 32 lanes x 16 B
      dma16(uniform_pointer((wave == 0 && !kFold ? p.s : p.t) + j0), (me & 31u) * 16u,
            lds0 + kBuffers * kRowBytes + (uint32_t)(k & (kTermSlots - 1)) * kTermBytes
                + (uint32_t)(kFold ? 1 : wave) * (kTileB * 4));
  };

  // stage the a-block through LDS once (coalesced), then keep all its fragments in registers
  {
    char* atile = smem + kRowBytes;   // buffer 1 (32 KB), not yet in use
    for (int i = t; i < kBlockA * 16; i += kThreads) {
      const int row = i >> 4, ch = i & 15;
      f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (a0 + row < p.n) v = *reinterpret_cast<const f16x8*>(p.a + (a0 + row) * 128 + ch * 8);
      *reinterpret_cast<f16x8*>(atile + off256(row, ch)) = v;
    }
  }
  if (j_begin < j_end) request(0);
  __syncthreads();
  f16x8 af[2][8];
#pragma unroll
  for (int at = 0; at < 2; ++at)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
      af[at][ks] = *reinterpret_cast<const f16x8*>(
          smem + kRowBytes + off256(64 * wa + 32 * at + r, 2 * ks + hq));

  __syncthreads();   // the a-block has left buffer 1
  const int tiles = j_begin < j_end ? (int)((j_end - j_begin + kTileB - 1) / kTileB) : 0;
  if (tiles > 1) request(1);

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
  const int jw = 32 * wb + 4 * hq;   // first of this lane's b-rows inside a tile
  auto multiply = [&](int k) __attribute__((always_inline)) {
    const char* tile = smem + (k & (kBuffers - 1)) * kRowBytes;
    f32x16 start = {};   // what every chain starts from: 0, or (kFold) -|b_j|^2 / 2 of the lane's 16 b-rows
    if constexpr (kFold) {
      const float* u_l = reinterpret_cast<const float*>(
          smem + kBuffers * kRowBytes + (k & (kTermSlots - 1)) * kTermBytes) + kTileB;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 uv = *reinterpret_cast<const f32x4*>(u_l + jw + 8 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) start[4 * g + i] = uv[i];
      }
    }
    constexpr int kAheadK = 2, kRing = kAheadK + 1;
    f16x8 bf[kRing];   // [ks % kRing]
#pragma unroll
    for (int ks = 0; ks < kAheadK; ++ks)
      bf[ks] = *reinterpret_cast<const f16x8*>(tile + off256(32 * wb + r, 2 * ks + hq));
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      if (ks + kAheadK < 8)
        bf[(ks + kAheadK) % kRing] = *reinterpret_cast<const f16x8*>(
            tile + off256(32 * wb + r, 2 * (ks + kAheadK) + hq));
      __builtin_amdgcn_sched_barrier(0);   // operand reads stay ahead of their MFMAs (pairwise.hip)
#pragma unroll
      for (int at = 0; at < 2; ++at)
        acc[at] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bf[ks % kRing], af[at][ks],
                                                         ks == 0 ? start : acc[at], 0, 0, 0);
    }
  };

  // what happens to the products of tile k (still in acc)
  auto reduce = [&](int k) __attribute__((always_inline)) {
    const int j0 = (int)(j_begin + (int64_t)k * kTileB);
    const int tile_end = j0 + kTileB < (int)j_end ? j0 + kTileB : (int)j_end;
    const int jb = j0 + jw;
    const int w_lo = j0 + 32 * wb, w_hi = w_lo + 32;   // this wave's b-rows
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!kFold) {
      const float* s_l = reinterpret_cast<const float*>(
          smem + kBuffers * kRowBytes + (k & (kTermSlots - 1)) * kTermBytes);
      const float* t_l = s_l + kTileB;
#pragma unroll
      for (int at = 0; at < 2; ++at)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const f32x4 sv = *reinterpret_cast<const f32x4*>(s_l + jw + 8 * q4);
          const f32x4 tv = *reinterpret_cast<const f32x4*>(t_l + jw + 8 * q4);
          f32x4 a4;
#pragma unroll
          for (int i = 0; i < 4; ++i) a4[i] = acc[at][4 * q4 + i];
          const f32x4 key = __builtin_elementwise_fma(a4, sv, tv);   // the key of k_pairwise<false>
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[at][4 * q4 + i] = -key[i];
        }
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

  // Two tiles per barrier: the ring holds the pair being consumed and the pair in flight; the
  // next pair is requested behind the first multiply (pairwise.hip).
  for (int ti = 0; ti < tiles; ti += 2) {
    __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0): this wave's share of the pair
    asm volatile("" ::: "memory");
    __syncthreads();                             // everybody's share; the previous pair is spent
    multiply(ti);
    if (ti + 2 < tiles) request(ti + 2);
    if (ti + 3 < tiles) request(ti + 3);
    reduce(ti);
    if (ti + 1 < tiles) {
      multiply(ti + 1);
      reduce(ti + 1);
    }
  }
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

struct RecordWorkspace {
  float *s, *t, *a_term;
  uint32_t* bits;
  int blocks_a, chunks;
  int64_t chunk_rows;
  size_t bytes;
};

// Layout: s and t (tiles_b * 128 floats each), a_term (n floats), bits ([records_b][n] words),
// every array rounded up to 256 bytes.  The split of b into chunks is that of carve_topk
// (pairwise_topk.hip) — a copy, change both: enough workgroups for four per CU, and of the next
// few counts the one whose grid ends in the fewest sweeps.
RecordWorkspace carve_records(void* base, int64_t n, int64_t m, int64_t records_b) {
  RecordWorkspace w;
  w.blocks_a = (int)((n + kBlockA - 1) / kBlockA);
  const int64_t tiles_b = (m + kTileB - 1) / kTileB;
  int64_t chunks = (1024 + w.blocks_a - 1) / w.blocks_a;
  {
    constexpr int64_t kCus = 256;   // MI355X; another part only loses the fit
    const int64_t least = chunks;
    double best = 1e300;
    for (int64_t c = least; c < least + 6; ++c) {
      const double sweeps = (double)((w.blocks_a * c + kCus - 1) / kCus) / (double)c;
      if (sweeps < best * 0.99) best = sweeps, chunks = c;   // a later count only for a real gain
    }
  }
  if (chunks > tiles_b) chunks = tiles_b;
  if (chunks < 1) chunks = 1;
  const int64_t tiles_per_chunk = (tiles_b + chunks - 1) / chunks;
  w.chunk_rows = tiles_per_chunk * kTileB;
  w.chunks = (int)((tiles_b + tiles_per_chunk - 1) / tiles_per_chunk);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    void* ptr = base ? (char*)base + off : nullptr;
    off += align_up(bytes, 256);
    return ptr;
  };
  w.s = (float*)take((size_t)tiles_b * kTileB * 4);   // padded to whole tiles
  w.t = (float*)take((size_t)tiles_b * kTileB * 4);
  w.a_term = (float*)take((size_t)n * 4);
  w.bits = (uint32_t*)take((size_t)records_b * (size_t)n * 4);
  w.bytes = off;
  return w;
}

template <bool kFold>
int launch_sweep(const RecordArgs& p, hipStream_t s) {
  static_assert(kRecordLds <= 160 * 1024, "the LDS of a compute unit");
  static PerDeviceOnce opt_in;   // > 64 KB of dynamic LDS: once per device (gfy_common.h)
  if (const int rc = opt_in.run([]() -> int {
        GFY_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_record_sweep<kFold>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, kRecordLds));
        return GFY_OK;
      }))
    return rc;
  k_record_sweep<kFold><<<p.blocks_a * p.chunks, kThreads, kRecordLds, s>>>(p);
  return GFY_OK;
}

}  // namespace

size_t pairwise_record_workspace_bytes(int64_t n, int64_t m, int64_t records_b) {
  return carve_records(nullptr, n, m, records_b).bytes;
}

int pairwise_record_chunks(int64_t n, int64_t m) { return carve_records(nullptr, n, m, 1).chunks; }

// ptr_a == nullptr: out is best [n][records_b]; else out is scores [records_a][records_b]
int launch_pairwise_records(const void* a, int64_t n, const void* b, int64_t m, int metric,
                            const int32_t* ptr_a, int64_t records_a, const int32_t* ptr_b,
                            int64_t records_b, float* out, void* ws, size_t ws_bytes,
                            hipStream_t s) {
  const char* who = ptr_a ? "gfy_pairwise_record_scores" : "gfy_pairwise_record_best";
  const RecordWorkspace w = carve_records(ws, n, m, records_b);
  GFY_REQUIRE(ws_bytes >= w.bytes, GFY_ERR_WORKSPACE, "%s: workspace %zu < required %zu", who,
              ws_bytes, w.bytes);
  const int64_t padded_m = (m + kTileB - 1) / kTileB * kTileB;
  const bool fold = metric == GFY_L2;
  if (const int rc = launch_pairwise_row_terms(b, m, padded_m, metric, fold, w.s, w.t, nullptr, s))
    return rc;
  if (const int rc = launch_pairwise_row_terms(a, n, n, metric, 0, nullptr, nullptr, w.a_term, s))
    return rc;
  GFY_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)w.bits, (int)kBelowAll,
                                  (size_t)records_b * (size_t)n, s));
  RecordArgs p{};
  p.a = (const f16*)a;
  p.b = (const f16*)b;
  p.s = w.s;
  p.t = w.t;
  p.n = n;
  p.m = m;
  p.blocks_a = w.blocks_a;
  p.chunks = w.chunks;
  p.chunk_rows = w.chunk_rows;
  p.ptr_b = ptr_b;
  p.records_b = (int)records_b;
  p.bits = w.bits;
  if (const int rc = fold ? launch_sweep<true>(p, s) : launch_sweep<false>(p, s)) return rc;
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
