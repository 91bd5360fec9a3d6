// The sweep of the exact top-k search: k_pairwise_topk<D, kFold, kRanges, kDistinct>, its
// launcher and the merge of the chunks' lists, topk_finish<kDistinct> (the design is told at the
// head of pairwise_topk.hip; the sweep, the cosine key and the mask of a skip range are those of
// pairwise_sweep.inc; the block geometry, the front of the kernel and the staging and union of
// the ranges are this kernel's own, as is its argument layout: told at the head of that file).
// Included by the three translation units that instantiate it: pairwise_topk.hip (kRanges =
// false: one excluded pair per a-row at most), pairwise_topk_ranges.hip (kRanges = true: an
// excluded range of b-rows per a-row) and pairwise_topk_distinct.hip (kDistinct = true: at most
// one hit per record of b, told at its head), so that the device code of the one does not move
// with the others.
#include "pairwise_sweep.inc"

namespace gfy {

struct TopkArgs {
  const f16* a;
  const f16* b;
  const float* s;       // [m] padded to whole tiles (k_row_terms)
  const float* t;
  int64_t n, m;
  int64_t exclude_offset;   // with exclude_on: the pair (i, i + exclude_offset) is skipped (any sign)
  int exclude_on;
  int blocks_a, chunks;
  int64_t chunk_rows;   // multiple of kTileB
  int k;
  float* part_key;      // [chunks][n][k]
  int32_t* part_idx;
  const int32_t* skip_lo;   // kRanges: a-row i skips the b-rows [skip_lo[i], skip_hi[i]), [n] each
  const int32_t* skip_hi;
  const int32_t* group_lo;  // kDistinct: b-row j lies in the record [group_lo[j], group_hi[j]), [m] each
  const int32_t* group_hi;
};

// pairwise_topk_ranges.hip: the sweep with per-row ranges, list depth from p.k
int launch_topk_sweep_ranges(const TopkArgs& p, bool fold, hipStream_t s);
// pairwise_topk_distinct.hip: the sweep that keeps one entry per record of b (p.group_lo,
// p.group_hi; exclusions as ranges), and the merge of the chunks' lists that does the same
int launch_topk_sweep_distinct(const TopkArgs& p, bool fold, hipStream_t s);
int launch_topk_finish_distinct(const TopkArgs& p, const float* a_term, int metric, float* top_val,
                                int32_t* top_idx, hipStream_t s);

namespace {

constexpr int kGroupBytes = 2 * kTileB * 4;    // kDistinct: (group_lo, group_hi) of a b-tile, a
constexpr int kGroupSlots = 4;                 // ring like that of the terms, behind the ranges
constexpr int kHolders = 8;                    // lists per a-row at the end of a sweep
static_assert(kHolders * GFY_PAIRWISE_TOPK_MAX * kFrameA * 8 <= kBuffers * kRowBytes,
              "the holders' lists are merged in the row ring");

// (ck, ci) into a list sorted by g descending; the entry that falls off the end is dropped.
// Strict: among equal values the entries already there (lower indices) stay in front.  From the
// position it takes on, every entry moves one place down, equal ones included: what is carried
// was in front of them.
template <int D>
__device__ __forceinline__ void list_insert(float (&lk)[D], int (&li)[D], float ck, int ci) {
  bool ahead = false;
#pragma unroll
  for (int p = 0; p < D; ++p) {
    ahead = ahead || ck > lk[p];
    const float nk = ahead ? lk[p] : ck;
    const int ni = ahead ? li[p] : ci;
    lk[p] = ahead ? ck : lk[p];
    li[p] = ahead ? ci : li[p];
    ck = nk;
    ci = ni;
  }
}

// The same for a list that holds at most one entry per record, (ck, ci) being a row of the
// record [first, first + count): an entry of that record in front of the place (ck, ci) would
// take is at least as good and was met earlier (lower index), so the candidate is dropped; one
// behind it is worse and is what leaves the list — the entries between the two move one place
// down, everything behind stays.  An empty entry (kNoIndex) lies in no record: first + count <=
// m <= kNoIndex.
template <int D>
__device__ __forceinline__ void list_insert_distinct(float (&lk)[D], int (&li)[D], float ck, int ci,
                                                     int first, int count) {
  bool ahead = false, live = true;
#pragma unroll
  for (int p = 0; p < D; ++p) {
    const bool same = (uint32_t)(li[p] - first) < (uint32_t)count;
    ahead = ahead || ck > lk[p];
    const bool write = ahead && live;
    const float nk = write ? lk[p] : ck;
    const int ni = write ? li[p] : ci;
    lk[p] = write ? ck : lk[p];
    li[p] = write ? ci : li[p];
    ck = nk;
    ci = ni;
    live = live && !same;
  }
}

// LDS-DMA of one dword per lane (global_load_lds_dword): lane L copies 4 bytes from gbase + goff
// to LDS address lds + 4 L; otherwise dma16 of gfy_common.h
__device__ __forceinline__ void dma4(const void* gbase /* uniform */, uint32_t goff, uint32_t lds) {
  asm volatile(
      "s_mov_b32 m0, %0\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dword %1, %2"
      :
      : "s"(__builtin_amdgcn_readfirstlane(lds)), "v"(goff), "s"(gbase)
      : "memory");
}

template <int D, bool kFold, bool kRanges, bool kDistinct>
__global__ __launch_bounds__(kThreads, 1) void k_pairwise_topk(const TopkArgs p) {
  static_assert(kRanges || !kDistinct, "the distinct sweep takes its exclusions as ranges");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int r = lane & 31, hq = lane >> 5;
  // wave owns a-rows [64wa, 64wa+64) and b-rows [32wb, 32wb+32) of each tile
  const int wa = wave & 1, wb = wave >> 1;
  const int chunk = blockIdx.x / p.blocks_a;
  const int block_a = blockIdx.x - chunk * p.blocks_a;
  const int64_t a0 = (int64_t)block_a * kFrameA;
  const int64_t j_begin = (int64_t)chunk * p.chunk_rows;
  const int64_t j_end = j_begin + p.chunk_rows < p.m ? j_begin + p.chunk_rows : p.m;

  auto request = [&](int k) __attribute__((always_inline)) {
    sweep_request<kFold>(p, lds0, wave, j_begin, k);
    if constexpr (kDistinct) {
      // the records of the tile's rows, behind the ranges: waves 4 .. 7 bring group_lo[0, 64),
      // group_lo[64, 128), group_hi[0, 64) and group_hi[64, 128), a dword per lane.  The arrays
      // end at m: the rows of a ragged tile past it re-read the last row's (their t never wins).
      if (wave >= 4) {
        const int64_t j0 = j_begin + (int64_t)k * kTileB;
        const int part = wave - 4;
        const int last = (int)(p.m - 1 - j0);
        uint32_t me = threadIdx.x;   // rebuilt per request, as in sweep_request
        asm volatile("" : "+v"(me));
        const int row = 64 * (part & 1) + (int)(me & 63u);
        dma4(uniform_pointer((part < 2 ? p.group_lo : p.group_hi) + j0),
             (uint32_t)(row < last ? row : last) * 4u,
             lds0 + kSweepLds + kRangeBytes + (uint32_t)(k & (kGroupSlots - 1)) * kGroupBytes
                 + (uint32_t)part * 256u);
      }
    }
  };

  stage_a_block<kFrameA>(smem, p.a, p.n, a0);
  // kRanges: every a-row's range, clipped to [0, m), as (first, count) with 0 <= first and
  // first + count <= m < 2^31 (count 0: nothing, also for the rows past n); it stays in LDS
  // behind the rings for the whole sweep, so that a tile that needs it reads two words per
  // a-row slot and no register holds a bound in between
  int2* const ranges = reinterpret_cast<int2*>(smem + kSweepLds);
  if constexpr (kRanges) {
    if (t < kFrameA) {
      int lo = 0, hi = 0;
      if (a0 + t < p.n) {
        lo = p.skip_lo[a0 + t];
        hi = p.skip_hi[a0 + t];
      }
      lo = lo > 0 ? lo : 0;
      hi = hi < (int)p.m ? hi : (int)p.m;
      ranges[t] = lo < hi ? int2{lo, hi - lo} : int2{0, 0};
    }
  }
  if (j_begin < j_end) request(0);
  __syncthreads();
  f16x8 af[2][8];
  load_a_fragments<2>(af, smem, wa, r, hq);

  // kRanges: [skip_from, skip_to) is the union of the block's non-empty ranges, the same in
  // every wave and held in SGPRs; a tile outside it takes the path of the other instantiations
  int skip_from = kNoIndex, skip_to = 0;
  if constexpr (kRanges) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int2 range = ranges[64 * half + lane];
      skip_from = range.y > 0 && range.x < skip_from ? range.x : skip_from;
      skip_to = range.y > 0 && range.x + range.y > skip_to ? range.x + range.y : skip_to;
    }
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) {
      const int from = __shfl_xor(skip_from, step), to = __shfl_xor(skip_to, step);
      skip_from = from < skip_from ? from : skip_from;
      skip_to = to > skip_to ? to : skip_to;
    }
    skip_from = __builtin_amdgcn_readfirstlane(skip_from);
    skip_to = __builtin_amdgcn_readfirstlane(skip_to);
  }

  float lk[2][D];   // per a-row slot: the lane's D best g, descending
  int li[2][D];
#pragma unroll
  for (int at = 0; at < 2; ++at)
#pragma unroll
    for (int q = 0; q < D; ++q) {
      lk[at][q] = -__builtin_inff();
      li[at][q] = kNoIndex;
    }

  __syncthreads();   // the a-block has left buffer 1
  const int tiles = j_begin < j_end ? (int)((j_end - j_begin + kTileB - 1) / kTileB) : 0;
  if (tiles > 1) request(1);

  f32x16 acc[2];   // [at]
  const int jw = 32 * wb + 4 * hq;   // first of this lane's b-rows inside a tile
  auto multiply = [&](int k) __attribute__((always_inline)) {
    sweep_multiply<2, kFold>(acc, af, smem, k, wb, r, hq);
  };

  // what happens to the products of tile k (still in acc)
  auto reduce = [&](int k) __attribute__((always_inline)) {
    const int64_t j0 = j_begin + (int64_t)k * kTileB;
    // does this tile contain an excluded (i, i + offset) pair of this block?
    const int64_t ex_lo = a0 + p.exclude_offset, ex_hi = ex_lo + kFrameA;
    const bool may_exclude = !kRanges && p.exclude_on && ex_lo < j0 + kTileB && ex_hi > j0;
    // kRanges: does it meet the union of the block's ranges?
    const bool may_skip = kRanges && skip_from < j0 + kTileB && skip_to > j0;
    const int jb = (int)(j0 + jw);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int at = 0; at < 2; ++at) {
      __builtin_amdgcn_sched_barrier(0);   // one a-row at a time: its terms are not read early
      f32x16& g = acc[at];   // one a-row's 16 values at a time, in place: the products are spent
      if constexpr (!kFold) cosine_key(g, smem, k, jw);
      if (may_exclude) {   // block-uniform, at most two tiles per block
        // the one excluded b-row of this a-row, as a position among the lane's 16 values
        const int64_t off = (a0 + p.exclude_offset - j0) + (64 * wa + 32 * at + r - jw);
        const int d = off >= 0 && off < 32 ? (int)off : 4;   // 4: not a position of this lane
        const int slot = (d & 4) ? -1 : (d >> 3) * 4 + (d & 3);
#pragma unroll
        for (int q = 0; q < 16; ++q) g[q] = q == slot ? -__builtin_inff() : g[q];
      }
      if (may_skip)   // block-uniform: the tiles under the block's own records, or every tile
        mask_skip_range(g, ranges[64 * wa + 32 * at + r], jb);
      float high = max16(g);
      bool better = high > lk[at][D - 1];   // strict: an earlier b-row keeps a tie
      while (__ballot(better)) {            // wave-uniform; rare once the sweep has settled
        int first = 15;                     // lowest position holding the maximum
#pragma unroll
        for (int q = 14; q >= 0; --q) first = g[q] == high ? q : first;
        if constexpr (kDistinct) {
          // only now the candidate's record is looked at: two words of the tile's ring
          const int* lo_l = reinterpret_cast<const int*>(
              smem + kSweepLds + kRangeBytes + (k & (kGroupSlots - 1)) * kGroupBytes);
          const int in_tile = jw + 8 * (first >> 2) + (first & 3);
          const int from = lo_l[in_tile];
          list_insert_distinct<D>(lk[at], li[at], better ? high : -__builtin_inff(),
                                  (int)j0 + in_tile, from, lo_l[kTileB + in_tile] - from);
        } else
        list_insert<D>(lk[at], li[at], better ? high : -__builtin_inff(),
                       jb + 8 * (first >> 2) + (first & 3));
        const int taken = better ? first : -1;
#pragma unroll
        for (int q = 0; q < 16; ++q) g[q] = q == taken ? -__builtin_inff() : g[q];
        high = max16(g);
        better = better && high > lk[at][D - 1];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  sweep_tile_pairs(tiles, multiply, request, reduce);
  __syncthreads();   // the merge below reuses the row ring

  // [holder][position][a-row]: a lane's stores and the merging thread's reads (at a position
  // of its own) both touch 32 consecutive words
  float* m_key = reinterpret_cast<float*>(smem);
  int* m_idx = reinterpret_cast<int*>(smem + kHolders * D * kFrameA * 4);
#pragma unroll
  for (int at = 0; at < 2; ++at)
#pragma unroll
    for (int q = 0; q < D; ++q) {
      const int at_row = ((2 * wb + hq) * D + q) * kFrameA + 64 * wa + 32 * at + r;
      m_key[at_row] = lk[at][q];
      m_idx[at_row] = li[at][q];
    }
  __syncthreads();
  if (t < kFrameA && a0 + t < p.n) {
    uint64_t heads = 0;   // 8 bits per holder: entries taken from its list
    float* out_key = p.part_key + ((int64_t)chunk * p.n + a0 + t) * p.k;
    int32_t* out_idx = p.part_idx + ((int64_t)chunk * p.n + a0 + t) * p.k;
    // the best of the eight holders' heads by (key, index): its holder, (bk, bi) the entry;
    // bi == kNoIndex when every list is at its end or at its empty entries
    auto best_head = [&](float& bk, int& bi) __attribute__((always_inline)) {
      int bh = 0;
      bk = -__builtin_inff();
      bi = kNoIndex;
#pragma unroll
      for (int h = 0; h < kHolders; ++h) {
        const int pos = (int)((heads >> (8 * h)) & 0xffu);
        if (pos < D) {
          const float hk = m_key[(h * D + pos) * kFrameA + t];
          const int hi = m_idx[(h * D + pos) * kFrameA + t];
          if (hk > bk || (hk == bk && hi < bi)) {
            bk = hk;
            bi = hi;
            bh = h;
          }
        }
      }
      return bh;
    };
    if constexpr (kDistinct) {
      // the best head is taken unless a column already holds a row of its record (looked up
      // where the caller keeps it: a record may lie in several holders' lists, its best row
      // comes first); `taken` is indexed by unrolled positions only, so it stays in registers
      int taken[D];
#pragma unroll
      for (int q = 0; q < D; ++q) taken[q] = kNoIndex;
      int c = 0;
      for (int step = 0; step < kHolders * D && c < p.k; ++step) {
        float bk;
        int bi;
        const int bh = best_head(bk, bi);
        if (bi == kNoIndex) break;
        heads += 1ull << (8 * bh);
        const int from = p.group_lo[bi], count = p.group_hi[bi] - from;
        bool seen = false;
#pragma unroll
        for (int q = 0; q < D; ++q) seen = seen || (uint32_t)(taken[q] - from) < (uint32_t)count;
        if (!seen) {
          out_key[c] = kFold ? -2.0f * bk : -bk;
          out_idx[c] = bi;
#pragma unroll
          for (int q = 0; q < D; ++q) taken[q] = q == c ? bi : taken[q];
          ++c;
        }
      }
      for (; c < p.k; ++c) {
        out_key[c] = __builtin_inff();
        out_idx[c] = kNoIndex;
      }
    } else
    for (int c = 0; c < p.k; ++c) {
      float bk;
      int bi;
      const int bh = best_head(bk, bi);
      heads += 1ull << (8 * bh);
      out_key[c] = kFold ? -2.0f * bk : -bk;   // back to keys: exact, order and ties carry over
      out_idx[c] = bi;
    }
  }
}

template <int D, bool kFold, bool kRanges, bool kDistinct = false>
int launch_topk_sweep(const TopkArgs& p, hipStream_t s) {
  constexpr int kLds = kSweepLds + (kRanges ? kRangeBytes : 0)
                       + (kDistinct ? kGroupSlots * kGroupBytes : 0);
  return launch_sweep<&k_pairwise_topk<D, kFold, kRanges, kDistinct>, kLds>(
      p, p.blocks_a * p.chunks, s);
}

// the sweep at the list depth p.k asks for, folded (L2) or not
template <bool kRanges, bool kDistinct = false>
int launch_topk_sweep(const TopkArgs& p, bool fold, hipStream_t s) {
  if (p.k <= 4)
    return fold ? launch_topk_sweep<4, true, kRanges, kDistinct>(p, s)
                : launch_topk_sweep<4, false, kRanges, kDistinct>(p, s);
  if (p.k <= 8)
    return fold ? launch_topk_sweep<8, true, kRanges, kDistinct>(p, s)
                : launch_topk_sweep<8, false, kRanges, kDistinct>(p, s);
  return fold ? launch_topk_sweep<16, true, kRanges, kDistinct>(p, s)
              : launch_topk_sweep<16, false, kRanges, kDistinct>(p, s);
}

// The body of the finish kernels, one thread per a-row: the chunks' lists (each sorted by (key,
// index), chunks in ascending index order, so that an equal key met later has the higher index)
// into one, then the values of k_nearest_finish.  kDistinct: the lists hold one entry per record
// (group_lo, group_hi) and so does the result.  The kernels themselves are k_topk_finish
// (pairwise_topk.hip) and k_topk_finish_distinct (pairwise_topk_distinct.hip).
template <bool kDistinct>
__device__ __forceinline__ void topk_finish(const float* __restrict__ part_key,
                                            const int32_t* __restrict__ part_idx,
                                            const float* __restrict__ a_term,
                                            const int32_t* __restrict__ group_lo,
                                            const int32_t* __restrict__ group_hi, int64_t n,
                                            int chunks, int k, int metric,
                                            float* __restrict__ top_val,
                                            int32_t* __restrict__ top_idx) {
  constexpr int D = kDistinct ? GFY_PAIRWISE_TOPK_DISTINCT_MAX : GFY_PAIRWISE_TOPK_MAX;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float lk[D];   // -key, descending
  int li[D];
#pragma unroll
  for (int q = 0; q < D; ++q) {
    lk[q] = -__builtin_inff();
    li[q] = kNoIndex;
  }
  for (int c = 0; c < chunks; ++c) {
    const float* keys = part_key + ((int64_t)c * n + i) * k;
    const int32_t* idx = part_idx + ((int64_t)c * n + i) * k;
    for (int q = 0; q < k; ++q) {
      const float g = -keys[q];
      if (!(g > lk[D - 1])) break;   // sorted: nothing behind it gets in either (empty: g = -inf)
      if constexpr (kDistinct) {
        const int j = idx[q];
        const int from = group_lo[j];
        list_insert_distinct<D>(lk, li, g, j, from, group_hi[j] - from);
      } else {
        list_insert<D>(lk, li, g, idx[q]);
      }
    }
  }
  const float at = a_term[i];
#pragma unroll
  for (int q = 0; q < D; ++q) {
    if (q < k) {
      top_val[i * k + q] = pair_value(-lk[q], at, metric);
      top_idx[i * k + q] = li[q] == kNoIndex ? -1 : li[q];
    }
  }
}

}  // namespace
}  // namespace gfy
