// The sweep of the exact top-k search: k_pairwise_topk<D, kFold, kRanges, kDistinct> and its
// launcher (the design is told at the head of pairwise_topk.hip).
// Included by the three translation units that instantiate it: pairwise_topk.hip (kRanges =
// false: one excluded pair per a-row at most), pairwise_topk_ranges.hip (kRanges = true: an
// excluded range of b-rows per a-row) and pairwise_topk_distinct.hip (kDistinct = true: at most
// one hit per record of b, told at its head), so that the device code of the one does not move
// with the others.

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

constexpr int kBlockA = 128;  // a-rows per workgroup
constexpr int kTileB = 128;   // b-rows per LDS tile
constexpr int kThreads = 512;
constexpr int kBuffers = 4;   // b-tile ring: the pair being consumed and the pair in flight
constexpr int kRowBytes = kTileB * 256;        // one b-tile of rows
constexpr int kTermBytes = 2 * kTileB * 4;     // its (s, t)
constexpr int kTermSlots = 4;                  // (s, t) ring, like the rows
constexpr int kTopkLds = kBuffers * kRowBytes + kTermSlots * kTermBytes;
constexpr int kRangeBytes = kBlockA * 8;       // kRanges: (first, count) of every a-row, behind the rings
constexpr int kGroupBytes = 2 * kTileB * 4;    // kDistinct: (group_lo, group_hi) of a b-tile, a
constexpr int kGroupSlots = 4;                 // ring like that of the terms, behind the ranges
constexpr int kHolders = 8;                    // lists per a-row at the end of a sweep
constexpr int kNoIndex = 0x7fffffff;
static_assert(kHolders * GFY_PAIRWISE_TOPK_MAX * kBlockA * 8 <= kBuffers * kRowBytes,
              "the holders' lists are merged in the row ring");

// COPIES of pairwise.hip, kept here so that the machine code of its kernels cannot move with
// this file: uniform_pointer, off256, the ring constants above (kTileB, kBuffers, kRowBytes,
// kTermBytes, kTermSlots) and the `request` lambda of the kernel (the LDS-DMA addressing of a
// b-tile and of its terms).  A fix to the DMA addressing or to the swizzle there has to be made
// here too, and the other way round.
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

__device__ __forceinline__ float max16(const f32x16& g) {
  float high = __builtin_fmaxf(g[0], g[1]);
#pragma unroll
  for (int q = 2; q < 16; q += 2)
    high = __builtin_fmaxf(__builtin_fmaxf(high, g[q]), g[q + 1]);   // v_max3_f32
  return high;
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
  const int64_t a0 = (int64_t)block_a * kBlockA;
  const int64_t j_begin = (int64_t)chunk * p.chunk_rows;
  const int64_t j_end = j_begin + p.chunk_rows < p.m ? j_begin + p.chunk_rows : p.m;

  // one b-tile -> its ring buffer, (s, t) -> the term ring: the request of pairwise.hip (per-lane
  // offsets rebuilt per request, the tile's base in SGPRs; the reasons are recorded there).
  // A copy: see the note at uniform_pointer — change both or neither.
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
    if constexpr (kDistinct) {
      // the records of the tile's rows, behind the ranges: waves 4 .. 7 bring group_lo[0, 64),
      // group_lo[64, 128), group_hi[0, 64) and group_hi[64, 128), a dword per lane.  The arrays
      // end at m: the rows of a ragged tile past it re-read the last row's (their t never wins).
      if (wave >= 4) {
        const int part = wave - 4;
        const int last = (int)(p.m - 1 - j0);
        const int row = 64 * (part & 1) + (int)(me & 63u);
        dma4(uniform_pointer((part < 2 ? p.group_lo : p.group_hi) + j0),
             (uint32_t)(row < last ? row : last) * 4u,
             lds0 + kTopkLds + kRangeBytes + (uint32_t)(k & (kGroupSlots - 1)) * kGroupBytes
                 + (uint32_t)part * 256u);
      }
    }
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
  // kRanges: every a-row's range, clipped to [0, m), as (first, count) with 0 <= first and
  // first + count <= m < 2^31 (count 0: nothing, also for the rows past n); it stays in LDS
  // behind the rings for the whole sweep, so that a tile that needs it reads two words per
  // a-row slot and no register holds a bound in between
  int2* const ranges = reinterpret_cast<int2*>(smem + kTopkLds);
  if constexpr (kRanges) {
    if (t < kBlockA) {
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
#pragma unroll
  for (int at = 0; at < 2; ++at)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
      af[at][ks] = *reinterpret_cast<const f16x8*>(
          smem + kRowBytes + off256(64 * wa + 32 * at + r, 2 * ks + hq));

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
    const int64_t j0 = j_begin + (int64_t)k * kTileB;
    // does this tile contain an excluded (i, i + offset) pair of this block?
    const int64_t ex_lo = a0 + p.exclude_offset, ex_hi = ex_lo + kBlockA;
    const bool may_exclude = !kRanges && p.exclude_on && ex_lo < j0 + kTileB && ex_hi > j0;
    // kRanges: does it meet the union of the block's ranges?
    const bool may_skip = kRanges && skip_from < j0 + kTileB && skip_to > j0;
    const int jb = (int)(j0 + jw);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int at = 0; at < 2; ++at) {
      __builtin_amdgcn_sched_barrier(0);   // one a-row at a time: its terms are not read early
      f32x16& g = acc[at];   // one a-row's 16 values at a time, in place: the products are spent
      if constexpr (!kFold) {
        const float* s_l = reinterpret_cast<const float*>(
            smem + kBuffers * kRowBytes + (k & (kTermSlots - 1)) * kTermBytes);
        const float* t_l = s_l + kTileB;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const f32x4 sv = *reinterpret_cast<const f32x4*>(s_l + jw + 8 * q4);
          const f32x4 tv = *reinterpret_cast<const f32x4*>(t_l + jw + 8 * q4);
          f32x4 a4;
#pragma unroll
          for (int i = 0; i < 4; ++i) a4[i] = g[4 * q4 + i];
          const f32x4 key = __builtin_elementwise_fma(a4, sv, tv);   // the key of k_pairwise<false>
#pragma unroll
          for (int i = 0; i < 4; ++i) g[4 * q4 + i] = -key[i];
        }
      }
      if (may_exclude) {   // block-uniform, at most two tiles per block
        // the one excluded b-row of this a-row, as a position among the lane's 16 values
        const int64_t off = (a0 + p.exclude_offset - j0) + (64 * wa + 32 * at + r - jw);
        const int d = off >= 0 && off < 32 ? (int)off : 4;   // 4: not a position of this lane
        const int slot = (d & 4) ? -1 : (d >> 3) * 4 + (d & 3);
#pragma unroll
        for (int q = 0; q < 16; ++q) g[q] = q == slot ? -__builtin_inff() : g[q];
      }
      if (may_skip) {   // block-uniform: the tiles under the block's own records, or every tile
        // b-row j is skipped iff first <= j < first + count: one unsigned comparison, since
        // 0 <= first <= first + count < 2^31 (the padded rows of a ragged tile lie past m)
        const int2 range = ranges[64 * wa + 32 * at + r];
#pragma unroll
        for (int q = 0; q < 16; ++q)
          g[q] = (uint32_t)(jb + 8 * (q >> 2) + (q & 3) - range.x) < (uint32_t)range.y
                     ? -__builtin_inff() : g[q];
      }
      float high = max16(g);
      bool better = high > lk[at][D - 1];   // strict: an earlier b-row keeps a tie
      while (__ballot(better)) {            // wave-uniform; rare once the sweep has settled
        int first = 15;                     // lowest position holding the maximum
#pragma unroll
        for (int q = 14; q >= 0; --q) first = g[q] == high ? q : first;
        if constexpr (kDistinct) {
          // only now the candidate's record is looked at: two words of the tile's ring
          const int* lo_l = reinterpret_cast<const int*>(
              smem + kTopkLds + kRangeBytes + (k & (kGroupSlots - 1)) * kGroupBytes);
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

  // Two tiles per barrier: the ring holds the pair being consumed and the pair in flight; the
  // next pair is requested behind the first multiply (pairwise.hip: right behind the barrier all
  // eight waves would pay the DMA issue at once with the matrix cores idle).
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
  __syncthreads();   // the merge below reuses the row ring

  // [holder][position][a-row]: a lane's stores and the merging thread's reads (at a position
  // of its own) both touch 32 consecutive words
  float* m_key = reinterpret_cast<float*>(smem);
  int* m_idx = reinterpret_cast<int*>(smem + kHolders * D * kBlockA * 4);
#pragma unroll
  for (int at = 0; at < 2; ++at)
#pragma unroll
    for (int q = 0; q < D; ++q) {
      const int at_row = ((2 * wb + hq) * D + q) * kBlockA + 64 * wa + 32 * at + r;
      m_key[at_row] = lk[at][q];
      m_idx[at_row] = li[at][q];
    }
  __syncthreads();
  if (t < kBlockA && a0 + t < p.n) {
    uint64_t heads = 0;   // 8 bits per holder: entries taken from its list
    float* out_key = p.part_key + ((int64_t)chunk * p.n + a0 + t) * p.k;
    int32_t* out_idx = p.part_idx + ((int64_t)chunk * p.n + a0 + t) * p.k;
    if constexpr (kDistinct) {
      // the best head is taken unless a column already holds a row of its record (looked up
      // where the caller keeps it: a record may lie in several holders' lists, its best row
      // comes first); `taken` is indexed by unrolled positions only, so it stays in registers
      int taken[D];
#pragma unroll
      for (int q = 0; q < D; ++q) taken[q] = kNoIndex;
      int c = 0;
      for (int step = 0; step < kHolders * D && c < p.k; ++step) {
        float bk = -__builtin_inff();
        int bi = kNoIndex, bh = 0;
#pragma unroll
        for (int h = 0; h < kHolders; ++h) {
          const int pos = (int)((heads >> (8 * h)) & 0xffu);
          if (pos < D) {
            const float hk = m_key[(h * D + pos) * kBlockA + t];
            const int hi = m_idx[(h * D + pos) * kBlockA + t];
            if (hk > bk || (hk == bk && hi < bi)) {
              bk = hk;
              bi = hi;
              bh = h;
            }
          }
        }
        if (bi == kNoIndex) break;   // every list is at its end or at its empty entries
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
      float bk = -__builtin_inff();
      int bi = kNoIndex, bh = 0;
#pragma unroll
      for (int h = 0; h < kHolders; ++h) {
        const int pos = (int)((heads >> (8 * h)) & 0xffu);
        if (pos < D) {
          const float hk = m_key[(h * D + pos) * kBlockA + t];
          const int hi = m_idx[(h * D + pos) * kBlockA + t];
          if (hk > bk || (hk == bk && hi < bi)) {
            bk = hk;
            bi = hi;
            bh = h;
          }
        }
      }
      heads += 1ull << (8 * bh);
      out_key[c] = kFold ? -2.0f * bk : -bk;   // back to keys: exact, order and ties carry over
      out_idx[c] = bi;
    }
  }
}

template <int D, bool kFold, bool kRanges, bool kDistinct = false>
int launch_sweep(const TopkArgs& p, hipStream_t s) {
  constexpr int kLds = kTopkLds + (kRanges ? kRangeBytes : 0)
                       + (kDistinct ? kGroupSlots * kGroupBytes : 0);
  static_assert(kLds <= 160 * 1024, "the LDS of a compute unit");
  static PerDeviceOnce opt_in;   // > 64 KB of dynamic LDS: once per device (gfy_common.h)
  if (const int rc = opt_in.run([]() -> int {
        GFY_CHECK_HIP(hipFuncSetAttribute(
            reinterpret_cast<const void*>(&k_pairwise_topk<D, kFold, kRanges, kDistinct>),
            hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
        return GFY_OK;
      }))
    return rc;
  k_pairwise_topk<D, kFold, kRanges, kDistinct><<<p.blocks_a * p.chunks, kThreads, kLds, s>>>(p);
  return GFY_OK;
}

}  // namespace
}  // namespace gfy
