// The all-pairs sweep that nearest (pairwise.hip), top-k (pairwise_topk.inc), the record scores
// (pairwise_records.hip) and the radius search (pairwise_within.hip) share — the ONLY copy of:
// the b-tile ring and its LDS-DMA request, the staging of the a-block, the MFMA multiply of one
// tile, the two-tiles-per-barrier loop, the value formula, the split of b into chunks, the front
// of the workspace and the launch with more than 64 KB of LDS.  For the kernels on a 128-row
// a-block (all but nearest) also: kFrameA, kRangeBytes, kNoIndex, the cosine key, the mask of a
// skip range, ordered / unordered and on the host the launchers' prologue (begin_sweep); and for
// k_record_sweep and the radius sweep the common argument fields (SweepArgs), the block geometry
// (BlockFrame), the front of the kernel up to the request of tile 1 and the staging and union of
// the skip ranges.  k_pairwise_topk keeps its own copy of those last pieces and its own argument
// layout: with them shared, three of its instantiations measured 0.7 to 1.0 % slower, their tile
// loops unchanged (profiles/sweep_frame_refactor_ab.txt).  Included after gfy_common.h;
// everything is inlined into the kernels of the including file, whose epilogue is their own.
//
// A workgroup of 8 waves keeps the MFMA fragments of its a-block in registers and sweeps its
// chunk of b in 128-row tiles that LDS-DMA lands in a ring of four buffers, XOR-swizzled so that
// the operand reads are conflict-free; the (s, t) terms of a tile travel the same way into a
// ring of their own behind the rows.  The product is (B-tile) x (A-block)^T: the a-row sits on
// the MFMA lane and a lane's 16 accumulator registers are 4 x 4 consecutive b-rows.

namespace gfy {
namespace {

constexpr int kTileB = 128;   // b-rows per LDS tile
constexpr int kThreads = 512;
constexpr int kBuffers = 4;   // b-tile ring: tile i is consumed while the next ones are in flight
constexpr int kRowBytes = kTileB * 256;        // one b-tile of rows
constexpr int kTermBytes = 2 * kTileB * 4;     // its (s, t)
constexpr int kTermSlots = 4;                  // (s, t) ring, like the rows
// row ring (its buffers from 1 on stage the a-block first) + (s, t) ring
constexpr int kSweepLds = kBuffers * kRowBytes + kTermSlots * kTermBytes;

template <class T>
__device__ __forceinline__ const T* uniform_pointer(const T* pointer) {
  const uint64_t bits = (uint64_t)(uintptr_t)pointer;
  const uint32_t low = __builtin_amdgcn_readfirstlane((uint32_t)bits);
  const uint32_t high = __builtin_amdgcn_readfirstlane((uint32_t)(bits >> 32));
  return reinterpret_cast<const T*>(((uint64_t)high << 32) | low);
}

// byte offset of 16-byte piece `chunk` of row `row` in a swizzled tile of 256-byte rows
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

// |row|^2 the way every key's terms take it (k_row_terms, pairwise.hip; the local aligner's
// rows, align_local.inc): 16 consecutive lanes hold the 16 pieces of a row, each adds its eight
// squares in order and a butterfly adds the 16 partial sums, so that all 16 lanes hold the sum.
__device__ __forceinline__ float row_square_sum(const f16x8& v) {
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) ss = __builtin_fmaf((float)v[j], (float)v[j], ss);
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) ss += __shfl_xor(ss, m, 64);
  return ss;
}

// 1 / max(|row|, 1e-12) of cosine: -s_j of a b-row, the a_term of an a-row
__device__ __forceinline__ float inverse_norm(float ss) {
  const float nrm = __builtin_sqrtf(ss);
  return 1.0f / (nrm > 1e-12f ? nrm : 1e-12f);
}

// What leaves every search for the pair with key `key` (key_ij = fma(dot_ij, s_j, t_j), head of
// pairwise.hip): L2 sqrt(max(|a_i|^2 + key, 0)) with a_term = |a_i|^2, cosine -key / |a_i| with
// a_term = 1 / |a_i|.
__device__ __forceinline__ float pair_value(float key, float a_term, int metric) {
  if (metric == GFY_L2) {
    const float d2 = a_term + key;
    return __builtin_sqrtf(d2 > 0.f ? d2 : 0.f);
  }
  return -key * a_term;
}

// Tile k of the sweep that starts at b-row j_begin -> buffer k % kBuffers: 128 rows as 32 DMA
// instructions (4 per wave, 4 rows each), (s, t) -> slot k % kTermSlots as one more by waves 0
// and 1 (kFold: t alone, by wave 0).  Rows past the end re-read the last row; their t never wins
// (k_row_terms pads s / t to whole tiles).  `p` is the kernel's argument struct (b, s, t, m).
// Per-lane byte offset of its 16-byte piece q inside a tile: row 16 wave + 4 q + sub, slot
// (lane & 15) ^ (row & 15)  =  (home ^ (q << 6)) + 1024 q  with ONE loop-invariant register
// (`home`); the tile's base travels in SGPRs.  (64-bit per-lane pointers, or the four
// offsets kept in registers, spilled — and a scratch reload is a vmcnt(0) wait that drains
// the DMA look-ahead.  The asm keeps hipcc from hoisting them out of the loop again.)
// `home` is rebuilt from threadIdx.x per request (six VALU operations): any loop-invariant
// register here is one that hipcc spills in k_pairwise, which sits at the 256-register ceiling.
template <bool kFold, class Args>
__device__ __forceinline__ void sweep_request(const Args& p, uint32_t lds0, int wave,
                                              int64_t j_begin, int k) {
  const int64_t j0 = j_begin + (int64_t)k * kTileB;
  const uint32_t base = lds0 + (uint32_t)(k & (kBuffers - 1)) * kRowBytes;
  // wave-uniform, and said so: with a reduce carried over the barrier in the loop (k_pairwise)
  // hipcc's divergence analysis puts j0 in vector registers, which the DMA's scalar base operand
  // cannot take
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
  } else {   // ragged last tile
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
}

// (s, t) of tile k in the term ring: s at [0, kTileB), t behind it
__device__ __forceinline__ const float* sweep_terms(const char* smem, int k) {
  return reinterpret_cast<const float*>(smem + kBuffers * kRowBytes
                                        + (k & (kTermSlots - 1)) * kTermBytes);
}

// The a-block [a0, a0 + kRows) through LDS once (coalesced; rows past n are zero), swizzled like
// a b-tile, into the ring from buffer 1 on (kRows / 128 buffers, not yet in use).  A barrier
// later load_a_fragments keeps ALL the fragments of the wave's 32 kTilesA a-rows in registers;
// another barrier later the buffers are the ring's again.
template <int kRows>
__device__ __forceinline__ void stage_a_block(char* smem, const f16* a, int64_t n, int64_t a0) {
  char* atile = smem + kRowBytes;
  for (int i = threadIdx.x; i < kRows * 16; i += kThreads) {
    const int row = i >> 4, ch = i & 15;
    f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (a0 + row < n) v = *reinterpret_cast<const f16x8*>(a + (a0 + row) * 128 + ch * 8);
    *reinterpret_cast<f16x8*>(atile + off256(row, ch)) = v;
  }
}

template <int kTilesA>
__device__ __forceinline__ void load_a_fragments(f16x8 (&af)[kTilesA][8], const char* smem, int wa,
                                                 int r, int hq) {
#pragma unroll
  for (int at = 0; at < kTilesA; ++at)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
      af[at][ks] = *reinterpret_cast<const f16x8*>(
          smem + kRowBytes + off256(32 * kTilesA * wa + 32 * at + r, 2 * ks + hq));
}

// The wave's 32 x (32 kTilesA) block of tile k into acc: kTilesA independent accumulator chains
// (a 32x32x16 MFMA that reads the previous one's result stalls the issue port), the b operand
// read kAheadK k-steps ahead.  Every chain starts from 0, or (kFold) from -|b_j|^2 / 2 of the
// lane's 16 b-rows, so that what comes out is g_ij = a_i.b_j - |b_j|^2 / 2 (k_row_terms).
template <int kTilesA, bool kFold>
__device__ __forceinline__ void sweep_multiply(f32x16 (&acc)[kTilesA],
                                               const f16x8 (&af)[kTilesA][8], const char* smem,
                                               int k, int wb, int r, int hq) {
  const char* tile = smem + (k & (kBuffers - 1)) * kRowBytes;
  f32x16 start = {};
  if constexpr (kFold) {
    const float* u_l = sweep_terms(smem, k) + kTileB;
    const int jw = 32 * wb + 4 * hq;   // first of this lane's b-rows inside a tile
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
    // hipcc otherwise sinks every operand read down to its MFMAs (one register quad,
    // read -> lgkmcnt(0) -> MFMAs: the LDS latency exposed eight times a tile)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int at = 0; at < kTilesA; ++at)
      acc[at] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bf[ks % kRing], af[at][ks],
                                                       ks == 0 ? start : acc[at], 0, 0, 0);
  }
}

// Two tiles per barrier: the ring holds the pair being consumed and the pair in flight (tiles 0
// and 1 are requested by the caller).  Between two barriers each wave runs multiply, reduce,
// multiply, reduce on its own, so the two waves of a SIMD interleave.  The next pair is requested
// BEHIND the first multiply: issuing a tile's DMA pieces costs a wave several hundred cycles, and
// right behind the barrier all eight waves would pay them at once with the matrix cores idle.
template <class Multiply, class Request, class Reduce>
__device__ __forceinline__ void sweep_tile_pairs(int tiles, Multiply&& multiply, Request&& request,
                                                 Reduce&& reduce) {
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
}

// ---- the 128-row block -------------------------------------------------------------------------
// What the kernels on a 128-row a-block share above the sweep: k_record_sweep and the radius
// search's within_sweep all of it, k_pairwise_topk the constants, cosine_key, mask_skip_range and
// begin_sweep.  (k_pairwise, 256 rows, keeps its own body.)

// The fields every sweep's argument struct starts with; RecordArgs and WithinArgs derive from it
// (TopkArgs holds the same nine under the same names, in the order its kernels were built for)
struct SweepArgs {
  const f16* a;
  const f16* b;
  const float* s;       // [m] padded to whole tiles (k_row_terms)
  const float* t;
  int64_t n, m;
  int blocks_a, chunks;
  int64_t chunk_rows;   // multiple of kTileB
};

constexpr int kFrameA = 128;                // a-rows per workgroup
constexpr int kRangeBytes = kFrameA * 8;    // (first, count) of every a-row, behind the rings
constexpr int kNoIndex = 0x7fffffff;

// Where a thread and its workgroup stand: workgroup (block_a, chunk) sweeps the b-rows
// [j_begin, j_end) in `tiles` tiles against the a-rows from a0 on.  A wave owns the a-rows
// [64 wa, 64 wa + 64) and the b-rows [32 wb, 32 wb + 32) of every tile; a lane holds, per a-row
// slot `at`, a-row 64 wa + 32 at + r against the 16 b-rows jw + 8 (q >> 2) + (q & 3) of a tile.
struct BlockFrame {
  int t, lane, wave, r, hq, wa, wb, jw;
  int chunk;
  int64_t a0, j_begin, j_end;
  int tiles;
};

__device__ __forceinline__ BlockFrame block_frame(const SweepArgs& p) {
  BlockFrame f;
  f.t = threadIdx.x;
  f.lane = f.t & 63;
  f.wave = __builtin_amdgcn_readfirstlane(f.t >> 6);
  f.r = f.lane & 31;
  f.hq = f.lane >> 5;
  f.wa = f.wave & 1;
  f.wb = f.wave >> 1;
  f.jw = 32 * f.wb + 4 * f.hq;
  f.chunk = blockIdx.x / p.blocks_a;
  const int block_a = blockIdx.x - f.chunk * p.blocks_a;
  f.a0 = (int64_t)block_a * kFrameA;
  f.j_begin = (int64_t)f.chunk * p.chunk_rows;
  f.j_end = f.j_begin + p.chunk_rows < p.m ? f.j_begin + p.chunk_rows : p.m;
  f.tiles = f.j_begin < f.j_end ? (int)((f.j_end - f.j_begin + kTileB - 1) / kTileB) : 0;
  return f;
}

// The front of every kernel, in three steps with the kernel's own set-up in between:
//   stage_a_block<kFrameA>     the a-block into the ring; then what the kernel itself puts into LDS
//   load_block_fragments       request tile 0, barrier, the fragments into registers; then what
//                              the kernel reads back from LDS (skip_union)
//   release_a_block            barrier: the a-block has left buffer 1; request tile 1
template <class Request>
__device__ __forceinline__ void load_block_fragments(f16x8 (&af)[2][8], const char* smem,
                                                     const BlockFrame& f, Request&& request) {
  if (f.j_begin < f.j_end) request(0);
  __syncthreads();
  load_a_fragments<2>(af, smem, f.wa, f.r, f.hq);
}

template <class Request>
__device__ __forceinline__ void release_a_block(const BlockFrame& f, Request&& request) {
  __syncthreads();
  if (f.tiles > 1) request(1);
}

// Per-row skip ranges.  Every a-row's range [skip_lo[i], skip_hi[i]), clipped to [0, m), as
// (first, count) with 0 <= first and first + count <= m < 2^31 (count 0: nothing, also for the
// rows past n); it stays in LDS behind the rings for the whole sweep, so that a tile that needs
// it reads two words per a-row slot and no register holds a bound in between.  In front of the
// first barrier.
__device__ __forceinline__ int2* skip_ranges(char* smem) {
  return reinterpret_cast<int2*>(smem + kSweepLds);
}

__device__ __forceinline__ void stage_skip_ranges(int2* ranges, const int32_t* skip_lo,
                                                  const int32_t* skip_hi, const SweepArgs& p,
                                                  const BlockFrame& f) {
  if (f.t < kFrameA) {
    int lo = 0, hi = 0;
    if (f.a0 + f.t < p.n) {
      lo = skip_lo[f.a0 + f.t];
      hi = skip_hi[f.a0 + f.t];
    }
    lo = lo > 0 ? lo : 0;
    hi = hi < (int)p.m ? hi : (int)p.m;
    ranges[f.t] = lo < hi ? int2{lo, hi - lo} : int2{0, 0};
  }
}

// [from, to): the union of the block's non-empty ranges, the same in every wave and held in
// SGPRs; a tile outside it takes the path of a kernel without ranges.  Empty until skip_union
// has run (behind the first barrier).
struct SkipUnion {
  int from = kNoIndex, to = 0;
  __device__ __forceinline__ bool meets_tile(int64_t j0) const {
    return from < j0 + kTileB && to > j0;
  }
};

__device__ __forceinline__ SkipUnion skip_union(const int2* ranges, int lane) {
  SkipUnion u;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int2 range = ranges[64 * half + lane];
    u.from = range.y > 0 && range.x < u.from ? range.x : u.from;
    u.to = range.y > 0 && range.x + range.y > u.to ? range.x + range.y : u.to;
  }
#pragma unroll
  for (int step = 32; step > 0; step >>= 1) {
    const int from = __shfl_xor(u.from, step), to = __shfl_xor(u.to, step);
    u.from = from < u.from ? from : u.from;
    u.to = to > u.to ? to : u.to;
  }
  u.from = __builtin_amdgcn_readfirstlane(u.from);
  u.to = __builtin_amdgcn_readfirstlane(u.to);
  return u;
}

// The lane's values of one a-row whose b-row lies in `range` (an entry of skip_ranges) to -inf;
// jb is the lane's first b-row of the tile.  b-row j is skipped iff first <= j < first + count:
// one unsigned comparison, since 0 <= first <= first + count < 2^31 (the padded rows of a ragged
// tile lie past m).
__device__ __forceinline__ void mask_skip_range(f32x16& g, int2 range, int jb) {
#pragma unroll
  for (int q = 0; q < 16; ++q)
    g[q] = (uint32_t)(jb + 8 * (q >> 2) + (q & 3) - range.x) < (uint32_t)range.y
               ? -__builtin_inff() : g[q];
}

// Cosine: one a-row's 16 products of tile k into g = -key in place, key = fma(dot, s, t) being
// the key of k_pairwise<false>.  (L2 has g out of the MFMAs: kFold.)
__device__ __forceinline__ void cosine_key(f32x16& g, const char* smem, int k, int jw) {
  const float* s_l = sweep_terms(smem, k);
  const float* t_l = s_l + kTileB;
#pragma unroll
  for (int q4 = 0; q4 < 4; ++q4) {
    const f32x4 sv = *reinterpret_cast<const f32x4*>(s_l + jw + 8 * q4);
    const f32x4 tv = *reinterpret_cast<const f32x4*>(t_l + jw + 8 * q4);
    f32x4 a4;
#pragma unroll
    for (int i = 0; i < 4; ++i) a4[i] = g[4 * q4 + i];
    const f32x4 key = __builtin_elementwise_fma(a4, sv, tv);
#pragma unroll
    for (int i = 0; i < 4; ++i) g[4 * q4 + i] = -key[i];
  }
}

// fp32 <-> uint32, monotone: x < y  <=>  ordered(x) < ordered(y) (no NaN comes out of a sweep)
__device__ __forceinline__ uint32_t ordered(float x) {
  const uint32_t u = __float_as_uint(x);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float unordered(uint32_t u) {
  return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xffffffffu));
}

// ---- host side ---------------------------------------------------------------------------------

// How a sweep of n a-rows (in blocks of block_a) against m b-rows is cut: b into `chunks` pieces
// of chunk_rows rows (whole tiles), one workgroup per (a-block, chunk).
struct BSplit {
  int blocks_a, chunks;
  int64_t chunk_rows;   // multiple of kTileB
};

// Enough workgroups for four per CU (1024), and of the next few chunk counts the one whose grid
// ends in the fewest sweeps.  One workgroup per CU at a time, all of one length: a grid of
// blocks_a x chunks workgroups ends after ceil(grid / CUs) of them, each 1 / chunks of a sweep
// long.  1,000,000 rows are 3,907 a-blocks of 256 = 15.26 per CU: one chunk ends after 16 sweeps,
// three after 46 / 3 = 15.33.  A few more chunks than the minimum cost a merge entry per a-row
// and chunk.  forced_chunks > 0 (diagnostic builds of pairwise.hip) replaces the choice.
inline BSplit split_b(int64_t n, int64_t m, int block_a, int64_t forced_chunks = 0) {
  BSplit w;
  w.blocks_a = (int)((n + block_a - 1) / block_a);
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
  if (forced_chunks > 0) chunks = forced_chunks;
  if (chunks > tiles_b) chunks = tiles_b;
  if (chunks < 1) chunks = 1;
  const int64_t tiles_per_chunk = (tiles_b + chunks - 1) / chunks;
  w.chunk_rows = tiles_per_chunk * kTileB;
  w.chunks = (int)((tiles_b + tiles_per_chunk - 1) / tiles_per_chunk);
  return w;
}

// A workspace handed out front to back, every array rounded up to 256 bytes (base == nullptr:
// only `bytes` is wanted).  Every sweep's workspace starts with terms(): s and t of b padded to
// whole tiles, then the a-side term; what follows is the caller's.
struct Carver {
  void* base;
  size_t bytes = 0;
  void* take(size_t size) {
    void* ptr = base ? (char*)base + bytes : nullptr;
    bytes += align_up(size, 256);
    return ptr;
  }
  void terms(int64_t n, int64_t m, float*& s, float*& t, float*& a_term) {
    const size_t padded = (size_t)((m + kTileB - 1) / kTileB) * kTileB;
    s = (float*)take(padded * 4);
    t = (float*)take(padded * 4);
    a_term = (float*)take((size_t)n * 4);
  }
};

// The front of a 128-row sweep's carved workspace (Carver::terms) with the split it was carved
// for and the size of the whole; a search's own workspace derives from it and adds its arrays.
struct SweepWorkspace {
  float *s, *t, *a_term;
  BSplit split;
  size_t bytes;
};

// What every launcher of a 128-row sweep starts with: refuse a workspace shorter than the carved
// one, launch the row terms of b (folded for L2: the kFold kernels) and of a, and fill the common
// argument fields of `p` (a SweepArgs, or TopkArgs with the same nine names).
template <class Args>
int begin_sweep(const char* who, const SweepWorkspace& w, size_t ws_bytes, const void* a, int64_t n,
                const void* b, int64_t m, int metric, hipStream_t s, Args& p) {
  GFY_REQUIRE(ws_bytes >= w.bytes, GFY_ERR_WORKSPACE, "%s: workspace %zu < required %zu", who,
              ws_bytes, w.bytes);
  const int64_t padded_m = (m + kTileB - 1) / kTileB * kTileB;
  const bool fold = metric == GFY_L2;
  if (const int rc = launch_pairwise_row_terms(b, m, padded_m, metric, fold, w.s, w.t, nullptr, s))
    return rc;
  if (const int rc = launch_pairwise_row_terms(a, n, n, metric, 0, nullptr, nullptr, w.a_term, s))
    return rc;
  p.a = (const f16*)a;
  p.b = (const f16*)b;
  p.s = w.s;
  p.t = w.t;
  p.n = n;
  p.m = m;
  p.blocks_a = w.split.blocks_a;
  p.chunks = w.split.chunks;
  p.chunk_rows = w.split.chunk_rows;
  return GFY_OK;
}

// kKernel<<<grid, kThreads, kLds>>>(p) with more than 64 KB of dynamic LDS: the opt-in once per
// device and kernel, thread-safe (PerDeviceOnce, gfy_common.h)
template <auto kKernel, int kLds, class Args>
int launch_sweep(const Args& p, int grid, hipStream_t s) {
  static_assert(kLds <= 160 * 1024, "the LDS of a compute unit");
  static PerDeviceOnce opt_in;
  if (const int rc = opt_in.run([]() -> int {
        GFY_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kKernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
        return GFY_OK;
      }))
    return rc;
  kKernel<<<grid, kThreads, kLds, s>>>(p);
  return GFY_OK;
}

}  // namespace
}  // namespace gfy
