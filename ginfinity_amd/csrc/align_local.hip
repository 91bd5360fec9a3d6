// Batched local alignment of record pairs (gfy_align_local; semantics: include/gfy.h): Smith-
// Waterman with affine gaps (Gotoh) over the cosine of the records' rows, the Lq x Lr matrix of a
// pair never written to memory.  Our own definition, as the whole distance path's is: not the
// external aligner of the reference, whose scoring formula is nowhere in its tree.
//
// One wave owns one pair; a workgroup is four waves that never meet (no barrier, no flag), and a
// wave takes pairs wave, wave + waves of the grid, ... until the list ends.
//   * The wave walks the a-record in strips of 64 rows, lane = row, and sweeps the b-record with
//     the usual skew: at step t lane l is at column t - l.  H and F of the row above come from
//     lane l - 1 (one wave shift each), H of the diagonal is last step's H from above, E and H
//     of the left neighbour are the lane's own registers.  Every cell is the fixed expression of
//     include/gfy.h of its three predecessors, so nothing depends on the schedule.
//   * The substitution scores come 32 columns at a time: the 32 b-rows go to LDS in the swizzled
//     layout of the sweep, sweep_multiply (pairwise_sweep.inc, the one multiply of the library)
//     forms the 64 x 32 products against the strip's fragments, which stay in registers, and the
//     epilogue turns them into the dense kernel's cosine (same key, same pair_value), scales and
//     shifts it with two rounded operations and stores it BY ANTI-DIAGONAL: cell (l, j) at
//     [(l + j) % 128][l], a ring of 128 diagonals of 64 lanes (32 KB).  A step reads one diagonal:
//     64 consecutive words, no bank conflict.  Before step t = 32 kb the ring holds diagonals
//     t .. t + 62 of earlier columns, the new columns add up to t + 94, and the quarter behind
//     them (t + 96 .. t + 127, spent by the last 32 steps) stages the b-rows.
//   * The strip's last row (H, F per column) goes to the workspace as lane 63 forms it and comes
//     back to lane 0 of the next strip 32 columns at a time, one load ahead, two buffers in turn.
//   * Each lane keeps its best (H, i, j) with a strict >, which is the lowest (i, j) of the lane's
//     rows; one butterfly at the end orders by (score descending, i ascending, j ascending).
// ptr_a, ptr_b and pairs are device arrays: they are compared and clipped, a pair outside them or
// longer than the limits gets NaN and (-2, -2), and nothing outside the caller's buffers is read.
#include "gfy_common.h"
#include "pairwise_sweep.inc"

namespace gfy {
namespace {

constexpr int kAlignWaves = 4;                 // pairs in flight per workgroup
constexpr int kAlignThreads = 64 * kAlignWaves;
constexpr int kStrip = 64;                     // a-rows per strip: lane = row
constexpr int kSub = 32;                       // b-rows per multiply
constexpr int kRingBytes = 128 * kStrip * 4;   // 128 anti-diagonals
constexpr int kWaveLds = kRingBytes + kStrip * 4 + kSub * 4;   // ring, 1/|a| of the strip, s of the b-rows
constexpr int kAlignLds = kAlignWaves * kWaveLds;
constexpr int kAlignGroupsMax = 256;           // one per compute unit (its LDS holds one): the waves loop
static_assert(kRingBytes == kBuffers * (kSub * 256), "a quarter of the ring stages 32 b-rows");

struct AlignArgs {
  const f16* a;
  const f16* b;
  const int32_t* ptr_a;
  const int32_t* ptr_b;
  const int32_t* pairs;   // [P][2]
  int64_t n, m, P;
  int records_a, records_b;
  float match_scale, match_shift, gap_open, gap_extend;
  float* out_score;       // [P]
  int32_t* out_end;       // [P][2]
  float2* carry;          // [waves of the grid][2][cap]: (H, F) of a strip's last row
  int cap;                // columns a carry buffer holds
};

// what one wave writes is read by its other lanes: LDS executes a wave's instructions in order,
// so only the compiler has to be told
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float lane_value(float x, int lane /* wave-uniform */) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
}

// record `index` of running sums `ptr` over `rows` rows, clipped into them
__device__ __forceinline__ void record_rows(const int32_t* ptr, int index, int64_t rows,
                                            int64_t& lo, int64_t& hi) {
  lo = ptr[index];
  hi = ptr[index + 1];
  lo = lo < 0 ? 0 : lo > rows ? rows : lo;
  hi = hi < lo ? lo : hi > rows ? rows : hi;
}

__global__ __launch_bounds__(kAlignThreads) void k_align_local(const AlignArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, hq = lane >> 5;
  char* ring = smem + wave * kWaveLds;
  float* ring_f = reinterpret_cast<float*>(ring);
  float* a_inv = reinterpret_cast<float*>(ring + kRingBytes);   // [kStrip]
  float* b_s = a_inv + kStrip;                                  // [kSub]
  const int64_t slot = (int64_t)blockIdx.x * kAlignWaves + wave;
  const int64_t slots = (int64_t)gridDim.x * kAlignWaves;
  float2* carry = p.carry + slot * 2 * p.cap;
  const float go = p.gap_open, ge = p.gap_extend;
  const float minus_inf = -__builtin_inff();

  for (int64_t pair = slot; pair < p.P; pair += slots) {
    const int q = __builtin_amdgcn_readfirstlane(p.pairs[2 * pair]);
    const int rec = __builtin_amdgcn_readfirstlane(p.pairs[2 * pair + 1]);
    bool ok = (uint32_t)q < (uint32_t)p.records_a && (uint32_t)rec < (uint32_t)p.records_b;
    int64_t a_lo = 0, a_hi = 0, b_lo = 0, b_hi = 0;
    if (ok) {
      record_rows(p.ptr_a, q, p.n, a_lo, a_hi);
      record_rows(p.ptr_b, rec, p.m, b_lo, b_hi);
    }
    ok = ok && a_hi - a_lo <= GFY_ALIGN_ROWS_MAX && b_hi - b_lo <= GFY_ALIGN_ROWS_MAX &&
         b_hi - b_lo <= p.cap;
    const int lq = __builtin_amdgcn_readfirstlane(ok ? (int)(a_hi - a_lo) : 0);
    const int lr = __builtin_amdgcn_readfirstlane(ok ? (int)(b_hi - b_lo) : 0);
    const f16* rows_a = p.a + a_lo * 128;
    const f16* rows_b = p.b + b_lo * 128;

    float best = 0.f;   // strict >: only a positive cell is ever kept
    int best_i = -1, best_j = -1;

    // 32 b-rows from column c0 on as this lane's eight 16-byte pieces: piece lane + 64 x is
    // chunk lane & 15 of row (lane >> 4) + 4 x — a row on 16 consecutive lanes (row_square_sum)
    auto load_b = [&](f16x8 (&v)[8], int c0) __attribute__((always_inline)) {
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        const int col = c0 + (lane >> 4) + 4 * x;
        v[x] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (col < lr) v[x] = *reinterpret_cast<const f16x8*>(rows_b + (int64_t)col * 128 + (lane & 15) * 8);
      }
    };

    const int strips = lq > 0 && lr > 0 ? (lq + kStrip - 1) / kStrip : 0;
    for (int strip = 0; strip < strips; ++strip) {
      const int i0 = strip * kStrip;
      const int rows = lq - i0 < kStrip ? lq - i0 : kStrip;
      const bool onward = strip + 1 < strips;   // lane 63's row feeds another strip
      const float2* carry_in = carry + (size_t)((strip + 1) & 1) * p.cap;
      float2* carry_out = carry + (size_t)(strip & 1) * p.cap;

      // the strip's rows through the ring's first half (free: no column is in flight) into the
      // MFMA fragments, and 1 / |a_i| next to them
#pragma unroll 4
      for (int x = 0; x < 16; ++x) {
        const int row = (lane >> 4) + 4 * x, ch = lane & 15;
        f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (row < rows) v = *reinterpret_cast<const f16x8*>(rows_a + (int64_t)(i0 + row) * 128 + ch * 8);
        const float ss = row_square_sum(v);
        *reinterpret_cast<f16x8*>(ring + off256(row, ch)) = v;
        if (ch == 0) a_inv[row] = inverse_norm(ss);
      }
      wave_sync();
      f16x8 af[2][8];
#pragma unroll
      for (int at = 0; at < 2; ++at)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
          af[at][ks] = *reinterpret_cast<const f16x8*>(ring + off256(32 * at + r, 2 * ks + hq));
      const float a_term[2] = {a_inv[r], a_inv[32 + r]};
      wave_sync();

      float h = 0.f, e = minus_inf, f = minus_inf;   // this lane's last cell
      float diag = 0.f;                              // H of the row above, one column back
      f16x8 b_next[8];
      load_b(b_next, 0);
      // (H, F) of the row above the strip for columns c0 + lane, lanes 0..31
      auto load_carry = [&](int c0) __attribute__((always_inline)) {
        float2 v = make_float2(0.f, minus_inf);
        if (strip > 0 && lane < kSub && c0 + lane < lr) v = carry_in[c0 + lane];
        return v;
      };
      float2 carry_next = load_carry(0);

      const int steps = lr + rows - 1;
      for (int t0 = 0; t0 < steps; t0 += kSub) {
        if (t0 < lr) {   // columns t0 .. t0 + 31 join the ring
          char* stage = ring + (((t0 >> 5) + 3) & 3) * (kSub * 256);
#pragma unroll
          for (int x = 0; x < 8; ++x) {
            const int row = (lane >> 4) + 4 * x, ch = lane & 15;
            const float ss = row_square_sum(b_next[x]);
            *reinterpret_cast<f16x8*>(stage + off256(row, ch)) = b_next[x];
            if (ch == 0) b_s[row] = -inverse_norm(ss);   // s_j of k_row_terms
          }
          wave_sync();
          f32x16 acc[2];
          sweep_multiply<2, false>(acc, af, stage, 0, 0, r, hq);
          if (t0 + kSub < lr) load_b(b_next, t0 + kSub);
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int jl = 4 * hq + 8 * g;   // 4 consecutive b-rows
            const f32x4 sv = *reinterpret_cast<const f32x4*>(b_s + jl);
#pragma unroll
            for (int at = 0; at < 2; ++at)
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const float key = __builtin_fmaf(acc[at][4 * g + i], sv[i], 0.0f);
                const float cosine = pair_value(key, a_term[at], GFY_COSINE);
                const float score = __fadd_rn(__fmul_rn(cosine, p.match_scale), p.match_shift);
                const int row = 32 * at + r;
                ring_f[((t0 + jl + i + row) & 127) * kStrip + row] = score;
              }
          }
          wave_sync();
        }
        const float2 from_above = carry_next;
        carry_next = load_carry(t0 + kSub);
        const int t_end = t0 + kSub < steps ? t0 + kSub : steps;
        for (int t = t0; t < t_end; ++t) {
          const int j = t - lane;
          float up_h = __shfl_up(h, 1, 64), up_f = __shfl_up(f, 1, 64);
          const float above_h = lane_value(from_above.x, t - t0);
          const float above_f = lane_value(from_above.y, t - t0);
          if (lane == 0) up_h = above_h, up_f = above_f;
          const float s = ring_f[(t & 127) * kStrip + lane];
          const bool live = (uint32_t)j < (uint32_t)lr && lane < rows;
          const float e_new = __builtin_fmaxf(e - ge, h - go);
          const float f_new = __builtin_fmaxf(up_f - ge, up_h - go);
          const float h_new = __builtin_fmaxf(__builtin_fmaxf(0.f, diag + s),
                                              __builtin_fmaxf(e_new, f_new));
          e = live ? e_new : e;
          f = live ? f_new : f;
          h = live ? h_new : h;
          diag = live ? up_h : diag;
          const bool better = live && h_new > best;
          best = better ? h_new : best;
          best_i = better ? i0 + lane : best_i;
          best_j = better ? j : best_j;
          if (onward && lane == kStrip - 1 && live) carry_out[j] = make_float2(h_new, f_new);
        }
      }
      // the next strip reads what lane 63 stored (and restages the ring)
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      wave_sync();
    }

#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) {
      const float ob = __shfl_xor(best, mask, 64);
      const int oi = __shfl_xor(best_i, mask, 64), oj = __shfl_xor(best_j, mask, 64);
      const bool take = ob > best || (ob == best && (oi < best_i || (oi == best_i && oj < best_j)));
      best = take ? ob : best;
      best_i = take ? oi : best_i;
      best_j = take ? oj : best_j;
    }
    if (lane == 0) {
      const bool none = !(best > 0.f);
      p.out_score[pair] = ok ? (none ? 0.f : best) : __builtin_nanf("");
      p.out_end[2 * pair] = ok ? (none ? -1 : best_i) : -2;
      p.out_end[2 * pair + 1] = ok ? (none ? -1 : best_j) : -2;
    }
  }
}

int align_groups(int64_t pairs) {
  const int64_t groups = (pairs + kAlignWaves - 1) / kAlignWaves;
  return (int)(groups < 1 ? 1 : groups > kAlignGroupsMax ? kAlignGroupsMax : groups);
}

}  // namespace

// two carry buffers of max_rows_b (H, F) pairs per wave of the grid
size_t align_workspace_bytes(int64_t pairs, int64_t max_rows_b) {
  const size_t waves = (size_t)align_groups(pairs) * kAlignWaves;
  return align_up(waves * 2 * (size_t)max_rows_b * sizeof(float2) + 1, 256);
}

int launch_align_local(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                       const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                       const int32_t* pairs, int64_t P, float match_scale, float match_shift,
                       float gap_open, float gap_extend, float* out_score, int32_t* out_end,
                       void* ws, size_t ws_bytes, hipStream_t s) {
  GFY_REQUIRE(ws_bytes >= align_workspace_bytes(P, 0), GFY_ERR_WORKSPACE,
              "gfy_align_local: workspace %zu < required %zu", ws_bytes,
              align_workspace_bytes(P, 0));
  const int groups = align_groups(P);
  const size_t columns = ws_bytes / ((size_t)groups * kAlignWaves * 2 * sizeof(float2));
  static_assert(kAlignLds <= 160 * 1024, "the LDS of a compute unit");
  static PerDeviceOnce opt_in;
  if (const int rc = opt_in.run([]() -> int {
        GFY_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_align_local),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, kAlignLds));
        return GFY_OK;
      }))
    return rc;
  AlignArgs p{};
  p.a = (const f16*)a;
  p.b = (const f16*)b;
  p.ptr_a = ptr_a;
  p.ptr_b = ptr_b;
  p.pairs = pairs;
  p.n = n;
  p.m = m;
  p.P = P;
  p.records_a = (int)records_a;
  p.records_b = (int)records_b;
  p.match_scale = match_scale;
  p.match_shift = match_shift;
  p.gap_open = gap_open;
  p.gap_extend = gap_extend;
  p.out_score = out_score;
  p.out_end = out_end;
  p.carry = (float2*)ws;
  p.cap = (int)(columns < GFY_ALIGN_ROWS_MAX ? columns : GFY_ALIGN_ROWS_MAX);
  k_align_local<<<groups, kAlignThreads, kAlignLds, s>>>(p);
  GFY_CHECK_HIP(hipGetLastError());
  return GFY_OK;
}

}  // namespace gfy
