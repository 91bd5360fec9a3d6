// Per-position values of aligned paths (gfy_align_path_values; semantics: include/gfy.h): for
// every op of every path the cosine of its cell and the running score behind it, and per path
// the score, the counts of matches and gap runs and the float64 sum of the matched cosines.
//
// One wave owns one path; a workgroup is four waves that never meet, and a wave takes paths
// wave, wave + waves of the launch, ... until the list ends.
//   * A counting pass over the ops decides whether the path is followed at all: every byte is
//     0, 1 or 2 and the cell behind the last op lies inside the two records, so every cell in
//     front of it does (a path only moves down and right).  Nothing read from a device array is
//     followed unchecked, and a refused path gets NaN and status -2.
//   * The ops are then taken 64 at a time, lane = op.  The cell of an op is the start plus the
//     number of earlier ops that consume a row of A (0 and 2) and of B (0 and 1): two prefix
//     counts out of three ballots, with the totals carried from block to block.
//   * The cosine of a matched cell has to be the dense kernel's, bit for bit, and those bits come
//     out of one particular chain of eight MFMAs.  So the wave runs that chain: 32 ops at a time,
//     slot t of the b-operand holds the b-row of op t and slot t of the a-operand its a-row, the
//     fragments straight from global memory in the chunk order 2 ks + hq of sweep_multiply, and
//     element (t, t) of the 32 x 32 result is the dot product wanted (an element of an MFMA
//     result does not depend on where its rows sit in the tile: the box and band aligners move
//     rows to other slots and stay bit-identical).  1,024 products for 32 values, on purpose; a
//     path is a few hundred ops.  A gap op holds a valid row of the pair in its slot and its
//     element is dropped.  Norms, key, value and substitution score are the functions of
//     pairwise_sweep.inc in their own lane layout and the expressions of align_local.inc.
//   * Running score, counts and the float64 sum are an ordered chain by definition: a uniform
//     loop over the block's lanes reads lane k's op, score and cosine and carries h, the op
//     before, the counts and the sum from block to block.
#include "align_local.inc"   // wave_sync, lane_value, record_rows; pairwise_sweep.inc behind it

namespace gfy {
namespace {

constexpr int kValueWaves = 4;                  // paths in flight per workgroup
constexpr int kValueThreads = 64 * kValueWaves;
constexpr int kValueBlock = 64;                 // ops per block: lane = op
constexpr int kValueWavesMost = 4096;           // 16 per compute unit
constexpr int kOpsMost = 2 * GFY_ALIGN_ROWS_MAX;   // a path inside two records has no more

struct ValueKernelArgs {
  AlignArgs align;
  PathValueArgs values;
  int64_t waves;   // waves that take paths; the others return at once
};

__global__ __launch_bounds__(kValueThreads) void k_align_path_values(const ValueKernelArgs p) {
  __shared__ float shared[kValueWaves][3][kValueBlock];
  const AlignArgs& c = p.align;
  const PathValueArgs& v = p.values;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, hq = lane >> 5;
  float* a_inv = shared[wave][0];   // 1 / |a-row| of the block's ops
  float* b_s = shared[wave][1];     // s_j of k_row_terms of their b-rows
  float* dots = shared[wave][2];    // element (t, t) of the two products
  const int64_t slot = (int64_t)blockIdx.x * kValueWaves + wave;
  if (slot >= p.waves) return;
  const float go = c.gap_open, ge = c.gap_extend;
  const float nan = __builtin_nanf("");
  const uint64_t below = (1ull << lane) - 1;

  for (int64_t pair = slot; pair < c.P; pair += p.waves) {
    // the pair, wave-uniformly: its records and its slot of ops compared and clipped
    const int q = __builtin_amdgcn_readfirstlane(c.pairs[2 * pair]);
    const int rec = __builtin_amdgcn_readfirstlane(c.pairs[2 * pair + 1]);
    bool ok = (uint32_t)q < (uint32_t)c.records_a && (uint32_t)rec < (uint32_t)c.records_b;
    int64_t a_lo = 0, a_hi = 0, b_lo = 0, b_hi = 0;
    if (ok) {
      record_rows(c.ptr_a, q, c.n, a_lo, a_hi);
      record_rows(c.ptr_b, rec, c.m, b_lo, b_hi);
    }
    ok = ok && a_hi - a_lo <= GFY_ALIGN_ROWS_MAX && b_hi - b_lo <= GFY_ALIGN_ROWS_MAX;
    const int lq = __builtin_amdgcn_readfirstlane(ok ? (int)(a_hi - a_lo) : 0);
    const int lr = __builtin_amdgcn_readfirstlane(ok ? (int)(b_hi - b_lo) : 0);
    const f16* rows_a = c.a + a_lo * 128;
    const f16* rows_b = c.b + b_lo * 128;
    const int si = __builtin_amdgcn_readfirstlane(v.starts[2 * pair]);
    const int sj = __builtin_amdgcn_readfirstlane(v.starts[2 * pair + 1]);
    int64_t op_lo = v.op_ptr[pair], op_hi = v.op_ptr[pair + 1];
    // a slot outside ops is refused and nothing of it is touched; a path of more ops than two
    // records have rows leaves them, and is refused without being counted
    const bool slot_ok = op_lo >= 0 && op_lo <= op_hi && op_hi <= v.n_ops;
    op_lo = op_lo < 0 ? 0 : op_lo > v.n_ops ? v.n_ops : op_lo;
    op_hi = op_hi < op_lo ? op_lo : op_hi > v.n_ops ? v.n_ops : op_hi;
    if (!slot_ok) op_hi = op_lo;
    ok = ok && slot_ok && op_hi - op_lo <= kOpsMost;
    const int64_t length = op_hi - op_lo;

    // the counting pass: every op byte, and where the path ends
    if (ok) {
      int rows_used = 0, cols_used = 0;
      bool bytes_ok = true;
      for (int64_t x0 = 0; x0 < length; x0 += kValueBlock) {
        const bool active = x0 + lane < length;
        const int op = active ? (int)v.ops[op_lo + x0 + lane] : 3;
        const uint64_t m0 = __ballot(op == 0), m1 = __ballot(op == 1), m2 = __ballot(op == 2);
        bytes_ok = bytes_ok && __ballot(active && op > 2) == 0;
        rows_used += __popcll(m0 | m2);
        cols_used += __popcll(m0 | m1);
      }
      const bool none = si == -1 && sj == -1;   // only an empty path may start there
      // no sum with a start, which may be any 32-bit number: the counts are at most kOpsMost
      // and a record has at most GFY_ALIGN_ROWS_MAX rows, so the differences cannot wrap
      ok = bytes_ok && (none ? length == 0
                             : si >= 0 && sj >= 0 && si <= lq - rows_used && sj <= lr - cols_used);
    }
    if (!ok) {
      for (int64_t x = lane; x < length; x += kValueBlock) {
        v.out_cosine[op_lo + x] = nan;
        v.out_running[op_lo + x] = nan;
      }
      if (lane == 0) {
        v.out_score[pair] = nan;
        v.out_cosine_sum[pair] = (double)nan;
        v.out_counts[4 * pair] = 0, v.out_counts[4 * pair + 1] = 0;
        v.out_counts[4 * pair + 2] = 0, v.out_counts[4 * pair + 3] = -2;
      }
      continue;
    }

    float h = 0.f;         // the running score
    int before = 0;        // the op in front: a gap op continues a run of its own kind only
    int matches = 0, runs_b = 0, runs_a = 0;
    double cosine_sum = 0.0;
    int base_i = si, base_j = sj;   // the cell of the block's first op
    for (int64_t x0 = 0; x0 < length; x0 += kValueBlock) {
      const int here = length - x0 < kValueBlock ? (int)(length - x0) : kValueBlock;
      const bool active = lane < here;
      const int op = active ? (int)v.ops[op_lo + x0 + lane] : 3;
      const uint64_t m0 = __ballot(op == 0), m1 = __ballot(op == 1), m2 = __ballot(op == 2);
      const int i = base_i + __popcll((m0 | m2) & below);
      const int j = base_j + __popcll((m0 | m1) & below);
      base_i += __popcll(m0 | m2);
      base_j += __popcll(m0 | m1);

      float cosine = nan, score = 0.f;
      if (m0 != 0) {   // wave-uniform; a matched cell exists, so both records have a row
        // a gap op and a lane past the path's end hold a valid row of the pair; clipped from
        // both sides, so that a row index is inside its record whatever the counting pass let by
        const int row_a = i < 0 ? 0 : i < lq - 1 ? i : lq - 1;
        const int row_b = j < 0 ? 0 : j < lr - 1 ? j : lr - 1;
        // the norms in the layout of row_square_sum: a row on 16 consecutive lanes, piece
        // lane + 64 x is chunk lane & 15 of the rows of op (lane >> 4) + 4 x.  Every row of the
        // block is read twice, here and as MFMA fragments below: the norms need this layout to
        // be the dense kernel's bits, and the second read is expected to hit in cache
#pragma unroll 4
        for (int x = 0; x < 16; ++x) {
          const int t = (lane >> 4) + 4 * x, ch = lane & 15;
          const int ta = __shfl(row_a, t, 64), tb = __shfl(row_b, t, 64);
          const f16x8 va = *reinterpret_cast<const f16x8*>(rows_a + (int64_t)ta * 128 + ch * 8);
          const f16x8 vb = *reinterpret_cast<const f16x8*>(rows_b + (int64_t)tb * 128 + ch * 8);
          const float ssa = row_square_sum(va), ssb = row_square_sum(vb);
          if (ch == 0) {
            a_inv[t] = inverse_norm(ssa);
            b_s[t] = -inverse_norm(ssb);   // s_j of k_row_terms
          }
        }
        // the products, 32 ops at a time: the eight steps of sweep_multiply, b the first operand
        // and a the second, the accumulator from 0
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          if ((uint32_t)(m0 >> (32 * half)) == 0) continue;   // wave-uniform: no match in it
          const int ta = __shfl(row_a, 32 * half + r, 64), tb = __shfl(row_b, 32 * half + r, 64);
          const f16* from_a = rows_a + (int64_t)ta * 128 + hq * 8;
          const f16* from_b = rows_b + (int64_t)tb * 128 + hq * 8;
          f16x8 af[8], bf[8];
#pragma unroll
          for (int ks = 0; ks < 8; ++ks) {
            af[ks] = *reinterpret_cast<const f16x8*>(from_a + 16 * ks);   // chunk 2 ks + hq
            bf[ks] = *reinterpret_cast<const f16x8*>(from_b + 16 * ks);
          }
          const f32x16 start = {};
          f32x16 acc = start;
#pragma unroll
          for (int ks = 0; ks < 8; ++ks)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(bf[ks], af[ks], ks == 0 ? start : acc,
                                                         0, 0, 0);
          // the a-slot is the lane's r, the b-slots of its registers are 8 (reg >> 2) + 4 hq +
          // (reg & 3): slot r is register 4 (r >> 3) + (r & 3) of the half with hq == (r >> 2) & 1
          float own = 0.f;
#pragma unroll
          for (int reg = 0; reg < 16; ++reg)
            own = reg == 4 * (r >> 3) + (r & 3) ? acc[reg] : own;
          if (hq == ((r >> 2) & 1)) dots[32 * half + r] = own;
        }
        wave_sync();
        if (op == 0) {
          // the expressions of align_local.inc's epilogue
          const float key = __builtin_fmaf(dots[lane], b_s[lane], 0.0f);
          cosine = pair_value(key, a_inv[lane], GFY_COSINE);
          score = __fadd_rn(__fmul_rn(cosine, c.match_scale), c.match_shift);
        }
        wave_sync();   // the next block writes the three arrays again
      }

      // the ordered chain, wave-uniformly
      float running = 0.f;
      for (int k = 0; k < here; ++k) {
        const int op_k = __builtin_amdgcn_readlane(op, k);
        if (op_k == 0) {
          h = __fadd_rn(h, lane_value(score, k));
          cosine_sum += (double)lane_value(cosine, k);
          ++matches;
        } else {
          h = __fsub_rn(h, op_k == before ? ge : go);
          if (op_k != before) op_k == 1 ? ++runs_b : ++runs_a;
        }
        before = op_k;
        running = lane == k ? h : running;
      }
      if (active) {
        v.out_cosine[op_lo + x0 + lane] = cosine;
        v.out_running[op_lo + x0 + lane] = running;
      }
    }
    if (lane == 0) {
      v.out_score[pair] = h;
      v.out_cosine_sum[pair] = cosine_sum;
      v.out_counts[4 * pair] = matches, v.out_counts[4 * pair + 1] = runs_b;
      v.out_counts[4 * pair + 2] = runs_a, v.out_counts[4 * pair + 3] = 0;
    }
  }
}

}  // namespace

int launch_align_path_values(const AlignArgs& call, const PathValueArgs& values, int64_t max_waves,
                             hipStream_t s) {
  ValueKernelArgs p{call, values, 0};
  const int64_t most = max_waves > 0 && max_waves < kValueWavesMost ? max_waves : kValueWavesMost;
  p.waves = call.P < most ? call.P : most;
  k_align_path_values<<<(int)((p.waves + kValueWaves - 1) / kValueWaves), kValueThreads, 0, s>>>(p);
  GFY_CHECK_HIP(hipGetLastError());
  return GFY_OK;
}

}  // namespace gfy
