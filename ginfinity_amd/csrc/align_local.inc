// The one alignment loop of the library (semantics: include/gfy.h), shared by the kernels of
// align_kernels.hip: k_align_local (mode 0: score and end), k_align_span (kSpan: score, start and
// end) and k_align_trace (kTrace: the aligned path of a given box), their three twins inside a
// band of diagonals (| kBand), the score and span kernels inside a box of rows the caller names
// (| kBand | kBox), the two global kernels (kGlobal) and their twins inside such a box (| kBox),
// and the score kernel of shuffled b-sides (kBand | kBox | kOrder), as pairwise_topk.inc is
// shared by the top-k family.
//
// One wave owns one pair; a workgroup is four waves that never meet (no barrier, no flag), and a
// wave takes pairs wave, wave + waves of the grid, ... until the list ends.
//   * The wave walks the a-record in strips of 64 rows, lane = row, and sweeps the b-record with
//     the usual skew: at step t lane l is at column t - l.  H and F of the row above come from
//     lane l - 1 (one wave shift each), H of the diagonal is last step's H from above, E and H
//     of the left neighbour are the lane's own registers.  Every cell is the fixed expression of
//     include/gfy.h of its three predecessors, so nothing depends on the schedule.
//   * The substitution scores come 32 columns at a time, through the one multiply of the library,
//     into a ring of 128 anti-diagonals in LDS of which a step reads one.
//   * The strip's last row goes to the workspace as lane 63 forms it and comes back to lane 0 of
//     the next strip 32 columns at a time, one load ahead, two buffers in turn.
//   * Each lane keeps its best cell and one butterfly at the end orders them.
// What a pair needs before and after its strips stands in front of the loop: resolve_pair (the
// pair's rows, its band, its box), trace_walk (kTrace: the path) and finish_pair (score, end
// and start).  align_pairs itself is the pair loop and, inline, the strip loop: stage the strip,
// the borders of kGlobal, the carry, the 32-column blocks and the cell step; what each mode adds
// is said at the statement that does it.  (The strip loop stays in one body on purpose: taking
// any of its parts out, as a function or as a lambda, changed the kernels' register counts.)
// ptr_a, ptr_b and pairs are device arrays: they are compared and clipped, a pair outside them or
// longer than the limits gets NaN and (-2, -2), and nothing outside the caller's buffers is read.
#pragma once
#include <type_traits>

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
constexpr int kOriginBits = 12;                // an origin is (i0 << 12) | j0
static_assert(kRingBytes == kBuffers * (kSub * 256), "a quarter of the ring stages 32 b-rows");
static_assert(kAlignLds <= 160 * 1024, "the LDS of a compute unit");
static_assert(GFY_ALIGN_ROWS_MAX == 1 << kOriginBits, "both coordinates of an origin fit its word");

// (AlignArgs, TraceArgs and OrderArgs, the kernels' arguments, and AlignMode, the modes of
// align_pairs<kMode>: gfy_common.h)

// a carry entry: (H, F) of a column, and with kSpan their origins behind them
template <bool kSpan>
using AlignCarry = std::conditional_t<kSpan, u32x4, float2>;

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

// a pair, resolved: with ok == false lq = lr = 0 and the pair gets the refusal values
struct AlignPair {
  bool ok;
  int lq, lr;            // rows of A and B that are aligned (kTrace, kBox: the box's sizes)
  const f16* rows_a;
  const f16* rows_b;
  int lo, hi;            // kBand: the band, clipped (kTrace, kBox: in the box's coordinates)
  int box_i, box_j;      // kBox: the box's first cell in the records' coordinates
  int64_t op_lo;         // kTrace: where the pair's slot starts
  int dir_pitch;         // kTrace: words of a row of the box
  const int32_t* order;  // kOrder: the lr entries of the virtual pair, every one in 0 .. lr - 1
};

// The pair, wave-uniformly: its records compared and clipped, and what the modes add to it.
//   kBand: the pair has a band (lo, hi) of diagonals d = j - i, both ends inclusive, read like the
//     pair itself from `bands` and clipped into +-GFY_ALIGN_ROWS_MAX; lo > hi is refused like a
//     pair out of range.  A cell outside the band is outside the matrix (H = 0, E = F = -inf, no
//     origin).
//   kTrace (without kSpan): the pair's records are replaced by the box start..end the caller names
//     (a-rows from start_i, b-rows from start_j, lq and lr the box's sizes; read from device
//     arrays, compared and clipped like the records).  With kBand the trace takes the band in the
//     records' coordinates and shifts it by start_j - start_i itself.
//   kTrace and kGlobal: the box is rows 0 .. Lq - 1 and columns 0 .. end_j, whose top-left corner
//     is the matrix's own.
//   kBox: the pair has a box (i_lo, i_hi, j_lo, j_hi) of rows of the two records, both ends
//     inclusive, read like the band from `boxes` and clipped into +-GFY_ALIGN_ROWS_MAX; i_lo > i_hi
//     or j_lo > j_hi as given is refused like a band with lo > hi.  The box is then clipped into
//     the records and replaces them as kTrace's box does: a-rows from i_lo, b-rows from j_lo, lq
//     and lr the box's sizes, the band shifted by j_lo - i_lo.  A box that holds no cell leaves lq
//     = lr = 0, the pair of a record of zero rows.  The carry has to hold the box's columns, not
//     the record's.  A null `bands` is the covering band.
//   kBox and kGlobal: there is no band; the box is the matrix, so row -1 and column -1 of the
//     definition are the rows just outside it and the loop needs nothing more.
//   kTrace, kGlobal and kBox: the caller's box is applied FIRST, and the checks of kTrace and
//     kGlobal then run on the box's sizes, with the given end shifted by -(i_lo, j_lo).
//   kOrder: `pair` is the virtual pair v = p * shuffles + k (p.P counts those); the records, the
//     band and the box are pair p's, and a null `boxes` is the covering box.  The b-side has
//     `side` columns: the b-rows of the box clipped into the record, whatever the a-side holds.
//     The orders of pair p lie back to back from order_ptr[p], `side` entries each; an order_ptr
//     that is negative or whose difference is not shuffles * side is refused, and so is a virtual
//     pair with an entry outside 0 .. side - 1: the 64 lanes read its entries once, here, before
//     any of them becomes an address.  (load_b compares again where it forms the address.)
template <unsigned kMode>
__device__ __forceinline__ void resolve_pair(const AlignArgs& p, const TraceArgs* trace,
                                             const OrderArgs* orders, bool within, int64_t pair,
                                             AlignPair& pr) {
  constexpr bool kTrace = kMode & AlignMode::kTrace, kGlobal = kMode & AlignMode::kGlobal;
  constexpr bool kBand = kMode & AlignMode::kBand, kBox = kMode & AlignMode::kBox;
  constexpr bool kOrder = kMode & AlignMode::kOrder;
  int shuffle = 0;   // kOrder: k of the virtual pair
  if constexpr (kOrder) {
    shuffle = (int)(pair % orders->shuffles);
    pair /= orders->shuffles;
  }
  const int q = __builtin_amdgcn_readfirstlane(p.pairs[2 * pair]);
  const int rec = __builtin_amdgcn_readfirstlane(p.pairs[2 * pair + 1]);
  bool ok = (uint32_t)q < (uint32_t)p.records_a && (uint32_t)rec < (uint32_t)p.records_b;
  int64_t a_lo = 0, a_hi = 0, b_lo = 0, b_hi = 0;
  int lo = 0, hi = 0;   // kBand: the band, from here on clipped
  int i_lo = 0, i_hi = 0, j_lo = 0, j_hi = 0;   // kBox: the box, from here on clipped
  if constexpr (kBox) {
    constexpr int most = GFY_ALIGN_ROWS_MAX;
    if (kOrder && p.boxes == nullptr) {   // a call without a box: the covering one
      i_lo = -most, i_hi = most, j_lo = -most, j_hi = most;
    } else {
      i_lo = __builtin_amdgcn_readfirstlane(p.boxes[4 * pair]);
      i_hi = __builtin_amdgcn_readfirstlane(p.boxes[4 * pair + 1]);
      j_lo = __builtin_amdgcn_readfirstlane(p.boxes[4 * pair + 2]);
      j_hi = __builtin_amdgcn_readfirstlane(p.boxes[4 * pair + 3]);
    }
    ok = ok && i_lo <= i_hi && j_lo <= j_hi;
    i_lo = i_lo < -most ? -most : i_lo > most ? most : i_lo;
    i_hi = i_hi < -most ? -most : i_hi > most ? most : i_hi;
    j_lo = j_lo < -most ? -most : j_lo > most ? most : j_lo;
    j_hi = j_hi < -most ? -most : j_hi > most ? most : j_hi;
  }
  if constexpr (kBand) {
    if (!kBox || p.bands != nullptr) {
      lo = __builtin_amdgcn_readfirstlane(p.bands[2 * pair]);
      hi = __builtin_amdgcn_readfirstlane(p.bands[2 * pair + 1]);
    } else {   // kBox, a call without a band: the covering one
      lo = -GFY_ALIGN_ROWS_MAX, hi = GFY_ALIGN_ROWS_MAX;
    }
    ok = ok && lo <= hi;
    lo = lo < -GFY_ALIGN_ROWS_MAX ? -GFY_ALIGN_ROWS_MAX : lo > GFY_ALIGN_ROWS_MAX ? GFY_ALIGN_ROWS_MAX : lo;
    hi = hi < -GFY_ALIGN_ROWS_MAX ? -GFY_ALIGN_ROWS_MAX : hi > GFY_ALIGN_ROWS_MAX ? GFY_ALIGN_ROWS_MAX : hi;
  }
  if (ok) {
    record_rows(p.ptr_a, q, p.n, a_lo, a_hi);
    record_rows(p.ptr_b, rec, p.m, b_lo, b_hi);
  }
  ok = ok && a_hi - a_lo <= GFY_ALIGN_ROWS_MAX && b_hi - b_lo <= GFY_ALIGN_ROWS_MAX &&
       (kTrace || kBox || b_hi - b_lo <= p.cap);
  pr.op_lo = 0;
  pr.box_i = 0, pr.box_j = 0;
  pr.order = nullptr;
  if constexpr (kBox) {
    // the box inside the records; a record of more than GFY_ALIGN_ROWS_MAX rows is refused above
    const int full_q = ok ? (int)(a_hi - a_lo) : 0, full_r = ok ? (int)(b_hi - b_lo) : 0;
    i_lo = i_lo < 0 ? 0 : i_lo;
    j_lo = j_lo < 0 ? 0 : j_lo;
    i_hi = i_hi > full_q - 1 ? full_q - 1 : i_hi;
    j_hi = j_hi > full_r - 1 ? full_r - 1 : j_hi;
    const bool box = ok && i_lo <= i_hi && j_lo <= j_hi;   // it holds a cell
    const int box_rows = box ? i_hi - i_lo + 1 : 0, box_cols = box ? j_hi - j_lo + 1 : 0;
    ok = ok && box_cols <= p.cap;
    if constexpr (kOrder) {
      const int side = ok && j_lo <= j_hi ? j_hi - j_lo + 1 : 0;
      int64_t first = 0, behind = 0;
      if (ok) first = orders->order_ptr[pair], behind = orders->order_ptr[pair + 1];
      ok = ok && first >= 0 && behind - first == (int64_t)orders->shuffles * side;
      const int32_t* mine = orders->order + first + (int64_t)shuffle * side;
      bool wrong = false;
      if (ok)
        for (int x = threadIdx.x & 63; x < side; x += 64)
          wrong = wrong || (uint32_t)mine[x] >= (uint32_t)side;
      ok = ok && __builtin_amdgcn_ballot_w64(wrong) == 0;
      pr.order = mine;
    }
    pr.box_i = box ? i_lo : 0, pr.box_j = box ? j_lo : 0;
    if constexpr (kBand) {   // the band in the box's coordinates
      lo -= pr.box_j - pr.box_i;
      hi -= pr.box_j - pr.box_i;
    }
    a_lo += pr.box_i;
    b_lo += pr.box_j;
    a_hi = a_lo + box_rows;
    b_hi = b_lo + box_cols;
  }
  if constexpr (kTrace) {
    // only a box that the span call (kGlobal: gfy_align_global) can have named, that fits the
    // wave's region and whose path fits the slot is followed; (-1, -1) is the empty alignment
    int si = 0, sj = 0;   // kGlobal: the box starts at the matrix's corner
    if constexpr (!kGlobal) {
      si = __builtin_amdgcn_readfirstlane(trace->starts[2 * pair]);
      sj = __builtin_amdgcn_readfirstlane(trace->starts[2 * pair + 1]);
    }
    int ei = __builtin_amdgcn_readfirstlane(trace->ends[2 * pair]);
    int ej = __builtin_amdgcn_readfirstlane(trace->ends[2 * pair + 1]);
    pr.op_lo = trace->op_ptr[pair];
    const int64_t op_hi = trace->op_ptr[pair + 1];
    bool none, box;
    int64_t box_rows, box_cols;
    if constexpr (kGlobal) {
      // rows 0 .. Lq - 1 and columns 0 .. end_j of the records (kBox: of the caller's box, which
      // stands in the records' place by now, the end in its coordinates)
      const int64_t full_q = a_hi - a_lo, full_r = b_hi - b_lo;
      none = ei == -1 && ej == -1;
      if constexpr (kBox) ei -= pr.box_i, ej -= pr.box_j;
      box = ok && !none && ei == full_q - 1 && ej >= 0 && ej < full_r &&
            (within || ej == full_r - 1);
      box_rows = box ? full_q : 0, box_cols = box ? (int64_t)ej + 1 : 0;
    } else {
      // the box inside the records
      none = si == -1 && sj == -1;
      box = ok && !none && si >= 0 && sj >= 0 && si <= ei && sj <= ej && ei < a_hi - a_lo &&
            ej < b_hi - b_lo;
      box_rows = box ? ei - si + 1 : 0, box_cols = box ? ej - sj + 1 : 0;
    }
    // a local path has at most rows + cols - 1 ops; a global one may be all gaps
    const int64_t ops_most = box_rows + box_cols - (kGlobal ? 0 : 1);
    box = box && box_cols <= p.cap && box_rows * ((box_cols + 7) >> 3) <= trace->region_words &&
          pr.op_lo >= 0 && op_hi - pr.op_lo >= ops_most;
    ok = ok && (none || box);
    if constexpr (kBand) {   // the band in the box's coordinates
      lo -= box ? sj - si : 0;
      hi -= box ? sj - si : 0;
    }
    a_lo += box ? si : 0;
    b_lo += box ? sj : 0;
    a_hi = a_lo + (box ? box_rows : 0);
    b_hi = b_lo + (box ? box_cols : 0);
  }
  pr.ok = ok;
  pr.lo = lo, pr.hi = hi;
  pr.lq = __builtin_amdgcn_readfirstlane(ok ? (int)(a_hi - a_lo) : 0);
  pr.lr = __builtin_amdgcn_readfirstlane(ok ? (int)(b_hi - b_lo) : 0);
  pr.rows_a = p.a + a_lo * 128;
  pr.rows_b = p.b + b_lo * 128;
  pr.dir_pitch = (pr.lr + 7) >> 3;
}

// kTrace: after the last strip (behind the fence the carry hand-over uses) the wave walks back
// from the box's last cell, uniformly: the 64 lanes load the words of the diagonal behind the
// current cell at once, so a run of matches costs one load per 64 ops, a gap position one load
// each.  The ops go to the ring (free by then) in reverse, one byte each, and the lanes copy them
// forward into the pair's slot.  h_last is a lane's H when its strip ended: H of the box's last
// cell is the last H of the lane that owns its row.
//   kGlobal: the walk has no "starts here", leaves the box over a border and the lanes add the
//     border's ops behind it; any H is walked back from, and a path that is all gaps has Lq + Lr
//     ops.  start_j is the first row of B the path consumes.  kBox: lq and lr are the box's, so
//     are the borders, and the start goes back into the records' coordinates.
//   kBand: a box whose last cell lies outside the band has no path.
template <unsigned kMode>
__device__ __forceinline__ void trace_walk(int lane, char* ring, const uint32_t* dir,
                                           const AlignPair& pr, const TraceArgs* trace,
                                           bool within, int64_t pair, int strips, float h_last,
                                           int32_t* out_start) {
  constexpr bool kGlobal = kMode & AlignMode::kGlobal, kBand = kMode & AlignMode::kBand;
  constexpr bool kBox = kMode & AlignMode::kBox;
  const int lq = pr.lq, lr = pr.lr;
  int length = 0;
  int start_j = 0;
  bool corner = strips > 0;   // the box's last cell exists (kBand: and lies in the band)
  if constexpr (kBand) corner = corner && (uint32_t)(lr - lq - pr.lo) <= (uint32_t)(pr.hi - pr.lo);
  if (corner && (kGlobal || lane_value(h_last, (lq - 1) & (kStrip - 1)) > 0.f)) {
    uint8_t* reversed = reinterpret_cast<uint8_t*>(ring);   // <= 8192 ops of a byte
    const int limit = lq + lr - (kGlobal ? 0 : 1);
    int i = lq - 1, j = lr - 1, state = 0;   // 0 in H, 1 in E, 2 in F
    int anchor_i = -1, anchor_j = -1;        // lane l holds the word of cell anchor - (l, l)
    uint32_t window = 0;
    while (length < limit && i >= 0 && j >= 0) {
      int k = anchor_i - i;
      if ((uint32_t)k >= 64u || anchor_j - j != k) {
        anchor_i = i, anchor_j = j, k = 0;
        const int wi = i - lane, wj = j - lane;
        window = 0;
        if (wi >= 0 && wj >= 0)
          window = __hip_atomic_load(dir + (size_t)wi * pr.dir_pitch + (wj >> 3),
                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      const uint32_t bits = ((uint32_t)__builtin_amdgcn_readlane((int)window, k) >> (4 * (j & 7))) & 15u;
      int op;
      bool last = false;
      if (state == 0) {
        const uint32_t how = bits & 3u;
        if (how >= 2u) {   // H is E's or F's value: the same cell in that state
          state = (int)how - 1;
          continue;
        }
        op = 0, last = !kGlobal && how == 0u;
        --i, --j;
      } else if (state == 1) {
        op = 1, state = bits & 4u ? 0 : 1;
        --j;
      } else {
        op = 2, state = bits & 8u ? 0 : 2;
        --i;
      }
      if (lane == 0) reversed[length] = (uint8_t)op;
      ++length;
      if (last) break;
    }
    if constexpr (kGlobal) {
      // the walk left the box in H (a gap that reaches a border opened there).  The left
      // border is a charged gap of i + 1 rows of A, the top border one of j + 1 rows of B, or
      // with `within` free: the path starts behind it.  They are the path's first ops.
      int more = 0, op = 2;
      if (j < 0) more = i + 1;
      else if (i < 0 && within) start_j = j + 1;
      else if (i < 0) more = j + 1, op = 1;
      more = more < limit - length ? more : limit - length;
      wave_sync();
      for (int x = lane; x < more; x += 64) reversed[length + x] = (uint8_t)op;
      length += more;
    }
    wave_sync();
    for (int x = lane; x < length; x += 64) trace->out_ops[pr.op_lo + x] = reversed[length - 1 - x];
    wave_sync();   // the next pair restages the ring
  }
  if (lane == 0) trace->out_len[pair] = pr.ok ? length : -2;
  if constexpr (kGlobal) {
    int start_i = 0;
    if constexpr (kBox) start_i = pr.box_i, start_j += pr.box_j;
    if (lane == 0) {
      out_start[2 * pair] = pr.ok ? (strips > 0 ? start_i : -1) : -2;
      out_start[2 * pair + 1] = pr.ok ? (strips > 0 ? start_j : -1) : -2;
    }
  }
}

// The pair's result (kOrder: the virtual pair's, the score alone).  kGlobal: the last cell, or (within) the first best cell of the last row:
// one lane holds either.  Otherwise one butterfly orders the lanes' best cells by (score
// descending, i ascending, j ascending), and with kSpan the origin goes along.  kBox: the cells
// of a positive score (kGlobal: a real end) go back into the records' coordinates; (-1, -1) and
// (-2, -2) stay.
template <unsigned kMode>
__device__ __forceinline__ void finish_pair(const AlignArgs& p, int lane, const AlignPair& pr,
                                            bool within, int64_t pair, int strips, float h_last,
                                            float best, int best_i, int best_j,
                                            uint32_t best_o, int32_t* out_start) {
  constexpr bool kSpan = kMode & AlignMode::kSpan, kGlobal = kMode & AlignMode::kGlobal;
  constexpr bool kBox = kMode & AlignMode::kBox, kOrder = kMode & AlignMode::kOrder;
  const bool ok = pr.ok;
  if constexpr (kGlobal) {
    const int owner = (pr.lq - 1) & (kStrip - 1);
    const float score = within ? lane_value(best, owner) : lane_value(h_last, owner);
    int end_i = pr.lq - 1;
    int end_j = within ? __builtin_amdgcn_readlane(best_j, owner) : pr.lr - 1;
    if constexpr (kBox) end_i += pr.box_i, end_j += pr.box_j;
    if (lane == 0) {
      const bool none = strips == 0;   // a record (kBox: a box) of zero rows: nothing to align
      p.out_score[pair] = ok ? (none ? 0.f : score) : __builtin_nanf("");
      p.out_end[2 * pair] = ok ? (none ? -1 : end_i) : -2;
      p.out_end[2 * pair + 1] = ok ? (none ? -1 : end_j) : -2;
    }
  } else {
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) {
      const float ob = __shfl_xor(best, mask, 64);
      const int oi = __shfl_xor(best_i, mask, 64), oj = __shfl_xor(best_j, mask, 64);
      const bool take = ob > best || (ob == best && (oi < best_i || (oi == best_i && oj < best_j)));
      if constexpr (kSpan) {
        const uint32_t oo = (uint32_t)__shfl_xor((int)best_o, mask, 64);
        best_o = take ? oo : best_o;
      }
      best = take ? ob : best;
      best_i = take ? oi : best_i;
      best_j = take ? oj : best_j;
    }
    if (lane == 0) {
      const bool none = !(best > 0.f);
      int start_i = 0, start_j = 0;   // kSpan: the origin
      if constexpr (kSpan) {
        start_i = (int)(best_o >> kOriginBits);
        start_j = (int)(best_o & ((1u << kOriginBits) - 1));
      }
      if constexpr (kBox) {
        best_i += pr.box_i, best_j += pr.box_j;
        start_i += pr.box_i, start_j += pr.box_j;
      }
      p.out_score[pair] = ok ? (none ? 0.f : best) : __builtin_nanf("");
      if constexpr (!kOrder) {   // kOrder: a cell of a shuffled matrix names no row of the record
        p.out_end[2 * pair] = ok ? (none ? -1 : best_i) : -2;
        p.out_end[2 * pair + 1] = ok ? (none ? -1 : best_j) : -2;
      }
      if constexpr (kSpan) {
        out_start[2 * pair] = ok ? (none ? -1 : start_i) : -2;
        out_start[2 * pair + 1] = ok ? (none ? -1 : start_j) : -2;
      }
    }
  }
}

// out_start ([P][2]) is written with kSpan, and with kTrace and kGlobal together; trace is read
// with kTrace alone, within (wave-uniform) with kGlobal alone, p.bands with kBand alone, p.boxes
// with kBox alone, orders with kOrder alone (p.P then counts the virtual pairs and p.out_end is
// not written)
template <unsigned kMode>
__device__ __forceinline__ void align_pairs(const AlignArgs& p, int32_t* out_start,
                                            const TraceArgs* trace = nullptr,
                                            bool within = false,
                                            const OrderArgs* orders = nullptr) {
  constexpr bool kSpan = kMode & AlignMode::kSpan, kTrace = kMode & AlignMode::kTrace;
  constexpr bool kGlobal = kMode & AlignMode::kGlobal, kBand = kMode & AlignMode::kBand;
  constexpr bool kOrder = kMode & AlignMode::kOrder;
  static_assert(!kOrder || kMode == (AlignMode::kBand | AlignMode::kBox | AlignMode::kOrder),
                "orders come with the one score kernel that takes a band, a box, both or neither");
  static_assert(!(kSpan && kTrace), "the trace runs on the plain (H, F) carry");
  static_assert(!(kSpan && kGlobal), "a global alignment starts at the matrix's corner");
  static_assert(!(kBand && kGlobal), "a band on the global modes: borders that leave the band");
  static_assert(!(kMode & AlignMode::kBox) || kBand || kGlobal,
                "a box comes with a band (local) or with the global modes");
  static_assert(!((kMode & AlignMode::kBox) && kTrace) || kGlobal,
                "a local path needs no boxed trace: start..end lies inside the box");
  using Carry = AlignCarry<kSpan>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, hq = lane >> 5;
  char* ring = smem + wave * kWaveLds;
  float* ring_f = reinterpret_cast<float*>(ring);
  float* a_inv = reinterpret_cast<float*>(ring + kRingBytes);   // [kStrip]
  float* b_s = a_inv + kStrip;                                  // [kSub]
  const int64_t slot = (int64_t)blockIdx.x * kAlignWaves + wave;
  int64_t slots = (int64_t)gridDim.x * kAlignWaves;
  Carry* carry = reinterpret_cast<Carry*>(p.carry) + slot * 2 * p.cap;
  uint32_t* dir = nullptr;   // kTrace: the wave's direction words
  if constexpr (kTrace) {
    if (slot >= trace->waves) return;
    slots = trace->waves;
    char* mine = reinterpret_cast<char*>(p.carry) + slot * trace->wave_bytes;
    carry = reinterpret_cast<Carry*>(mine);
    dir = reinterpret_cast<uint32_t*>(mine + (size_t)2 * p.cap * sizeof(Carry));
  }
  const float go = p.gap_open, ge = p.gap_extend;
  const float minus_inf = -__builtin_inff();

  for (int64_t pair = slot; pair < p.P; pair += slots) {
    AlignPair pr;
    resolve_pair<kMode>(p, trace, orders, within, pair, pr);
    const int lq = pr.lq, lr = pr.lr, lo = pr.lo, hi = pr.hi, dir_pitch = pr.dir_pitch;
    const f16* rows_a = pr.rows_a;
    const f16* rows_b = pr.rows_b;

    // strict >: only a positive cell is ever kept; kGlobal: any cell of row Lq - 1
    float best = kGlobal ? -__builtin_inff() : 0.f;
    int best_i = -1, best_j = -1;
    uint32_t best_o = 0;   // kSpan: the origin of the best cell
    float h_last = 0.f;                    // kTrace, kGlobal: a lane's H when its strip ended
    float left_run = 0.f;                  // kGlobal: H[i0 - 1][-1], down the left border

    // kOrder: the rows that the columns of the NEXT load_b hold, order[col] for this lane's eight
    // columns.  They are loaded one tile ahead of the rows, as the rows are one tile ahead of the
    // multiply, so the dependent load stands in front of the prefetch and not in the step loop.
    int rows_next[kOrder ? 8 : 1];
    auto load_order = [&](int c0) __attribute__((always_inline)) {
      if constexpr (kOrder) {
#pragma unroll
        for (int x = 0; x < 8; ++x) {
          const int col = c0 + (lane >> 4) + 4 * x;
          rows_next[x] = col < lr ? pr.order[col] : 0;
        }
      }
    };
    // 32 b-rows from column c0 on as this lane's eight 16-byte pieces: piece lane + 64 x is
    // chunk lane & 15 of row (lane >> 4) + 4 x — a row on 16 consecutive lanes (row_square_sum).
    // kOrder: the row of column col is rows_next's, compared once more before it is an address.
    auto load_b = [&](f16x8 (&v)[8], int c0) __attribute__((always_inline)) {
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        const int col = c0 + (lane >> 4) + 4 * x;
        v[x] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if constexpr (kOrder) {
          const int row = rows_next[x];
          if (col < lr && (uint32_t)row < (uint32_t)lr)
            v[x] = *reinterpret_cast<const f16x8*>(rows_b + (int64_t)row * 128 + (lane & 15) * 8);
        } else {
          if (col < lr) v[x] = *reinterpret_cast<const f16x8*>(rows_b + (int64_t)col * 128 + (lane & 15) * 8);
        }
      }
    };

    const int strips = lq > 0 && lr > 0 ? (lq + kStrip - 1) / kStrip : 0;
    for (int strip = 0; strip < strips; ++strip) {
      const int i0 = strip * kStrip;
      const int rows = lq - i0 < kStrip ? lq - i0 : kStrip;
      const bool onward = strip + 1 < strips;   // lane 63's row feeds another strip
      int c_lo = 0, c_hi = lr - 1;              // kBand: the columns that hold the strip's band cells
      // kBand: the work outside the band is NOT DONE: a strip of rows i0 .. i0 + rows - 1 holds
      // band cells in the one column range c_lo = max(0, i0 + lo) .. c_hi = min(lr - 1, i0 +
      // rows - 1 + hi).  A strip with c_lo > c_hi is skipped whole (no staging of its a-rows, no
      // multiply) and the strip loop ends once i0 + lo is past the last column; the step loop
      // runs t from c_lo & ~31 to c_hi + rows - 1, which is c_hi - (c_lo & ~31) + rows steps
      // against lr + rows - 1; b-rows are loaded from c_lo & ~31 on and 32-column blocks are
      // staged and multiplied only while t0 <= c_hi.
      if constexpr (kBand) {
        c_lo = i0 + lo > 0 ? i0 + lo : 0;
        c_hi = i0 + rows - 1 + hi < lr - 1 ? i0 + rows - 1 + hi : lr - 1;
        if (i0 + lo > lr - 1) break;   // the band has left the matrix below
        if (c_lo > c_hi) continue;     // not yet in it
      }
      const int t_first = kBand ? c_lo & ~(kSub - 1) : 0;
      const Carry* carry_in = carry + (size_t)((strip + 1) & 1) * p.cap;
      Carry* carry_out = carry + (size_t)(strip & 1) * p.cap;

      // stage the strip: its rows through the ring's first half (free: no column is in flight)
      // into the MFMA fragments, which stay in registers, and 1 / |a_i| next to them
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
      float top_run = 0.f;                           // kGlobal: H[-1][c0 - 1], along the top border
      bool tracks = false;                           // kGlobal: this lane owns row Lq - 1 (within)
      if constexpr (kGlobal) {
        // kGlobal: the same recurrences without the 0 candidate and with charged borders (global
        // alignment, and with the wave-uniform flag `within` the query-in-target mode whose top
        // border is free; semantics: include/gfy.h, gfy_align_global).  The borders are iterated
        // sums, and they are iterated here.  The left border: a wave-uniform running value goes
        // down it across the strips, H[0][-1] = 0 - gap_open, H[i][-1] = H[i-1][-1] -
        // gap_extend, 64 subtractions per strip of which lane k keeps step k (its initial H) and
        // step k - 1 (its initial diagonal).
#pragma unroll 8
        for (int k = 0; k < kStrip; ++k) {
          diag = lane == k ? left_run : diag;
          left_run = i0 + k == 0 ? 0.f - go : left_run - ge;
          h = lane == k ? left_run : h;
        }
        tracks = within && !onward && lane == ((lq - 1) & (kStrip - 1));
      }
      uint32_t o_h = 0, o_e = 0, o_f = 0, o_diag = 0;   // kSpan: their origins
      uint32_t dir_word = 0;                            // kTrace: the row's 8 columns in the making
      f16x8 b_next[8];
      load_order(t_first);
      load_b(b_next, t_first);
      load_order(t_first + kSub);
      // the carry entries of the row above the strip for columns c0 + lane, lanes 0..31: the
      // strip's last row comes back to lane 0 of the next strip 32 columns at a time, one load
      // ahead, from the two buffers in turn
      auto load_carry = [&](int c0) __attribute__((always_inline)) {
        Carry v;
        if constexpr (kSpan) v = Carry{__float_as_uint(0.f), __float_as_uint(minus_inf), 0u, 0u};
        else v = make_float2(0.f, minus_inf);
        if constexpr (kBand) {
          // kBand: lane 63 stores only live cells, so this (and the first diagonal below)
          // substitutes the outside entry for every column c with c - (i0 - 1) outside [lo, hi],
          // per lane and without reading memory; that also covers a predecessor strip that was
          // skipped
          if (strip > 0 && lane < kSub && c0 + lane < lr &&
              (uint32_t)(c0 + lane - (i0 - 1) - lo) <= (uint32_t)(hi - lo))
            v = carry_in[c0 + lane];
        } else {
          if (strip > 0 && lane < kSub && c0 + lane < lr) v = carry_in[c0 + lane];
        }
        if constexpr (kGlobal) {
          // the top border of kGlobal: a running value goes along it 32 columns at a time into
          // what strip 0 takes for its carry, iterated like the left one (F stays -inf); within:
          // the rows of B in front of the alignment are free, H = 0
          if (strip == 0 && !within) {
#pragma unroll 8
            for (int k = 0; k < kSub; ++k) {
              top_run = c0 + k == 0 ? 0.f - go : top_run - ge;
              v.x = lane == k ? top_run : v.x;
            }
          }
        }
        return v;
      };
      Carry carry_next = load_carry(t_first);
      if constexpr (kBand) {
        // kBand: lane 0 has no step in front of a start t_first = c_lo & ~31 > 0, so it takes
        // its first diagonal predecessor, column t_first - 1 of the row above, (i0 - 1, t_first
        // - 1), from the carry: no step brings it
        if (strip > 0 && t_first > 0 && lane == 0 &&
            (uint32_t)(t_first - 1 - (i0 - 1) - lo) <= (uint32_t)(hi - lo)) {
          const Carry v = carry_in[t_first - 1];
          if constexpr (kSpan) diag = __uint_as_float(v.x), o_diag = v.z;
          else diag = v.x;
        }
      }

      const int steps = kBand ? c_hi + rows : lr + rows - 1;   // the step behind the last one
      for (int t0 = t_first; t0 < steps; t0 += kSub) {
        // Columns t0 .. t0 + 31 join the ring.  The substitution scores come 32 columns at a
        // time: the 32 b-rows go to LDS in the swizzled layout of the sweep, sweep_multiply
        // (pairwise_sweep.inc, the one multiply of the library) forms the 64 x 32 products against
        // the strip's fragments, and the epilogue turns them into the dense kernel's cosine (same
        // key, same pair_value), scales and shifts it with two rounded operations and stores it
        // BY ANTI-DIAGONAL: cell (l, j) at [(l + j) % 128][l], a ring of 128 diagonals of 64
        // lanes (32 KB).  A step reads one diagonal: 64 consecutive words, no bank conflict.
        // Before step t = 32 kb the ring holds diagonals t .. t + 62 of earlier columns, the new
        // columns add up to t + 94, and the quarter behind them (t + 96 .. t + 127, spent by the
        // last 32 steps) stages the b-rows.
        //   kBand: the ring needs no change: its slot (t & 127) and the staging quarter ((t0 >>
        //   5) + 3) & 3 depend on t0 modulo 128 alone and every block still starts at a multiple
        //   of 32, so a block writes the three quarters in front of its own start and stages in
        //   the fourth, whatever the first block was; at the first block nothing is in flight
        //   and every quarter is free.
        if (kBand ? t0 <= c_hi : t0 < lr) {
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
          if (kBand ? t0 + kSub <= c_hi : t0 + kSub < lr) {
            load_b(b_next, t0 + kSub);
            load_order(t0 + 2 * kSub);
          }
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
        const Carry from_above = carry_next;
        carry_next = load_carry(t0 + kSub);
        const int t_end = t0 + kSub < steps ? t0 + kSub : steps;
        for (int t = t0; t < t_end; ++t) {
          // the recurrence proper, the same expressions in every mode but for kGlobal's missing 0
          const int j = t - lane;
          float up_h = __shfl_up(h, 1, 64), up_f = __shfl_up(f, 1, 64);
          float above_h, above_f;
          if constexpr (kSpan) {
            above_h = __uint_as_float(__builtin_amdgcn_readlane(from_above.x, t - t0));
            above_f = __uint_as_float(__builtin_amdgcn_readlane(from_above.y, t - t0));
          } else {
            above_h = lane_value(from_above.x, t - t0);
            above_f = lane_value(from_above.y, t - t0);
          }
          if (lane == 0) up_h = above_h, up_f = above_f;
          const float s = ring_f[(t & 127) * kStrip + lane];
          const bool inside = (uint32_t)j < (uint32_t)lr && lane < rows;   // in the matrix
          bool live = inside;
          if constexpr (kBand) live = inside && (uint32_t)(j - (i0 + lane) - lo) <= (uint32_t)(hi - lo);
          const float e_ext = e - ge, e_open = h - go;
          const float f_ext = up_f - ge, f_open = up_h - go;
          const float match = diag + s;
          const float e_new = __builtin_fmaxf(e_ext, e_open);
          const float f_new = __builtin_fmaxf(f_ext, f_open);
          float h_new;
          if constexpr (kGlobal)   // no 0 candidate
            h_new = __builtin_fmaxf(match, __builtin_fmaxf(e_new, f_new));
          else
            h_new = __builtin_fmaxf(__builtin_fmaxf(0.f, match), __builtin_fmaxf(e_new, f_new));
          uint32_t o_new = 0;
          // kSpan: every positive H, E and F has an origin, the first matched cell of the path
          // behind it, one word (i0 << 12) | j0.  A lane keeps the origins of h, e, f and diag
          // and that of its best cell; the two values that cross lanes each step take theirs
          // along, and so does the butterfly.  An origin is SELECTED where its value is formed,
          // by comparing the very operands of the max — the max expressions themselves are those
          // of the mode without kSpan, so scores and ends are the same bits.
          if constexpr (kSpan) {
            uint32_t up_oh = (uint32_t)__shfl_up((int)o_h, 1, 64);
            uint32_t up_of = (uint32_t)__shfl_up((int)o_f, 1, 64);
            const uint32_t above_oh = __builtin_amdgcn_readlane(from_above.z, t - t0);
            const uint32_t above_of = __builtin_amdgcn_readlane(from_above.w, t - t0);
            if (lane == 0) up_oh = above_oh, up_of = above_of;
            // opening wins a tie; diagonal, then E, then F; a path starts where its diagonal
            // predecessor is not positive
            const uint32_t here = ((uint32_t)(i0 + lane) << kOriginBits) | (uint32_t)j;
            const uint32_t oe_new = e_open >= e_ext ? o_h : o_e;
            const uint32_t of_new = f_open >= f_ext ? up_oh : up_of;
            o_new = h_new == match ? (diag > 0.f ? o_diag : here) : h_new == e_new ? oe_new : of_new;
            o_e = live ? oe_new : o_e;
            o_f = live ? of_new : o_f;
            o_h = live ? o_new : o_h;
            o_diag = inside ? up_oh : o_diag;
          }
          // kTrace: every cell leaves 4 direction bits, selected like the origins from the
          // operands of the max: which candidate H took (0 starts here, 1 diagonal continuing, 2
          // E, 3 F), bit 2 E opened, bit 3 F opened.  A lane packs the 8 consecutive columns of
          // its row into a word and stores it when it fills or the row ends: [box rows][ceil(box
          // cols / 8)] words, row-major, in the wave's region of the workspace (the only thing
          // proportional to Lq x Lr the library ever writes, and the box alone).
          if constexpr (kTrace) {
            // the same selections as kSpan's, kept as bits: diagonal, then E, then F; opening
            // wins a tie
            // (kGlobal: no path starts inside the matrix, 0 is unused)
            const uint32_t how =
                h_new == match ? (kGlobal || diag > 0.f ? 1u : 0u) : h_new == e_new ? 2u : 3u;
            const uint32_t bits = how | (e_open >= e_ext ? 4u : 0u) | (f_open >= f_ext ? 8u : 0u);
            if (live) {
              dir_word = (j & 7) == 0 ? bits : dir_word | (bits << (4 * (j & 7)));
              // kBand: a row's band may begin and end inside an 8-column direction word, so the
              // word is also stored at the row's last band cell (d == hi).  A word that is never
              // written is never walked (a path cell is positive, hence in the band); the
              // 64-lane window load of trace_walk may read it, inside the wave's own region.
              // The region stays sized for the whole box.
              if ((j & 7) == 7 || j == lr - 1 || (kBand && j - (i0 + lane) == hi))
                dir[(size_t)(i0 + lane) * dir_pitch + (j >> 3)] = dir_word;
            }
          }
          if constexpr (kBand) {
            // a lane's registers are what its neighbours read.  A cell in the matrix but outside
            // the band sets h = 0, e = f = -inf instead of keeping the lane's registers;
            // otherwise lane l + 1 would take the last band cell of lane l for "the row above"
            // when that row has already left the band at hi.
            e = live ? e_new : inside ? minus_inf : e;
            f = live ? f_new : inside ? minus_inf : f;
            h = live ? h_new : inside ? 0.f : h;
          } else {
            e = live ? e_new : e;
            f = live ? f_new : f;
            h = live ? h_new : h;
          }
          // kBand: diag (and its origin, above) follows up_h on every step in the matrix, in the
          // band or not; otherwise a lane's first band cell at d == lo would find a stale
          // diagonal predecessor, which lies on the same diagonal and hence in the band.
          diag = inside ? up_h : diag;
          // Each lane keeps its best (H, i, j) with a strict >, which is the lowest (i, j) of the
          // lane's rows.  kGlobal: the score is the last H of the lane that owns row Lq - 1
          // (global) or that lane's best with a strict > from -inf (within, `tracks`); no other
          // lane tracks anything.
          const bool better = live && (!kGlobal || tracks) && h_new > best;
          best = better ? h_new : best;
          best_i = better ? i0 + lane : best_i;
          best_j = better ? j : best_j;
          if constexpr (kSpan) best_o = better ? o_new : best_o;
          // the strip's last row goes to the workspace as lane 63 forms it: (H, F) per column, 8
          // bytes, and with kSpan (H, F, origin of H, origin of F), 16 bytes in one store and one
          // load
          if (onward && lane == kStrip - 1 && live) {
            if constexpr (kSpan)
              carry_out[j] = Carry{__float_as_uint(h_new), __float_as_uint(f_new), o_h, o_f};
            else
              carry_out[j] = make_float2(h_new, f_new);
          }
        }
      }
      if constexpr (kTrace || kGlobal) h_last = h;
      // the next strip reads what lane 63 stored (and restages the ring); kTrace: the walk reads
      // the direction words the lanes stored
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      wave_sync();
    }

    if constexpr (kTrace)
      trace_walk<kMode>(lane, ring, dir, pr, trace, within, pair, strips, h_last, out_start);
    else
      finish_pair<kMode>(p, lane, pr, within, pair, strips, h_last, best, best_i, best_j, best_o,
                         out_start);
  }
}

}  // namespace
}  // namespace gfy
