// The fused layer as TWO 4-wave workgroups per CU with the weights STREAMED through a window
// (included by gine_f16.hip behind gine_layer_q.inc; same tile plans, gather_tile / gather_direct,
// pipelines, layer_norm_*, and around them load_plan_words, store_row, store_taps_zvw,
// head_row_dest, head_row_square_sum and raise_wave_priority of gine_layer.inc: results are
// bit-identical to k_gine_layer_f16 / k_gine_layer_q).
//
// Why.  In k_gine_layer_q the eight waves of a CU are one workgroup and walk the phases of a
// round together, because [W0 | W1] (128 KB) overlay the eight gather stages (144 KB): what
// separates the phases is exposed — the 128-KB weight fill (3.3 k cycles: the L2 -> LDS rate of
// a CU, ~37 B per cycle), the barrier until the slower wave of every SIMD has spent the weights
// (3.4-4.8 k), the wait for the next stage (2 k).  Here a workgroup is FOUR waves, one per
// SIMD, with 80 KB of LDS, and a CU holds two of them.  They share nothing and synchronise with
// nobody but themselves: a barrier is among four waves on four different SIMDs that arrive
// together (~100 cycles, measured), and while one workgroup waits for a fill the other one
// computes.  The price: every workgroup streams its own copy of the weights, 256 KB of
// L2 -> LDS traffic per CU and round instead of 128 KB.  The two designs end within a few
// percent of each other, and so does an 8-wave workgroup around this window that streams the
// weights once: what bounds all three is the vector issue port — a launch without the epilogue
// arithmetic is 10 % faster, one without any weight read out of LDS is not faster at all
// (profiles/r04_sensitivity.txt, profiles/README.md, round 4).
//
// LDS of one workgroup (81,920 B; two per CU = all 160 KB):
//   [0, 73,728)        four gather stages (18 KB each: 32 own + 40 far rows) and, over rows
//                      0..63 of every spent stage, the WINDOW: two buffers of 32 1-KB pieces (buffer 0 over rows 32..63, buffer 1 over rows 0..31).
//                      The update MLP reads its weights as four 32-KB chunks in pipeline order
//                      — c0, c1 = W0 (block pairs 0-1, 2-3), c2, c3 = W1 (output pairs 0, 1) —
//                      chunk c in buffer c & 1; the last launch appends c4 = head.0, c5 = head.2.
//                      Piece p of a chunk lives in the stage of wave p & 3, so every wave
//                      streams an equal share of every chunk into its OWN stage.
//   [73,728, 81,408)   the layer's constant image; rows 12..15 of its edge table (never read:
//                      edge types are < edge_dim <= 12) hold the four waves' plan-head slots
//   [81,408, 81,920)   the head's biases
//
// One round (four tiles, one per wave):
//   plan head of round r+1 requested -> gather (stage r landed) -> c0, c1 requested over the own
//   spent stage -> c0 landed, barrier -> products; step 12: c1 landed, c0 spent, barrier, c2
//   requested; step 28: c2 landed, c1 spent, barrier, c3 requested; step 44: c3 landed, c2 spent,
//   barrier, the FAR rows of round r+1 requested into c2's place; step 60: every read of the
//   window is done, barrier, the own rows of round r+1 requested: they stream into the stages
//   under the last steps of the pipeline and the LayerNorm -> store -> round r+1.
//
// No flags, no polling: every synchronisation is an s_barrier that all four waves of a
// workgroup execute the same number of times (the round loop is workgroup-uniform, waves
// without a tile walk the round on zeros).
//
// The two workgroups of a CU: the matrix pipe and the vector issue of a SIMD serve the OLDER
// wave first, and the second-dispatched workgroup of every CU ran a round in 35 k cycles while
// the first one took 27 k.  `priority` (GFY_OPT_PRIORITY) raises the second workgroup's waves
// to s_setprio 1 while they multiply: 63 -> 58.5 us per launch of 240,000 nodes.

constexpr int kWWaves = 4;                          // tiles per workgroup and round
constexpr int kWThreads = 64 * kWWaves;
constexpr int kWChunkPieces = 32;                   // 1-KB pieces of a weight chunk
constexpr int kWLdsImage = kWWaves * kLdsStageBytes;              // 73,728
constexpr int kWLdsHeads = kWLdsImage + 12 * 256;   // table rows 12..15: plan-head slots
constexpr int kWLdsBytes = kWLdsImage + kLdsImageBytes + 512;     // 81,920
constexpr int kWMaxEdgeTypes = 12;                  // table rows a launch of this kernel may read
static_assert(2 * kWLdsBytes <= 160 * 1024, "two workgroups per CU");
// The window: two buffers of 32 pieces.  Piece p of a chunk lives in the stage of wave p & 3
// (every wave streams an equal share of every chunk into its own stage: the first two chunks
// need no barrier before they are requested), buffer b in rows 32 (1 - b) .. 32 (1 - b) + 31 of that stage
// (GFY_W_SPLIT_FILL below);
// rows 64..71 of a stage are never overlaid.
// GFY_W_SPLIT_FILL 1: a plain layer launch requests the next round's FAR rows at step 44 and
// only the own rows at step 60.  For that the window's buffers trade places — chunk c lies in
// rows 32..63 of the stages for even c, in rows 0..31 for odd c — so that what c2 leaves behind
// at step 44 is the far rows' place (stage rows 64..71 are never overlaid).  0: everything at
// step 60, buffers in stage order (55.7-55.8 against 56.2 us per launch of four shards on one
// box, profiles/README.md round 5; bit-identical).
#ifndef GFY_W_SPLIT_FILL
#define GFY_W_SPLIT_FILL 1
#endif
constexpr int kWFirstBufferRows = GFY_W_SPLIT_FILL ? 32 : 0;   // stage rows of buffer 0
struct WindowLayout {
  static constexpr int kImage = kWLdsImage;
  static constexpr int kBase1 = 2 * kLdsStageBytes;   // second base register: stages 2 and 3
  static constexpr int base_of(int q) { return (q >> 1) & 1; }
  static constexpr int buffer_kb(int chunk) {         // where a chunk's buffer starts in a stage
    return ((chunk & 1) * 32 + kWFirstBufferRows) % 64 / 4;
  }
  static constexpr int offset_of(int q) {   // from the base: 16-bit offsets
    return (q & 1) * kLdsStageBytes + (buffer_kb(q >> 5) + ((q & 31) >> 2)) * 1024;
  }
  static constexpr int address_of(int q) { return base_of(q) * kBase1 + offset_of(q); }
};
static_assert(WindowLayout::offset_of(127) < 65536 && WindowLayout::address_of(31) + 1024 <=
                  3 * kLdsStageBytes + 16 * 1024, "window inside the first 64 rows of a stage");

// this wave's eight pieces (p = 4 i + wave) of chunk `chunk` of an image -> the window
__device__ __forceinline__ void issue_chunk_dma(const void* image, int chunk, uint32_t lds0,
                                                int wave, int lane) {
  const uint32_t buffer_rows = (uint32_t)WindowLayout::buffer_kb(chunk) * 1024u;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t p = 4u * i + (uint32_t)wave;
    dma16(image, ((uint32_t)chunk * kWChunkPieces + p) * 1024u + (uint32_t)lane * 16u,
          lds0 + (uint32_t)wave * kLdsStageBytes + buffer_rows + (uint32_t)i * 1024u);
  }
}
__device__ __forceinline__ void window_barrier() {   // the caller has waited for what it must
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// The stage fill in two parts (stage_dma, gine_layer_q.inc, is both): the own rows, and the far
// rows straight from the plan-head slot (a lane group's twelve far rows are twelve consecutive
// dwords there)
__device__ __forceinline__ void stage_dma_own(const f16* h_in, int tile, int n, uint32_t lds_stage,
                                              int lane) {
  const uint32_t sub = (uint32_t)lane >> 4, p16 = (uint32_t)lane & 15u;
#pragma unroll
  for (int g = 0; g < kLTile / 4; ++g) {
    const uint32_t q = 4u * g + sub;
    int own = tile * kLTile + (int)q;
    own = own < n ? own : n - 1;
    dma16(h_in, (uint32_t)own * 256u + ((p16 ^ (q & 15u)) << 4), lds_stage + (uint32_t)g * 1024u);
  }
}
__device__ __forceinline__ void stage_dma_far(const f16* h_in, uint32_t lds_stage, int lane,
                                              int count, const char* slot) {
  if (count > kLFar) return;                       // the direct path stages nothing
  const uint32_t sub = (uint32_t)lane >> 4, p16 = (uint32_t)lane & 15u;
  const u32x4* const far_at = reinterpret_cast<const u32x4*>(slot + 16 + sub * 48);
#pragma unroll
  for (int g4 = 0; 4 * g4 < kLFar / 4; ++g4) {
    if (16 * g4 < count) {                         // wave-uniform
      const u32x4 fars = far_at[g4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int g = 4 * g4 + i;
        if (g < kLFar / 4 && 4 * g < count) {
          const uint32_t q = (uint32_t)kLTile + 4u * g + sub;
          dma16(h_in, fars[i] * 256u + ((p16 ^ (q & 15u)) << 4),
                lds_stage + (uint32_t)(kLTile / 4 + g) * 1024u);
        }
      }
    }
  }
}

// The window's schedule inside mlp_pipeline_on: at the start of step kT the reads of steps
// < kT have been issued; they target the fragments of steps < kT + 4.
//   step 12  c1 landed (its last pieces were requested before the products), c0 spent -> c2
//   step 28  c2 landed, c1 spent -> c3
//   step 44  c3 landed, c2 spent -> the next round's far rows (head launch: c4)
//   step 60  c3 spent: the window is free -> the next round's own rows (head launch: c5)
template <bool kHead, class NextRound, class NextEarly>
struct WindowHooks {
  const LayerF16& p;
  const HeadF16& head;
  uint32_t lds0;
  int wave, lane;
  NextRound& next_round;   // issues the next round's stage fill (plain layers: at step 60)
  NextEarly& next_early;   // ... the part of it that fits behind c2 (plain layers: at step 44)
#ifdef GFY_STAMPS
  int stamp_row;           // diagnostic build: cycles spent waiting in the four hooks
  __device__ __forceinline__ void waited(unsigned long long since, int slot) const {
    if (stamp_row >= 0 && lane == 0) g_stamps[stamp_row][slot] += __builtin_amdgcn_s_memtime() - since;
  }
#define HOOK_BEGIN const unsigned long long hook_t0 = __builtin_amdgcn_s_memtime()
#define HOOK_WAITED(slot) waited(hook_t0, slot)
#else
#define HOOK_BEGIN
#define HOOK_WAITED(slot)
#endif
  template <int kT>
  __device__ __forceinline__ void before_mlp_step() const {
    if constexpr (kT == 12 || kT == 28 || kT == 44 || kT == 60) {
      HOOK_BEGIN;
      if constexpr (kT == 12) {
        dma_wait_all();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        window_barrier();
        HOOK_WAITED(8);
        issue_chunk_dma(p.w01_image, 2, lds0, wave, lane);
      } else if constexpr (kT == 28) {
        dma_wait_all();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        window_barrier();
        HOOK_WAITED(9);
        issue_chunk_dma(p.w01_image, 3, lds0, wave, lane);
      } else if constexpr (kT == 44) {
        dma_wait_all();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        window_barrier();
        HOOK_WAITED(12);
        if constexpr (kHead) issue_chunk_dma(head.w_image, 0, lds0, wave, lane);   // c4
        else next_early();
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        window_barrier();
        HOOK_WAITED(13);
        if constexpr (kHead) issue_chunk_dma(head.w_image, 1, lds0, wave, lane);   // c5
        else next_round();
        HOOK_WAITED(14);
#if defined(GFY_STAMPS) && defined(GFY_DIAG_FILL)
        // diagnostic: how long the stage fill takes by itself, from its last request to landed
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        HOOK_WAITED(15);
#endif
      }
    }
  }
};
#undef HOOK_BEGIN
#undef HOOK_WAITED

template <bool kResidual, bool kTap = false, bool kHead = false>
__global__ __launch_bounds__(kWThreads, 2) void k_gine_layer_w(
    const LayerF16 p, const f16* __restrict__ h_in, f16* __restrict__ h_out,
    const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const uint8_t* __restrict__ typ, const char* __restrict__ plans, int n, int num_tiles,
    int stagger, int priority, int32_t* __restrict__ spent_tile_sums,
    unsigned long long* __restrict__ span, int tap, f16* __restrict__ tap_out,
    const HeadOut head_out) {
  static_assert(!(kTap && kHead), "the tap instantiation is a plain layer");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const char* const tbytes = smem + kWLdsImage;      // the edge table opens the constant image
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const char* const stage = smem + wave * kLdsStageBytes;
  const uint32_t lds_stage = lds0 + (uint32_t)wave * kLdsStageBytes;
  if (span && t == 0) atomicMin(&span[0], (unsigned long long)__builtin_amdgcn_s_memrealtime());
  // The workgroups of an XCD are dealt to its CUs in order: the second half of them are the
  // second residents of the CUs (observed with in-kernel stamps, not promised: only speed
  // depends on it).
  const int per_xcd = (int)(gridDim.x >> 3), half = (per_xcd + 1) >> 1;
  const int slot_in_xcd = (int)(blockIdx.x >> 3);
  const bool second = slot_in_xcd >= half;
  // (not raise_wave_priority: every form of it that folds `second` in reschedules the kernel)
  if (second && ((priority >> 4) & 3) == 1) __builtin_amdgcn_s_setprio(1);
  else if (second && ((priority >> 4) & 3) == 2) __builtin_amdgcn_s_setprio(2);
  else if (second && ((priority >> 4) & 3) == 3) __builtin_amdgcn_s_setprio(3);
  {
    const unsigned long long delay =
        (unsigned long long)(second ? slot_in_xcd - half : slot_in_xcd) * (unsigned)stagger;
    if (delay > 0) {
      const unsigned long long until = __builtin_amdgcn_s_memtime() + delay;
      while (__builtin_amdgcn_s_memtime() < until) __builtin_amdgcn_s_sleep(8);
    }
  }
#ifdef GFY_STAMPS
#define STAMP_W(slot)                                                                         \
  do {                                                                                        \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();                             \
    if (t == kStampThread && stamp_row >= 0) g_stamps[stamp_row][slot] += now_ - last_stamp;   \
    last_stamp = now_;                                                                        \
  } while (0)
  constexpr int kStampThread = 64 * (GFY_STAMP_WAVE & 3);
  // every other workgroup of an XCD reports: rows 0..127 first residents, 128..255 second ones
  const int stamp_row = (slot_in_xcd & 1) == 0 && slot_in_xcd < 64 ? (int)(blockIdx.x & 7) + 8 * (slot_in_xcd >> 1) : -1;
  unsigned long long last_stamp = __builtin_amdgcn_s_memtime();
  const unsigned long long first_stamp = last_stamp;
  if (t == 0 && blockIdx.x < 512) g_real[blockIdx.x][0] = __builtin_amdgcn_s_memrealtime();
#else
#define STAMP_W(slot)
#endif

  // ---- rounds: XCD (blockIdx & 7) owns the tiles [xbase, xend); in round rd the workgroups of
  //      the XCD take consecutive groups of four tiles -----------------------------------------
  const int tpx = (num_tiles + 7) >> 3;
  const int xbase = (int)(blockIdx.x & 7) * tpx;
  const int xend = xbase + tpx < num_tiles ? xbase + tpx : num_tiles;
  const int group_stride = (int)(gridDim.x >> 3) * kWWaves;
  int first = xbase + (int)(blockIdx.x >> 3) * kWWaves;      // first tile of this round's group
  auto tile_of = [&](int group) { return group + wave; };
  auto active_in = [&](int group) { return group + wave < xend; };   // wave-uniform

  // the constant image (and the head's biases behind it): once per workgroup
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int at = t + i * kWThreads;
    if (at < kLdsImageBytes / 16)
      reinterpret_cast<u32x4*>(smem + kWLdsImage)[at] = reinterpret_cast<const u32x4*>(p.image)[at];
    else if (kHead && at < kLdsImageBytes / 16 + 32)
      reinterpret_cast<u32x4*>(smem + kWLdsImage)[at] =
          reinterpret_cast<const u32x4*>(head_out.head.image)[at - kLdsImageBytes / 16];
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  window_barrier();                                 // the image is in place before a slot is filled
  // the first round's plan head -> LDS slot, rows -> stage, slot words -> registers
  const char* const head_slot = smem + kWLdsHeads + wave * 256;
  const uint32_t lds_head_slot = lds0 + (uint32_t)kWLdsHeads + (uint32_t)wave * 256u;
  int count = 0, deepest = 0;                       // of the current round's tile (uniform)
  uint32_t word[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool active = first < xend && active_in(first);
  if (active) {
    const int tile = tile_of(first);
    const char* plan = plans + (size_t)tile * kPlanBytes;
    plan_head_dma(plan, lds_head_slot, lane);
    dma_wait_all();
    const PlanHeadQ head = plan_head_read(head_slot, lane);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    count = head.count, deepest = head.deepest;
    stage_dma(h_in, tile, n, lds_stage, lane, count, head.far4);
    load_plan_words(plan, lane & 31, word);
  }
  dma_wait_all();
  STAMP_W(0);

  const f16 scale16 = (f16)p.scale;
  while (first < xend) {                            // workgroup-uniform
    const int tile = tile_of(first);
    const int next_first = first + group_stride;
    const bool next_active = next_first < xend && active_in(next_first);
    if (spent_tile_sums && active && lane == 0) spent_tile_sums[tile] = 0;
    const bool staged = count <= kLFar;
    // the next round's plan head: requested now, read when the next stage fill is issued
    const char* const next_plan =
        plans + (size_t)(next_active ? tile_of(next_first) : tile) * kPlanBytes;
    if (next_active) plan_head_dma(next_plan, lds_head_slot, opaque(lane));

    // ---- own rows -> registers (z, residual), gather-sum -> z ------------------------------
    f16x8 h[8], z[8];
    {
      const int lane_a = opaque(lane), r_a = lane_a & 31, hq_a = lane_a >> 5;
      const uint32_t own = (uint32_t)r_a * 256u, x16 = (((uint32_t)r_a & 15u) ^ (uint32_t)hq_a) * 16u;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks)
        h[ks] = *reinterpret_cast<const f16x8*>(stage + own + (x16 ^ (32u * ks)));
      if (active) {
        if (staged) {
          if (deepest <= 3) gather_tile<3>(h, z, word, tbytes, stage, r_a, hq_a, scale16);
          else if (deepest == 4) gather_tile<4>(h, z, word, tbytes, stage, r_a, hq_a, scale16);
          else if (deepest == 5) gather_tile<5>(h, z, word, tbytes, stage, r_a, hq_a, scale16);
          else if (deepest == 6) gather_tile<6>(h, z, word, tbytes, stage, r_a, hq_a, scale16);
          else gather_tile<8>(h, z, word, tbytes, stage, r_a, hq_a, scale16);
        } else {
          const int node = tile * kLTile + r_a;
          gather_direct(h, z, reinterpret_cast<const char*>(h_in), row_ptr, col, typ, tbytes, node,
                        node < n, n, hq_a, scale16, p.edge_types);
        }
      } else {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) h[ks] = zero8(), z[ks] = zero8();
      }
    }
    STAMP_W(1);
    // ---- this wave's stage is spent: the pieces of c0 | c1 that lie over it come in; one
    //      barrier later the first two chunks are resident ----------------------------------
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    issue_chunk_dma(p.w01_image, 0, lds0, wave, opaque(lane));
    issue_chunk_dma(p.w01_image, 1, lds0, wave, opaque(lane));
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // c0 has landed, c1 is on its way
    window_barrier();
    STAMP_W(2);

    // what issues the next round's stage fill: `early` at step 44 of a plain layer launch (the
    // far rows, into the place c2 has left: GFY_W_SPLIT_FILL), the rest at step 60 (every wave
    // is past the window); the head launch runs the whole fill behind its head pipeline
    constexpr bool kSplit = !kHead && GFY_W_SPLIT_FILL != 0;
    auto next_round_early = [&]() {
      if constexpr (kSplit) {
        if (next_active) {
          const int4 header = *reinterpret_cast<const int4*>(head_slot);
          stage_dma_far(h_in, lds_stage, opaque(lane), __builtin_amdgcn_readfirstlane(header.x),
                        head_slot);
        }
      }
    };
    auto start_next_round = [&]() {
      if (next_active) {
        const int lane_b = opaque(lane);
        if constexpr (kSplit) {
          const int4 header = *reinterpret_cast<const int4*>(head_slot);
          count = __builtin_amdgcn_readfirstlane(header.x);
          deepest = __builtin_amdgcn_readfirstlane(header.y);
          stage_dma_own(h_in, tile_of(next_first), n, lds_stage, lane_b);
        } else {
          const PlanHeadQ next = plan_head_read(head_slot, lane_b);
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          count = next.count, deepest = next.deepest;
          stage_dma(h_in, tile_of(next_first), n, lds_stage, lane_b, count, next.far4);
        }
        load_plan_words(next_plan, lane_b & 31, word);
      } else {   // nothing of this round is carried into a round that does not gather
#pragma unroll
        for (int i = 0; i < 8; ++i) word[i] = 0;
      }
    };
#ifdef GFY_STAMPS
    const WindowHooks<kHead, decltype(start_next_round), decltype(next_round_early)> hooks{
        p, head_out.head, lds0, wave, opaque(lane), start_next_round, next_round_early,
        t == kStampThread ? stamp_row : -1};
#else
    const WindowHooks<kHead, decltype(start_next_round), decltype(next_round_early)> hooks{
        p, head_out.head, lds0, wave, opaque(lane), start_next_round, next_round_early};
#endif
    // the products at a raised priority: a wave that multiplies is served before a partner (the
    // other workgroup's wave on this SIMD) that gathers or normalises
    // priority: bits 1:0 first workgroup's level in the products, 3:2 the second one's,
    // 5:4 the second one's level everywhere else
    const int raise = second ? (priority >> 2) & 3 : priority & 3;
    const int rest = second ? (priority >> 4) & 3 : 0;
    raise_wave_priority(raise);
    f16x8 wrow[8];
    if constexpr (kTap) {
      const int lane_t = opaque(lane), row_t = tile * kLTile + (lane_t & 31), hq_t = lane_t >> 5;
      f16x8 v[16];
      mlp_pipeline_on<WindowLayout>(smem, lds0, lane_t, hq_t, z, v, wrow, hooks);
      store_taps_zvw(tap, tap_out, active, row_t, hq_t, z, v, wrow);
    } else {
      const int lane_c = opaque(lane);
      f16x8 v[16];
      mlp_pipeline_on<WindowLayout>(smem, lds0, lane_c, lane_c >> 5, z, v, wrow, hooks);
    }
    if (raise != rest) {
      if (rest == 0) __builtin_amdgcn_s_setprio(0);
      else raise_wave_priority(rest);
    }
    STAMP_W(3);
    f16x8 hn[8];
    if constexpr (!kHead) {
      // ---- the next round's rows have been streaming into the stages since step 60; this
      //      round's LayerNorm + residual + store run under that fill --------------------------
      const int lane_d = opaque(lane);
      layer_norm_residual<kResidual>(wrow, h, hn, smem + kWLdsImage + (kLdsGamma - kLdsImage),
                                     smem + kWLdsImage + (kLdsBeta - kLdsImage), lane_d >> 5);
      if constexpr (kTap) {
        if (active && tap == kTapY) {
          f16x8 y[8];
          layer_norm_residual<false>(wrow, h, y, smem + kWLdsImage + (kLdsGamma - kLdsImage),
                                     smem + kWLdsImage + (kLdsBeta - kLdsImage), lane_d >> 5);
          store_row(tap_out, (size_t)(tile * kLTile + (lane_d & 31)), lane_d >> 5, y);
        }
      }
      // every row of an active tile has storage (padded hidden-state buffers)
      if (active) store_row(h_out, (size_t)(tile * kLTile + (lane_d & 31)), lane_d >> 5, hn);
      STAMP_W(6);
      // the next stage (and its slot words) have landed; this round's stores may still fly
      if (active && !kTap) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      STAMP_W(7);
    } else {
      // ---- LayerNorm, then the head from the registers (c4 | c5 have been landing since steps
      //      44 and 60); the next round's rows stream in under the float64 normalise ------------
      const int lane_d = opaque(lane), r_d = lane_d & 31, hq_d = lane_d >> 5;
      layer_norm_residual<kResidual>(wrow, h, hn, smem + kWLdsImage + (kLdsGamma - kLdsImage),
                                     smem + kWLdsImage + (kLdsBeta - kLdsImage), hq_d);
      STAMP_W(6);
      const HeadRowDest to = head_row_dest(head_out.shards, tile, r_d, active);
      dma_wait_all();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      window_barrier();                               // head.0 | head.2 resident in the window
      f16x8 o[8];
#ifdef GFY_DIAG_W_BLOCK_HEAD   // diagnostic: the block form of the head pipeline on the whole-image window
      {
        NoBlockHooks no_hooks;
        block_head_pipeline<WindowLayout>(lds0, lane_d, hq_d, hn, o, no_hooks);
      }
#else
      head_pipeline<WindowLayout>(smem, lds0, lane_d, hq_d, hn, o);
#endif
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      window_barrier();                               // every wave is done with the head image
      STAMP_W(4);
      start_next_round();
      STAMP_W(5);
      const double total = head_row_square_sum(o);
      const bool stores = __ballot(to.dest >= 0) != 0;   // wave-uniform: eight store instructions
      if (to.dest >= 0) {
        char* rowp = to.out + (size_t)to.dest * (kOutDim * 2) + hq_d * 16;
        if (head_out.normalise) {   // see the head pass of k_gine_layer_f16
          const double nrm = __builtin_sqrt(total);
          const double inv = 1.0 / (nrm > 1e-12 ? nrm : 1e-12);
          const float invf = (float)inv, sign_keeping_zero = -0.0f;
          const float inv_up = __builtin_fmaf(invf, 0x1p-22f, invf);
          const float inv_dn = __builtin_fmaf(invf, -0x1p-22f, invf);
#pragma unroll
          for (int ks = 0; ks < 8; ++ks) {
            const u32x4 w4 = __builtin_bit_cast(u32x4, o[ks]);
            u32x4 up;
            uint32_t differ = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              up[q] = cvt_pk_f16(fma_half<0>(w4[q], inv_up, sign_keeping_zero),
                                 fma_half<1>(w4[q], inv_up, sign_keeping_zero));
              differ |= up[q] ^ cvt_pk_f16(fma_half<0>(w4[q], inv_dn, sign_keeping_zero),
                                           fma_half<1>(w4[q], inv_dn, sign_keeping_zero));
            }
            f16x8 scaled = __builtin_bit_cast(f16x8, up);
            if (differ) {
#pragma unroll
              for (int j = 0; j < 8; ++j) scaled[j] = f64_to_f16_rne((double)(float)o[ks][j] * inv);
            }
            *reinterpret_cast<f16x8*>(rowp + 32 * ks) = scaled;
          }
        } else {
#pragma unroll
          for (int ks = 0; ks < 8; ++ks) *reinterpret_cast<f16x8*>(rowp + 32 * ks) = o[ks];
        }
      }
      if (stores) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      STAMP_W(7);
    }
#ifdef GFY_STAMPS
    if (t == kStampThread && stamp_row >= 0) g_stamps[stamp_row][11] += 1;
#endif
    first = next_first;
    active = next_active;
  }
#ifdef GFY_STAMPS
  if (t == kStampThread && stamp_row >= 0) g_stamps[stamp_row][10] += last_stamp - first_stamp;
  if (t == 0 && blockIdx.x < 512) g_real[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();
#endif
  if (span && lane == 0) atomicMax(&span[1], (unsigned long long)__builtin_amdgcn_s_memrealtime());
#undef STAMP_W
}
