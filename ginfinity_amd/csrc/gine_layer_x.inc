// The fused layer with THREE waves per SIMD: three 4-wave workgroups per CU, <= 168 registers
// and 48 KB of LDS each (included by gine_f16.hip behind gine_block_pipe.inc; same tile plans,
// gather arithmetic, epilogue slices, LayerNorm and head arithmetic in the same order as
// k_gine_layer_f16 / _q / _w — layer_norm_moments / _affine, store_row, store_taps_zvw,
// head_row_dest, head_row_square_sum and raise_wave_priority are gine_layer.inc's own: results
// are bit-identical).
//
// Why.  Round 4's counters for k_gine_layer_w: matrix pipe busy 44.6 % of a launch, vector work
// 41.8 % at a lone wave's issue pace, and the two ADD UP — two in-order 250-register waves per
// SIMD leave it idle whenever both wait (MFMA results, LDS, barriers, the L2 -> LDS stream).  The
// SIMD executes a wave64 vector instruction in 2 cycles; one wave alone issues one every 4-5.5.
// What fills it is a third instruction stream per SIMD, and that needs a third of the registers
// and a third of the LDS:
//
//  * registers (<= 168): the products are block_mlp_pipeline (gine_block_pipe.inc): one
//    accumulator chain, a ring of four weight fragments, the previous block drained in the
//    chain's gaps; the residual rows are NOT held across the products (32 registers) but read
//    again from L2 under the LayerNorm moments;
//  * LDS (49,152 B per workgroup): a gather stage holds HALF of every row — 72 rows x 128 B =
//    9 KB — and is filled twice per tile: channels 0..63 (requested a round ahead, under the
//    previous tile's last MFMAs and LayerNorm), gather k-steps 0..3, channels 64..127 into the
//    same 9 KB, gather k-steps 4..7.  The second fill is exposed to its wave and hidden by the
//    SIMD's other two;
//  * the weights stream through a window of two 16-KB buffers laid over the four spent stages:
//    the [W0 | W1] image is walked front to back by the block pipeline, chunk c = pieces
//    16 c .. 16 c + 15, piece i of a chunk in the stage of wave i & 3 (every wave streams an
//    equal share into its own stage: c0 and c1 are requested right behind the gather, without
//    a barrier).  At the step of piece 16 c + 13 (the step that requests piece 16 (c + 1)):
//    own DMAs landed + own reads landed + barrier -> chunk c + 1 is visible, chunk c is spent
//    -> chunk c + 2 is requested into its buffer.  Eight such barriers per tile among four
//    waves on four SIMDs; the head launch appends the head's four chunks;
//  * plan head (208 B) and slot words (1 KB) of the next tile travel by LDS-DMA into per-wave
//    slots: no registers are held for the next round.
//
// No flags, no polling: every synchronisation is an s_barrier that all four waves of a
// workgroup execute the same number of times (the round loop is workgroup-uniform, waves without
// a tile walk the round on zeros and stream their share of the weights).

constexpr int kXWaves = 4;
constexpr int kXThreads = 64 * kXWaves;
constexpr int kXRowBytes = 128;                                   // half a hidden row
constexpr int kXStageBytes = kLStageRows * kXRowBytes;            // 9,216
constexpr int kXLdsImage = kXWaves * kXStageBytes;                // 36,864: constant image
constexpr int kXLdsHeads = kXLdsImage + 12 * 256;                 // table rows 12..15: plan-head slots
constexpr int kXLdsWords = kXLdsImage + kLdsImageBytes + 512;     // 45,056: slot words, 1 KB per wave
constexpr int kXLdsBytes = kXLdsWords + kXWaves * 1024;           // 49,152
constexpr int kXChunkPieces = 16;
static_assert(3 * kXLdsBytes <= 160 * 1024, "three workgroups per CU");
static_assert(kXStageBytes % 1024 == 0, "a half stage is filled by whole 1-KB DMA instructions");

// piece q of a streamed image: chunk q >> 4 in buffer (q >> 4) & 1, piece i = q & 15 of the chunk
// in slot 4 buffer + (i >> 2) of the stage of wave i & 3; one base register reaches everything
struct XWindowLayout {
  static constexpr int kImage = kXLdsImage;
  static constexpr int kBase1 = 0;
  static constexpr int base_of(int) { return 0; }
  static constexpr int offset_of(int q) {
    return (q & 3) * kXStageBytes + ((((q >> 4) & 1) << 2) + ((q & 15) >> 2)) * 1024;
  }
};
static_assert(XWindowLayout::offset_of(15) + 1024 <= kXLdsImage &&
                  XWindowLayout::offset_of(31) + 1024 <= kXLdsImage,
              "the window lies inside the stages");

// this wave's four pieces (i = 4 j + wave) of chunk `chunk` of an image -> the window
__device__ __forceinline__ void x_chunk_dma(const void* image, int chunk, uint32_t lds_stage,
                                            int wave, int lane) {
#ifdef GFY_DIAG_X_NO_WEIGHT_DMA   // diagnostic (wrong results): what streaming the weights costs
  return;
#endif
  const uint32_t buffer = (uint32_t)(chunk & 1) * 4u * 1024u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t piece = (uint32_t)chunk * kXChunkPieces + 4u * j + (uint32_t)wave;
    dma16(image, piece * 1024u + (uint32_t)lane * 16u, lds_stage + buffer + (uint32_t)j * 1024u);
  }
}

// Half `half` (channels 64 half .. 64 half + 63) of the rows of one tile -> the wave's stage:
// own rows 0..31, then the far rows the plan names.  Eight rows per DMA instruction, eight
// 16-byte positions per row; position p of stage row q holds chunk p ^ ((q >> 1) & 7) of the
// half (a 256-byte LDS bank row is TWO stage rows: sixteen consecutive rows at one chunk hit
// sixteen different 16-byte slots).  `fars` = the twelve far-list entries of lane group
// (lane >> 3) & 3 (plan layout [sub][g] = far[4 g + sub]).
__device__ __forceinline__ void x_stage_dma(const f16* h_in, int tile, int n, uint32_t lds_stage,
                                            int lane, int count, const u32x4 (&far4)[3],
                                            int half) {
#ifdef GFY_DIAG_X_NO_STAGE_DMA   // diagnostic (wrong results): what the stage fills cost
  return;
#endif
  const uint32_t rho = (uint32_t)lane >> 3, p8 = (uint32_t)lane & 7u;
  const uint32_t half_off = (uint32_t)half * (uint32_t)kXRowBytes;
#pragma unroll
  for (int g = 0; g < kLTile / 8; ++g) {
    const uint32_t q = 8u * g + rho;
    int own = tile * kLTile + (int)q;
    own = own < n ? own : n - 1;
    dma16(h_in, (uint32_t)own * 256u + half_off + ((p8 ^ ((q >> 1) & 7u)) << 4),
          lds_stage + (uint32_t)g * 1024u);
  }
  if (count <= kLFar) {
    const bool odd = (lane >> 5) != 0;   // far[8 g + rho] = entry 2 g + (rho >> 2) of sub rho & 3
    const uint32_t fars[5] = {odd ? far4[0][1] : far4[0][0], odd ? far4[0][3] : far4[0][2],
                              odd ? far4[1][1] : far4[1][0], odd ? far4[1][3] : far4[1][2],
                              odd ? far4[2][1] : far4[2][0]};
#pragma unroll
    for (int g = 0; g < kLFar / 8; ++g) {
      if (8 * g < count) {   // wave-uniform
        const uint32_t q = (uint32_t)kLTile + 8u * g + rho;
        dma16(h_in, fars[g] * 256u + half_off + ((p8 ^ ((q >> 1) & 7u)) << 4),
              lds_stage + (uint32_t)(kLTile / 8 + g) * 1024u);
      }
    }
  }
}
static_assert(kLFar % 8 == 0 && kLFar / 8 == 5, "five far-row DMA instructions per half");
__device__ __forceinline__ PlanHeadQ x_plan_head_read(const char* slot, int lane) {
  PlanHeadQ q;
  const int4 header = *reinterpret_cast<const int4*>(slot);
  const u32x4* far_at = reinterpret_cast<const u32x4*>(slot + 16 + ((lane >> 3) & 3) * 48);
  q.far4[0] = far_at[0], q.far4[1] = far_at[1], q.far4[2] = far_at[2];
  q.count = __builtin_amdgcn_readfirstlane(header.x);
  q.deepest = __builtin_amdgcn_readfirstlane(header.y);
  return q;
}

// gather_tile (gine_layer.inc) over a HALF stage: k-steps 4 half .. 4 half + 3, rows of 128 B
template <int S>
__device__ __forceinline__ void x_gather_half(f16x8 (&z)[8], const uint32_t (&word)[8],
                                              const char* tbytes, const char* stage, int r, int hq,
                                              f16 scale16, int half) {
  uint32_t toff[S], saddr[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const uint32_t q = word[s] & 0xFFu;
    toff[s] = (word[s] >> 8) * 256u + (uint32_t)hq * 16u + (uint32_t)half * 128u;
    // chunk 2 k + hq (k = 0..3) of stage row q sits at position (2 k + hq) ^ ((q >> 1) & 7): row
    // base and position bits do not overlap, so one XOR with 32 k yields the address of k-step k
    saddr[s] = q * (uint32_t)kXRowBytes + ((((q >> 1) & 7u) ^ (uint32_t)hq) << 4);
  }
  const uint32_t own = (uint32_t)r * (uint32_t)kXRowBytes + (((((uint32_t)r >> 1) & 7u) ^ (uint32_t)hq) << 4);
  f16x8 sel = zero8();
  {
    const int want_half = (r >> 2) & 1, want_j = (r & 3) + 4 * (r >> 3);
#pragma unroll
    for (int jj = 0; jj < 8; ++jj)
      if (r < 16 && hq == want_half && jj == want_j) sel[jj] = (f16)1.0f;
  }
  constexpr bool kAhead = S <= 4;   // registers: one chunk ahead only for shallow tiles
  f16x8 hv[kAhead ? 2 : 1][S], ev[kAhead ? 2 : 1][S];
  auto fetch = [&](int k, f16x8 (&hd)[S], f16x8 (&ed)[S]) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      hd[s] = *reinterpret_cast<const f16x8*>(stage + (saddr[s] ^ (32u * k)));
      ed[s] = *reinterpret_cast<const f16x8*>(tbytes + toff[s] + 32 * k);
    }
  };
  auto reduce = [&](int k, const f16x8 (&hd)[S], const f16x8 (&ed)[S], f16x8& zk) {
    const f16x8 hk = *reinterpret_cast<const f16x8*>(stage + (own ^ (32u * k)));
    f32x16 acc = {0};
#pragma unroll
    for (int s = 0; s < S; ++s)   // CSR order: slot s is the s-th in-edge
      acc = mfma(sel, __builtin_elementwise_max(hd[s] + ed[s], zero8()), acc);
    f16x8 agg;
#pragma unroll
    for (int j = 0; j < 8; ++j) agg[j] = (f16)acc[j];   // ONE rounding of the fp32 sum
    zk = hk * scale16 + agg;                            // two fp16 ops, two roundings
  };
  if constexpr (kAhead) {
    fetch(0, hv[0], ev[0]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k + 1 < 4) fetch(k + 1, hv[(k + 1) & 1], ev[(k + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
        if (hf == half) reduce(k, hv[k & 1], ev[k & 1], z[4 * hf + k]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      fetch(k, hv[0], ev[0]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
        if (hf == half) reduce(k, hv[0], ev[0], z[4 * hf + k]);
    }
  }
}
template <int kHalf>
__device__ __forceinline__ void x_gather_dispatch(f16x8 (&z)[8], const uint32_t (&word)[8],
                                                  const char* tbytes, const char* stage, int r,
                                                  int hq, f16 scale16, int deepest) {
  if (deepest <= 3) x_gather_half<3>(z, word, tbytes, stage, r, hq, scale16, kHalf);
  else if (deepest == 4) x_gather_half<4>(z, word, tbytes, stage, r, hq, scale16, kHalf);
  else if (deepest == 5) x_gather_half<5>(z, word, tbytes, stage, r, hq, scale16, kHalf);
  else if (deepest == 6) x_gather_half<6>(z, word, tbytes, stage, r, hq, scale16, kHalf);
  else x_gather_half<8>(z, word, tbytes, stage, r, hq, scale16, kHalf);
}

// The window's schedule inside the block pipelines.  At the start of the step of piece q the
// reads of pieces <= q + 2 have been issued; the step requests piece q + 3.
//   update MLP, piece 16 c + 13 (c = 0..7): chunk c + 1 landed, chunk c spent -> chunk c + 2
//       (c = 6, 7 of the head launch: the head's chunks 0, 1; c = 7 of a plain layer: the window
//       is spent -> the tile's own rows, whole, into the stage: the residual of the LayerNorm)
//   head, piece 16 c + 13 (c = 0..3): head chunk c + 1 landed, c spent -> head chunk c + 2;
//       c = 3: the window is spent -> the next round's first stage fill
template <bool kHead, class WindowSpent, class NextRound>
struct XWindowHooks {
  const LayerF16& p;
  const HeadF16& head;
  uint32_t lds_stage;
  int wave, lane;
  WindowSpent& window_spent;   // plain layer: the residual rows start streaming into the stage
  NextRound& next_round;       // head launch: the next round's first stage fill
  __device__ __forceinline__ void turn() const {   // own DMAs and reads landed, then the barrier
#ifdef GFY_DIAG_X_NO_TURNS   // diagnostic (wrong results): what the window's waits and barriers cost
    return;
#endif
    dma_wait_all();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    window_barrier();
  }
  template <int kT>
  __device__ __forceinline__ void before_mlp_step() const {
    constexpr BlockStep d = block_mlp_step(kT);
    if constexpr (d.piece >= 0 && d.piece % kXChunkPieces == 13) {
      constexpr int c = d.piece / kXChunkPieces;
      turn();
      if constexpr (c + 2 < 8) x_chunk_dma(p.w01_image, c + 2, lds_stage, wave, lane);
      else if constexpr (kHead) x_chunk_dma(head.w_image, c + 2 - 8, lds_stage, wave, lane);
      else if constexpr (c == 7) window_spent();
    }
  }
  template <int kT>
  __device__ __forceinline__ void before_head_step() const {
    constexpr BlockStep d = block_head_step(kT);
    if constexpr (d.piece >= 0 && d.piece % kXChunkPieces == 13) {
      constexpr int c = d.piece / kXChunkPieces;
      turn();
      if constexpr (c + 2 < 4) x_chunk_dma(head.w_image, c + 2, lds_stage, wave, lane);
      else if constexpr (c == 3) next_round();
    }
  }
};

// `priority`: s_setprio level of the CU's first / second / third resident workgroup while it
// multiplies (bits 1:0, 3:2, 5:4); `stagger`: start offset between the workgroups of an XCD
template <bool kResidual, bool kTap = false, bool kHead = false>
__global__ __launch_bounds__(kXThreads, 3) void k_gine_layer_x(
    const LayerF16 p, const f16* __restrict__ h_in, f16* __restrict__ h_out,
    const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const uint8_t* __restrict__ typ, const char* __restrict__ plans, int n, int num_tiles,
    int stagger, int priority, int32_t* __restrict__ spent_tile_sums,
    unsigned long long* __restrict__ span, int tap, f16* __restrict__ tap_out,
    const HeadOut head_out) {
  static_assert(!(kTap && kHead), "the tap instantiation is a plain layer");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const char* const tbytes = smem + kXLdsImage;      // the edge table opens the constant image
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const char* const stage = smem + wave * kXStageBytes;
  const uint32_t lds_stage = lds0 + (uint32_t)wave * kXStageBytes;
  if (span && t == 0) atomicMin(&span[0], (unsigned long long)__builtin_amdgcn_s_memrealtime());
  // The workgroups of an XCD are dealt to its CUs in order: the k-th third of them are the k-th
  // residents of the CUs (observed, not promised: only speed depends on it).
  const int per_xcd = (int)(gridDim.x >> 3), third = (per_xcd + 2) / 3;
  const int slot_in_xcd = (int)(blockIdx.x >> 3);
  const int resident = slot_in_xcd / third;          // 0, 1, 2
  {
    const unsigned long long delay =
        (unsigned long long)(slot_in_xcd - resident * third) * (unsigned)stagger;
    if (delay > 0) {
      const unsigned long long until = __builtin_amdgcn_s_memtime() + delay;
      while (__builtin_amdgcn_s_memtime() < until) __builtin_amdgcn_s_sleep(8);
    }
  }
#ifdef GFY_STAMPS
#define STAMP_X(slot)                                                                         \
  do {                                                                                        \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();                             \
    if (t == kStampThread && stamp_row >= 0) g_stamps[stamp_row][slot] += now_ - last_stamp;   \
    last_stamp = now_;                                                                        \
  } while (0)
  constexpr int kStampThread = 64 * (GFY_STAMP_WAVE & 3);
  // rows 0..63 first residents, 64..127 second, 128..191 third (eight per XCD and resident)
  const int stamp_row = slot_in_xcd - resident * third < 8 && resident < 3
                            ? resident * 64 + (int)(blockIdx.x & 7) * 8 + (slot_in_xcd - resident * third)
                            : -1;
  unsigned long long last_stamp = __builtin_amdgcn_s_memtime();
  const unsigned long long first_stamp = last_stamp;
  if (t == 0 && blockIdx.x < 512) g_real[blockIdx.x][0] = __builtin_amdgcn_s_memrealtime();
#else
#define STAMP_X(slot)
#endif

  // ---- rounds: XCD (blockIdx & 7) owns the tiles [xbase, xend); in round rd the workgroups of
  //      the XCD take consecutive groups of four tiles -----------------------------------------
  const int tpx = (num_tiles + 7) >> 3;
  const int xbase = (int)(blockIdx.x & 7) * tpx;
  const int xend = xbase + tpx < num_tiles ? xbase + tpx : num_tiles;
  const int group_stride = (int)(gridDim.x >> 3) * kXWaves;
  int first = xbase + (int)(blockIdx.x >> 3) * kXWaves;      // first tile of this round's group
  auto tile_of = [&](int group) { return group + wave; };
  auto active_in = [&](int group) { return group + wave < xend; };   // wave-uniform

  // the constant image (and the head's biases behind it): once per workgroup
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int at = t + i * kXThreads;
    if (at < kLdsImageBytes / 16)
      reinterpret_cast<u32x4*>(smem + kXLdsImage)[at] = reinterpret_cast<const u32x4*>(p.image)[at];
    else if (kHead && at < kLdsImageBytes / 16 + 32)
      reinterpret_cast<u32x4*>(smem + kXLdsImage)[at] =
          reinterpret_cast<const u32x4*>(head_out.head.image)[at - kLdsImageBytes / 16];
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  window_barrier();                                 // the image is in place before a slot is filled
  // the first round's plan head -> LDS slot, first half of the rows -> stage, slot words -> slot
  const char* const head_slot = smem + kXLdsHeads + wave * 256;
  const uint32_t lds_head_slot = lds0 + (uint32_t)kXLdsHeads + (uint32_t)wave * 256u;
  const char* const word_slot = smem + kXLdsWords + wave * 1024;
  const uint32_t lds_word_slot = lds0 + (uint32_t)kXLdsWords + (uint32_t)wave * 1024u;
  int count = 0, deepest = 0;                       // of the current round's tile (uniform)
  bool active = first < xend && active_in(first);
  if (active) {
    const int tile = tile_of(first);
    const char* plan = plans + (size_t)tile * kPlanBytes;
    plan_head_dma(plan, lds_head_slot, lane);
    dma_wait_all();
    const PlanHeadQ head = x_plan_head_read(head_slot, lane);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    count = head.count, deepest = head.deepest;
    x_stage_dma(h_in, tile, n, lds_stage, lane, count, head.far4, 0);
    dma16(plan, (uint32_t)kPlanWords + (uint32_t)lane * 16u, lds_word_slot);
  }
  dma_wait_all();
  STAMP_X(0);

  const f16 scale16 = (f16)p.scale;
  // the products at a raised priority (see gine_layer_w.inc): by residency order on the CU
  const int raise = (priority >> (2 * (resident < 3 ? resident : 2))) & 3;
  while (first < xend) {                            // workgroup-uniform
    const int tile = tile_of(first);
    const int next_first = first + group_stride;
    const bool next_active = next_first < xend && active_in(next_first);
    if (spent_tile_sums && active && lane == 0) spent_tile_sums[tile] = 0;
    const bool staged = count <= kLFar;
    const char* const next_plan =
        plans + (size_t)(next_active ? tile_of(next_first) : tile) * kPlanBytes;

    // ---- gather-sum -> z, half by half ------------------------------------------------------
    f16x8 z[8];
    if (active && staged) {
      uint32_t word[8];
      {
        const int lane_a = opaque(lane);
        const u32x4 wa = reinterpret_cast<const u32x4*>(word_slot + (lane_a & 31) * 32)[0];
        const u32x4 wb = reinterpret_cast<const u32x4*>(word_slot + (lane_a & 31) * 32)[1];
        word[0] = wa[0], word[1] = wa[1], word[2] = wa[2], word[3] = wa[3];
        word[4] = wb[0], word[5] = wb[1], word[6] = wb[2], word[7] = wb[3];
        x_gather_dispatch<0>(z, word, tbytes, stage, lane_a & 31, lane_a >> 5, scale16, deepest);
      }
      STAMP_X(1);
      {   // the other half of the same rows over the spent first half
        const int lane_b = opaque(lane);
        const PlanHeadQ again = x_plan_head_read(head_slot, lane_b);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        x_stage_dma(h_in, tile, n, lds_stage, lane_b, count, again.far4, 1);
        // the next round's plan head: requested now (its slot has just been read for the last
        // time), read when the next first stage fill is issued
        if (next_active) plan_head_dma(next_plan, lds_head_slot, lane_b);
        dma_wait_all();
      }
      STAMP_X(2);
      {
        const int lane_c = opaque(lane);
        x_gather_dispatch<1>(z, word, tbytes, stage, lane_c & 31, lane_c >> 5, scale16, deepest);
      }
    } else {
      if (active) {   // a hub row or too many far rows: CSR and rows straight from memory
        const int lane_a = opaque(lane), r_a = lane_a & 31, hq_a = lane_a >> 5;
        const int node = tile * kLTile + r_a;
        const char* own = reinterpret_cast<const char*>(h_in) +
                          ((size_t)(node < n ? node : n - 1) * 256 + hq_a * 16);
        f16x8 h[8];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) h[ks] = *reinterpret_cast<const f16x8*>(own + 32 * ks);
        gather_direct(h, z, reinterpret_cast<const char*>(h_in), row_ptr, col, typ, tbytes, node,
                      node < n, n, hq_a, scale16, p.edge_types);
      } else {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) z[ks] = zero8();
      }
      STAMP_X(1);
      if (next_active) plan_head_dma(next_plan, lds_head_slot, opaque(lane));
      STAMP_X(2);
    }
    STAMP_X(3);
    // ---- this wave's stage is spent: its pieces of c0 | c1 come in; one barrier later c0 is
    //      resident ---------------------------------------------------------------------------
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    x_chunk_dma(p.w01_image, 0, lds_stage, wave, opaque(lane));
    x_chunk_dma(p.w01_image, 1, lds_stage, wave, opaque(lane));
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // the plan head and c0 have landed
    window_barrier();
    STAMP_X(4);

    // what issues the next round's first stage fill (every wave is past the window)
    auto start_next_round = [&]() {
      if (next_active) {
        const int lane_n = opaque(lane);
        const PlanHeadQ next = x_plan_head_read(head_slot, lane_n);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        count = next.count, deepest = next.deepest;
        x_stage_dma(h_in, tile_of(next_first), n, lds_stage, lane_n, count, next.far4, 0);
        dma16(next_plan, (uint32_t)kPlanWords + (uint32_t)lane_n * 16u, lds_word_slot);
      }
    };
    // the residual rows of this tile -> the (spent) stage, rows of 256 B as in gine_layer.inc:
    // three waves per SIMD have no registers to keep them across the products
    auto fetch_residual = [&]() {
      if (kResidual && active) {
        const int lane_r = opaque(lane);
        const uint32_t sub = (uint32_t)lane_r >> 4, p16 = (uint32_t)lane_r & 15u;
#pragma unroll
        for (int g = 0; g < kLTile / 4; ++g) {
          const uint32_t q = 4u * g + sub;
          dma16(h_in, (uint32_t)(tile * kLTile + (int)q) * 256u + ((p16 ^ (q & 15u)) << 4),
                lds_stage + (uint32_t)g * 1024u);
        }
      }
    };
    const XWindowHooks<kHead, decltype(fetch_residual), decltype(start_next_round)> hooks{
        p, head_out.head, lds_stage, wave, opaque(lane), fetch_residual, start_next_round};
    raise_wave_priority(raise);
    f16x8 wrow[8];
    {
      const int lane_p = opaque(lane);
      f16x8 v[16];
      block_mlp_pipeline<XWindowLayout>(lds0, lane_p, lane_p >> 5, z, v, wrow, hooks);
      if constexpr (kTap) {
        const int row_t = tile * kLTile + (lane_p & 31), hq_t = lane_p >> 5;
        store_taps_zvw(tap, tap_out, active, row_t, hq_t, z, v, wrow);
      }
    }
    if (raise != 0) __builtin_amdgcn_s_setprio(0);
    STAMP_X(5);
    // ---- LayerNorm + residual.  Plain layer: the residual rows have been landing in the stage
    //      since the window was spent; they are read between the moments and the affine part, and
    //      the next round's first stage fill goes out right behind them, under the affine part.
    //      Head launch (the window is busy with the head's chunks): plain loads from L2 ---------
    f16x8 hn[8];
    {
      const int lane_d = opaque(lane), r_d = lane_d & 31, hq_d = lane_d >> 5;
      const char* const gamma = smem + kXLdsImage + (kLdsGamma - kLdsImage);
      const char* const beta = smem + kXLdsImage + (kLdsBeta - kLdsImage);
      f16x8 h[8];
      if constexpr (kHead) {
        if (kResidual && active) {
          const char* own = reinterpret_cast<const char*>(h_in) +
                            ((size_t)(tile * kLTile + r_d) * 256 + hq_d * 16);
#pragma unroll
          for (int ks = 0; ks < 8; ++ks) h[ks] = *reinterpret_cast<const f16x8*>(own + 32 * ks);
        } else {
#pragma unroll
          for (int ks = 0; ks < 8; ++ks) h[ks] = zero8();
        }
      }
      const RowMoments moments = layer_norm_moments(wrow);
      if constexpr (!kHead) {
        dma_wait_all();
        const uint32_t own = (uint32_t)r_d * 256u, x16 = (((uint32_t)r_d & 15u) ^ (uint32_t)hq_d) * 16u;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
          h[ks] = kResidual && active
                      ? *reinterpret_cast<const f16x8*>(stage + own + (x16 ^ (32u * ks)))
                      : zero8();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        start_next_round();
        STAMP_X(9);
      }
      layer_norm_affine<kResidual>(wrow, moments, h, hn, gamma, beta, hq_d);
      if constexpr (kTap) {
        if (active && tap == kTapY) {
          f16x8 y[8];
          layer_norm_affine<false>(wrow, moments, h, y, gamma, beta, hq_d);
          store_row(tap_out, (size_t)(tile * kLTile + r_d), hq_d, y);
        }
      }
    }
    if constexpr (!kHead) {
      const int lane_e = opaque(lane);
      // every row of an active tile has storage (padded hidden-state buffers)
      if (active) store_row(h_out, (size_t)(tile * kLTile + (lane_e & 31)), lane_e >> 5, hn);
      STAMP_X(6);
      // the next stage half (and its slot words) have landed; this round's stores may still fly
      if (active && !kTap) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      STAMP_X(7);
    } else {
      // ---- the head from the registers (its chunks 0 | 1 have been landing since the last
      //      steps of the products); the next round's rows stream in under the normalise -------
      const int lane_e = opaque(lane), r_e = lane_e & 31, hq_e = lane_e >> 5;
      const HeadRowDest to = head_row_dest(head_out.shards, tile, r_e, active);
      STAMP_X(6);
      dma_wait_all();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      window_barrier();                               // head chunk 0 resident in the window
      f16x8 o[8];
      block_head_pipeline<XWindowLayout>(lds0, lane_e, hq_e, hn, o, hooks);
      STAMP_X(8);
      const double total = head_row_square_sum(o);
      const bool stores = __ballot(to.dest >= 0) != 0;   // wave-uniform: eight store instructions
      if (to.dest >= 0) {
        char* rowp = to.out + (size_t)to.dest * (kOutDim * 2) + hq_e * 16;
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
      STAMP_X(7);
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
#undef STAMP_X
}
