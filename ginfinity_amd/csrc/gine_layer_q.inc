// Persistent form of the fused layer kernel of gine_layer.inc (included by gine_f16.hip):
// one 512-thread workgroup per CU walks ROUNDS of eight tiles (one per wave), same phases, same
// LDS overlay ([W0 | W1] over the eight spent gather stages) and the shared pieces around the
// pipelines (load_plan_words, store_row, store_taps_zvw, head_row_dest, head_row_square_sum),
// with what a round can hide of the next one hidden:
//
//   round r:  stage(r) landed -> gather -> [W0 | W1] over the stages -> barrier -> products
//             -> plan head of round r+1 requested -> barrier (every wave is done with the
//             weights) -> the rows of round r+1 start streaming into the stages by LDS-DMA
//             -> LayerNorm + residual + store of round r UNDER that fill -> round r+1
//
// so hop 1 (plan header + far list) and most of hop 2 (the rows) of every round but the first
// cost nothing, the constant image is loaded once per workgroup, and a launch pays its ramp
// once for all rounds.  What stays exposed per round: the 128-KB weight fill and the skew of
// the barrier behind the products.
//
// `stagger`: the workgroups of one XCD start (blockIdx / 8) x stagger shader cycles apart.  All
// CUs of a launch otherwise run their fill bursts at the same moments (equal rounds, started
// together): 37 MB requested at once, nothing in between — measured 10 k cycles per burst at
// 720,000 nodes against 3 k when a quarter of the CUs run.  Spread over a round, the bursts see
// the memory system's unloaded latency instead.
//
// The head is not part of this kernel (k_head_d runs behind the last layer).

// A copy of a lane-dependent value the optimiser cannot trace back: what is computed from it
// inside the tile loop is recomputed per phase instead of being hoisted out of the loop and
// held in registers across every phase (the loop body needs all 256 of them)
__device__ __forceinline__ int opaque(int value) {
  asm volatile("" : "+v"(value));
  return value;
}

// the rows of one tile -> the wave's stage: own rows 0..31, then the far rows the plan names
__device__ __forceinline__ void stage_dma(const f16* h_in, int tile, int n, uint32_t lds_stage,
                                          int lane, int count, const u32x4 (&far4)[3]) {
  const uint32_t sub = (uint32_t)lane >> 4, p16 = (uint32_t)lane & 15u;
#pragma unroll
  for (int g = 0; g < kLTile / 4; ++g) {
    const uint32_t q = 4u * g + sub;
    int own = tile * kLTile + (int)q;
    own = own < n ? own : n - 1;
    dma16(h_in, (uint32_t)own * 256u + ((p16 ^ (q & 15u)) << 4), lds_stage + (uint32_t)g * 1024u);
  }
  if (count <= kLFar) {
    const uint32_t fars[12] = {far4[0][0], far4[0][1], far4[0][2], far4[0][3],
                               far4[1][0], far4[1][1], far4[1][2], far4[1][3],
                               far4[2][0], far4[2][1], far4[2][2], far4[2][3]};
#pragma unroll
    for (int g = 0; g < kLFar / 4; ++g) {
      if (4 * g < count) {   // wave-uniform
        const uint32_t q = (uint32_t)kLTile + 4u * g + sub;
        dma16(h_in, fars[g] * 256u + ((p16 ^ (q & 15u)) << 4),
              lds_stage + (uint32_t)(kLTile / 4 + g) * 1024u);
      }
    }
  }
}

// plan header + far list of one tile (208 B) -> this wave's 256-byte slot behind the constant
// image, by ONE LDS-DMA instruction (lane 0 fetches the header, lanes 1..12 the far list): no
// registers are held while it is in flight, nothing for the compiler to spill or wait for
constexpr int kQLdsHeads = kLdsBytes;                        // 8 slots of 256 B
constexpr int kQLdsBytes = kQLdsHeads + kLWaves * 256;       // 157,696
static_assert(kQLdsBytes <= 160 * 1024, "one workgroup per CU");
__device__ __forceinline__ void plan_head_dma(const char* plan /* uniform */, uint32_t lds_slot,
                                              int lane) {
  if (lane < 13)
    dma16(plan, lane == 0 ? 0u : (uint32_t)kPlanFar + (uint32_t)(lane - 1) * 16u, lds_slot);
}
struct PlanHeadQ {
  int count, deepest;
  u32x4 far4[3];
};
__device__ __forceinline__ PlanHeadQ plan_head_read(const char* slot, int lane) {
  PlanHeadQ q;
  const int4 header = *reinterpret_cast<const int4*>(slot);
  const u32x4* far_at = reinterpret_cast<const u32x4*>(slot + 16 + (lane >> 4) * 48);
  q.far4[0] = far_at[0], q.far4[1] = far_at[1], q.far4[2] = far_at[2];
  q.count = __builtin_amdgcn_readfirstlane(header.x);
  q.deepest = __builtin_amdgcn_readfirstlane(header.y);
  return q;
}

// kTap: see store_taps_zvw (gine_layer.inc).
// kHead: the launch also runs head + float64 normalise on every tile's new hidden state (fp16
// output), straight from the registers: h_out is not written at all, the head's 64-KB image
// replaces W0 under the second product (as in k_gine_layer_f16), and the NORMALISE of round r
// is what runs under the stage fill of round r + 1.
struct HeadOut {   // kHead only: where the rows go
  HeadF16 head;
  ShardTable shards;
  int normalise;
};
template <bool kResidual, bool kTap = false, bool kHead = false>
__global__ __launch_bounds__(kLThreads) void k_gine_layer_q(
    const LayerF16 p, const f16* __restrict__ h_in, f16* __restrict__ h_out,
    const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const uint8_t* __restrict__ typ, const char* __restrict__ plans, int n, int num_tiles,
    int stagger, int32_t* __restrict__ spent_tile_sums, unsigned long long* __restrict__ span,
    int tap, f16* __restrict__ tap_out, const HeadOut head_out) {
  static_assert(!(kTap && kHead), "the tap instantiation is a plain layer");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const char* const tbytes = smem + kLdsTable;
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const char* const stage = smem + wave * kLdsStageBytes;
  const uint32_t lds_stage = lds0 + (uint32_t)wave * kLdsStageBytes;
  if (span && t == 0) atomicMin(&span[0], (unsigned long long)__builtin_amdgcn_s_memrealtime());
  if (stagger > 0) {
    const unsigned long long until =
        __builtin_amdgcn_s_memtime() + (unsigned long long)(blockIdx.x >> 3) * (unsigned)stagger;
    while (__builtin_amdgcn_s_memtime() < until) __builtin_amdgcn_s_sleep(8);
  }
#ifdef GFY_STAMPS
#define STAMP_Q(slot)                                                                         \
  do {                                                                                        \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();                             \
    if (t == kStampThread && blockIdx.x < 256) g_stamps[blockIdx.x][slot] += now_ - last_stamp; \
    last_stamp = now_;                                                                        \
  } while (0)
  constexpr int kStampThread = 64 * (GFY_STAMP_WAVE & 7);
  unsigned long long last_stamp = __builtin_amdgcn_s_memtime();
  const unsigned long long first_stamp = last_stamp;
  if (t == 0 && blockIdx.x < 512) g_real[blockIdx.x][0] = __builtin_amdgcn_s_memrealtime();
#else
#define STAMP_Q(slot)
#endif

  // ---- rounds: XCD (blockIdx & 7) owns the tiles [xbase, xend); in round rd the workgroups of
  //      the XCD take consecutive groups of eight tiles ---------------------------------------
  const int tpx = (num_tiles + 7) >> 3;
  const int xbase = (int)(blockIdx.x & 7) * tpx;
  const int xend = xbase + tpx < num_tiles ? xbase + tpx : num_tiles;
  const int group_stride = (int)(gridDim.x >> 3) * kLWaves;
  int first = xbase + (int)(blockIdx.x >> 3) * kLWaves;      // first tile of this round's group
  auto tile_of = [&](int group) { return group + wave; };
  auto active_in = [&](int group) { return group + wave < xend; };   // wave-uniform

  // the constant image (and the head's biases behind it): once per workgroup
  {
    u32x4 image_chunk = {0, 0, 0, 0};
    if (t < kLdsImageBytes / 16) image_chunk = reinterpret_cast<const u32x4*>(p.image)[t];
    else if (kHead) image_chunk = reinterpret_cast<const u32x4*>(head_out.head.image)[t - kLdsImageBytes / 16];
    if (t < kLdsImageBytes / 16 || kHead) reinterpret_cast<u32x4*>(smem + kLdsImage)[t] = image_chunk;
  }
  // the first round's plan head -> LDS slot, rows -> stage, slot words -> registers
  const char* const head_slot = smem + kQLdsHeads + wave * 256;
  const uint32_t lds_head_slot = lds0 + (uint32_t)kQLdsHeads + (uint32_t)wave * 256u;
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
  lds_barrier();                                    // constants visible
  STAMP_Q(0);

  const f16 scale16 = (f16)p.scale;
  HeadF16 no_head{};
  while (first < xend) {                            // workgroup-uniform
    const int tile = tile_of(first);
    const int next_first = first + group_stride;
    const bool next_active = next_first < xend && active_in(next_first);
    if (spent_tile_sums && active && lane == 0) spent_tile_sums[tile] = 0;
    const bool staged = count <= kLFar;

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
    STAMP_Q(1);
    // ---- this wave's stage is spent: its slice of [W0 | W1] comes in; one barrier later both
    //      matrices are resident -----------------------------------------------------------
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    issue_weight_slice_dma(p.w01_image, lds0 + kLdsWeights, wave, opaque(lane), 0,
                           kLdsStageBytes / 1024);
    dma_wait_all();
    lds_barrier();
    STAMP_Q(2);
    // the next round's plan head is requested now and lands under the products (hop 1 of the
    // next round: 1-7 k cycles of latency, by how far the plans are from the caches)
    const char* const next_plan =
        plans + (size_t)(next_active ? tile_of(next_first) : tile) * kPlanBytes;
    if (next_active) plan_head_dma(next_plan, lds_head_slot, opaque(lane));
    f16x8 wrow[8];
    if constexpr (kTap) {
      const int lane_t = opaque(lane), row_t = tile * kLTile + (lane_t & 31), hq_t = lane_t >> 5;
      f16x8 v[16];
      mlp_pipeline<false>(smem, lds0, wave, lane_t, hq_t, z, v, wrow, no_head);
      store_taps_zvw(tap, tap_out, active, row_t, hq_t, z, v, wrow);
    } else {
      const int lane_c = opaque(lane);
      mlp_pipeline<kHead>(smem, lds0, wave, lane_c, lane_c >> 5, z, wrow,
                          kHead ? head_out.head : no_head);
    }
    STAMP_Q(3);
    // what issues the next round's stage fill (all waves are past the weights / the head image)
    auto start_next_round = [&]() {
      if (next_active) {
        const int lane_b = opaque(lane);
        dma_wait_all();
        const PlanHeadQ next = plan_head_read(head_slot, lane_b);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        count = next.count, deepest = next.deepest;
        stage_dma(h_in, tile_of(next_first), n, lds_stage, lane_b, count, next.far4);
        load_plan_words(next_plan, lane_b & 31, word);
      } else {   // nothing of this round is carried into a round that does not gather
#pragma unroll
        for (int i = 0; i < 8; ++i) word[i] = 0;
      }
    };
    f16x8 hn[8];
    if constexpr (!kHead) {
      // ---- every wave is done with the weights: the next round's rows stream into the stages
      //      under this round's LayerNorm ---------------------------------------------------
      lds_barrier();
      STAMP_Q(4);
      start_next_round();
      STAMP_Q(5);
      const int lane_d = opaque(lane);
      layer_norm_residual<kResidual>(wrow, h, hn, smem + kLdsGamma, smem + kLdsBeta, lane_d >> 5);
      if constexpr (kTap) {
        if (active && tap == kTapY) {
          f16x8 y[8];
          layer_norm_residual<false>(wrow, h, y, smem + kLdsGamma, smem + kLdsBeta, lane_d >> 5);
          store_row(tap_out, (size_t)(tile * kLTile + (lane_d & 31)), lane_d >> 5, y);
        }
      }
      // every row of an active tile has storage (padded hidden-state buffers)
      if (active) store_row(h_out, (size_t)(tile * kLTile + (lane_d & 31)), lane_d >> 5, hn);
      STAMP_Q(6);
      // the next stage (and its slot words) have landed; this round's stores may still fly
      if (active && !kTap) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      STAMP_Q(7);
    } else {
      // ---- LayerNorm, then the head from the registers; the next round's rows stream in under
      //      the float64 normalise ------------------------------------------------------------
      const int lane_d = opaque(lane), r_d = lane_d & 31, hq_d = lane_d >> 5;
      layer_norm_residual<kResidual>(wrow, h, hn, smem + kLdsGamma, smem + kLdsBeta, hq_d);
      STAMP_Q(6);
      const HeadRowDest to = head_row_dest(head_out.shards, tile, r_d, active);
      dma_wait_all();
      lds_barrier();                                  // head.0 | head.2 resident over W0
      f16x8 o[8];
      head_pipeline(smem, lds0, lane_d, hq_d, hn, o);
      lds_barrier();                                  // every wave is done with the head image
      STAMP_Q(4);
      start_next_round();
      STAMP_Q(5);
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
      STAMP_Q(7);
    }
#ifdef GFY_STAMPS
    if (t == kStampThread && blockIdx.x < 256) g_stamps[blockIdx.x][11] += 1;
#endif
    first = next_first;
    active = next_active;
  }
#ifdef GFY_STAMPS
  if (t == kStampThread && blockIdx.x < 256) g_stamps[blockIdx.x][10] += last_stamp - first_stamp;
  if (t == 0 && blockIdx.x < 512) g_real[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();
#endif
  if (span && lane == 0) atomicMax(&span[1], (unsigned long long)__builtin_amdgcn_s_memrealtime());
#undef STAMP_Q
}

// =====================================================================================
// k_head_d: head (_model.py:61-63,72) + float64 normalise (api.py:250-259) for fp16 output, with
// head.0 | head.2 (64 KB) resident in LDS and eight free-running waves per CU (no barrier after
// the prologue), each tile's hidden rows loaded straight into the MFMA operand registers (stored
// order), head_pipeline from the registers, core-row compaction at the store (out_rows).
// =====================================================================================
__global__ __launch_bounds__(kLThreads) void k_head_d(
    const HeadF16 head, const f16* __restrict__ h, const ShardTable shards, int num_tiles,
    int normalise) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int tpx = (num_tiles + 7) >> 3;
  const int stride = (int)(gridDim.x >> 3) * kLWaves;
  const int xbase = (int)(blockIdx.x & 7) * tpx;
  int local = (int)(blockIdx.x >> 3) * kLWaves + wave;
  auto exists = [&](int loc) { return loc < tpx && xbase + loc < num_tiles; };
  issue_head_dma(head.w_image, lds0 + kLdsWeights, wave, lane);       // 8 KB per wave
  if (t < 32) reinterpret_cast<u32x4*>(smem + kLdsHeadBa)[t] = reinterpret_cast<const u32x4*>(head.image)[t];
  dma_wait_all();
  lds_barrier();                                    // the only one
  // the rows of a tile are requested one tile ahead: they land under the previous tile's
  // normalise (ordinary loads: the compiler's counted waits are exact)
  auto load_rows = [&](int loc, f16x8 (&rows)[8]) {
    const int lane_l = opaque(lane);
    const char* own = reinterpret_cast<const char*>(h) +
                      ((uint32_t)((xbase + loc) * kLTile + (lane_l & 31)) * 256u +
                       (uint32_t)(lane_l >> 5) * 16u);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) rows[ks] = *reinterpret_cast<const f16x8*>(own + 32 * ks);
  };
  f16x8 ahead[8];
  if (exists(local)) load_rows(local, ahead);
  while (exists(local)) {
    const int tile = xbase + local;
    const int lane_a = opaque(lane), r = lane_a & 31, hq = lane_a >> 5;
    // (not head_row_dest: this kernel has no wave without a tile and fetches the shard's output
    // block before it knows whether the row is stored)
    const int node = tile * kLTile + r;
    const int shard = shards.shard_of_tile(tile);
    const int row = node - shards.tile_base[shard] * kLTile;          // shard-local
    const bool node_ok = row < shards.nodes[shard];
    int dest = row;
    if (shards.out_rows[shard] && node_ok) dest = shards.out_rows[shard][row];
    f16* const out = reinterpret_cast<f16*>(shards.out[shard]);
    f16x8 hn[8], o[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) hn[ks] = ahead[ks];
    if (exists(local + stride)) load_rows(local + stride, ahead);
    head_pipeline(smem, lds0, lane_a, hq, hn, o);
    const double total = head_row_square_sum(o);
    if (node_ok && dest >= 0) {
      char* rowp = reinterpret_cast<char*>(out) + (size_t)dest * (kOutDim * 2) + hq * 16;
      if (normalise) {   // see the head pass of k_gine_layer_f16
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
    local += stride;
  }
}
