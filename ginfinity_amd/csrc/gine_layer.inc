// Fused GINE layer (included by gine_f16.hip): ONE WAVE PER 32-NODE TILE.
//
// The round-1 kernel kept the 128 KB of layer weights in the registers of a 4-wave workgroup
// and walked every tile through four barrier-separated phases; its waves spent 69 % of their
// cycles parked or issue-stalled and residency was pinned at two tiles per CU by the weights
// (profiles/README.md).  Here the allocation is the opposite:
//
//  * the WEIGHTS live in LDS, once per CU, shared by the eight waves of the one 512-thread
//    workgroup a CU holds, streamed in by LDS-DMA;
//  * the ACTIVATIONS of a tile never leave the registers of the one wave that owns it.  Lane
//    (r, hq) = (lane & 31, lane >> 5) holds node r; element j of k-step s is channel
//    16 s + 8 (j >> 2) + 4 hq + (j & 3): the C/D layout of v_mfma_f32_32x32x16_f16 read as a
//    B operand.  So the result of one product IS the operand of the next (BatchNorm + ReLU,
//    bias, LayerNorm, residual all run in place), LayerNorm is 64 in-lane values plus one
//    half-swap, and nothing goes through LDS between the phases of a tile.  The k order this
//    implies inside an MFMA is undone on the host (pack_k_chained).  Hidden rows are STORED in
//    this order too (16-byte chunk 2 s + hq of a row = the lane's eight values: within every
//    16 channels the groups 4-7 and 8-11 trade places, weight_image.h stored_channel);
//  * the gather-sum reads source rows (in-tile and out-of-tile alike) and edge-type rows out
//    of LDS with ds_read_b128, forms relu(h + T) in packed fp16, and ACCUMULATES ON THE MATRIX
//    CORES: one MFMA with a 0/1 selection matrix adds a slot's 16 channels x 32 nodes into an
//    fp32 accumulator (products by 1.0 are exact; the sum is the fp32 add of the reference) —
//    the vector unit, which bounds this phase, issues 8 instructions per slot and chunk instead
//    of 16.
//
// LDS (152 KB): eight 18-KB gather stages (a tile's 32 own rows + up to 40 far rows, filled by
// LDS-DMA); when a wave has finished its gather it refills ITS OWN stage with the slice of
// [W0 | W1] (128 KB) that belongs there, and one barrier later both products run without
// another one; the head's 64 KB later replace W0 under the second product.  Two workgroup
// barriers per launch (four with the head).  A launch holds 8 x ceil(tiles / 64) workgroups,
// XCD x = workgroups x, x + 8, ... owning a contiguous range of tiles; at the benchmark shape
// (1,875 tiles) every wave of the chip does exactly one tile.
//
// The products are software pipelines (mlp_pipeline, head_pipeline): hipcc (ROCm 7.2)
// serialises "ds_read -> wait -> mfma" when the A operand comes from LDS (209 cycles per MFMA,
// tools/isa_semantics.hip), so every LDS read of a pipeline is inline asm with ONE counted
// s_waitcnt per step, while the MFMAs are builtins: the compiler interleaves the epilogue
// slices of the previous block pair with them and pads the MFMA hazards.  A step = one k-step
// of a block pair = two MFMAs on two accumulator chains, so that one wave keeps the matrix
// pipe busy (a single dependent chain issues every ~45 cycles, not 32).
//
// Rounding points are the reference's (SURVEY §8-A): every R16 is a v_cvt_pk_f16_f32 of an
// fp32 value that was itself rounded once (v_fma_mix_f32) — v_fma_mixlo_f16 rounds the exact
// result once and is NOT R16(R32(.)) (tools/isa_semantics.hip, 12 % of crafted ties differ).

constexpr int kLTile = 32;               // nodes per tile = per wave
constexpr int kLWaves = 8;               // tiles per workgroup
constexpr int kLThreads = 64 * kLWaves;
constexpr int kLSlots = 8;               // in-edge slots per node in a plan
constexpr int kLFar = 40;                // far rows staged per tile (an RNA tile needs <= 38)
constexpr int kLStageRows = kLTile + kLFar;   // a stage: the tile's own rows, then the far rows
constexpr int kLDirect = 1 << 20;        // far count that sends a tile down the direct path

// ---- tile plan (global memory) ---------------------------------------------------------
constexpr int kPlanCount = 0;            // int: far rows (+ kLDirect: some in-degree > kLSlots)
constexpr int kPlanDegree = 4;           // int: largest in-degree
constexpr int kPlanWords = 16;           // u32[32][8]: stage row | type << 8
constexpr int kPlanFar = kPlanWords + kLTile * kLSlots * 4;   // int[4][12]: [sub][g] = far[4g+sub]
constexpr int kPlanBytes = kPlanFar + 4 * 12 * 4;             // 1,232
static_assert(kLFar <= 48 && kLFar % 4 == 0, "far list is fetched as 12 entries per lane group");
static_assert(kPlanBytes % 16 == 0, "plans are read with 16-byte loads");

// ---- LDS map (bytes) -----------------------------------------------------------------
constexpr int kLdsWeights = 0;                       // [W0 | W1] over the spent stages
constexpr int kLdsW1 = 64 * 1024;
constexpr int kLdsWeightBytes = 128 * 1024;
constexpr int kLdsStageBytes = kLStageRows * 256;    // 18,432: row q, 16-byte position p holds
                                                     // chunk p ^ (q & 15)
constexpr int kLdsImage = kLWaves * kLdsStageBytes;  // per-layer constant image, then the head's:
constexpr int kLdsTable = kLdsImage + kImageTable;   // layer_image.h has the fields and their
constexpr int kLdsAlpha = kLdsImage + kImageAlpha;   // layouts, weight_image.cpp writes them
constexpr int kLdsShift = kLdsImage + kImageShift;
constexpr int kLdsB0 = kLdsImage + kImageB0;
constexpr int kLdsB1 = kLdsImage + kImageB1;
constexpr int kLdsGamma = kLdsImage + kImageGamma;
constexpr int kLdsBeta = kLdsImage + kImageBeta;
constexpr int kLdsImageBytes = kImageBytes;                              // 7,680
constexpr int kLdsHeadBa = kLdsImage + kImageBytes + kHeadImageBa;
constexpr int kLdsHeadBb = kLdsImage + kImageBytes + kHeadImageBb;
constexpr int kLdsBytes = kLdsImage + kImageBytes + kHeadImageBytes;     // 155,648
static_assert(kLdsStageBytes * kLWaves >= kLdsWeightBytes, "the weights overlay the stages");
static_assert(kLdsStageBytes % 1024 == 0, "a stage is refilled by whole 1-KB DMA instructions");
static_assert(kLdsImageBytes == 480 * 16, "one 16-byte chunk per thread 0..479");
static_assert(kHeadImageBytes == 32 * 16, "the head image: 32 more chunks (512 bytes of LDS)");
static_assert(kLdsBytes <= 160 * 1024, "one workgroup per CU");

// ---------------------------------------------------------------------------------
// tile plans: one 256-thread workgroup per 32-node tile, eight threads per row.  Each thread
// brings one in-edge of its row (or none) and the CSR position `slot` that edge has inside
// the row; threads without an edge own the remaining slots.  Layer-invariant: once per encode.
// ---------------------------------------------------------------------------------
static_assert(kCsrSlots == kLSlots && kCsrTileRows == kLTile && kCsrStageFarRows == kLFar,
              "csr_finish.inc finishes one tile per block and knows what a stage holds");

__device__ __forceinline__ void tile_plan_from_edges(char* __restrict__ plans, int tile,
                                                     int row, int slot, bool live, int src,
                                                     uint32_t ty, int degree, int type_limit) {
  __shared__ int s_count, s_degree, s_far[48];
  const int t = threadIdx.x, lane = t & 63;
  const int base = tile * kLTile;
  char* const plan = plans + (size_t)tile * kPlanBytes;
  if (t < 48) s_far[t] = 0;
  if (t == 0) s_count = 0, s_degree = 0;
  __syncthreads();
  if (!live) ty = kMaxEdgeTypes;   // idle slot: own row + the -inf table row
  const uint32_t rel = (uint32_t)(src - base);
  // `src` is a global row, or -1 for a source outside its shard (csr_finish.inc); such sources
  // and types the model has no table row for (>= edge_dim) cannot come from a validated shard
  // (graph.py:318-323): the edge is IGNORED — kept out of every address computation (idle
  // slot) instead of being trusted; the direct path does the same (gather_direct)
  const bool bad = live && (src < 0 || ty >= (uint32_t)type_limit);
  if (bad) ty = kMaxEdgeTypes;
  const bool outside = live && !bad && rel >= (uint32_t)kLTile;
  uint32_t stage_row = (live && !bad) ? rel : (uint32_t)row;
  const unsigned long long mask = __ballot(outside);
  if (mask) {   // wave-uniform: far rows get stage rows in arrival order
    const int before = __builtin_amdgcn_mbcnt_hi(
        (uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
    int first = 0;
    if (lane == 0) first = atomicAdd(&s_count, __popcll(mask));
    first = __builtin_amdgcn_readfirstlane(first);
    const int far_slot = first + before;
    if (outside) {
      stage_row = (uint32_t)(kLTile + (far_slot < kLFar ? far_slot : 0));
      if (far_slot < kLFar) s_far[far_slot] = src;
    }
  }
  reinterpret_cast<uint32_t*>(plan + kPlanWords)[row * kLSlots + slot] = stage_row | (ty << 8);
  // largest in-degree of the wave's 8 rows; a row with more in-edges than slots sends the
  // whole tile down the direct path
  const int capped = degree < kLSlots ? degree : kLSlots;
  int deepest = capped;
#pragma unroll
  for (int off = 8; off < 64; off <<= 1) {
    const int other = __shfl_xor(deepest, off, 64);
    deepest = other > deepest ? other : deepest;
  }
  const unsigned long long over = __ballot(degree > kLSlots);
  if (lane == 0) {
    if (deepest) atomicMax(&s_degree, deepest);
    if (over) atomicAdd(&s_count, kLDirect);
  }
  __syncthreads();
  if (t < 48) {
    const int q = 4 * (t % 12) + t / 12;
    reinterpret_cast<int*>(plan + kPlanFar)[t] = q < kLFar ? s_far[q] : 0;
  }
  if (t == 0) {
    const int4 header = {s_count, s_degree, 0, 0};
    *reinterpret_cast<int4*>(plan) = header;
  }
}

// from a finished CSR (gfy_encode behind gfy_build_csr; one shard, global = local numbering):
// thread (row, s) takes in-edge s
__device__ __forceinline__ void tile_plan_block(
    const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const uint8_t* __restrict__ typ, int n, char* __restrict__ plans, int tile, int type_limit) {
  const int row = threadIdx.x >> 3, s = threadIdx.x & 7;
  const int node = tile * kLTile + row;
  const int lo = row_ptr[node < n ? node : n], hi = row_ptr[node + 1 < n ? node + 1 : n];
  const bool live = lo + s < hi;
  int src = 0;
  uint32_t ty = kMaxEdgeTypes;
  if (live) {
    src = col[lo + s];
    ty = typ[lo + s];
    if ((uint32_t)src >= (uint32_t)n) src = -1;
  }
  tile_plan_from_edges(plans, tile, row, s, live, src, ty, hi - lo, type_limit);
}

// per-encode setup in ONE launch: workgroups [0, plan_blocks) write the tile plans, the rest
// compute the input Linear — two independent jobs on disjoint data
__global__ __launch_bounds__(256) void k_encode_setup(
    const ShardTable shards, const f16* __restrict__ w_in, const f16* __restrict__ b_in,
    f16* __restrict__ h0, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const uint8_t* __restrict__ typ, char* __restrict__ plans, int plan_blocks, int type_limit) {
  if ((int)blockIdx.x < plan_blocks)
    tile_plan_block(row_ptr, col, typ, shards.nodes[0], plans, blockIdx.x, type_limit);
  else
    input_linear_block(shards, w_in, b_in, h0, blockIdx.x - plan_blocks, gridDim.x - plan_blocks);
}

// the same from COO (gfy_encode_coo, one shard or a batch): workgroups [0, plan_blocks) FINISH
// THE CSR of their 32 rows (csr_finish.inc: col/typ written for the direct path) and plan the
// tile from the edges they have just ranked; the rest compute the input Linear
template <bool kScanned>
#ifndef GFY_SETUP_MIN_BLOCKS
#define GFY_SETUP_MIN_BLOCKS 8   // 44 instead of 88 registers: eight blocks per CU hide the latency chain (39.2 -> 32.1 us per 4 shards)
#endif
__global__ __launch_bounds__(256, GFY_SETUP_MIN_BLOCKS) void k_encode_setup_coo(
    const ShardTable shards, const f16* __restrict__ w_in, const f16* __restrict__ b_in,
    f16* __restrict__ h0, const CsrScratch scratch, int32_t* __restrict__ row_ptr,
    int32_t* __restrict__ col, uint8_t* __restrict__ typ, char* __restrict__ plans,
    int plan_blocks, int type_limit) {
  if ((int)blockIdx.x < plan_blocks) {
    const CsrEdge edge =
        csr_finish_tile<kScanned, true>(scratch, shards, row_ptr, blockIdx.x, col, typ);
    tile_plan_from_edges(plans, blockIdx.x, threadIdx.x >> 3,
                         edge.live ? edge.rank : (int)(threadIdx.x & 7), edge.live, edge.source,
                         edge.type, edge.degree, type_limit);
    csr_finish_release(scratch, plan_blocks);
  } else {
    input_linear_block(shards, w_in, b_in, h0, blockIdx.x - plan_blocks, gridDim.x - plan_blocks);
  }
}

// ---- single-rounding building blocks (all results are fp32 rounded once, or R16 of such) --
// fp32(acc + (float)half): fma((float)half, 1, acc), which hipcc selects as ONE v_fma_mix_f32
// (conversion, product by one and sum in one rounding).  Compiler-visible on purpose: this is
// the instruction that reads MFMA results, and the compiler pads the MFMA -> VALU hazard only
// for instructions it can see (an inline-asm reader behind the last MFMAs of a pipeline got
// register 0 of the chain stale).  The 1.0 comes out of an SGPR the optimiser cannot fold
// (fma(x, 1, y) would become cvt + add: two instructions).
__device__ __forceinline__ float opaque_one() {
  float one;
  asm("s_mov_b32 %0, 1.0" : "=s"(one));
  return one;
}
template <int kHi>
__device__ __forceinline__ float add_half(float acc, uint32_t packed) {
  return __builtin_fmaf((float)__builtin_bit_cast(f16x2, packed)[kHi], opaque_one(), acc);
}
// fp32 fma((float)half, b, c)
template <int kHi>
__device__ __forceinline__ float fma_half(uint32_t packed, float b, float c) {
  float d;
  if constexpr (kHi)
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
        : "=v"(d) : "v"(packed), "v"(b), "v"(c));
  else
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]"
        : "=v"(d) : "v"(packed), "v"(b), "v"(c));
  return d;
}
// fp32 fma(a, (float)half_b, (float)half_c): LayerNorm's affine, gamma/beta kept as fp16
template <int kHi>
__device__ __forceinline__ float fma_f32_hh(float a, uint32_t b_packed, uint32_t c_packed) {
  float d;
  if constexpr (kHi)
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,1] op_sel_hi:[0,1,1]"
        : "=v"(d) : "v"(a), "v"(b_packed), "v"(c_packed));
  else
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]"
        : "=v"(d) : "v"(a), "v"(b_packed), "v"(c_packed));
  return d;
}
// fp32((float)half * (float)half): exact (22 significant bits)
template <int kHi>
__device__ __forceinline__ float square_half(uint32_t packed) {
  float d;
  if constexpr (kHi)
    asm("v_fma_mix_f32 %0, %1, %1, 0 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "=v"(d) : "v"(packed));
  else
    asm("v_fma_mix_f32 %0, %1, %1, 0 op_sel_hi:[1,1,0]" : "=v"(d) : "v"(packed));
  return d;
}
// fp32 fma((float)half, (float)half, acc): the square of one half added to an fp32 sum, one
// rounding (the product itself is exact)
template <int kHi>
__device__ __forceinline__ float fma_hh_acc(uint32_t packed, float acc) {
  float d;
  if constexpr (kHi)
    asm("v_fma_mix_f32 %0, %1, %1, %2 op_sel:[1,1,0] op_sel_hi:[1,1,0]"
        : "=v"(d) : "v"(packed), "v"(acc));
  else
    asm("v_fma_mix_f32 %0, %1, %1, %2 op_sel_hi:[1,1,0]" : "=v"(d) : "v"(packed), "v"(acc));
  return d;
}
__device__ __forceinline__ uint32_t cvt_pk_f16(float lo, float hi) {   // two RNE conversions
  uint32_t d;
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(d) : "v"(lo), "v"(hi));
  return d;
}
__device__ __forceinline__ uint32_t pk_relu(uint32_t v) {
  uint32_t d;
  asm("v_pk_max_f16 %0, %1, 0" : "=v"(d) : "v"(v));
  return d;
}
// x + (value of the lane 32 away): one v_permlane32_swap of two copies
__device__ __forceinline__ float add_other_half(float x) {
  uint32_t a = __builtin_bit_cast(uint32_t, x), b = a;
  asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b);
}
__device__ __forceinline__ double add_other_half(double x) {
  const unsigned long long bits = __builtin_bit_cast(unsigned long long, x);
  uint32_t lo_a = (uint32_t)bits, lo_b = lo_a, hi_a = (uint32_t)(bits >> 32), hi_b = hi_a;
  asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(lo_a), "+v"(lo_b));
  asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(hi_a), "+v"(hi_b));
  const double a = __builtin_bit_cast(double, ((unsigned long long)hi_a << 32) | lo_a);
  const double b = __builtin_bit_cast(double, ((unsigned long long)hi_b << 32) | lo_b);
  return a + b;
}

// ---------------------------------------------------------------------------------
// gather-sum of one tile, slots 0 .. S-1 of every node (S = the tile's largest in-degree).
// Lane (r, hq), 16-channel chunk ks: the 2 S LDS reads of chunk ks + 1 are in flight while
// chunk ks is reduced — m_s = relu(h_src + T_type) in packed fp16 (exact: 24 >= 2*11+2 bits,
// then RNE: the same value as the fp32 add rounded to fp16), acc += SEL . m_s on the matrix
// cores in CSR order (SEL picks each of the 16 channels once: fp32 add of an exact product),
// ONE rounding, z = R(R(s h) + agg).
// ---------------------------------------------------------------------------------
template <int S>
__device__ __forceinline__ void gather_tile(const f16x8 (&h)[8], f16x8 (&z)[8],
                                            const uint32_t (&word)[8], const char* tbytes,
                                            const char* stage, int r, int hq, f16 scale16) {
  uint32_t toff[S], saddr[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const uint32_t q = word[s] & 0xFFu;
    toff[s] = (word[s] >> 8) * 256u + (uint32_t)hq * 16u;
    // chunk 2 ks + hq of stage row q sits at position (2 ks + hq) ^ (q & 15): row base and
    // position bits do not overlap, so one XOR with 32 ks yields the address of chunk ks
    saddr[s] = q * 256u + ((q & 15u) ^ (uint32_t)hq) * 16u;
  }
  // A operand that copies channel c (of 16) of the B operand into row c of the result:
  // lane (m, half) element jj is 1 where (half, jj) is the B position of channel m
  f16x8 sel = zero8();
  {
    const int want_half = (r >> 2) & 1, want_j = (r & 3) + 4 * (r >> 3);
#pragma unroll
    for (int jj = 0; jj < 8; ++jj)
      if (r < 16 && hq == want_half && jj == want_j) sel[jj] = (f16)1.0f;
  }
  constexpr bool kAhead = S <= 6;   // deeper tiles: registers for one chunk in flight only
  f16x8 hv[kAhead ? 2 : 1][S], ev[kAhead ? 2 : 1][S];
  auto fetch = [&](int ks, f16x8 (&hd)[S], f16x8 (&ed)[S]) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      hd[s] = *reinterpret_cast<const f16x8*>(stage + (saddr[s] ^ (32u * ks)));
      ed[s] = *reinterpret_cast<const f16x8*>(tbytes + toff[s] + 32 * ks);
    }
  };
  auto reduce = [&](int ks, const f16x8 (&hd)[S], const f16x8 (&ed)[S]) {
    f32x16 acc = {0};
#pragma unroll
    for (int s = 0; s < S; ++s)   // CSR order: slot s is the s-th in-edge
#ifdef GFY_DIAG_NO_GATHER_VALU   // diagnostic (wrong results)
      acc = mfma(sel, hd[s], acc);
#else
      acc = mfma(sel, __builtin_elementwise_max(hd[s] + ed[s], zero8()), acc);
#endif
    // rows 0..15 of the result = registers 0..7 = this lane's eight channels.  Plain casts,
    // not inline asm: the compiler pads the MFMA -> VALU hazard only for instructions it sees
    f16x8 agg;
#pragma unroll
    for (int j = 0; j < 8; ++j) agg[j] = (f16)acc[j];   // ONE rounding of the fp32 sum
    z[ks] = h[ks] * scale16 + agg;   // two fp16 ops, two roundings
  };
  if constexpr (kAhead) {
    fetch(0, hv[0], ev[0]);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      if (ks + 1 < 8) fetch(ks + 1, hv[(ks + 1) & 1], ev[(ks + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
      reduce(ks, hv[ks & 1], ev[ks & 1]);
    }
  } else {
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      fetch(ks, hv[0], ev[0]);
      __builtin_amdgcn_sched_barrier(0);
      reduce(ks, hv[0], ev[0]);
    }
  }
}

// direct path (a node with more than kLSlots in-edges, or more than kLFar far rows in the
// tile): CSR and neighbour rows straight from memory, per-lane edge loops, fp32 adds
__device__ __forceinline__ void gather_direct(const f16x8 (&h)[8], f16x8 (&z)[8],
                                              const char* __restrict__ hbytes,
                                              const int32_t* __restrict__ row_ptr,
                                              const int32_t* __restrict__ col,
                                              const uint8_t* __restrict__ typ,
                                              const char* tbytes, int node, bool node_ok,
                                              int n, int hq, f16 scale16, int type_limit) {
  const int lo = node_ok ? row_ptr[node] : 0, hi = node_ok ? row_ptr[node + 1] : 0;
#pragma unroll 1
  for (int ks = 0; ks < 8; ++ks) {
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    const uint32_t c16 = (uint32_t)(2 * ks + hq) * 16u;
    for (int e = lo; e < hi; ++e) {
      const uint32_t src = (uint32_t)col[e];
      const uint32_t ty = typ[e];
      if (src >= (uint32_t)n || ty >= (uint32_t)type_limit) continue;   // see tile_plan_from_edges
      const f16x8 hv = *reinterpret_cast<const f16x8*>(hbytes + (src * 256u + c16));
      const f16x8 ev = *reinterpret_cast<const f16x8*>(tbytes + ty * 256u + c16);
      const u32x4 m = __builtin_bit_cast(u32x4, __builtin_elementwise_max(hv + ev, zero8()));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[2 * q] = add_half<0>(acc[2 * q], m[q]);
        acc[2 * q + 1] = add_half<1>(acc[2 * q + 1], m[q]);
      }
    }
    u32x4 agg;
#pragma unroll
    for (int q = 0; q < 4; ++q) agg[q] = cvt_pk_f16(acc[2 * q], acc[2 * q + 1]);
    // z[ks] with a run-time ks would send z to scratch: select statically
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k == ks) z[k] = h[k] * scale16 + __builtin_bit_cast(f16x8, agg);
  }
}

// every wave's LDS writes done, then the workgroup barrier (LDS-DMA: a counted vmcnt first)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// instructions [first, last) of the 1-KB pieces of the 128-KB [W0 | W1] image that lie over
// this wave's own (spent) stage; pieces past the image (the last wave's stage ends behind W1)
// are skipped
__device__ __forceinline__ void issue_weight_slice_dma(const void* image, uint32_t lds0, int wave,
                                                       int lane, int first, int last) {
  const uint32_t begin = (uint32_t)wave * (uint32_t)kLdsStageBytes;
#pragma unroll
  for (int i = 0; i < kLdsStageBytes / 1024; ++i) {
    const uint32_t at = begin + (uint32_t)i * 1024u;
    if (i >= first && i < last && at < (uint32_t)kLdsWeightBytes)   // wave-uniform
      dma16(image, at + (uint32_t)lane * 16u, lds0 + at);
  }
}
// 8 KB of the head's 64-KB image per wave, over W0
__device__ __forceinline__ void issue_head_dma(const void* image, uint32_t lds0, int wave,
                                               int lane) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t at = (uint32_t)(wave * 8 + i) * 1024u;
    dma16(image, at + (uint32_t)lane * 16u, lds0 + at);
  }
}

// ---------------------------------------------------------------------------------
// LDS reads the compiler does not see (it would wait for each before the next MFMA), and the
// wait that hands their results over: all but the `kKeep` youngest LDS operations of the wave
// have landed.  `landed(x)` ties a consumer behind the wait; the caller fences the scheduler.
// ---------------------------------------------------------------------------------
template <int kOffA, int kOffB, typename T>
__device__ __forceinline__ void lds_read2_b128(T& x, T& y, uint32_t base) {
  static_assert(sizeof(T) == 16 && kOffA >= 0 && kOffA < 65536 && kOffB >= 0 && kOffB < 65536,
                "16-bit offset field");
  asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4"
               : "=&v"(x), "=&v"(y) : "v"(base), "n"(kOffA), "n"(kOffB));
}
template <int kOff, typename T>
__device__ __forceinline__ void lds_read_b128(T& x, uint32_t base) {
  static_assert(sizeof(T) == 16 && kOff >= 0 && kOff < 65536, "16-bit offset field");
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(x) : "v"(base), "n"(kOff));
}
template <int kOff>
__device__ __forceinline__ void lds_read_b64(u32x2& x, uint32_t base) {
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=&v"(x) : "v"(base), "n"(kOff));
}
template <int kOff>
__device__ __forceinline__ void lds_read_u16(uint32_t& x, uint32_t base) {   // zero-extended
  asm volatile("ds_read_u16 %0, %1 offset:%2" : "=&v"(x) : "v"(base), "n"(kOff));
}
__device__ __forceinline__ uint32_t opaque_zero() {   // a register the compiler does not keep
  uint32_t z;
  asm volatile("v_mov_b32 %0, 0" : "=v"(z));
  return z;
}
template <int kKeep>
__device__ __forceinline__ void lds_wait_keep() {
  asm volatile("s_waitcnt lgkmcnt(%0)" : : "n"(kKeep));
}
template <typename T>
__device__ __forceinline__ void landed(T& x) {
  asm volatile("" : "+v"(x));
}
// One slice of the first product's epilogue: registers 4g .. 4g+3 of one 32-channel block,
// u = R(acc + b0), v = relu(R(fma(u, alpha, shift))) -> two dwords of the next B operand.
// The bias is already in the accumulator: the last k-step of a block pair is followed by one
// more MFMA per block, b . 1 — a product by one is exact, so the accumulator is fp32(acc + b),
// what four v_fma_mix_f32 per slice computed before (the kernel's time follows its vector
// instruction count: profiles/r04_sensitivity.txt).
__device__ __forceinline__ void bn_slice(const f32x16& acc, int g, const f32x4& al,
                                         const f32x4& sh, uint32_t& out0, uint32_t& out1) {
#ifdef GFY_DIAG_NO_EPILOGUE   // diagnostic (wrong results): what the vector work of the slices costs
  out0 = __builtin_bit_cast(uint32_t, acc[4 * g]), out1 = __builtin_bit_cast(uint32_t, acc[4 * g + 2]);
  return;
#endif
  const uint32_t u01 = cvt_pk_f16(acc[4 * g], acc[4 * g + 1]);       // R(acc + b0)
  const uint32_t u23 = cvt_pk_f16(acc[4 * g + 2], acc[4 * g + 3]);
  const float y0 = fma_half<0>(u01, al[0], sh[0]), y1 = fma_half<1>(u01, al[1], sh[1]);
  const float y2 = fma_half<0>(u23, al[2], sh[2]), y3 = fma_half<1>(u23, al[3], sh[3]);
  out0 = pk_relu(cvt_pk_f16(y0, y1));
  out1 = pk_relu(cvt_pk_f16(y2, y3));
}
// ... and of the second product's: registers 8 sp .. 8 sp + 7 of a block, w = R(acc + b1)
__device__ __forceinline__ f16x8 round_slice(const f32x16& acc, int sp) {
  u32x4 packed;
#ifdef GFY_DIAG_NO_EPILOGUE
  for (int q = 0; q < 4; ++q) packed[q] = __builtin_bit_cast(uint32_t, acc[8 * sp + 2 * q]);
  return __builtin_bit_cast(f16x8, packed);
#endif
#pragma unroll
  for (int q = 0; q < 4; ++q) packed[q] = cvt_pk_f16(acc[8 * sp + 2 * q], acc[8 * sp + 2 * q + 1]);
  return __builtin_bit_cast(f16x8, packed);
}
// One slice of a bias epilogue on the vector pipe (the head's two products): registers
// 8 sp .. 8 sp + 7 of a block = one B-operand k-step
template <bool kRelu>
__device__ __forceinline__ f16x8 bias_slice(const f32x16& acc, int sp, const u32x4& bias) {
  u32x4 packed;
#ifdef GFY_DIAG_NO_EPILOGUE
  for (int q = 0; q < 4; ++q) packed[q] = __builtin_bit_cast(uint32_t, acc[8 * sp + 2 * q]);
  return __builtin_bit_cast(f16x8, packed);
#endif
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    packed[q] = cvt_pk_f16(add_half<0>(acc[8 * sp + 2 * q], bias[q]),
                           add_half<1>(acc[8 * sp + 2 * q + 1], bias[q]));
    if constexpr (kRelu) packed[q] = pk_relu(packed[q]);
  }
  return __builtin_bit_cast(f16x8, packed);
}

// ---------------------------------------------------------------------------------
// The update MLP of a tile as ONE software pipeline: V^T = relu(BN(W0 . Z^T + b0)), then
// W^T = W1 . V^T + b1.  A step is one k-step of a block pair = two MFMAs on two accumulator
// chains; in their shadow the wave issues one SLICE of an epilogue that is due: the BatchNorm
// epilogue of the previous pair of the first product (its last pair runs under the first steps
// of the second product, which do not need those channels yet), the bias epilogue of the
// second product's first pair under its second.  All LDS reads of the pipeline are asm — per
// step the two fragments the next unit needs at the same k and the constants of the next
// step's slice, then ONE counted wait — and the MFMAs are builtins, so the compiler interleaves
// the slice with them and pads their hazards.
//
//   step  0..31  first product:  pair t/8, k-step t%8            slices  8..39: BN, pair (t-8)/8
//   step 32..63  second product: pair (t-32)/16, k-step (t-32)%16   slices 48..51: round, pair 0
//   step 64..67  rounding slices of the second product's pair 1
// The last k-step of every block pair (steps 7, 15, 23, 31, 47, 63) carries two MFMAs more:
// acc += b . 1 for the pair's two blocks.  Their A operand is a fragment register quad the unit
// has spent, with b[32 block + lane % 32] (one ds_read_u16, a step ahead) at k = 0 — what else
// the quad holds are finite weights that meet zeros; their B operand is 1 at k = 0 of every
// node and zero at every other k.  fp32(acc + b . 1) is the value the slices used to compute
// with one v_fma_mix_f32 per element: 155 vector instructions per tile less, 12 MFMAs more.
// ---------------------------------------------------------------------------------
// Where a pipeline finds its operands in LDS.  Resident: [W0 | W1] (head: head.0 | head.2 over
// W0) at fixed addresses, the constant image behind the eight stages.  The windowed layout of
// gine_layer_w.inc streams the same images through two 32-KB buffers at the bottom of LDS, so
// the second matrix of a product pair is found where the first one was.
// A pipeline names a weight fragment by its 1-KB piece q of the image it streams ([W0 | W1]:
// 0..127, head.0 | head.2: 0..63); the layout says which of the pipe's two base registers and
// which 16-bit offset reach it.
struct ResidentLayout {
  static constexpr int kImage = kLdsImage;   // constant image; head biases right behind it
  static constexpr int kBase1 = kLdsW1;      // second base register: W1
  static constexpr int base_of(int q) { return q >> 6; }
  static constexpr int offset_of(int q) { return (q & 63) * 1024; }
  static constexpr int address_of(int q) { return kLdsWeights + (q >> 6) * kBase1 + offset_of(q); }
};
// What a pipeline does besides arithmetic at the start of step kT (barriers, weight DMA)
template <bool kHead>
struct ResidentHooks {
  const HeadF16& head;
  uint32_t lds0;
  int wave, lane;
  template <int kT>
  __device__ __forceinline__ void before_mlp_step() const {
    if constexpr (kHead && kT == 32) {
      lds_barrier();                                  // every wave is done with W0 ...
      issue_head_dma(head.w_image, lds0 + kLdsWeights, wave, lane);   // ... the head replaces it
    }
  }
};

struct MlpPipe {
  f32x16 acc[2][2];       // [pair parity][block of the pair]
  f16x8 fa[8], fb[8];     // fragments of the current / next unit (four k-steps x two blocks)
  f32x4 al[2], sh[2];     // constants of the current / next slice, by step parity
  u32x4 b1[2];            // the head's bias constants (its slices add them on the vector pipe)
  uint32_t frag_base[2];  // W0, W1: LDS address of this lane's 16 bytes of fragment 0
  uint32_t alpha_base, b0_base, b1_base;
  uint32_t one_at_k0;     // bias MFMAs: fp16 1.0 in the lanes that hold k = 0, else 0
  uint32_t bias_row[2];   //   ... and b[row] of the pair's two blocks, fetched one step ahead
};

struct MlpStep {   // what step t does (all compile-time)
  bool mfma;
  int product, pair, unit /* global: 0..15 */, kstep, k;
  int slice;       // 0 none, 1 BatchNorm, 2 bias
  int sl_pair, sl_index;
};
__host__ __device__ constexpr MlpStep mlp_step(int t) {
  MlpStep d{};
  d.mfma = t < 64;
  if (t < 32) {
    d.product = 0, d.pair = t / 8, d.unit = t / 4, d.kstep = t % 8, d.k = t % 4;
  } else if (t < 64) {
    d.product = 1, d.pair = (t - 32) / 16, d.unit = 8 + (t - 32) / 4, d.kstep = (t - 32) % 16,
    d.k = t % 4;
  }
  if (t >= 8 && t < 40) d.slice = 1, d.sl_pair = (t - 8) / 8, d.sl_index = (t - 8) % 8;
  else if (t >= 48 && t < 52) d.slice = 2, d.sl_pair = 0, d.sl_index = t - 48;
  else if (t >= 64 && t < 68) d.slice = 2, d.sl_pair = 1, d.sl_index = t - 64;
  return d;
}
constexpr int kMlpSteps = 68;
// 1-KB piece of [W0 | W1] that holds block 2 pair's fragment at a k-step; the pair's second
// block follows ksteps pieces later
__host__ __device__ constexpr int mlp_frag_piece(int product, int pair, int kstep) {
  return product * 64 + (2 * pair) * (product ? 16 : 8) + kstep;
}

template <class Layout, int kT, class Hooks>
__device__ __forceinline__ void mlp_pipe_step(MlpPipe& m, const f16x8 (&z)[8], f16x8 (&v)[16],
                                              f16x8 (&wrow)[8], Hooks& hooks) {
  constexpr MlpStep d = mlp_step(kT);
  constexpr MlpStep nx = mlp_step(kT + 1 < kMlpSteps ? kT + 1 : kT);
  constexpr bool kNextUnit = d.mfma && d.unit < 15;
  constexpr int kNextSlice = kT + 1 < kMlpSteps ? nx.slice : 0;
  // the last k-step of a block pair carries the pair's two bias MFMAs; their A operands are
  // fetched one step ahead and put at k = 0 of fragment registers the unit has already spent
  constexpr bool kBiasStep = d.mfma && d.kstep == (d.product ? 15 : 7);
  constexpr bool kBiasNext = kT + 1 < kMlpSteps && nx.mfma && nx.kstep == (nx.product ? 15 : 7);
  static_assert(!kBiasStep || d.k == 3, "fragments 0 and 4 of the unit are spent");
#ifdef GFY_DIAG_NO_FRAGMENT_READS
  constexpr int kReads = (kNextSlice == 1 ? 2 : 0) + (kBiasNext ? 2 : 0);
#else
  constexpr int kReads = (kNextUnit ? 2 : 0) + (kNextSlice == 1 ? 2 : 0) + (kBiasNext ? 2 : 0);
#endif
  f16x8(&cur)[8] = (d.unit & 1) ? m.fb : m.fa;
  f16x8(&nxt)[8] = (d.unit & 1) ? m.fa : m.fb;
  hooks.template before_mlp_step<kT>();
  if constexpr (kNextUnit) {                         // fragments k and 4 + k of the next unit
    constexpr MlpStep un = mlp_step(kT + 4);         // same k, one unit on
    constexpr int q = mlp_frag_piece(un.product, un.pair, un.kstep);
    constexpr int q2 = q + (un.product ? 16 : 8);
    static_assert(Layout::base_of(q) == Layout::base_of(q2), "one base register per block pair");
#ifdef GFY_DIAG_NO_FRAGMENT_READS   // diagnostic (wrong results): the weight reads of the MLP
    nxt[d.k] = cur[d.k], nxt[4 + d.k] = cur[4 + d.k];
#else
    lds_read2_b128<Layout::offset_of(q), Layout::offset_of(q2)>(nxt[d.k], nxt[4 + d.k],
                                                                m.frag_base[Layout::base_of(q)]);
#endif
  }
  if constexpr (kNextSlice == 1) {                   // constants of the slice of the next step
    constexpr int b = 2 * nx.sl_pair + nx.sl_index / 4, g = nx.sl_index % 4;
    lds_read2_b128<b * 128 + g * 16, 1024 + b * 128 + g * 16>(m.al[(kT + 1) & 1],
                                                             m.sh[(kT + 1) & 1], m.alpha_base);
  }
  if constexpr (kBiasNext) {   // b[32 block + lane % 32] -> k = 0 of the spent fragments 0 and 4
    constexpr int block = 2 * nx.pair, table = nx.product ? 512 : 0;   // b1 behind b0 (natural order)
    lds_read_u16<table + block * 64>(m.bias_row[0], m.b0_base);
    lds_read_u16<table + (block + 1) * 64>(m.bias_row[1], m.b0_base);
  }
  // everything older than this step's reads has landed: the fragments of this step (read four
  // steps ago) and the constants of this slice (read one step ago)
  lds_wait_keep<kReads>();
  if constexpr (d.mfma) landed(cur[d.k]), landed(cur[4 + d.k]);
  if constexpr (d.slice == 1) landed(m.al[kT & 1]), landed(m.sh[kT & 1]);
  if constexpr (kBiasStep) landed(m.bias_row[0]), landed(m.bias_row[1]);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (d.mfma) {
    f32x16(&a2)[2] = m.acc[d.pair & 1];
    const f32x16 zero = {0};
    f16x8 operand;
    if constexpr (d.product) operand = v[d.kstep];
    else operand = z[d.kstep];
    a2[0] = mfma(cur[d.k], operand, d.kstep == 0 ? zero : a2[0]);
    a2[1] = mfma(cur[4 + d.k], operand, d.kstep == 0 ? zero : a2[1]);
    if constexpr (kBiasStep) {
      // acc += b . 1: the A operands carry b[row] at k = 0 (whatever finite weights the spent
      // fragments still hold elsewhere meets zeros), the B operand is 1 at k = 0 of every node
      // and zero at every other k — built in the spent fragment 1
      u32x4 ones = {m.one_at_k0, opaque_zero(), opaque_zero(), opaque_zero()};
      u32x4 b_first = __builtin_bit_cast(u32x4, cur[0]), b_second = __builtin_bit_cast(u32x4, cur[4]);
      b_first[0] = m.bias_row[0], b_second[0] = m.bias_row[1];
      a2[0] = mfma(__builtin_bit_cast(f16x8, b_first), __builtin_bit_cast(f16x8, ones), a2[0]);
      a2[1] = mfma(__builtin_bit_cast(f16x8, b_second), __builtin_bit_cast(f16x8, ones), a2[1]);
    }
  }
  if constexpr (d.slice == 1) {
    constexpr int b = 2 * d.sl_pair + d.sl_index / 4, g = d.sl_index % 4;
    u32x4& dst = reinterpret_cast<u32x4&>(v[2 * b + (g >> 1)]);
    uint32_t out0, out1;
    bn_slice(m.acc[d.sl_pair & 1][d.sl_index / 4], g, m.al[kT & 1], m.sh[kT & 1], out0, out1);
    dst[2 * (g & 1)] = out0;
    dst[2 * (g & 1) + 1] = out1;
  } else if constexpr (d.slice == 2) {
    constexpr int b = 2 * d.sl_pair + d.sl_index / 2, sp = d.sl_index % 2;
    wrow[2 * b + sp] = round_slice(m.acc[d.sl_pair & 1][d.sl_index / 2], sp);
  }
  __builtin_amdgcn_sched_barrier(0);
}

template <class Layout, class Hooks, int... kT>
__device__ __forceinline__ void mlp_pipe_steps(std::integer_sequence<int, kT...>, MlpPipe& m,
                                               const f16x8 (&z)[8], f16x8 (&v)[16],
                                               f16x8 (&wrow)[8], Hooks& hooks) {
  (mlp_pipe_step<Layout, kT>(m, z, v, wrow, hooks), ...);
}

template <class Layout, class Hooks>
__device__ __forceinline__ void mlp_pipeline_on(const char* smem, uint32_t lds0, int lane, int hq,
                                                const f16x8 (&z)[8], f16x8 (&v)[16],
                                                f16x8 (&wrow)[8], Hooks& hooks) {
  MlpPipe m;
  m.frag_base[0] = lds0 + (uint32_t)kLdsWeights + (uint32_t)lane * 16u;
  m.frag_base[1] = lds0 + (uint32_t)Layout::kBase1 + (uint32_t)lane * 16u;
  m.alpha_base = lds0 + (uint32_t)(Layout::kImage + kLdsAlpha - kLdsImage) +
                 (uint32_t)hq * 64u;                               // shift: 1,024 B behind
  // b0 | b1 in natural channel order: A-operand row lane % 32 of block b is channel 32 b + row
  m.b0_base = lds0 + (uint32_t)(Layout::kImage + kLdsB0 - kLdsImage) + ((uint32_t)lane & 31u) * 2u;
  m.b1_base = 0;
  m.one_at_k0 = hq ? 0u : 0x3C00u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {   // the first unit's fragments: pieces k and 8 + k (both on base 0)
    m.fa[k] = *reinterpret_cast<const f16x8*>(smem + lane * 16 + Layout::address_of(k));
    m.fa[4 + k] = *reinterpret_cast<const f16x8*>(smem + lane * 16 + Layout::address_of(8 + k));
  }
  mlp_pipe_steps<Layout>(std::make_integer_sequence<int, kMlpSteps>{}, m, z, v, wrow, hooks);
}
template <bool kHead>
__device__ __forceinline__ void mlp_pipeline(const char* smem, uint32_t lds0, int wave, int lane,
                                             int hq, const f16x8 (&z)[8], f16x8 (&v)[16],
                                             f16x8 (&wrow)[8], const HeadF16& head) {
  const ResidentHooks<kHead> hooks{head, lds0, wave, lane};
  mlp_pipeline_on<ResidentLayout>(smem, lds0, lane, hq, z, v, wrow, hooks);
}
// ... when nobody wants v (the activations between the two products) afterwards
template <bool kHead>
__device__ __forceinline__ void mlp_pipeline(const char* smem, uint32_t lds0, int wave, int lane,
                                             int hq, const f16x8 (&z)[8], f16x8 (&wrow)[8],
                                             const HeadF16& head) {
  f16x8 v[16];
  mlp_pipeline<kHead>(smem, lds0, wave, lane, hq, z, v, wrow, head);
}

// ---------------------------------------------------------------------------------
// The head of a tile, t = relu(head.0 h' + ba), o = head.2 t + bb, as the same kind of pipeline:
//   step  0..15  head.0: pair t/8, k-step t%8        slices  8..11, 16..19: bias + ReLU -> t
//   step 16..31  head.2: pair (t-16)/8, k-step t%8   slices 24..27, 32..35: bias -> o
// (head.2's first four k-steps need only the first pair of t, so the second pair's slices run
// under them.)
// ---------------------------------------------------------------------------------
__host__ __device__ constexpr MlpStep head_step(int t) {
  MlpStep d{};
  d.mfma = t < 32;
  if (t < 16) d.product = 0, d.pair = t / 8, d.unit = t / 4, d.kstep = t % 8, d.k = t % 4;
  else if (t < 32)
    d.product = 1, d.pair = (t - 16) / 8, d.unit = 4 + (t - 16) / 4, d.kstep = t % 8, d.k = t % 4;
  if (t >= 8 && t < 12) d.slice = 1, d.sl_pair = 0, d.sl_index = t - 8;
  else if (t >= 16 && t < 20) d.slice = 1, d.sl_pair = 1, d.sl_index = t - 16;
  else if (t >= 24 && t < 28) d.slice = 2, d.sl_pair = 0, d.sl_index = t - 24;
  else if (t >= 32 && t < 36) d.slice = 2, d.sl_pair = 1, d.sl_index = t - 32;
  return d;
}
constexpr int kHeadSteps = 36;

template <class Layout, int kT>
__device__ __forceinline__ void head_pipe_step(MlpPipe& m, const f16x8 (&hn)[8], f16x8 (&tf)[8],
                                               f16x8 (&o)[8]) {
  constexpr MlpStep d = head_step(kT);
  constexpr MlpStep nx = head_step(kT + 1 < kHeadSteps ? kT + 1 : kT);
  constexpr bool kNextUnit = d.mfma && d.unit < 7;
  constexpr int kNextSlice = kT + 1 < kHeadSteps ? nx.slice : 0;
  constexpr int kReads = (kNextUnit ? 2 : 0) + (kNextSlice ? 1 : 0);
  f16x8(&cur)[8] = (d.unit & 1) ? m.fb : m.fa;
  f16x8(&nxt)[8] = (d.unit & 1) ? m.fa : m.fb;
  if constexpr (kNextUnit) {
    constexpr MlpStep un = head_step(kT + 4);
    constexpr int q = un.product * 32 + (2 * un.pair) * 8 + un.kstep, q2 = q + 8;
    static_assert(Layout::base_of(q) == Layout::base_of(q2), "one base register per block pair");
    lds_read2_b128<Layout::offset_of(q), Layout::offset_of(q2)>(nxt[d.k], nxt[4 + d.k],
                                                                m.frag_base[Layout::base_of(q)]);
  }
  if constexpr (kNextSlice == 1) {       // ba: [block][half][16], as b1
    constexpr int b = 2 * nx.sl_pair + nx.sl_index / 2, sp = nx.sl_index % 2;
    lds_read_b128<b * 64 + sp * 16>(m.b1[(kT + 1) & 1], m.b0_base);
  } else if constexpr (kNextSlice == 2) {   // bb: [half][natural 16-byte chunk 2 b + sp]
    constexpr int b = 2 * nx.sl_pair + nx.sl_index / 2, sp = nx.sl_index % 2;
    lds_read_b128<(2 * b + sp) * 16>(m.b1[(kT + 1) & 1], m.b1_base);
  }
  lds_wait_keep<kReads>();
  if constexpr (d.mfma) landed(cur[d.k]), landed(cur[4 + d.k]);
  if constexpr (d.slice != 0) landed(m.b1[kT & 1]);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (d.mfma) {
    f32x16(&a2)[2] = m.acc[d.pair & 1];
    const f32x16 zero = {0};
    f16x8 operand;
    if constexpr (d.product) operand = tf[d.kstep];
    else operand = hn[d.kstep];
    a2[0] = mfma(cur[d.k], operand, d.kstep == 0 ? zero : a2[0]);
    a2[1] = mfma(cur[4 + d.k], operand, d.kstep == 0 ? zero : a2[1]);
  }
  if constexpr (d.slice != 0) {
    constexpr int b = 2 * d.sl_pair + d.sl_index / 2, sp = d.sl_index % 2;
    const f32x16& acc = m.acc[d.sl_pair & 1][d.sl_index / 2];
    if constexpr (d.slice == 1) tf[2 * b + sp] = bias_slice<true>(acc, sp, m.b1[kT & 1]);
    else o[2 * b + sp] = bias_slice<false>(acc, sp, m.b1[kT & 1]);
  }
  __builtin_amdgcn_sched_barrier(0);
}

template <class Layout, int... kT>
__device__ __forceinline__ void head_pipe_steps(std::integer_sequence<int, kT...>, MlpPipe& m,
                                                const f16x8 (&hn)[8], f16x8 (&tf)[8],
                                                f16x8 (&o)[8]) {
  (head_pipe_step<Layout, kT>(m, hn, tf, o), ...);
}

template <class Layout = ResidentLayout>
__device__ __forceinline__ void head_pipeline(const char* smem, uint32_t lds0, int lane, int hq,
                                              const f16x8 (&hn)[8], f16x8 (&o)[8]) {
  MlpPipe m;
  m.frag_base[0] = lds0 + (uint32_t)kLdsWeights + (uint32_t)lane * 16u;   // head.0 | head.2
  m.frag_base[1] = lds0 + (uint32_t)Layout::kBase1 + (uint32_t)lane * 16u;
  m.b0_base = lds0 + (uint32_t)(Layout::kImage + kLdsHeadBa - kLdsImage) + (uint32_t)hq * 32u;
  m.b1_base = lds0 + (uint32_t)(Layout::kImage + kLdsHeadBb - kLdsImage) + (uint32_t)hq * 128u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    m.fa[k] = *reinterpret_cast<const f16x8*>(smem + lane * 16 + Layout::address_of(k));
    m.fa[4 + k] = *reinterpret_cast<const f16x8*>(smem + lane * 16 + Layout::address_of(8 + k));
  }
  f16x8 tf[8];
  head_pipe_steps<Layout>(std::make_integer_sequence<int, kHeadSteps>{}, m, hn, tf, o);
}

// LayerNorm + residual (_model.py:69-71); gamma / beta in MFMA result order at `gamma`, `beta`
// (LDS).  Moments in fp32 over the 128 fp16 values of a row:
//   sum       on the matrix cores: ones (32 x 16) . w^T accumulated over the eight k-steps puts
//             the row's sum into every result register of the row's lanes (products by 1.0
//             are exact) — 8 MFMAs instead of 64 dependent adds and one half-swap;
//   squares   one v_fma_mix_f32 per value (the product of two halves is exact in fp32), under
//             those MFMAs; var = E[w^2] - mean^2.
// E[w^2] - mean^2 loses log2(1 + mean^2 / var) bits of the variance; LayerNorm inputs here have
// mean^2 / var <= 0.04 (oracle, rouskin and synthetic shards: tests/test_oracle_golden.py keeps
// the bound), so nothing is lost — but a wave that sees a row with mean^2 > 15 var (weights this
// model does not have: at most 4 of the variance's 24 bits may cancel before the fallback)
// recomputes its variances from the centred values, as before.
struct RowMoments {   // of a lane's node row: y = fma(w, rstd, offset) before gamma / beta
  float rstd, offset;
};
__device__ __forceinline__ RowMoments layer_norm_moments(const f16x8 (&wrow)[8]) {
  f32x16 sums = {0};
  {
    const f16 one = (f16)opaque_one();
    const f16x8 ones = {one, one, one, one, one, one, one, one};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) sums = mfma(ones, wrow[ks], sums);
  }
  float sq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    const u32x4 w4 = __builtin_bit_cast(u32x4, wrow[ks]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sq[q] = fma_hh_acc<0>(w4[q], sq[q]);
      sq[q] = fma_hh_acc<1>(w4[q], sq[q]);
    }
  }
  const float mean = sums[0] * (1.0f / kHidden);
  const float mean_square = add_other_half((sq[0] + sq[1]) + (sq[2] + sq[3])) * (1.0f / kHidden);
  float var = __builtin_fmaf(-mean, mean, mean_square);
  // cancellation guard: beyond mean^2 = 15 var (4 of var's 24 bits gone) the variances are
  // recomputed from centred values; never with this model's weights (mean^2 / var <= 0.04)
  if (__ballot(!(var * 16.0f > mean_square)) != 0) {   // wave-uniform
    const float neg_mean = -mean;
    float centred[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const u32x4 w4 = __builtin_bit_cast(u32x4, wrow[ks]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float d0 = add_half<0>(neg_mean, w4[q]), d1 = add_half<1>(neg_mean, w4[q]);
        centred[q] = __builtin_fmaf(d0, d0, centred[q]);
        centred[q] = __builtin_fmaf(d1, d1, centred[q]);
      }
    }
    var = add_other_half((centred[0] + centred[1]) + (centred[2] + centred[3])) * (1.0f / kHidden);
  }
  const float rstd = fast_rsqrt(var + 1e-5f);
  return RowMoments{rstd, -rstd * mean};
}
// y[ks] = R(fma(fma(w, rstd, offset), gamma, beta)), + the residual row where kResidual
template <bool kResidual>
__device__ __forceinline__ void layer_norm_affine(const f16x8 (&wrow)[8], const RowMoments& m,
                                                  const f16x8 (&h)[8], f16x8 (&hn)[8],
                                                  const char* gamma, const char* beta, int hq) {
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    const u32x4 w4 = __builtin_bit_cast(u32x4, wrow[ks]);
    const int at = ((ks >> 1) * 2 + hq) * 32 + (ks & 1) * 16;
    const u32x4 gm = *reinterpret_cast<const u32x4*>(gamma + at);
    const u32x4 bt = *reinterpret_cast<const u32x4*>(beta + at);
    u32x4 y;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float t0 = fma_half<0>(w4[q], m.rstd, m.offset), t1 = fma_half<1>(w4[q], m.rstd, m.offset);
      y[q] = cvt_pk_f16(fma_f32_hh<0>(t0, gm[q], bt[q]), fma_f32_hh<1>(t1, gm[q], bt[q]));
    }
    const f16x8 y8 = __builtin_bit_cast(f16x8, y);
    hn[ks] = kResidual ? (h[ks] + y8) : y8;
  }
}
template <bool kResidual>
__device__ __forceinline__ void layer_norm_residual(const f16x8 (&wrow)[8], const f16x8 (&h)[8],
                                                    f16x8 (&hn)[8], const char* gamma,
                                                    const char* beta, int hq) {
  const RowMoments m = layer_norm_moments(wrow);
  layer_norm_affine<kResidual>(wrow, m, h, hn, gamma, beta, hq);
}

// ---------------------------------------------------------------------------------
// What every layer kernel (this file, gine_layer_q.inc, _w.inc, _x.inc) and k_head_d do around
// the pipelines, once.  A kernel whose loop re-derives its lane pieces per phase (opaque,
// gine_layer_q.inc) hands (r, hq) of that phase in: nothing here looks at threadIdx.
// Each of these compiles to the instructions of the code it replaced.  Two blocks that every
// kernel still carries do not when they are wrapped — the gather dispatch (gather_tile<3..8> |
// gather_direct | zeros) and the bracketed normalise behind head_row_square_sum — and stay
// where they are, as do the three call sites that say so (profiles/layer_shared_refactor.txt).
// ---------------------------------------------------------------------------------
// Raise the wave to s_setprio level 1..3 (the builtin takes an immediate); level 0 leaves the
// priority as it is — going back to 0 is the caller's own s_setprio(0)
__device__ __forceinline__ void raise_wave_priority(int level) {
  if (level == 1) __builtin_amdgcn_s_setprio(1);
  else if (level == 2) __builtin_amdgcn_s_setprio(2);
  else if (level == 3) __builtin_amdgcn_s_setprio(3);
}

// the eight slot words (stage row | type << 8) of row r of a tile plan
__device__ __forceinline__ void load_plan_words(const char* plan, int r, uint32_t (&word)[8]) {
  const u32x4 wa = reinterpret_cast<const u32x4*>(plan + kPlanWords + r * 32)[0];
  const u32x4 wb = reinterpret_cast<const u32x4*>(plan + kPlanWords + r * 32)[1];
  word[0] = wa[0], word[1] = wa[1], word[2] = wa[2], word[3] = wa[3];
  word[4] = wb[0], word[5] = wb[1], word[6] = wb[2], word[7] = wb[3];
}

// kSteps k-steps of lane (., hq) -> row `row` of a tensor in stored order: 16-byte chunk
// 2 ks + hq of the row (hidden rows, z, w, y, the embeddings: eight, 256 B; v: sixteen, 512 B)
template <int kSteps>
__device__ __forceinline__ void store_row(void* base, size_t row, int hq,
                                          const f16x8 (&regs)[kSteps]) {
  char* rowp = reinterpret_cast<char*>(base) + (row * (32 * kSteps) + hq * 16);
#pragma unroll
  for (int ks = 0; ks < kSteps; ++ks) *reinterpret_cast<f16x8*>(rowp + 32 * ks) = regs[ks];
}

// kTap (parity tests only, gfy_debug_layer): the instantiation of a persistent kernel that also
// writes one of the layer's phase tensors, rows in stored order — tap 1: z (after the gather),
// 2: v (after BatchNorm + ReLU, 256 channels), 3: w (second product + bias), 4: y (LayerNorm,
// before the residual; stored by the kernel, which knows how it normalises).  The production
// instantiation (kTap = false) has none of this code.
enum { kTapNone = 0, kTapZ = 1, kTapV = 2, kTapW = 3, kTapY = 4 };
__device__ __forceinline__ void store_taps_zvw(int tap, f16* tap_out, bool active, int row, int hq,
                                               const f16x8 (&z)[8], const f16x8 (&v)[16],
                                               const f16x8 (&wrow)[8]) {
  if (active && tap == kTapZ) store_row(tap_out, (size_t)row, hq, z);
  if (active && tap == kTapV) store_row(tap_out, (size_t)row, hq, v);
  if (active && tap == kTapW) store_row(tap_out, (size_t)row, hq, wrow);
}

// Where row r of a tile goes in the head's output: its shard's block and the row there (the
// caller's out_rows compaction, else the shard-local row); dest = -1: no store — a wave without
// a tile, padding behind the shard's last node (for which out_rows has no entry and is not
// read), or a row out_rows itself leaves out
struct HeadRowDest {
  char* out;
  int dest;
};
__device__ __forceinline__ HeadRowDest head_row_dest(const ShardTable& shards, int tile, int r,
                                                     bool active) {
  HeadRowDest d{nullptr, -1};
  if (active) {
    const int shard = shards.shard_of_tile(tile);
    const int local = tile * kLTile + r - shards.tile_base[shard] * kLTile;
    if (local < shards.nodes[shard]) {
      const int32_t* rows = shards.out_rows[shard];
      d.dest = rows ? rows[local] : local;
      d.out = reinterpret_cast<char*>(shards.out[shard]);
    }
  }
  return d;
}

// The cross-lane half of the head's tail (api.py:250-259): sum of squares of a row of o in float64 
// (each square is exact in fp32: 22 significant bits, one v_fma_mix_f32 from the packed pair).  The order of the additions is part of the result,
// and ALL 64 lanes execute the exchange of the two half-waves: call outside any per-lane guard.
__device__ __forceinline__ double head_row_square_sum(const f16x8 (&o)[8]) {
  double ss[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    const u32x4 w4 = __builtin_bit_cast(u32x4, o[ks]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      ss[q] += (double)square_half<0>(w4[q]);
      ss[q] += (double)square_half<1>(w4[q]);
    }
  }
  return add_other_half((ss[0] + ss[1]) + (ss[2] + ss[3]));
}

// kHead: the launch also runs head + float64 normalise on the tile's new hidden state
// (fp16 output), straight from the registers; h_out is then not written at all.
template <bool kResidual, bool kHead>
__global__ __launch_bounds__(kLThreads) void k_gine_layer_f16(
    const LayerF16 p, const f16* __restrict__ h_in, f16* __restrict__ h_out,
    const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const uint8_t* __restrict__ typ, const char* __restrict__ plans,
    int n /* rows with a row_ptr entry and a hidden row: the padded rows, or the caller's n */,
    int num_tiles, const HeadF16 head, const ShardTable shards /* kHead: where the rows go */,
    int normalise, int32_t* __restrict__ spent_tile_sums /* gfy_encode_coo, first layer */,
    unsigned long long* __restrict__ span /* timing mode 3: device clock at start / end */) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const char* const tbytes = smem + kLdsTable;

  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int r = lane & 31, hq = lane >> 5;
  // XCD (blockIdx & 7) owns a contiguous range of tiles: a partner row is then usually an
  // own row of a workgroup of the same XCD and is served by that XCD's L2 the second time
  const int tiles_per_xcd = (int)(gridDim.x >> 3) * kLWaves;
  const int tile = (int)(blockIdx.x & 7) * tiles_per_xcd + (int)(blockIdx.x >> 3) * kLWaves + wave;
  const bool active = tile < num_tiles;                       // wave-uniform
  const int node = tile * kLTile + r;
  const bool node_ok = active && node < n;
  const char* const plan = plans + (size_t)(active ? tile : 0) * kPlanBytes;
  // the per-tile edge counts of the scan-free CSR build have been consumed by the setup
  // launch: zero again for the next call on this workspace (csr_finish.inc)
  if (spent_tile_sums && active && lane == 0) spent_tile_sums[tile] = 0;
  if (span && t == 0) atomicMin(&span[0], (unsigned long long)__builtin_amdgcn_s_memrealtime());
  const char* const stage = smem + wave * kLdsStageBytes;
  const uint32_t lds_stage = lds0 + (uint32_t)wave * kLdsStageBytes;
  const uint32_t sub = (uint32_t)lane >> 4, p16 = (uint32_t)lane & 15u;

#ifdef GFY_STAMPS
#define STAMP_L(slot)                                                                      \
  do {                                                                                     \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();                          \
    if (t == kStampThread && blockIdx.x < 256) g_stamps[blockIdx.x][slot] += now_ - last_stamp; \
    last_stamp = now_;                                                                     \
  } while (0)
#ifndef GFY_STAMP_WAVE
#define GFY_STAMP_WAVE 0   // which wave of every workgroup reports (-DGFY_STAMP_WAVE=7: the last)
#endif
  constexpr int kStampThread = 64 * GFY_STAMP_WAVE;
  unsigned long long last_stamp = __builtin_amdgcn_s_memtime();
  const unsigned long long first_stamp = last_stamp;
  if (t == 0 && blockIdx.x < 512) g_real[blockIdx.x][0] = __builtin_amdgcn_s_memrealtime();
#else
#define STAMP_L(slot)
#endif
  // ---- hop 1: the part of the plan hop 2 needs (header, far list) FIRST, then the own rows
  //      -> stage rows 0..31.  vmcnt retires in order: with the four plan reads in front of the
  //      eight row DMAs, `vmcnt(8)` hands over the far list while the rows are still arriving
  //      and hop 2 goes out under hop 1's tail (asm reads: the compiler would count only its
  //      own loads and wait for the DMAs too) ---------------------------------------------------
  u32x4 header, far4[3];
  {
    const char* far_at = plan + kPlanFar + (lane >> 4) * 48;
    asm volatile("global_load_dwordx4 %0, %4, off\n\t"
                 "global_load_dwordx4 %1, %5, off\n\t"
                 "global_load_dwordx4 %2, %5, off offset:16\n\t"
                 "global_load_dwordx4 %3, %5, off offset:32"
                 : "=&v"(header), "=&v"(far4[0]), "=&v"(far4[1]), "=&v"(far4[2])
                 : "v"(plan), "v"(far_at)
                 : "memory");
  }
  if (active) {
#pragma unroll
    for (int g = 0; g < kLTile / 4; ++g) {
      const uint32_t q = 4u * g + sub;
      int own = tile * kLTile + (int)q;
      own = own < n ? own : n - 1;
      dma16(h_in, (uint32_t)own * 256u + ((p16 ^ (q & 15u)) << 4), lds_stage + (uint32_t)g * 1024u);
    }
  }
  if (active) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  landed(header), landed(far4[0]), landed(far4[1]), landed(far4[2]);
  const int count = __builtin_amdgcn_readfirstlane((int)header[0]);
  const int deepest = __builtin_amdgcn_readfirstlane((int)header[1]);
  const bool staged = count <= kLFar;
  STAMP_L(0);

  // ---- hop 2: far rows -> stage rows 32.. -------------------------------------------------
  if (active && staged) {
    const uint32_t fars[12] = {far4[0][0], far4[0][1], far4[0][2], far4[0][3],
                               far4[1][0], far4[1][1], far4[1][2], far4[1][3],
                               far4[2][0], far4[2][1], far4[2][2], far4[2][3]};
#pragma unroll
    for (int g = 0; g < kLFar / 4; ++g) {
      if (4 * g < count) {
        const uint32_t q = (uint32_t)kLTile + 4u * g + sub;
        dma16(h_in, fars[g] * 256u + ((p16 ^ (q & 15u)) << 4),
              lds_stage + (uint32_t)(kLTile / 4 + g) * 1024u);
      }
    }
  }
  // the rest of the plan (slot words) and the per-launch constants ride behind both hops
  uint32_t word[8];
  load_plan_words(plan, r, word);
  u32x4 image_chunk;
  if (t < 480) image_chunk = reinterpret_cast<const u32x4*>(p.image)[t];
  else image_chunk = reinterpret_cast<const u32x4*>(head.image)[t - 480];
  HeadRowDest to{nullptr, -1};   // kHead: where the output row of this lane's node goes
  if constexpr (kHead) to = head_row_dest(shards, tile, r, active);
  reinterpret_cast<u32x4*>(smem + kLdsImage)[t] = image_chunk;
  dma_wait_all();                                   // this wave's stage is complete
  STAMP_L(1);
  lds_barrier();                                    // #1: table and constants visible
  STAMP_L(2);

  // ---- own rows -> registers (z, residual), gather-sum -> z -------------------------------
  const f16 scale16 = (f16)p.scale;
  f16x8 h[8], z[8];
  {
    const uint32_t own = (uint32_t)r * 256u, x16 = (((uint32_t)r & 15u) ^ (uint32_t)hq) * 16u;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
      h[ks] = *reinterpret_cast<const f16x8*>(stage + own + (x16 ^ (32u * ks)));
  }
  if (active) {
    if (staged) {
      if (deepest <= 3) gather_tile<3>(h, z, word, tbytes, stage, r, hq, scale16);
      else if (deepest == 4) gather_tile<4>(h, z, word, tbytes, stage, r, hq, scale16);
      else if (deepest == 5) gather_tile<5>(h, z, word, tbytes, stage, r, hq, scale16);
      else if (deepest == 6) gather_tile<6>(h, z, word, tbytes, stage, r, hq, scale16);
      else gather_tile<8>(h, z, word, tbytes, stage, r, hq, scale16);
    } else {
      gather_direct(h, z, reinterpret_cast<const char*>(h_in), row_ptr, col, typ, tbytes, node,
                    node_ok, n, hq, scale16, p.edge_types);
    }
  } else {
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) h[ks] = zero8(), z[ks] = zero8();
  }
  STAMP_L(3);
  // This wave's stage is spent: the slice of [W0 | W1] that lives there comes in.  Both
  // matrices are resident behind ONE barrier; the products then run without another one.
  // (Measured alternatives: W0 first and W1 behind a second barrier under the first product —
  // the second barrier costs the skew of the first product, 2.0 k cycles, for 1.5 k saved
  // here; W0 slice by slice behind the block pairs of the first product — three more barriers,
  // 36.6 k cycles per wave instead of 33.6 k.)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  issue_weight_slice_dma(p.w01_image, lds0 + kLdsWeights, wave, lane, 0, kLdsStageBytes / 1024);
  dma_wait_all();
  lds_barrier();                                    // #2: W0 and W1 resident, every stage spent
  STAMP_L(4);

  // ---- update MLP: V^T = relu(BN(W0 . Z^T + b0)), W^T = W1 . V^T + b1 -> w, laid out as h;
  //      with the head, barrier #3 + its image over W0 between the two products ------------
  f16x8 wrow[8];
  mlp_pipeline<kHead>(smem, lds0, wave, lane, hq, z, wrow, head);
  STAMP_L(5);

  // ---- LayerNorm + residual ------------------------------------------------------------
  f16x8 hn[8];
  layer_norm_residual<kResidual>(wrow, h, hn, smem + kLdsGamma, smem + kLdsBeta, hq);
  if constexpr (!kHead) {
    if (node_ok) {   // (not store_row: this site adds row and chunk to the base one after the other)
      char* rowp = reinterpret_cast<char*>(h_out) + (size_t)node * 256 + hq * 16;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) *reinterpret_cast<f16x8*>(rowp + 32 * ks) = hn[ks];
    }
    STAMP_L(8);
#ifdef GFY_STAMPS
    if (t == kStampThread && blockIdx.x < 256) {
      g_stamps[blockIdx.x][10] += last_stamp - first_stamp;
      g_stamps[blockIdx.x][11] += 1;
    }
    if (t == 0 && blockIdx.x < 512) g_real[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();
#endif
    if (span) {   // after every wave's stores have been issued
      __syncthreads();
      if (t == 0) atomicMax(&span[1], (unsigned long long)__builtin_amdgcn_s_memrealtime());
    }
    return;
  } else {
    STAMP_L(8);
    // ---- head (_model.py:61-63,72) + float64 normalise (api.py:250-259) ------------------
    dma_wait_all();
    lds_barrier();                                  // #4: head.0 | head.2 resident over W0
    // head.2's rows are dealt so that o comes out as natural 16-byte chunks of the output row
    f16x8 o[8];
    STAMP_L(6);
    head_pipeline(smem, lds0, lane, hq, hn, o);
    STAMP_L(7);
    const double total = head_row_square_sum(o);
    if (to.dest >= 0) {
      char* rowp = to.out + (size_t)to.dest * (kOutDim * 2) + hq * 16;
      if (normalise) {
        const double nrm = __builtin_sqrt(total);
        const double inv = 1.0 / (nrm > 1e-12 ? nrm : 1e-12);
        // fp16(o * inv) rounded ONCE from the float64 product (numpy's astype): the fp32
        // products with inv (1 + 2^-22) and inv (1 - 2^-22) bracket the float64 product
        // strictly (three fp32 roundings of 2^-24 each), and rounding is monotone — where both
        // give the same fp16 that is the answer (4 instructions per value); where they differ
        // (a tie or fp16's subnormal grid in between, 0.07 % of the values) the lane redoes its
        // eight values in float64.
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
    STAMP_L(9);
#ifdef GFY_STAMPS
    if (t == kStampThread && blockIdx.x < 256) {
      g_stamps[blockIdx.x][12] += last_stamp - first_stamp;
      g_stamps[blockIdx.x][13] += 1;
    }
    if (t == 0 && blockIdx.x < 512) g_real[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();
#endif
    if (span) {
      __syncthreads();
      if (t == 0) atomicMax(&span[1], (unsigned long long)__builtin_amdgcn_s_memrealtime());
    }
  }
#undef STAMP_L
}
