// Windowed (sliced) RNA records -> model-ready graph arrays, on the device.
//
// Replaces GraphBuilder._slice_graph (src/ginfinity/graph.py:608-695) on top of _build_full:
// the reference builds a window's WHOLE molecule and cuts the window out of it; here nothing
// of the whole graph is ever written.  A record is at most 4,096 nt (MAXIMUM_LENGTH_NT,
// _validation.py), so the set of chosen positions is a 4,096-bit map: ONE 64-bit word per
// lane of a wave.  The whole graph's neighbourhood is closed-form (i±1, the pair partner,
// i±2 where the spec has skip-2 edges), so selection, the context hops, node ranks and every
// edge rank are shifts, ballots and popcounts over that map: no sort, no hash, no global
// atomic except the first_invalid word.  Integer / one-hot work: the arrays are bit-identical
// to the reference's, including the order of the edges (graph_build.hip header) — the whole
// molecule's edges with both ends chosen, in the whole molecule's order, renumbered.
//
// Three kernels, every wave independent (no workgroup barrier):
//   k_window_pairs   one wave per DISTINCT molecule: bracket matching as in k_build_graphs
//                    (a ')' at level l pairs with the most recent '(' of level l), writing
//                    partner[i] (-1 = unpaired) and a per-molecule "unusable" flag.  Windows
//                    of one transcript share its pair table.
//   k_window_select  one wave per record: the chosen map (core window, crossing-pair
//                    partners, context hops until the frontier is empty), the map of kept
//                    pair-opening positions, and the record's node and edge count.
//   k_window_emit    one wave per record of a micro-batch: node_features, edge_index,
//                    edge_types, residue_index, node_roles and out_rows from the maps.
// The host reads the counts between select and emit: it lays out node_ptr / edge_ptr and the
// micro-batches from them.
#include "gfy_common.h"

namespace gfy {
namespace {

constexpr int kMaxNt = 4096;        // MAXIMUM_LENGTH_NT: 64 lanes x 64 bits
constexpr int kLevels = 2049;       // nesting levels carried per wave (depth <= 2048)
constexpr int kWaves = 4;
typedef unsigned long long u64;

struct Molecules {
  const uint8_t* bases;
  const uint8_t* marks;
  const int64_t* mol_ptr;
  int molecules;
  int64_t molecule_nt;
};

struct WindowScratch {              // carved from the caller's workspace
  int32_t* partner;                 // [molecule_nt]
  int32_t* mol_bad;                 // [molecules]
  u64* maps;                        // [records][2][64]: chosen, kept pair-opening positions
};

__host__ __device__ inline size_t pad256(size_t v) { return (v + 255) / 256 * 256; }

inline size_t window_scratch_bytes(int64_t molecules, int64_t molecule_nt, int64_t records) {
  return pad256((size_t)molecule_nt * 4) + pad256((size_t)molecules * 4)
       + pad256((size_t)records * 128 * 8);
}

inline WindowScratch carve(void* ws, int64_t molecules, int64_t molecule_nt) {
  char* at = (char*)ws;
  WindowScratch w;
  w.partner = (int32_t*)at;  at += pad256((size_t)molecule_nt * 4);
  w.mol_bad = (int32_t*)at;  at += pad256((size_t)molecules * 4);
  w.maps = (u64*)at;
  return w;
}

// ---- the 4,096-bit map: lane l owns positions 64 l .. 64 l + 63 ---------------------------
__device__ __forceinline__ u64 range_word(int lane, int lo, int hi) {
  const int a = lo - 64 * lane > 0 ? lo - 64 * lane : 0;
  const int b = hi - 64 * lane < 64 ? hi - 64 * lane : 64;
  if (b <= a) return 0ull;
  const u64 upper = b == 64 ? ~0ull : (1ull << b) - 1ull;
  return upper & ~((1ull << a) - 1ull);
}
__device__ __forceinline__ u64 lane_below(u64 x, int lane) {     // word of lane - 1, 0 for lane 0
  const u64 v = __shfl_up(x, 1, 64);
  return lane == 0 ? 0ull : v;
}
__device__ __forceinline__ u64 lane_above(u64 x, int lane) {     // word of lane + 1, 0 for lane 63
  const u64 v = __shfl_down(x, 1, 64);
  return lane == 63 ? 0ull : v;
}
// bit i of the result = bit i - d of x (d = 1, 2)
__device__ __forceinline__ u64 towards_3prime(u64 x, int lane, int d) {
  return (x << d) | (lane_below(x, lane) >> (64 - d));
}
// bit i of the result = bit i + d of x
__device__ __forceinline__ u64 towards_5prime(u64 x, int lane, int d) {
  return (x >> d) | (lane_above(x, lane) << (64 - d));
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ int exclusive_scan(int v, int lane) {
  int sum = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int other = __shfl_up(sum, d, 64);
    if (lane >= d) sum += other;
  }
  return sum - v;
}
// LDS written by one lane and read by another of the SAME wave: DS operations of a wave are
// performed in issue order; this keeps the compiler from moving them across the hand-over.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the molecule of a record, range-checked: false = unusable
__device__ __forceinline__ bool molecule_of(const Molecules& t, int m, int64_t* base, int* length) {
  if (m < 0 || m >= t.molecules) return false;
  const int64_t first = t.mol_ptr[0], b = t.mol_ptr[m] - first;
  const int64_t l = t.mol_ptr[m + 1] - t.mol_ptr[m];
  if (l < 1 || l > kMaxNt || b < 0 || b + l > t.molecule_nt) return false;
  *base = b;
  *length = (int)l;
  return true;
}

// ---- pair table, one wave per distinct molecule ---------------------------------------------
// partner[] is -1 everywhere when the kernel starts (memset); only paired positions are written.
__global__ __launch_bounds__(64 * kWaves) void k_window_pairs(Molecules t, WindowScratch w) {
  __shared__ int lds_open[kWaves][kLevels];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x * kWaves + wave;
  if (m >= t.molecules) return;
  int* stack = lds_open[wave];            // most recent '(' of every level
  int64_t base = 0;
  int length = 0;
  if (!molecule_of(t, m, &base, &length)) {          // wave-uniform
    if (lane == 0) w.mol_bad[m] = 1;
    return;
  }
  bool bad = false;
  int depth = 0;
  for (int c = 0; c < length; c += 64) {
    const int p = c + lane;
    const bool in = p < length;
    const uint32_t mark = in ? t.marks[base + p] : (uint32_t)'.';
    const uint32_t letter = in ? t.bases[base + p] : (uint32_t)'A';
    if (!(letter == 'A' || letter == 'C' || letter == 'G' || letter == 'U')) bad = true;
    if (!(mark == '(' || mark == ')' || mark == '.')) bad = true;
    const bool open = mark == '(', close = mark == ')';
    const u64 opened = __ballot(open), closed = __ballot(close);
    const u64 below = (1ull << lane) - 1ull, upto = below | (1ull << lane);
    const int level = depth + __popcll(opened & upto) - __popcll(closed & upto) + (close ? 1 : 0);
    // lanes of this step whose '(' has my level (see k_build_graphs)
    u64 same = 0;
    for (u64 rest = opened; rest; rest &= rest - 1ull) {
      const int i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(rest));
      const int level_i = __builtin_amdgcn_readlane(level, i);
      same |= level_i == level ? (1ull << i) : 0ull;
    }
    const u64 lower = same & below;
    const int mate = (close && lower) ? 63 - __builtin_clzll(lower) : -1;
    const bool superseded = open && (same & ~upto) != 0;
    wave_sync();
    int partner = -1;
    if (close) {
      if (level < 1 || level >= kLevels) bad = true;
      else partner = mate >= 0 ? c + mate : stack[level];
    }
    wave_sync();                          // carried entries are read above, replaced below
    if (open && !superseded && level < kLevels) stack[level] = p;
    wave_sync();
    if (close && !bad) {
      if (partner < 0 || partner >= p) {  // (an unbalanced text can leave a stale entry)
        bad = true;
      } else {
        w.partner[base + p] = partner;
        w.partner[base + partner] = p;
      }
    }
    depth += __popcll(opened) - __popcll(closed);
    if (depth < 0) bad = true;
  }
  if (depth != 0) bad = true;
  const bool any_bad = __any(bad);
  if (lane == 0) w.mol_bad[m] = any_bad ? 1 : 0;
}

// ---- per-wave LDS of select / emit ----------------------------------------------------------
struct WaveLds {
  int16_t partner[kMaxNt];   // the molecule's pair table (-1 = unpaired)
  uint32_t hit[128];         // scatter target: partners of a set of positions
  uint32_t chosen[128];      // the chosen map, addressable by position
};

// partners of the positions in x (one word per lane), as a map; unpaired ones give nothing
__device__ __forceinline__ u64 partners_of(WaveLds& lds, u64 x, int words, int lane) {
  lds.hit[2 * lane] = 0u;
  lds.hit[2 * lane + 1] = 0u;
  wave_sync();
  for (int k = 0; k < words; ++k) {
    const u64 word = __shfl(x, k, 64);                 // wave-uniform
    if (word == 0ull) continue;
    if ((word >> lane) & 1ull) {
      const int q = lds.partner[64 * k + lane];
      if (q >= 0) atomicOr(&lds.hit[q >> 5], 1u << (q & 31));
    }
  }
  wave_sync();
  return (u64)lds.hit[2 * lane] | ((u64)lds.hit[2 * lane + 1] << 32);
}

struct Windows {
  const int32_t* mol;      // [records] molecule of the record
  const int32_t* start;    // [records] window [start, end) in the molecule
  const int32_t* end;
};

__global__ __launch_bounds__(64 * kWaves) void k_window_select(
    Molecules t, Windows rec, int records, int keep, int hops, int skip2, WindowScratch w,
    int32_t* __restrict__ counts, uint32_t* first_invalid) {
  __shared__ WaveLds lds_all[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * kWaves + wave;
  if (r >= records) return;
  WaveLds& lds = lds_all[wave];
  u64* maps = w.maps + (size_t)r * 128;

  const int m = rec.mol[r], start = rec.start[r], end = rec.end[r];
  int64_t base = 0;
  int length = 0;
  bool usable = molecule_of(t, m, &base, &length);
  if (usable) usable = w.mol_bad[m] == 0 && start >= 0 && start < end && end <= length;
  if (!usable) {                                         // wave-uniform
    maps[lane] = 0ull;
    maps[64 + lane] = 0ull;
    if (lane == 0) {
      counts[2 * r] = 0;
      counts[2 * r + 1] = 0;
      atomicMin(first_invalid, (uint32_t)r);
    }
    return;
  }
  const int words = (length + 63) >> 6;
  for (int k = 0; k < words; ++k) {
    const int p = 64 * k + lane;
    int q = p < length ? w.partner[base + p] : -1;
    if (q < -1 || q >= length) q = -1;
    lds.partner[p] = (int16_t)q;
  }
  wave_sync();

  const u64 valid = range_word(lane, 0, length);
  u64 chosen = range_word(lane, start, end);
  if (keep) {
    // hop 1 = the partners of the core; further hops follow every edge of the whole graph
    u64 frontier = partners_of(lds, chosen, words, lane) & valid & ~chosen;
    chosen |= frontier;
    for (int hop = 1; hop < hops && __any(frontier != 0ull); ++hop) {
      u64 reached = towards_3prime(frontier, lane, 1) | towards_5prime(frontier, lane, 1)
                  | partners_of(lds, frontier, words, lane);
      if (skip2)
        reached |= towards_3prime(frontier, lane, 2) | towards_5prime(frontier, lane, 2);
      frontier = reached & valid & ~chosen;
      chosen |= frontier;
    }
  }

  // kept edges: both ends chosen.  backbone i -> i + 1, skip-2 i -> i + 2, pairs by their '('
  const u64 backbone = chosen & towards_5prime(chosen, lane, 1);
  const u64 skips = skip2 ? chosen & towards_5prime(chosen, lane, 2) : 0ull;
  lds.chosen[2 * lane] = (uint32_t)chosen;
  lds.chosen[2 * lane + 1] = (uint32_t)(chosen >> 32);
  wave_sync();
  u64 pair_opens = 0ull;
  for (int k = 0; k < words; ++k) {
    const u64 word = __shfl(chosen, k, 64);              // wave-uniform
    if (word == 0ull) continue;
    const int p = 64 * k + lane;
    bool kept = false;
    if ((word >> lane) & 1ull) {
      const int q = lds.partner[p];
      kept = q > p && ((lds.chosen[q >> 5] >> (q & 31)) & 1u);
    }
    const u64 mine = __ballot(kept);
    if (lane == k) pair_opens = mine;
  }
  const int nodes = wave_sum(__popcll(chosen));
  const int edges = 2 * wave_sum(__popcll(backbone) + __popcll(skips) + __popcll(pair_opens));
  maps[lane] = chosen;
  maps[64 + lane] = pair_opens;
  if (lane == 0) {
    counts[2 * r] = nodes;
    counts[2 * r + 1] = edges;
  }
}

struct EmitOut {
  float* features;         // [nodes][dim]
  int32_t* src;            // [edges]
  int32_t* dst;            // [edges]
  uint8_t* types;          // [edges]
  int32_t* residue;        // [nodes]
  uint8_t* roles;          // [nodes]
  int32_t* out_rows;       // [nodes] or NULL
};

__global__ __launch_bounds__(64 * kWaves) void k_window_emit(
    Molecules t, Windows rec, int first_record, int records, WindowScratch w,
    const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ edge_ptr,
    const int64_t* __restrict__ core_ptr, int64_t n_nodes, int64_t n_edges, int64_t n_core,
    int struct_states, int positional_cols, int skip2, const float* __restrict__ positional,
    EmitOut out, uint32_t* first_invalid) {
  __shared__ u64 lds_chosen[kWaves][64];
  __shared__ int lds_before[kWaves][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * kWaves + wave;              // record of the micro-batch
  if (i >= records) return;
  const int r = first_record + i;
  const u64* maps = w.maps + (size_t)r * 128;

  const int m = rec.mol[r], start = rec.start[r], end = rec.end[r];
  int64_t base = 0;
  int length = 0;
  bool usable = molecule_of(t, m, &base, &length);
  if (usable) usable = w.mol_bad[m] == 0 && start >= 0 && start < end && end <= length;
  const u64 valid = usable ? range_word(lane, 0, length) : 0ull;
  const u64 chosen = maps[lane] & valid;
  const u64 pair_opens = maps[64 + lane] & chosen;
  const u64 backbone = chosen & towards_5prime(chosen, lane, 1);
  const u64 skips = skip2 ? chosen & towards_5prime(chosen, lane, 2) : 0ull;
  const int before = exclusive_scan(__popcll(chosen), lane);
  const int before_backbone = exclusive_scan(__popcll(backbone), lane);
  const int before_pairs = exclusive_scan(__popcll(pair_opens), lane);
  const int before_skips = exclusive_scan(__popcll(skips), lane);
  const int nodes = wave_sum(__popcll(chosen));
  const int n_backbone = wave_sum(__popcll(backbone));
  const int n_pairs = wave_sum(__popcll(pair_opens));
  const int n_skips = wave_sum(__popcll(skips));

  // the caller's layout must be the one the counts gave: nothing is written outside it
  const int64_t node_base = node_ptr[i] - node_ptr[0], edge_base = edge_ptr[i] - edge_ptr[0];
  if (usable)
    usable = node_ptr[i + 1] - node_ptr[i] == nodes
          && edge_ptr[i + 1] - edge_ptr[i] == 2 * (int64_t)(n_backbone + n_pairs + n_skips)
          && node_base >= 0 && node_base + nodes <= n_nodes
          && edge_base >= 0 && edge_base + 2 * (int64_t)(n_backbone + n_pairs + n_skips) <= n_edges;
  int64_t core_base = 0;
  if (usable && out.out_rows) {
    core_base = core_ptr[i] - core_ptr[0];
    usable = core_ptr[i + 1] - core_ptr[i] == end - start && core_base >= 0
          && core_base + (end - start) <= n_core;
  }
  if (!usable) {                                         // wave-uniform
    if (lane == 0) atomicMin(first_invalid, (uint32_t)r);
    return;
  }
  lds_chosen[wave][lane] = chosen;
  lds_before[wave][lane] = before;
  wave_sync();

  const int dim = 4 + struct_states + positional_cols;
  const int e_reverse = (int)edge_base + n_backbone;
  const int e_pair = (int)edge_base + 2 * n_backbone, e_skip = e_pair + 2 * n_pairs;
  const u64 below = (1ull << lane) - 1ull;
  const int words = (length + 63) >> 6;
  bool bad = false;
  for (int k = 0; k < words; ++k) {
    const u64 word = __shfl(chosen, k, 64);              // all of these wave-uniform
    if (word == 0ull) continue;
    const u64 word_backbone = __shfl(backbone, k, 64), word_pairs = __shfl(pair_opens, k, 64);
    const u64 word_skips = __shfl(skips, k, 64);
    const int rank0 = __shfl(before, k, 64), backbone0 = __shfl(before_backbone, k, 64);
    const int pairs0 = __shfl(before_pairs, k, 64), skips0 = __shfl(before_skips, k, 64);
    if (!((word >> lane) & 1ull)) continue;
    const int p = 64 * k + lane;
    const int node = (int)node_base + rank0 + __popcll(word & below);
    const bool core = p >= start && p < end;
    out.residue[node] = p;
    out.roles[node] = core ? 0 : 1;
    if (out.out_rows) out.out_rows[node] = core ? (int32_t)(core_base + (p - start)) : -1;

    const uint8_t letter = t.bases[base + p], mark = t.marks[base + p];
    const int code = letter == 'A' ? 0 : letter == 'C' ? 1 : letter == 'G' ? 2 : 3;
    const int state = mark == '(' ? 0 : mark == ')' ? 2 : 1;
    float* row = out.features + (int64_t)node * dim;
#pragma unroll
    for (int col = 0; col < 4; ++col) row[col] = col == code ? 1.f : 0.f;
    if (struct_states == 1) {
      row[4] = state != 1 ? 1.f : 0.f;
    } else {
#pragma unroll
      for (int col = 0; col < 3; ++col) row[4 + col] = col == state ? 1.f : 0.f;
    }
    for (int col = 0; col < positional_cols; ++col)
      row[4 + struct_states + col] = positional[(base + p) * positional_cols + col];

    if ((word_backbone >> lane) & 1ull) {                // p + 1 is chosen: the next rank
      const int at = backbone0 + __popcll(word_backbone & below);
      out.src[edge_base + at] = node;      out.dst[edge_base + at] = node + 1;
      out.types[edge_base + at] = 0;
      out.src[e_reverse + at] = node + 1;  out.dst[e_reverse + at] = node;
      out.types[e_reverse + at] = 1;
    }
    if ((word_pairs >> lane) & 1ull) {
      const int q = w.partner[base + p];
      const bool there = q > p && q < length && ((lds_chosen[wave][q >> 6] >> (q & 63)) & 1ull);
      if (!there) {
        bad = true;                                      // maps that disagree with the text
      } else {
        const int mate = (int)node_base + lds_before[wave][q >> 6]
                       + __popcll(lds_chosen[wave][q >> 6] & ((1ull << (q & 63)) - 1ull));
        const int forward = e_pair + pairs0 + __popcll(word_pairs & below);
        const int reverse = forward + n_pairs;
        out.src[forward] = node;  out.dst[forward] = mate;  out.types[forward] = 2;
        out.src[reverse] = mate;  out.dst[reverse] = node;  out.types[reverse] = 3;
      }
    }
    if ((word_skips >> lane) & 1ull) {                   // rank of p + 2: + 1 if p + 1 is chosen
      const u64 next = lane < 63 ? (word >> (lane + 1)) & 1ull : lds_chosen[wave][k + 1] & 1ull;
      const int far = node + 1 + (int)next;
      const int at = e_skip + 2 * (skips0 + __popcll(word_skips & below));
      out.src[at] = node;     out.dst[at] = far;      out.types[at] = 4;
      out.src[at + 1] = far;  out.dst[at + 1] = node; out.types[at + 1] = 5;
    }
  }
  if (__any(bad) && lane == 0) atomicMin(first_invalid, (uint32_t)r);
}

}  // namespace

size_t window_workspace_bytes(int64_t molecules, int64_t molecule_nt, int64_t records) {
  return window_scratch_bytes(molecules, molecule_nt, records);
}

int launch_window_select(const uint8_t* bases, const uint8_t* marks, const int64_t* mol_ptr,
                         int64_t molecules, int64_t molecule_nt, const int32_t* rec_mol,
                         const int32_t* rec_start, const int32_t* rec_end, int64_t records,
                         int keep, int hops, int skip2, int32_t* counts, int32_t* first_invalid,
                         void* ws, hipStream_t s) {
  const WindowScratch w = carve(ws, molecules, molecule_nt);
  const Molecules t{bases, marks, mol_ptr, (int)molecules, molecule_nt};
  const Windows rec{rec_mol, rec_start, rec_end};
  GFY_CHECK_HIP(hipMemsetAsync(first_invalid, 0xFF, sizeof(int32_t), s));   // -1 = all valid
  GFY_CHECK_HIP(hipMemsetAsync(w.partner, 0xFF, (size_t)molecule_nt * 4, s));   // -1 = unpaired
  hipLaunchKernelGGL(k_window_pairs, dim3((unsigned)((molecules + kWaves - 1) / kWaves)),
                     dim3(64 * kWaves), 0, s, t, w);
  GFY_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_window_select, dim3((unsigned)((records + kWaves - 1) / kWaves)),
                     dim3(64 * kWaves), 0, s, t, rec, (int)records, keep, hops, skip2, w, counts,
                     (uint32_t*)first_invalid);
  GFY_CHECK_HIP(hipGetLastError());
  return GFY_OK;
}

int launch_window_emit(const uint8_t* bases, const uint8_t* marks, const int64_t* mol_ptr,
                       int64_t molecules, int64_t molecule_nt, const int32_t* rec_mol,
                       const int32_t* rec_start, const int32_t* rec_end, int64_t first_record,
                       int64_t records, const int64_t* node_ptr, const int64_t* edge_ptr,
                       const int64_t* core_ptr, int64_t n, int64_t e, int64_t n_core,
                       int struct_states, int positional_cols, int skip2,
                       const float* positional, float* features, int32_t* edge_index,
                       uint8_t* edge_types, int32_t* residue_index, uint8_t* node_roles,
                       int32_t* out_rows, int32_t* first_invalid, void* ws, hipStream_t s) {
  const WindowScratch w = carve(ws, molecules, molecule_nt);
  const Molecules t{bases, marks, mol_ptr, (int)molecules, molecule_nt};
  const Windows rec{rec_mol, rec_start, rec_end};
  const EmitOut out{features, edge_index, edge_index + e, edge_types, residue_index, node_roles,
                    out_rows};
  GFY_CHECK_HIP(hipMemsetAsync(first_invalid, 0xFF, sizeof(int32_t), s));
  hipLaunchKernelGGL(k_window_emit, dim3((unsigned)((records + kWaves - 1) / kWaves)),
                     dim3(64 * kWaves), 0, s, t, rec, (int)first_record, (int)records, w,
                     node_ptr, edge_ptr, core_ptr, n, e, n_core, struct_states, positional_cols,
                     skip2, positional, out, (uint32_t*)first_invalid);
  GFY_CHECK_HIP(hipGetLastError());
  return GFY_OK;
}

}  // namespace gfy
