// The alignment kernels (semantics of every call: include/gfy.h): the one loop of align_local.inc,
// Smith-Waterman with affine gaps (Gotoh) over the cosine of the records' rows, instantiated once
// per mode, and the one launcher behind the entry points of gfy_api.hip.  What a mode bit means
// is said at AlignMode (gfy_common.h) and, statement by statement, in align_local.inc; which
// modes exist is the table below and nothing else.  Two kinds of call:
//   * score and span calls keep, per wave of the grid, two carry buffers of a strip's last row in
//     the caller's workspace: (H, F) entries, with kSpan their origins behind them (16 bytes, not
//     8).  A box or an order changes no buffer: it has to hold the widest matrix's columns.
//     kOrder runs over the virtual pairs p * shuffles + k as the others run over pairs.
//   * trace calls cut the workspace into equal parts, one per wave: two carry buffers of (H, F)
//     entries, then 4 direction bits per cell of the largest box, the only thing proportional to
//     L_q x L_r the library writes.  Fewer parts than waves of the grid means fewer waves.
// A local call with a box and no band has the covering band (a null `bands`), and a local path
// needs no boxed trace (start..end lies inside the box): both save instantiations.
#include "align_local.inc"

namespace gfy {
namespace {

// Every kernel takes the same argument; a mode that does not read a field never loads it.
struct KernelArgs {
  AlignArgs align;
  AlignExtras extra;
};

template <unsigned kMode>
__device__ __forceinline__ void run(const KernelArgs& p) {
  align_pairs<kMode>(p.align, p.extra.out_start, &p.extra.trace, p.extra.within != 0,
                     &p.extra.orders);
}

#define GFY_ALIGN_KERNEL(name, mode) \
  __global__ __launch_bounds__(kAlignThreads) void name(const KernelArgs p) { run<mode>(p); }
GFY_ALIGN_KERNEL(k_align_local, 0)
GFY_ALIGN_KERNEL(k_align_span, kSpan)
GFY_ALIGN_KERNEL(k_align_trace, kTrace)
GFY_ALIGN_KERNEL(k_align_local_band, kBand)
GFY_ALIGN_KERNEL(k_align_span_band, kSpan | kBand)
GFY_ALIGN_KERNEL(k_align_trace_band, kTrace | kBand)
GFY_ALIGN_KERNEL(k_align_local_box, kBand | kBox)
GFY_ALIGN_KERNEL(k_align_span_box, kSpan | kBand | kBox)
GFY_ALIGN_KERNEL(k_align_local_null, kBand | kBox | kOrder)
GFY_ALIGN_KERNEL(k_align_global, kGlobal)
GFY_ALIGN_KERNEL(k_align_global_trace, kTrace | kGlobal)
GFY_ALIGN_KERNEL(k_align_global_box, kGlobal | kBox)
GFY_ALIGN_KERNEL(k_align_global_trace_box, kTrace | kGlobal | kBox)
#undef GFY_ALIGN_KERNEL

// A mode's kernel, the entry point that a refusal names, whether the workspace is a trace's, and
// the bytes of a carry entry; `opt_in` is the kernel's opt-in to kAlignLds, once per device.
struct ModeRow {
  unsigned mode;
  void (*kernel)(KernelArgs);
  const char* who;
  bool trace;
  size_t carry;
  PerDeviceOnce opt_in;
};
#define GFY_ALIGN_ROW(mode, kernel, who) \
  {mode, kernel, who, ((mode) & kTrace) != 0, sizeof(AlignCarry<((mode) & kSpan) != 0>), {}}
ModeRow mode_rows[] = {
    GFY_ALIGN_ROW(0, k_align_local, "gfy_align_local"),
    GFY_ALIGN_ROW(kSpan, k_align_span, "gfy_align_local_span"),
    GFY_ALIGN_ROW(kTrace, k_align_trace, "gfy_align_trace"),
    GFY_ALIGN_ROW(kBand, k_align_local_band, "gfy_align_local_band"),
    GFY_ALIGN_ROW(kSpan | kBand, k_align_span_band, "gfy_align_local_span_band"),
    GFY_ALIGN_ROW(kTrace | kBand, k_align_trace_band, "gfy_align_trace_band"),
    GFY_ALIGN_ROW(kBand | kBox, k_align_local_box, "gfy_align_local_box"),
    GFY_ALIGN_ROW(kSpan | kBand | kBox, k_align_span_box, "gfy_align_local_span_box"),
    GFY_ALIGN_ROW(kBand | kBox | kOrder, k_align_local_null, "gfy_align_local_null"),
    GFY_ALIGN_ROW(kGlobal, k_align_global, "gfy_align_global"),
    GFY_ALIGN_ROW(kTrace | kGlobal, k_align_global_trace, "gfy_align_global_trace"),
    GFY_ALIGN_ROW(kGlobal | kBox, k_align_global_box, "gfy_align_global_box"),
    GFY_ALIGN_ROW(kTrace | kGlobal | kBox, k_align_global_trace_box, "gfy_align_global_trace_box"),
};
#undef GFY_ALIGN_ROW

int align_groups(int64_t pairs) {
  const int64_t groups = (pairs + kAlignWaves - 1) / kAlignWaves;
  return (int)(groups < 1 ? 1 : groups > kAlignGroupsMax ? kAlignGroupsMax : groups);
}

// two carry buffers of max_rows_b entries of `entry` bytes per wave of the grid
size_t align_carry_bytes(size_t entry, int64_t pairs, int64_t max_rows_b) {
  const size_t waves = (size_t)align_groups(pairs) * kAlignWaves;
  return align_up(waves * 2 * (size_t)max_rows_b * entry + 1, 256);
}

// the carry of a score or span call in the caller's workspace: the check, then `carry` and `cap`
// of `p`, the launcher's copy of the call
int align_take_carry(const ModeRow& row, AlignArgs* p, void* ws, size_t ws_bytes) {
  const size_t least = align_carry_bytes(row.carry, p->P, 0);
  GFY_REQUIRE(ws_bytes >= least, GFY_ERR_WORKSPACE, "%s: workspace %zu < required %zu", row.who,
              ws_bytes, least);
  const size_t columns = ws_bytes / ((size_t)align_groups(p->P) * kAlignWaves * 2 * row.carry);
  p->carry = ws;
  p->cap = (int)(columns < GFY_ALIGN_ROWS_MAX ? columns : GFY_ALIGN_ROWS_MAX);
  return GFY_OK;
}

int64_t trace_region_words(int64_t max_box_rows, int64_t max_box_cols) {
  return max_box_rows * ((max_box_cols + 7) / 8);
}

// a wave's part of a trace workspace: two carry buffers of max_box_cols (H, F) entries and the
// direction words of the largest box
size_t trace_wave_bytes(int64_t max_box_rows, int64_t max_box_cols) {
  return align_up((size_t)2 * max_box_cols * sizeof(AlignCarry<false>) +
                      (size_t)trace_region_words(max_box_rows, max_box_cols) * 4 + 1, 256);
}

// the caller's workspace cut into such parts: the check, then what the launcher's copies `p` and
// `trace` of a trace call say about it
int trace_take_workspace(const ModeRow& row, AlignArgs* p, AlignExtras* extra, void* ws,
                         size_t ws_bytes) {
  const size_t wave_bytes = trace_wave_bytes(extra->max_box_rows, extra->max_box_cols);
  GFY_REQUIRE(ws_bytes >= wave_bytes, GFY_ERR_WORKSPACE,
              "%s: workspace %zu < the %zu of one wave", row.who, ws_bytes, wave_bytes);
  const size_t fit = ws_bytes / wave_bytes, waves = (size_t)align_groups(p->P) * kAlignWaves;
  p->carry = ws;
  p->cap = (int)extra->max_box_cols;
  extra->trace.waves = (int64_t)(fit < waves ? fit : waves);
  extra->trace.wave_bytes = (int64_t)wave_bytes;
  extra->trace.region_words = trace_region_words(extra->max_box_rows, extra->max_box_cols);
  return GFY_OK;
}

}  // namespace

size_t align_workspace_bytes(int64_t pairs, int64_t max_rows_b) {
  return align_carry_bytes(sizeof(AlignCarry<false>), pairs, max_rows_b);
}

size_t align_span_workspace_bytes(int64_t pairs, int64_t max_rows_b) {
  return align_carry_bytes(sizeof(AlignCarry<true>), pairs, max_rows_b);
}

size_t align_trace_workspace_bytes(int64_t pairs, int64_t max_box_rows, int64_t max_box_cols) {
  return (size_t)align_groups(pairs) * kAlignWaves * trace_wave_bytes(max_box_rows, max_box_cols);
}

int launch_align(unsigned mode, const AlignArgs& call, const AlignExtras& extras, void* ws,
                 size_t ws_bytes, hipStream_t s) {
  ModeRow* row = nullptr;
  for (ModeRow& candidate : mode_rows)
    if (candidate.mode == mode) row = &candidate;
  GFY_REQUIRE(row, GFY_ERR_INVALID, "launch_align: no kernel of mode %u", mode);
  KernelArgs p{call, extras};
  int groups;
  if (row->trace) {
    if (const int rc = trace_take_workspace(*row, &p.align, &p.extra, ws, ws_bytes)) return rc;
    // whole workgroups of the waves that have a part; the rest of the last one returns at once
    groups = (int)((p.extra.trace.waves + kAlignWaves - 1) / kAlignWaves);
  } else {
    // kOrder: P counts the virtual pairs (the entry point has checked that the product fits)
    if (mode & kOrder) p.align.P = call.P * extras.orders.shuffles;
    if (const int rc = align_take_carry(*row, &p.align, ws, ws_bytes)) return rc;
    groups = align_groups(p.align.P);
  }
  // kernel<<<groups, kAlignThreads, kAlignLds>>>(p): the opt-in to that much dynamic LDS once per
  // device and kernel, as launch_sweep (pairwise_sweep.inc) does it
  if (const int rc = row->opt_in.run([row]() -> int {
        GFY_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(row->kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, kAlignLds));
        return GFY_OK;
      }))
    return rc;
  row->kernel<<<groups, kAlignThreads, kAlignLds, s>>>(p);
  GFY_CHECK_HIP(hipGetLastError());
  return GFY_OK;
}

}  // namespace gfy
