// What BOTH shared objects need and no HIP call is in: the per-thread error channel, the ABI
// version and the weight pack's reader (weight_pack.h).  libgfy.so (HIP kernels + C ABI) links
// it, and so does libgfy_host.so = this file + gine_host.cpp, built with the host compiler
// alone: the reference's default device (Ginfinity.load(device="cpu"),
// src/ginfinity/api.py:64-76) then works on a box that has no ROCm runtime at all.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#include "../../include/gfy.h"
#include "weight_pack.h"

namespace gfy {

static thread_local std::string g_error;

void set_error(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_error = buf;
}
void clear_error() { g_error.clear(); }

// ---- the weight pack (weight_pack.h; layout: ginfinity_amd/weights.py, tensor_order) ---------
namespace {

// Walks the floats behind the header in pack order.  Without a pack it only counts.
struct PackCursor {
  const float* base;
  size_t at = 0;
  const float* take(size_t count) {
    const float* here = base ? base + at : nullptr;
    at += count;
    return here;
  }
};

void walk_input(PackCursor& c, size_t in_dim, size_t h, PackView& v) {
  v.w_in = c.take(h * in_dim);
  v.b_in = c.take(h);
}

void walk_layer(PackCursor& c, size_t h, size_t edge_dim, PackLayer& l) {
  const size_t m = 2 * h;
  l.eps = c.take(1);
  l.edge_w = c.take(h * edge_dim);
  l.edge_b = c.take(h);
  l.w0 = c.take(m * h);
  l.b0 = c.take(m);
  l.bn_gamma = c.take(m);
  l.bn_beta = c.take(m);
  l.bn_mean = c.take(m);
  l.bn_var = c.take(m);
  l.w1 = c.take(h * m);
  l.b1 = c.take(h);
  l.ln_gamma = c.take(h);
  l.ln_beta = c.take(h);
}

void walk_head(PackCursor& c, size_t h, size_t out_dim, PackView& v) {
  v.wa = c.take(h * h);
  v.ba = c.take(h);
  v.wb = c.take(out_dim * h);
  v.bb = c.take(out_dim);
}

}  // namespace

size_t pack_floats(uint32_t in_dim, uint32_t h, uint32_t layers, uint32_t edge_dim,
                   uint32_t out_dim) {
  PackView nowhere;
  PackCursor input{nullptr}, layer{nullptr}, head{nullptr};
  walk_input(input, in_dim, h, nowhere);
  walk_layer(layer, h, edge_dim, nowhere.layer[0]);
  walk_head(head, h, out_dim, nowhere);
  return input.at + layers * layer.at + head.at;
}

int read_weight_pack(const char* who, const void* pack, size_t bytes, int model_dtype,
                     PackView* view) {
  PackHeader hd;
  if (!pack || bytes < sizeof hd) {
    set_error("%s: weight pack missing or truncated", who);
    return GFY_ERR_INVALID;
  }
  std::memcpy(&hd, pack, sizeof hd);
  if (hd.magic != kPackMagic || hd.version != kPackVersion) {
    set_error("%s: bad weight-pack magic/version", who);
    return GFY_ERR_INVALID;
  }
  if (hd.in_dim != (uint32_t)kInDim || hd.hidden != (uint32_t)kHidden ||
      hd.out_dim != (uint32_t)kOutDim || hd.layers < 1 || hd.layers > (uint32_t)kMaxLayers ||
      hd.edge_dim < 1 || hd.edge_dim > (uint32_t)kMaxEdgeTypes) {
    set_error("%s: built for in_dim=%d hidden=%d out_dim=%d, 1..%d layers, 1..%d edge types "
              "(got in_dim=%u hidden=%u out_dim=%u, %u layers, %u edge types)",
              who, kInDim, kHidden, kOutDim, kMaxLayers, kMaxEdgeTypes, hd.in_dim, hd.hidden,
              hd.out_dim, hd.layers, hd.edge_dim);
    return GFY_ERR_UNSUPPORTED;
  }
  const size_t expected =
      gfy_weight_pack_bytes(hd.in_dim, hd.hidden, hd.layers, hd.edge_dim, hd.out_dim);
  if (bytes != expected) {
    set_error("%s: weight pack is %zu bytes, expected %zu", who, bytes, expected);
    return GFY_ERR_INVALID;
  }
  if (model_dtype != GFY_F16 && model_dtype != GFY_F32) {
    set_error("%s: model_dtype must be GFY_F16 or GFY_F32", who);
    return GFY_ERR_INVALID;
  }
  *view = PackView{};
  view->layers = (int)hd.layers;
  view->edge_dim = (int)hd.edge_dim;
  view->residual = (int)(hd.flags & 1u);
  PackCursor c{reinterpret_cast<const float*>(static_cast<const char*>(pack) + sizeof hd)};
  walk_input(c, hd.in_dim, hd.hidden, *view);
  for (int l = 0; l < view->layers; ++l) walk_layer(c, hd.hidden, hd.edge_dim, view->layer[l]);
  walk_head(c, hd.hidden, hd.out_dim, *view);
  return GFY_OK;
}

// Copies into page-locked staging memory (gfy_pack_microbatch).  The destination is written
// once and next read by the copy engine, never by this core: streaming stores leave it out of
// the cache and spare the read-for-ownership of every destination line (a third of the copy's
// memory traffic).  GFY_PACK_STREAM=0 keeps memcpy (A/B runs: tools/bench_host_feed.py).
static bool stream_stores() {   // read per call (once per ~4 MB): tests and A/B runs switch it
  const char* text = std::getenv("GFY_PACK_STREAM");
  return text == nullptr || text[0] != '0';
}

// to[i] = from[i] - shift for `count` 32-bit values; returns the OR of (value | (limit - value))
// over all of them: negative exactly when some value lies outside [0, limit].  `*inside` takes
// the OR of ((value - low) | (high - value)): negative when a value inside [0, limit] lies
// outside [low, high] — the node range of the record these edges belong to.
static int32_t copy_rebased(int32_t* to, const int32_t* from, int64_t count, int32_t shift,
                            int32_t limit, int32_t low, int32_t high, int32_t* inside,
                            bool stream) {
  int32_t seen = 0, kept = 0;
  int64_t i = 0;
#if defined(__SSE2__)
  if (stream) {
    for (; i < count && (reinterpret_cast<uintptr_t>(to + i) & 15) != 0; ++i) {
      const int32_t value = (int32_t)((uint32_t)from[i] - (uint32_t)shift);
      to[i] = value;
      seen |= value | (int32_t)((uint32_t)limit - (uint32_t)value);
      kept |= (int32_t)((uint32_t)value - (uint32_t)low) | (int32_t)((uint32_t)high - (uint32_t)value);
    }
    const __m128i shifts = _mm_set1_epi32(shift), limits = _mm_set1_epi32(limit);
    const __m128i lows = _mm_set1_epi32(low), highs = _mm_set1_epi32(high);
    __m128i any = _mm_setzero_si128(), own = _mm_setzero_si128();
    for (; i + 16 <= count; i += 16) {
      __m128i v[4];
      for (int k = 0; k < 4; ++k)
        v[k] = _mm_sub_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i*>(from + i + 4 * k)),
                             shifts);
      for (int k = 0; k < 4; ++k) {
        any = _mm_or_si128(any, _mm_or_si128(v[k], _mm_sub_epi32(limits, v[k])));
        own = _mm_or_si128(own, _mm_or_si128(_mm_sub_epi32(v[k], lows), _mm_sub_epi32(highs, v[k])));
        _mm_stream_si128(reinterpret_cast<__m128i*>(to + i + 4 * k), v[k]);
      }
    }
    alignas(16) int32_t lanes[4];
    _mm_store_si128(reinterpret_cast<__m128i*>(lanes), any);
    seen |= lanes[0] | lanes[1] | lanes[2] | lanes[3];
    _mm_store_si128(reinterpret_cast<__m128i*>(lanes), own);
    kept |= lanes[0] | lanes[1] | lanes[2] | lanes[3];
  }
#endif
  for (; i < count; ++i) {
    const int32_t value = (int32_t)((uint32_t)from[i] - (uint32_t)shift);
    to[i] = value;
    seen |= value | (int32_t)((uint32_t)limit - (uint32_t)value);
    kept |= (int32_t)((uint32_t)value - (uint32_t)low) | (int32_t)((uint32_t)high - (uint32_t)value);
  }
  *inside |= kept;
  return seen;
}

static void copy_bytes(void* to_, const void* from_, size_t bytes, bool stream) {
#if defined(__SSE2__)
  if (stream && bytes >= 4096) {
    char* to = static_cast<char*>(to_);
    const char* from = static_cast<const char*>(from_);
    const size_t head = (16 - (reinterpret_cast<uintptr_t>(to) & 15)) & 15;
    memcpy(to, from, head);
    size_t at = head;
    for (; at + 64 <= bytes; at += 64) {
      __m128i v[4];
      for (int k = 0; k < 4; ++k)
        v[k] = _mm_loadu_si128(reinterpret_cast<const __m128i*>(from + at + 16 * k));
      for (int k = 0; k < 4; ++k)
        _mm_stream_si128(reinterpret_cast<__m128i*>(to + at + 16 * k), v[k]);
    }
    memcpy(to + at, from + at, bytes - at);
    return;
  }
#endif
  memcpy(to_, from_, bytes);
}

}  // namespace gfy

extern "C" {

const char* gfy_last_error(void) { return gfy::g_error.c_str(); }
int gfy_abi_version(void) { return GFY_ABI_VERSION; }

// One micro-batch of a host shard -> a staging block (include/gfy.h; the byte-for-byte twin of
// ginfinity_amd/api.py:_pack_microbatch_at + _Uploader.pack_at, which stay as the reference
// the tests compare it with).
int gfy_pack_microbatch(const float* node_features, int feature_dim, const int32_t* edge_index,
                        int64_t edges_total, const uint8_t* edge_types,
                        const uint8_t* node_roles, const int64_t* node_ptr,
                        const int64_t* edge_ptr, int64_t start, int64_t stop, int with_records,
                        void* slot, int64_t base, int64_t* offsets, int64_t* counts) {
  gfy::clear_error();
  if (!node_features || !node_ptr || !edge_ptr || !node_roles || !slot || !offsets || !counts ||
      feature_dim <= 0 || start < 0 || stop < start || base < 0 || (base & 255) != 0) {
    gfy::set_error("gfy_pack_microbatch: NULL argument, empty record range or unaligned base");
    return GFY_ERR_INVALID;
  }
  const int64_t n0 = node_ptr[start], n1 = node_ptr[stop], e0 = edge_ptr[start], e1 = edge_ptr[stop];
  const int64_t n = n1 - n0, e = e1 - e0;
  if (n < 0 || e < 0 || e0 < 0 || e1 > edges_total || (e > 0 && (!edge_index || !edge_types))) {
    gfy::set_error("gfy_pack_microbatch: records [%lld, %lld) have no valid node / edge range",
                   (long long)start, (long long)stop);
    return GFY_ERR_INVALID;
  }
  auto pad = [](int64_t bytes) { return (bytes + 255) / 256 * 256; };
  char* const out = static_cast<char*>(slot);
  const bool stream = gfy::stream_stores();
  int64_t at = base;
  // node rows
  offsets[0] = at;
  gfy::copy_bytes(out + at, node_features + n0 * feature_dim, (size_t)(n * feature_dim) * 4, stream);
  at += pad(n * feature_dim * 4);
  // record boundaries travel only where every record's edge list is short (engine.py,
  // records_pay) ...
  bool records = with_records != 0 && stop > start;
  for (int64_t r = start; r < stop && records; ++r)
    records = edge_ptr[r + 1] >= edge_ptr[r] && edge_ptr[r + 1] - edge_ptr[r] <= (int64_t)1 << 16;
  // edge_index, rebased; an index outside [0, n) in either row is the caller's error.  Where
  // boundaries would travel the copy goes record by record and also looks whether both ends of
  // every edge lie in the record that owns it (by list position): the record-range set-up finds
  // a row's in-edges only there (gfy.h, gfy_shard), the reference honours the edge wherever it
  // points inside the micro-batch.
  offsets[1] = at;
  int32_t seen = 0, inside = 0;
  for (int row = 0; row < 2 && e > 0; ++row) {   // (no edges: edge_index may be NULL, no offset to it)
    const int32_t* from = edge_index + (int64_t)row * edges_total + e0;
    int32_t* to = reinterpret_cast<int32_t*>(out + at) + (int64_t)row * e;
    if (!records) {
      seen |= gfy::copy_rebased(to, from, e, (int32_t)n0, (int32_t)(n - 1), 0, (int32_t)(n - 1),
                                &inside, stream);
      continue;
    }
    for (int64_t r = start; r < stop; ++r) {
      const int64_t first = edge_ptr[r] - e0;
      seen |= gfy::copy_rebased(to + first, from + first, edge_ptr[r + 1] - edge_ptr[r],
                                (int32_t)n0, (int32_t)(n - 1), (int32_t)(node_ptr[r] - n0),
                                (int32_t)(node_ptr[r + 1] - 1 - n0), &inside, stream);
    }
  }
  if (e > 0 && seen < 0) {
    gfy::set_error("edge index outside shard node range");
    return GFY_ERR_INVALID;
  }
  if (inside < 0) records = false;   // an edge joins two records: this micro-batch is counted
  at += pad(2 * e * 4);
  offsets[2] = at;
  if (e > 0) gfy::copy_bytes(out + at, edge_types + e0, (size_t)e, stream);
  at += pad(e);
  // core rows: present only where a node of the range is not a core node (role != 0)
  bool any = false;
  for (int64_t i = n0; i < n1 && !any; ++i) any = node_roles[i] != 0;
  int64_t kept = n;
  offsets[3] = -1;
  if (any) {
    offsets[3] = at;
    int32_t* rows = reinterpret_cast<int32_t*>(out + at);
    int32_t next = 0;
    for (int64_t i = 0; i < n; ++i) rows[i] = node_roles[n0 + i] == 0 ? next++ : -1;
    kept = next;
    at += pad(n * 4);
  }
  // record boundaries, as they are (the set-up kernel reads them relative to their first entry)
  offsets[4] = offsets[5] = -1;
  if (records) {
    const int64_t bytes = (stop - start + 1) * 8;
    offsets[4] = at;
    memcpy(out + at, node_ptr + start, (size_t)bytes);
    at += pad(bytes);
    offsets[5] = at;
    memcpy(out + at, edge_ptr + start, (size_t)bytes);
    at += pad(bytes);
  }
  counts[0] = n, counts[1] = e, counts[2] = records ? stop - start : 0, counts[3] = kept;
#if defined(__SSE2__)
  if (stream) _mm_sfence();   // the streamed lines are in memory before the copy engine is told
#endif
  return GFY_OK;
}

size_t gfy_weight_pack_bytes(uint32_t in_dim, uint32_t hidden, uint32_t layers,
                             uint32_t edge_dim, uint32_t out_dim) {
  return sizeof(gfy::PackHeader) + 4 * gfy::pack_floats(in_dim, hidden, layers, edge_dim, out_dim);
}

}  // extern "C"
