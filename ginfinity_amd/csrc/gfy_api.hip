// C ABI of libgfy (include/gfy.h): argument checking and the calls into the launchers.  The
// weight pack is read by gfy_base.cpp (weight_pack.h) and turned into what the kernels consume
// by weight_image.cpp; encoder creation here uploads that image and binds pointers to it.
#include <memory>
#include <string>

#include "gfy_common.h"

namespace gfy {
namespace {

// Makes `device` current for the life of the guard and gives the caller's device back: the
// library never leaves the calling thread on another device than it came with.
struct DeviceGuard {
  int previous = -1;
  hipError_t status;
  explicit DeviceGuard(int device) {
    status = hipGetDevice(&previous);
    if (status == hipSuccess && previous != device) status = hipSetDevice(device);
  }
  ~DeviceGuard() {
    if (previous >= 0) (void)hipSetDevice(previous);
  }
};

// Every launching entry point runs on the CALLER's current device (streams and buffers are the
// caller's): an encoder built for another device is refused instead of faulting or silently
// going through peer access.
static int check_current_device(const gfy_encoder* enc, const char* who) {
  int current = -1;
  GFY_CHECK_HIP(hipGetDevice(&current));
  GFY_REQUIRE(current == enc->device, GFY_ERR_INVALID,
              "%s: the encoder lives on HIP device %d but the calling thread's current device is "
              "%d (hipSetDevice / torch.cuda.device first)", who, enc->device, current);
  return GFY_OK;
}

// One place per model where blob offsets (weight_image.h) become the pointers the launchers read
void bind_f16(gfy_encoder* enc, const ImageF16& o) {
  const char* base = static_cast<const char*>(enc->device_blob);
  auto at = [&](size_t off) { return reinterpret_cast<const f16*>(base + off); };
  enc->f16.w_in = at(o.input.w);
  enc->f16.b_in = at(o.input.b);
  for (int l = 0; l < enc->layers; ++l)
    enc->f16.layer[l] = LayerF16{o.layer[l].scale, enc->edge_dim, at(o.layer[l].w01),
                                 base + o.layer[l].image};
  enc->f16.head = HeadF16{at(o.head.wa), at(o.head.ba), at(o.head.wb), at(o.head.bb),
                          at(o.head.w_image), base + o.head.image};
}

void bind_f32(gfy_encoder* enc, const ImageF32& o) {
  const char* base = static_cast<const char*>(enc->device_blob);
  auto at = [&](size_t off) { return reinterpret_cast<const float*>(base + off); };
  enc->f32.w_in_t = at(o.input.w);
  enc->f32.b_in = at(o.input.b);
  for (int l = 0; l < enc->layers; ++l) {
    const LayerF32Off& from = o.layer[l];
    enc->f32.layer[l] = LayerF32{at(from.table), from.one_plus_eps, at(from.w0t), at(from.b0),
                                 at(from.alpha), at(from.shift), at(from.w1t), at(from.b1),
                                 at(from.ln_g), at(from.ln_b)};
  }
  enc->f32.ha_wt = at(o.head.wa_t);
  enc->f32.ha_b = at(o.head.ba);
  enc->f32.hb_wt = at(o.head.wb_t);
  enc->f32.hb_b = at(o.head.bb);
}

}  // namespace
}  // namespace gfy

using namespace gfy;

struct gfy_upload_ring {     // include/gfy.h: one event per staging slot of the caller
  int slots = 0;
  hipEvent_t done[64] = {};
  bool used[64] = {};
};

extern "C" {

int gfy_encoder_create(const void* weight_pack_host, size_t bytes,
                       int model_dtype, int device, gfy_encoder** out) {
  clear_error();
  GFY_REQUIRE(out != nullptr, GFY_ERR_INVALID, "gfy_encoder_create: out is NULL");
  *out = nullptr;
  PackView pack;
  if (const int rc = read_weight_pack("gfy_encoder_create", weight_pack_host, bytes, model_dtype,
                                      &pack))
    return rc;
  DeviceGuard guard(device);   // the caller's current device is restored on every way out
  GFY_CHECK_HIP(guard.status);
  if (model_dtype == GFY_F16)
    if (const int rc = prepare_device_f16()) return rc;

  std::unique_ptr<gfy_encoder> enc(new gfy_encoder());   // ours until *out is set
  enc->device = device;
  enc->model_dtype = model_dtype;
  enc->layers = pack.layers;
  enc->edge_dim = pack.edge_dim;
  enc->residual = pack.residual;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
      cus >= 8)
    enc->cus = cus & ~7;

  // one host image of every derived tensor, one upload, then offsets become pointers
  Blob blob;
  ImageF16 f16_at{};
  ImageF32 f32_at{};
  if (model_dtype == GFY_F16) f16_at = build_image_f16(blob, pack);
  else f32_at = build_image_f32(blob, pack);
  void* dev = nullptr;
  hipError_t err = hipMalloc(&dev, blob.host.size());
  if (err == hipSuccess)
    err = hipMemcpy(dev, blob.host.data(), blob.host.size(), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    if (dev) (void)hipFree(dev);
    set_error("gfy_encoder_create: device upload failed: %s", hipGetErrorString(err));
    return GFY_ERR_HIP;
  }
  enc->device_blob = dev;
  enc->device_blob_bytes = blob.host.size();
  if (model_dtype == GFY_F16) bind_f16(enc.get(), f16_at);
  else bind_f32(enc.get(), f32_at);
  *out = enc.release();
  return GFY_OK;
}

int gfy_encoder_set_timing(gfy_encoder* enc, int enable) {
  clear_error();
  GFY_REQUIRE(enc != nullptr, GFY_ERR_INVALID, "gfy_encoder_set_timing: encoder is NULL");
  GFY_REQUIRE(enable != 3 || enc->model_dtype == GFY_F16, GFY_ERR_UNSUPPORTED,
              "gfy_encoder_set_timing: mode 3 (device-clock spans) exists for the fp16 model only");
  DeviceGuard guard(enc->device);
  GFY_CHECK_HIP(guard.status);
  if (enable && !enc->events[0])
    for (auto& ev : enc->events) GFY_CHECK_HIP(hipEventCreate(&ev));
  if (enable == 3 && !enc->device_spans) {
    GFY_CHECK_HIP(hipMalloc((void**)&enc->device_spans, 2 * kMaxLayers * sizeof(unsigned long long)));
    // start = +inf, end = 0: a launch that never ran reads as "no span", not as garbage
    unsigned long long init[2 * kMaxLayers];
    for (int l = 0; l < kMaxLayers; ++l) init[2 * l] = ~0ull, init[2 * l + 1] = 0;
    GFY_CHECK_HIP(hipMemcpy(enc->device_spans, init, sizeof init, hipMemcpyHostToDevice));
  }
  enc->timing = enable == 2 || enable == 3 ? enable : enable != 0;
  enc->events_recorded = 0;
  return GFY_OK;
}

int gfy_encoder_set_option(gfy_encoder* enc, int option, int value) {
  clear_error();
  GFY_REQUIRE(enc != nullptr, GFY_ERR_INVALID, "gfy_encoder_set_option: encoder is NULL");
  switch (option) {
    case GFY_OPT_SEPARATE_HEAD:
      GFY_REQUIRE(value == 0 || value == 1, GFY_ERR_INVALID,
                  "gfy_encoder_set_option: GFY_OPT_SEPARATE_HEAD must be 0 or 1 (got %d)", value);
      enc->separate_head = value;
      return GFY_OK;
    case GFY_OPT_LAYER_KERNEL:
      GFY_REQUIRE(value == -1 || value == 1 || value == 3 || value == 4 || value == 5,
                  GFY_ERR_INVALID,
                  "gfy_encoder_set_option: GFY_OPT_LAYER_KERNEL must be -1 (by rounds), 1 (round-2 "
                  "kernel), 3 (persistent rounds), 4 (two windowed workgroups per CU) or 5 (three "
                  "workgroups per CU), got %d", value);
      enc->layer_kernel = value;
      return GFY_OK;
    case GFY_OPT_STAGGER:
      GFY_REQUIRE(value >= -1 && value <= 100000, GFY_ERR_INVALID,
                  "gfy_encoder_set_option: GFY_OPT_STAGGER must be -1 (default) or 0..100000 "
                  "cycles (got %d)", value);
      enc->stagger = value;
      return GFY_OK;
    case GFY_OPT_PRIORITY:
      GFY_REQUIRE(value >= -1 && value <= 63, GFY_ERR_INVALID,
                  "gfy_encoder_set_option: GFY_OPT_PRIORITY must be -1 (default) or 0..63 (got %d)",
                  value);
      enc->priority = value;
      return GFY_OK;
    default:
      set_error("gfy_encoder_set_option: unknown option %d", option);
      return GFY_ERR_INVALID;
  }
}

int gfy_upload_ring_create(int slots, gfy_upload_ring** ring_out) {
  clear_error();
  GFY_REQUIRE(ring_out && slots >= 1 && slots <= 64, GFY_ERR_INVALID,
              "gfy_upload_ring_create: NULL argument or slots %d outside 1..64", slots);
  gfy_upload_ring* ring = new gfy_upload_ring();
  ring->slots = slots;
  for (int slot = 0; slot < slots; ++slot) {
    hipError_t err = hipEventCreateWithFlags(&ring->done[slot], hipEventDisableTiming);
    if (err != hipSuccess) {
      set_error("hipEventCreateWithFlags failed: %s", hipGetErrorString(err));
      ring->slots = slot;
      gfy_upload_ring_destroy(ring);
      return GFY_ERR_HIP;
    }
  }
  *ring_out = ring;
  return GFY_OK;
}

void gfy_upload_ring_destroy(gfy_upload_ring* ring) {
  if (!ring) return;
  for (int slot = 0; slot < ring->slots; ++slot) (void)hipEventDestroy(ring->done[slot]);
  delete ring;
}

int gfy_upload_async(gfy_upload_ring* ring, int slot, void* device_dst, const void* pinned_src,
                     size_t bytes, void* copy_stream, void* consumer_stream) {
  clear_error();
  GFY_REQUIRE(ring && slot >= 0 && slot < ring->slots, GFY_ERR_INVALID,
              "gfy_upload_async: NULL ring or slot %d outside its slots", slot);
  GFY_REQUIRE(bytes == 0 || (device_dst && pinned_src), GFY_ERR_INVALID,
              "gfy_upload_async: NULL source or destination");
  hipStream_t copies = static_cast<hipStream_t>(copy_stream);
  if (bytes)
    GFY_CHECK_HIP(hipMemcpyAsync(device_dst, pinned_src, bytes, hipMemcpyHostToDevice, copies));
  GFY_CHECK_HIP(hipEventRecord(ring->done[slot], copies));
  ring->used[slot] = true;
  if (consumer_stream != copy_stream)
    GFY_CHECK_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(consumer_stream),
                                     ring->done[slot], 0));
  return GFY_OK;
}

int gfy_upload_wait(gfy_upload_ring* ring, int slot) {
  clear_error();
  GFY_REQUIRE(ring && slot >= 0 && slot < ring->slots, GFY_ERR_INVALID,
              "gfy_upload_wait: NULL ring or slot %d outside its slots", slot);
  if (ring->used[slot]) GFY_CHECK_HIP(hipEventSynchronize(ring->done[slot]));
  return GFY_OK;
}

int gfy_encoder_last_layer_kernel(const gfy_encoder* enc) {
  return enc ? enc->last_layer_kernel : 0;
}

int gfy_encoder_get_timing(gfy_encoder* enc, float* ms_host, int capacity, int* count) {
  clear_error();
  GFY_REQUIRE(enc && ms_host && count, GFY_ERR_INVALID, "gfy_encoder_get_timing: NULL argument");
  if (enc->timing == 3) {   // device clock spans of the layer launches, 100 MHz
    GFY_REQUIRE(capacity >= enc->layers, GFY_ERR_INVALID,
                "gfy_encoder_get_timing: capacity %d < %d", capacity, enc->layers);
    unsigned long long spans[2 * kMaxLayers];
    // the encode may have run on a non-blocking stream, which a plain hipMemcpy does not wait for
    if (const int rc = check_current_device(enc, "gfy_encoder_get_timing")) return rc;
    GFY_CHECK_HIP(hipStreamSynchronize(enc->last_stream));
    GFY_CHECK_HIP(hipMemcpy(spans, enc->device_spans, sizeof spans, hipMemcpyDeviceToHost));
    for (int l = 0; l < enc->layers; ++l) {
      GFY_REQUIRE(spans[2 * l + 1] >= spans[2 * l], GFY_ERR_INVALID,
                  "gfy_encoder_get_timing: layer launch %d left no span (no fp16 encode since "
                  "timing was set to 3?)", l);
      ms_host[l] = (float)((double)(spans[2 * l + 1] - spans[2 * l]) * 1e-5);   // 10 ns ticks
    }
    *count = enc->layers;
    return GFY_OK;
  }
  const int spans = enc->events_recorded - 1;
  GFY_REQUIRE(enc->timing && spans >= 1, GFY_ERR_INVALID,
              "gfy_encoder_get_timing: timing is off or nothing was recorded");
  GFY_REQUIRE(capacity >= spans, GFY_ERR_INVALID,
              "gfy_encoder_get_timing: capacity %d < %d", capacity, spans);
  GFY_CHECK_HIP(hipEventSynchronize(enc->events[spans]));
  const int L = enc->layers;
  for (int i = 0; i < spans; ++i) {
    if (enc->timing == 2 && i >= 1 && i < L) {   // layers 1 .. L-1: one span, reported as its mean
      if (i == 1) {
        float block = 0.f;
        GFY_CHECK_HIP(hipEventElapsedTime(&block, enc->events[1], enc->events[L]));
        for (int k = 1; k < L; ++k) ms_host[k] = block / (float)(L - 1);
      }
      continue;
    }
    GFY_CHECK_HIP(hipEventElapsedTime(&ms_host[i], enc->events[i], enc->events[i + 1]));
  }
  *count = spans;
  return GFY_OK;
}

void gfy_encoder_destroy(gfy_encoder* enc) {
  if (!enc) return;
  for (auto& ev : enc->events)
    if (ev) (void)hipEventDestroy(ev);
  if (enc->device_blob) (void)hipFree(enc->device_blob);
  if (enc->device_spans) (void)hipFree(enc->device_spans);
  delete enc;
}

size_t gfy_csr_workspace_bytes(int64_t n, int64_t e) {
  return csr_workspace_bytes(n < 1 ? 1 : n, e < 0 ? 0 : e);
}

int gfy_build_csr(const int32_t* edge_index, const uint8_t* edge_types,
                  int64_t n, int64_t e, int32_t* row_ptr, int32_t* col,
                  uint8_t* typ, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  GFY_REQUIRE(row_ptr && ws, GFY_ERR_INVALID, "gfy_build_csr: NULL output/workspace");
  GFY_REQUIRE(e == 0 || (edge_index && edge_types && col && typ), GFY_ERR_INVALID,
              "gfy_build_csr: NULL edge array with E=%lld", (long long)e);
  return launch_build_csr(edge_index, edge_types, n, e, row_ptr, col, typ, ws,
                          ws_bytes, (hipStream_t)stream);
}

int gfy_build_graphs(const uint8_t* bases, const uint8_t* marks, const int64_t* node_ptr,
                     const int64_t* edge_ptr, int64_t records, int64_t n, int64_t e,
                     int struct_states, int positional_columns, int skip2,
                     const float* positional, float* node_features, int32_t* edge_index,
                     uint8_t* edge_types, int32_t* first_invalid, void* stream) {
  clear_error();
  GFY_REQUIRE(records >= 0 && n >= 0 && n < INT32_MAX && e >= 0 && e < INT32_MAX,
              GFY_ERR_INVALID, "gfy_build_graphs: records=%lld n=%lld e=%lld out of range",
              (long long)records, (long long)n, (long long)e);
  GFY_REQUIRE(struct_states == 1 || struct_states == 3, GFY_ERR_INVALID,
              "gfy_build_graphs: struct_states must be 1 (paired flag) or 3 (one-hot)");
  GFY_REQUIRE(positional_columns == 0 || positional_columns == 2, GFY_ERR_INVALID,
              "gfy_build_graphs: positional_columns must be 0 or 2");
  GFY_REQUIRE(node_ptr && edge_ptr && first_invalid, GFY_ERR_INVALID,
              "gfy_build_graphs: NULL argument");
  GFY_REQUIRE(n == 0 || (bases && marks && node_features), GFY_ERR_INVALID,
              "gfy_build_graphs: NULL node array with N=%lld", (long long)n);
  GFY_REQUIRE(n == 0 || positional_columns == 0 || positional, GFY_ERR_INVALID,
              "gfy_build_graphs: positional columns requested but positional is NULL");
  GFY_REQUIRE(e == 0 || (edge_index && edge_types), GFY_ERR_INVALID,
              "gfy_build_graphs: NULL edge array with E=%lld", (long long)e);
  return launch_build_graphs(bases, marks, node_ptr, edge_ptr, records, n, e, struct_states,
                             positional_columns, skip2 ? 1 : 0, positional, node_features,
                             edge_index, edge_types, first_invalid, (hipStream_t)stream);
}

// ---- windowed records ---------------------------------------------------------------------
namespace {
int check_window_text(const char* who, const uint8_t* bases, const uint8_t* marks,
                      const int64_t* mol_ptr, int64_t molecules, int64_t molecule_nt,
                      const int32_t* rec_mol, const int32_t* rec_start, const int32_t* rec_end,
                      int64_t records, const void* ws, size_t ws_bytes) {
  GFY_REQUIRE(molecules >= 1 && molecules < INT32_MAX && molecule_nt >= 1 &&
                  molecule_nt < INT32_MAX && records >= 1 && records < INT32_MAX,
              GFY_ERR_INVALID, "%s: molecules=%lld nt=%lld records=%lld out of range", who,
              (long long)molecules, (long long)molecule_nt, (long long)records);
  GFY_REQUIRE(bases && marks && mol_ptr && rec_mol && rec_start && rec_end && ws,
              GFY_ERR_INVALID, "%s: NULL argument", who);
  const size_t need = gfy::window_workspace_bytes(molecules, molecule_nt, records);
  GFY_REQUIRE(ws_bytes >= need, GFY_ERR_WORKSPACE, "%s: workspace %zu < required %zu", who,
              ws_bytes, need);
  return GFY_OK;
}
}  // namespace

size_t gfy_window_workspace_bytes(int64_t n_molecules, int64_t molecule_nt, int64_t n_records) {
  if (n_molecules < 0 || molecule_nt < 0 || n_records < 0) return 0;
  return gfy::window_workspace_bytes(n_molecules, molecule_nt, n_records);
}

int gfy_window_select(const uint8_t* bases, const uint8_t* marks, const int64_t* mol_ptr,
                      int64_t molecules, int64_t molecule_nt, const int32_t* rec_mol,
                      const int32_t* rec_start, const int32_t* rec_end, int64_t records,
                      int keep_paired_neighbours, int context_hops, int skip2, int32_t* counts,
                      int32_t* first_invalid, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const int status = check_window_text("gfy_window_select", bases, marks, mol_ptr, molecules,
                                       molecule_nt, rec_mol, rec_start, rec_end, records, ws,
                                       ws_bytes);
  if (status != GFY_OK) return status;
  GFY_REQUIRE(context_hops >= 1, GFY_ERR_INVALID, "gfy_window_select: context_hops must be >= 1");
  GFY_REQUIRE(counts && first_invalid, GFY_ERR_INVALID, "gfy_window_select: NULL output");
  return launch_window_select(bases, marks, mol_ptr, molecules, molecule_nt, rec_mol, rec_start,
                              rec_end, records, keep_paired_neighbours ? 1 : 0, context_hops,
                              skip2 ? 1 : 0, counts, first_invalid, ws, (hipStream_t)stream);
}

int gfy_window_emit(const uint8_t* bases, const uint8_t* marks, const int64_t* mol_ptr,
                    int64_t molecules, int64_t molecule_nt, const int32_t* rec_mol,
                    const int32_t* rec_start, const int32_t* rec_end, int64_t records,
                    int64_t first_record, int64_t batch_records, const int64_t* node_ptr,
                    const int64_t* edge_ptr, const int64_t* core_ptr, int64_t n, int64_t e,
                    int64_t n_core, int struct_states, int positional_columns, int skip2,
                    const float* positional, float* node_features, int32_t* edge_index,
                    uint8_t* edge_types, int32_t* residue_index, uint8_t* node_roles,
                    int32_t* out_rows, int32_t* first_invalid, void* ws, size_t ws_bytes,
                    void* stream) {
  clear_error();
  const int status = check_window_text("gfy_window_emit", bases, marks, mol_ptr, molecules,
                                       molecule_nt, rec_mol, rec_start, rec_end, records, ws,
                                       ws_bytes);
  if (status != GFY_OK) return status;
  GFY_REQUIRE(first_record >= 0 && batch_records >= 1 && first_record + batch_records <= records,
              GFY_ERR_INVALID, "gfy_window_emit: records [%lld, +%lld) outside 0..%lld",
              (long long)first_record, (long long)batch_records, (long long)records);
  GFY_REQUIRE(n >= 1 && n < INT32_MAX && e >= 0 && e < INT32_MAX && n_core >= 0 && n_core <= n,
              GFY_ERR_INVALID, "gfy_window_emit: n=%lld e=%lld core=%lld out of range",
              (long long)n, (long long)e, (long long)n_core);
  GFY_REQUIRE(struct_states == 1 || struct_states == 3, GFY_ERR_INVALID,
              "gfy_window_emit: struct_states must be 1 (paired flag) or 3 (one-hot)");
  GFY_REQUIRE(positional_columns == 0 || positional_columns == 2, GFY_ERR_INVALID,
              "gfy_window_emit: positional_columns must be 0 or 2");
  GFY_REQUIRE(positional_columns == 0 || positional, GFY_ERR_INVALID,
              "gfy_window_emit: positional columns requested but positional is NULL");
  GFY_REQUIRE(node_ptr && edge_ptr && node_features && residue_index && node_roles &&
                  first_invalid && (e == 0 || (edge_index && edge_types)) &&
                  (!out_rows || core_ptr),
              GFY_ERR_INVALID, "gfy_window_emit: NULL argument");
  return launch_window_emit(bases, marks, mol_ptr, molecules, molecule_nt, rec_mol, rec_start,
                            rec_end, first_record, batch_records, node_ptr, edge_ptr, core_ptr, n,
                            e, n_core, struct_states, positional_columns, skip2 ? 1 : 0,
                            positional, node_features, edge_index, edge_types, residue_index,
                            node_roles, out_rows, first_invalid, ws, (hipStream_t)stream);
}

size_t gfy_encode_workspace_bytes(const gfy_encoder* enc, int64_t n, int64_t e) {
  if (!enc) return 0;
  n = n < 1 ? 1 : n;
  return enc->model_dtype == GFY_F16 ? encode_f16_workspace_bytes(n, e)
                                     : encode_f32_workspace_bytes(n, e);
}

static int encode_common(gfy_encoder* enc, const float* x, const int32_t* row_ptr,
                         const int32_t* col, const uint8_t* typ, int64_t n,
                         int64_t e, const int32_t* out_rows, void* out,
                         int out_dtype, int normalise, int tap, void* ws,
                         size_t ws_bytes, void* stream) {
  clear_error();
  GFY_REQUIRE(enc != nullptr, GFY_ERR_INVALID, "gfy_encode: encoder is NULL");
  GFY_REQUIRE(n > 0 && n < INT32_MAX && e >= 0 && e < INT32_MAX, GFY_ERR_INVALID,
              "gfy_encode: n=%lld e=%lld out of range", (long long)n, (long long)e);
  GFY_REQUIRE(x && row_ptr && out && ws, GFY_ERR_INVALID, "gfy_encode: NULL argument");
  GFY_REQUIRE(e == 0 || (col && typ), GFY_ERR_INVALID, "gfy_encode: NULL CSR arrays");
  GFY_REQUIRE(out_dtype == GFY_F16 || out_dtype == GFY_F32 || out_dtype == GFY_F64,
              GFY_ERR_INVALID, "gfy_encode: unsupported out_dtype %d", out_dtype);
  GFY_REQUIRE(tap < 0 || tap <= enc->layers, GFY_ERR_INVALID,
              "gfy_encode_hidden: stage %d outside 0..%d", tap, enc->layers);
  if (const int rc = check_current_device(enc, "gfy_encode")) return rc;
  enc->last_stream = (hipStream_t)stream;
  if (enc->model_dtype == GFY_F16)
    return launch_encode_f16(enc, x, row_ptr, col, typ, n, e, out_rows, out,
                             out_dtype, normalise, tap, ws, ws_bytes,
                             (hipStream_t)stream);
  return launch_encode_f32(enc, x, row_ptr, col, typ, n, e, out_rows, out,
                           out_dtype, normalise, tap, ws, ws_bytes,
                           (hipStream_t)stream);
}

static int64_t padded_rows(int64_t n) { return (n + 31) / 32 * 32; }   // whole 32-row tiles

size_t gfy_encode_coo_clear_bytes(int64_t n) { return csr_clear_bytes(padded_rows(n < 1 ? 1 : n)); }

// fp32 model: plain sequence (CSR build, then encode), CSR arrays in front
static size_t encode_coo_f32_workspace_bytes(int64_t n, int64_t e) {
  return align_up(csr_workspace_bytes(n, e), 256) + align_up((size_t)(n + 1) * 4, 256) +
         align_up((size_t)(e > 0 ? e : 1) * 4, 256) + align_up((size_t)(e > 0 ? e : 1), 256) +
         encode_f32_workspace_bytes(n, e);
}

size_t gfy_encode_coo_workspace_bytes(const gfy_encoder* enc, int64_t n, int64_t e) {
  if (!enc) return 0;
  n = n < 1 ? 1 : n;
  e = e < 0 ? 0 : e;
  if (enc->model_dtype == GFY_F16) return encode_coo_f16_workspace_bytes(padded_rows(n), e);
  return encode_coo_f32_workspace_bytes(n, e);
}

int gfy_encode_coo_prepare(void* ws, size_t ws_bytes, int64_t n, void* stream) {
  clear_error();
  GFY_REQUIRE(ws && n > 0 && n < INT32_MAX - 64, GFY_ERR_INVALID,
              "gfy_encode_coo_prepare: bad arguments");
  GFY_REQUIRE(ws_bytes >= csr_clear_bytes(padded_rows(n)), GFY_ERR_WORKSPACE,
              "gfy_encode_coo_prepare: workspace %zu < %zu", ws_bytes,
              csr_clear_bytes(padded_rows(n)));
  return launch_csr_clear(ws, padded_rows(n), (hipStream_t)stream);
}

// fp32 model (parity path, MFMA-bound): CSR build and encode behind one entry point
static int encode_coo_f32(gfy_encoder* enc, const float* x, const int32_t* edge_index,
                          const uint8_t* edge_types, int64_t n, int64_t e,
                          const int32_t* out_rows, void* out, int out_dtype, int normalise,
                          void* ws, size_t ws_bytes, hipStream_t stream) {
  char* at = (char*)ws;
  void* csr_ws = at;
  const size_t csr_bytes = align_up(csr_workspace_bytes(n, e), 256);
  at += csr_bytes;
  int32_t* row_ptr = (int32_t*)at;
  at += align_up((size_t)(n + 1) * 4, 256);
  int32_t* col = (int32_t*)at;
  at += align_up((size_t)(e > 0 ? e : 1) * 4, 256);
  uint8_t* typ = (uint8_t*)at;
  at += align_up((size_t)(e > 0 ? e : 1), 256);
  if (const int rc = launch_build_csr(edge_index, edge_types, n, e, row_ptr, col, typ, csr_ws,
                                      csr_bytes, stream))
    return rc;
  return launch_encode_f32(enc, x, row_ptr, col, typ, n, e, out_rows, out, out_dtype, normalise,
                           -1, at, ws_bytes - (size_t)(at - (char*)ws), stream);
}

int gfy_encode_coo(gfy_encoder* enc, const float* x, const int32_t* edge_index,
                   const uint8_t* edge_types, int64_t n, int64_t e, const int32_t* out_rows,
                   void* out, int out_dtype, int normalise, void* ws, size_t ws_bytes,
                   void* stream) {
  clear_error();
  GFY_REQUIRE(enc != nullptr, GFY_ERR_INVALID, "gfy_encode_coo: encoder is NULL");
  GFY_REQUIRE(n > 0 && n < INT32_MAX - 64 && e >= 0 && e < INT32_MAX, GFY_ERR_INVALID,
              "gfy_encode_coo: n=%lld e=%lld out of range", (long long)n, (long long)e);
  GFY_REQUIRE(x && out && ws, GFY_ERR_INVALID, "gfy_encode_coo: NULL argument");
  GFY_REQUIRE(e == 0 || (edge_index && edge_types), GFY_ERR_INVALID,
              "gfy_encode_coo: NULL edge array with E=%lld", (long long)e);
  GFY_REQUIRE(out_dtype == GFY_F16 || out_dtype == GFY_F32 || out_dtype == GFY_F64,
              GFY_ERR_INVALID, "gfy_encode_coo: unsupported out_dtype %d", out_dtype);
  const size_t need = gfy_encode_coo_workspace_bytes(enc, n, e);
  GFY_REQUIRE(ws_bytes >= need, GFY_ERR_WORKSPACE, "gfy_encode_coo: workspace %zu < required %zu",
              ws_bytes, need);
  if (const int rc = check_current_device(enc, "gfy_encode_coo")) return rc;
  enc->last_stream = (hipStream_t)stream;
  if (enc->model_dtype == GFY_F16)
    return launch_encode_coo_f16(enc, single_shard(x, edge_index, edge_types, n, e, out_rows, out),
                                 nullptr, out_dtype, normalise, ws, ws_bytes, (hipStream_t)stream);
  return encode_coo_f32(enc, x, edge_index, edge_types, n, e, out_rows, out, out_dtype, normalise,
                        ws, ws_bytes, (hipStream_t)stream);
}

// ---- a batch of shards in one sequence of launches ---------------------------------------
static int batch_table(const gfy_shard* shards, int count, const char* who, ShardTable* table,
                       RecordTable* records = nullptr, bool* has_records = nullptr) {
  GFY_REQUIRE(shards && count >= 1 && count <= GFY_MAX_BATCH_SHARDS, GFY_ERR_INVALID,
              "%s: 1..%d shards per call (got %d)", who, GFY_MAX_BATCH_SHARDS, count);
  ShardTable t{};
  t.shards = count;
  int64_t tiles = 0, edges = 0, blocks = 0;
  for (int s = 0; s < count; ++s) {
    const gfy_shard& one = shards[s];
    GFY_REQUIRE(one.n_nodes > 0 && one.n_edges >= 0, GFY_ERR_INVALID,
                "%s: shard %d has n=%lld e=%lld", who, s, (long long)one.n_nodes,
                (long long)one.n_edges);
    GFY_REQUIRE(one.node_features && one.out, GFY_ERR_INVALID, "%s: shard %d: NULL argument", who,
                s);
    GFY_REQUIRE(one.n_edges == 0 || (one.edge_index && one.edge_types), GFY_ERR_INVALID,
                "%s: shard %d: NULL edge array with E=%lld", who, s, (long long)one.n_edges);
    t.tile_base[s] = (int)tiles;
    t.edge_base[s] = (int)edges;
    t.count_block_base[s] = (int)blocks;
    t.nodes[s] = (int)one.n_nodes;
    t.edges[s] = (int)one.n_edges;
    t.x[s] = one.node_features;
    t.edge_index[s] = one.edge_index;
    t.edge_types[s] = one.edge_types;
    t.out_rows[s] = one.out_rows;
    t.out[s] = one.out;
    tiles += (one.n_nodes + 31) / 32;
    edges += one.n_edges;
    blocks += (one.n_edges + kCsrCountEdgesPerBlock - 1) / kCsrCountEdgesPerBlock;
    GFY_REQUIRE(tiles * 32 < kCsrMaxRows && edges < INT32_MAX, GFY_ERR_UNSUPPORTED,
                "%s: a batch holds at most 16,777,215 (padded) nodes and 2^31 - 1 edges", who);
  }
  t.tile_base[count] = (int)tiles;
  t.edge_base[count] = (int)edges;
  t.count_block_base[count] = (int)blocks;
  *table = t;
  if (records && has_records) {   // record boundaries: all shards or none
    RecordTable r{};
    bool all = true;
    int ranges = 0;
    r.range_rows = t.total_rows() <= kRecLoneBatchRows    ? kRecRowsLone
                   : t.total_rows() <= kRecSmallBatchRows ? kRecRowsSmall
                                                          : kRecRowsLarge;
    for (int s = 0; s < count; ++s) {
      const gfy_shard& one = shards[s];
      const bool given = one.node_ptr && one.edge_ptr && one.n_records > 0;
      GFY_REQUIRE(given || (!one.node_ptr && !one.edge_ptr), GFY_ERR_INVALID,
                  "%s: shard %d: node_ptr, edge_ptr and n_records go together", who, s);
      GFY_REQUIRE(!given || one.n_records <= one.n_nodes, GFY_ERR_INVALID,
                  "%s: shard %d: %lld records for %lld nodes", who, s, (long long)one.n_records,
                  (long long)one.n_nodes);
      all = all && given;
      r.node_ptr[s] = one.node_ptr;
      r.edge_ptr[s] = one.edge_ptr;
      r.records[s] = (int)one.n_records;
      r.range_base[s] = ranges;
      ranges += (int)((one.n_nodes + r.range_rows - 1) / r.range_rows);
    }
    r.range_base[count] = ranges;
    *records = r;
    *has_records = all;
  }
  return GFY_OK;
}

size_t gfy_encode_coo_batch_workspace_bytes(const gfy_encoder* enc, const gfy_shard* shards,
                                            int count) {
  clear_error();
  ShardTable t;
  if (!enc || batch_table(shards, count, "gfy_encode_coo_batch_workspace_bytes", &t)) return 0;
  if (enc->model_dtype == GFY_F16)
    return encode_coo_f16_workspace_bytes(t.total_rows(), t.total_edges());
  size_t most = 0;   // fp32 model: the shards run one after the other in one workspace
  for (int s = 0; s < count; ++s) {
    const size_t one = encode_coo_f32_workspace_bytes(shards[s].n_nodes, shards[s].n_edges);
    most = one > most ? one : most;
  }
  return most;
}

size_t gfy_encode_coo_batch_clear_bytes(const gfy_shard* shards, int count) {
  clear_error();
  ShardTable t;
  if (batch_table(shards, count, "gfy_encode_coo_batch_clear_bytes", &t)) return 0;
  return csr_clear_bytes(t.total_rows());
}

int gfy_encode_coo_batch(gfy_encoder* enc, const gfy_shard* shards, int count, int out_dtype,
                         int normalise, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  GFY_REQUIRE(enc != nullptr && ws != nullptr, GFY_ERR_INVALID,
              "gfy_encode_coo_batch: NULL encoder or workspace");
  GFY_REQUIRE(out_dtype == GFY_F16 || out_dtype == GFY_F32 || out_dtype == GFY_F64,
              GFY_ERR_INVALID, "gfy_encode_coo_batch: unsupported out_dtype %d", out_dtype);
  ShardTable t;
  RecordTable records;
  bool has_records = false;
  if (const int rc = batch_table(shards, count, "gfy_encode_coo_batch", &t, &records, &has_records))
    return rc;
  const size_t need = gfy_encode_coo_batch_workspace_bytes(enc, shards, count);
  GFY_REQUIRE(ws_bytes >= need, GFY_ERR_WORKSPACE,
              "gfy_encode_coo_batch: workspace %zu < required %zu", ws_bytes, need);
  if (const int rc = check_current_device(enc, "gfy_encode_coo_batch")) return rc;
  enc->last_stream = (hipStream_t)stream;
  if (enc->model_dtype == GFY_F16)
    return launch_encode_coo_f16(enc, t, has_records ? &records : nullptr, out_dtype, normalise, ws,
                                 ws_bytes, (hipStream_t)stream);
  for (int s = 0; s < count; ++s)
    if (const int rc = encode_coo_f32(enc, shards[s].node_features, shards[s].edge_index,
                                      shards[s].edge_types, shards[s].n_nodes, shards[s].n_edges,
                                      shards[s].out_rows, shards[s].out, out_dtype, normalise, ws,
                                      ws_bytes, (hipStream_t)stream))
      return rc;
  return GFY_OK;
}

int gfy_encode(gfy_encoder* enc, const float* x, const int32_t* row_ptr,
               const int32_t* col, const uint8_t* typ, int64_t n, int64_t e,
               const int32_t* out_rows, void* out, int out_dtype, int normalise,
               void* ws, size_t ws_bytes, void* stream) {
  return encode_common(enc, x, row_ptr, col, typ, n, e, out_rows, out, out_dtype,
                       normalise, -1, ws, ws_bytes, stream);
}

int gfy_encode_hidden(gfy_encoder* enc, const float* x, const int32_t* row_ptr,
                      const int32_t* col, const uint8_t* typ, int64_t n,
                      int64_t e, int stage, void* out, void* ws, size_t ws_bytes,
                      void* stream) {
  GFY_REQUIRE(stage >= 0, GFY_ERR_INVALID, "gfy_encode_hidden: negative stage");
  return encode_common(enc, x, row_ptr, col, typ, n, e, nullptr, out,
                       enc ? enc->model_dtype : GFY_F16, 0, stage, ws, ws_bytes,
                       stream);
}

size_t gfy_debug_layer_workspace_bytes(const gfy_encoder* enc, int64_t n, int64_t /*e*/) {
  if (!enc || enc->model_dtype != GFY_F16) return 0;
  return debug_layer_f16_workspace_bytes(n < 1 ? 1 : n);
}

int gfy_debug_layer(gfy_encoder* enc, int layer, const void* hidden_in, const int32_t* row_ptr,
                    const int32_t* col, const uint8_t* typ, int64_t n, int64_t e, int tap,
                    void* out, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  GFY_REQUIRE(enc != nullptr, GFY_ERR_INVALID, "gfy_debug_layer: encoder is NULL");
  GFY_REQUIRE(enc->model_dtype == GFY_F16, GFY_ERR_UNSUPPORTED,
              "gfy_debug_layer: fp16 model only");
  GFY_REQUIRE(layer >= 0 && layer < enc->layers, GFY_ERR_INVALID,
              "gfy_debug_layer: layer %d outside 0..%d", layer, enc->layers - 1);
  GFY_REQUIRE(tap >= GFY_TAP_H && tap <= GFY_TAP_Y, GFY_ERR_INVALID,
              "gfy_debug_layer: unknown tap %d", tap);
  GFY_REQUIRE(n > 0 && n < INT32_MAX - 64 && e >= 0 && e < INT32_MAX, GFY_ERR_INVALID,
              "gfy_debug_layer: n=%lld e=%lld out of range", (long long)n, (long long)e);
  GFY_REQUIRE(hidden_in && row_ptr && out && ws && (e == 0 || (col && typ)), GFY_ERR_INVALID,
              "gfy_debug_layer: NULL argument");
  if (const int rc = check_current_device(enc, "gfy_debug_layer")) return rc;
  enc->last_stream = (hipStream_t)stream;
  return launch_debug_layer_f16(enc, layer, hidden_in, row_ptr, col, typ, n, e, tap, out, ws,
                                ws_bytes, (hipStream_t)stream);
}

int gfy_pairwise_dense(const void* a, int64_t n, const void* b, int64_t m,
                       int metric, float* out, void* ws, size_t ws_bytes,
                       void* stream) {
  clear_error();
  GFY_REQUIRE(a && b && out && ws && n > 0 && m > 0, GFY_ERR_INVALID,
              "gfy_pairwise_dense: bad arguments");
  GFY_REQUIRE(metric == GFY_L2 || metric == GFY_COSINE, GFY_ERR_INVALID,
              "gfy_pairwise_dense: unknown metric %d", metric);
  return launch_pairwise_dense(a, n, b, m, metric, out, ws, ws_bytes, (hipStream_t)stream);
}

size_t gfy_pairwise_workspace_bytes(int64_t n, int64_t m) {
  return pairwise_workspace_bytes(n < 1 ? 1 : n, m < 1 ? 1 : m);
}

// the checks the nearest and top-k calls share, in the style of check_record_call below; `who`
// names the call in the message
static int check_pairwise_call(const char* who, const void* a, int64_t n, const void* b, int64_t m,
                               int metric, const void* out_val, const void* out_idx,
                               const void* ws) {
  GFY_REQUIRE(a && b && out_val && out_idx && ws && n > 0 && m > 0 && m < INT32_MAX,
              GFY_ERR_INVALID, "%s: bad arguments", who);
  GFY_REQUIRE(metric == GFY_L2 || metric == GFY_COSINE, GFY_ERR_INVALID, "%s: unknown metric %d",
              who, metric);
  return GFY_OK;
}

static int check_topk_k(const char* who, int k, int most) {
  GFY_REQUIRE(k >= 1 && k <= most, GFY_ERR_INVALID, "%s: k = %d outside 1..%d", who, k, most);
  return GFY_OK;
}

static int check_pairwise_window(const char* who, int64_t window_first, int64_t n, int64_t m) {
  GFY_REQUIRE(window_first >= 0 && window_first + m <= n, GFY_ERR_INVALID,
              "%s: b must be rows [%lld, %lld) of the %lld rows of a", who, (long long)window_first,
              (long long)(window_first + m), (long long)n);
  return GFY_OK;
}

int gfy_pairwise_nearest(const void* a, int64_t n, const void* b, int64_t m,
                         int metric, int64_t exclude_offset, float* best_val,
                         int32_t* best_idx, void* ws, size_t ws_bytes,
                         void* stream) {
  clear_error();
  if (const int rc = check_pairwise_call("gfy_pairwise_nearest", a, n, b, m, metric, best_val,
                                         best_idx, ws))
    return rc;
  return launch_pairwise_nearest(a, n, b, m, metric, exclude_offset, exclude_offset >= 0 ? 1 : 0,
                                 best_val, best_idx, ws, ws_bytes, (hipStream_t)stream);
}

int gfy_pairwise_nearest_window(const void* a, int64_t n, const void* b, int64_t m, int metric,
                                int64_t window_first, float* best_val, int32_t* best_idx,
                                void* ws, size_t ws_bytes, void* stream) {
  const char* who = "gfy_pairwise_nearest_window";
  clear_error();
  if (const int rc = check_pairwise_call(who, a, n, b, m, metric, best_val, best_idx, ws))
    return rc;
  if (const int rc = check_pairwise_window(who, window_first, n, m)) return rc;
  return launch_pairwise_nearest(a, n, b, m, metric, -window_first, 1, best_val, best_idx, ws,
                                 ws_bytes, (hipStream_t)stream);
}

size_t gfy_pairwise_topk_workspace_bytes(int64_t n, int64_t m, int k) {
  k = k < 1 ? 1 : k > GFY_PAIRWISE_TOPK_MAX ? GFY_PAIRWISE_TOPK_MAX : k;
  return pairwise_topk_workspace_bytes(n < 1 ? 1 : n, m < 1 ? 1 : m, k);
}

int gfy_pairwise_topk(const void* a, int64_t n, const void* b, int64_t m, int metric, int k,
                      int64_t exclude_offset, float* top_val, int32_t* top_idx, void* ws,
                      size_t ws_bytes, void* stream) {
  const char* who = "gfy_pairwise_topk";
  clear_error();
  if (const int rc = check_pairwise_call(who, a, n, b, m, metric, top_val, top_idx, ws)) return rc;
  if (const int rc = check_topk_k(who, k, GFY_PAIRWISE_TOPK_MAX)) return rc;
  return launch_pairwise_topk(a, n, b, m, metric, k, exclude_offset, exclude_offset >= 0 ? 1 : 0,
                              nullptr, nullptr, nullptr, nullptr, top_val, top_idx, ws, ws_bytes,
                              (hipStream_t)stream);
}

int gfy_pairwise_topk_window(const void* a, int64_t n, const void* b, int64_t m, int metric,
                             int k, int64_t window_first, float* top_val, int32_t* top_idx,
                             void* ws, size_t ws_bytes, void* stream) {
  const char* who = "gfy_pairwise_topk_window";
  clear_error();
  if (const int rc = check_pairwise_call(who, a, n, b, m, metric, top_val, top_idx, ws)) return rc;
  if (const int rc = check_topk_k(who, k, GFY_PAIRWISE_TOPK_MAX)) return rc;
  if (const int rc = check_pairwise_window(who, window_first, n, m)) return rc;
  return launch_pairwise_topk(a, n, b, m, metric, k, -window_first, 1, nullptr, nullptr, nullptr,
                              nullptr, top_val, top_idx, ws, ws_bytes, (hipStream_t)stream);
}

int gfy_pairwise_topk_ranges(const void* a, int64_t n, const void* b, int64_t m, int metric, int k,
                             const int32_t* skip_lo, const int32_t* skip_hi, float* top_val,
                             int32_t* top_idx, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "gfy_pairwise_topk_ranges";
  clear_error();
  if (const int rc = check_pairwise_call(who, a, n, b, m, metric, top_val, top_idx, ws)) return rc;
  if (const int rc = check_topk_k(who, k, GFY_PAIRWISE_TOPK_MAX)) return rc;
  GFY_REQUIRE(skip_lo && skip_hi, GFY_ERR_INVALID, "%s: skip_lo or skip_hi is NULL", who);
  return launch_pairwise_topk(a, n, b, m, metric, k, 0, 0, skip_lo, skip_hi, nullptr, nullptr,
                              top_val, top_idx, ws, ws_bytes, (hipStream_t)stream);
}

int gfy_pairwise_topk_distinct(const void* a, int64_t n, const void* b, int64_t m, int metric, int k,
                               const int32_t* skip_lo, const int32_t* skip_hi,
                               const int32_t* group_lo, const int32_t* group_hi, float* top_val,
                               int32_t* top_idx, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "gfy_pairwise_topk_distinct";
  clear_error();
  if (const int rc = check_pairwise_call(who, a, n, b, m, metric, top_val, top_idx, ws)) return rc;
  if (const int rc = check_topk_k(who, k, GFY_PAIRWISE_TOPK_DISTINCT_MAX)) return rc;
  GFY_REQUIRE(skip_lo && skip_hi, GFY_ERR_INVALID, "%s: skip_lo or skip_hi is NULL", who);
  GFY_REQUIRE(group_lo && group_hi, GFY_ERR_INVALID, "%s: group_lo or group_hi is NULL", who);
  return launch_pairwise_topk(a, n, b, m, metric, k, 0, 0, skip_lo, skip_hi, group_lo, group_hi,
                              top_val, top_idx, ws, ws_bytes, (hipStream_t)stream);
}

size_t gfy_pairwise_record_workspace_bytes(int64_t n, int64_t m, int64_t records_a,
                                           int64_t records_b) {
  (void)records_a;   // the scores need nothing per record of a
  return pairwise_record_workspace_bytes(n < 1 ? 1 : n, m < 1 ? 1 : m,
                                         records_b < 1 ? 1 : records_b);
}

int gfy_pairwise_record_chunks(int64_t n, int64_t m) {
  return pairwise_record_chunks(n < 1 ? 1 : n, m < 1 ? 1 : m);
}

// the checks the two record calls share; `who` names the call in the message
static int check_record_call(const char* who, const void* a, int64_t n, const void* b, int64_t m,
                             int metric, const int32_t* ptr_b, int64_t records_b, const void* out,
                             const char* out_name, const void* ws) {
  GFY_REQUIRE(a, GFY_ERR_INVALID, "%s: a is NULL", who);
  GFY_REQUIRE(b, GFY_ERR_INVALID, "%s: b is NULL", who);
  GFY_REQUIRE(ptr_b, GFY_ERR_INVALID, "%s: ptr_b is NULL", who);
  GFY_REQUIRE(out, GFY_ERR_INVALID, "%s: %s is NULL", who, out_name);
  GFY_REQUIRE(ws, GFY_ERR_INVALID, "%s: workspace is NULL", who);
  GFY_REQUIRE(n > 0 && m > 0 && n < INT32_MAX && m < INT32_MAX, GFY_ERR_INVALID,
              "%s: bad arguments: n = %lld, m = %lld", who, (long long)n, (long long)m);
  GFY_REQUIRE(records_b > 0 && records_b <= GFY_PAIRWISE_RECORDS_MAX, GFY_ERR_INVALID,
              "%s: records_b = %lld outside 1..%d", who, (long long)records_b,
              GFY_PAIRWISE_RECORDS_MAX);
  GFY_REQUIRE(metric == GFY_L2 || metric == GFY_COSINE, GFY_ERR_INVALID, "%s: unknown metric %d",
              who, metric);
  return GFY_OK;
}

int gfy_pairwise_record_best(const void* a, int64_t n, const void* b, int64_t m, int metric,
                             const int32_t* ptr_b, int64_t records_b, float* out_best, void* ws,
                             size_t ws_bytes, void* stream) {
  clear_error();
  if (const int rc = check_record_call("gfy_pairwise_record_best", a, n, b, m, metric, ptr_b,
                                       records_b, out_best, "out_best", ws))
    return rc;
  return launch_pairwise_records(a, n, b, m, metric, nullptr, 0, ptr_b, records_b, out_best, ws,
                                 ws_bytes, (hipStream_t)stream);
}

int gfy_pairwise_record_scores(const void* a, int64_t n, const void* b, int64_t m, int metric,
                               const int32_t* ptr_a, int64_t records_a, const int32_t* ptr_b,
                               int64_t records_b, float* out_scores, void* ws, size_t ws_bytes,
                               void* stream) {
  clear_error();
  GFY_REQUIRE(ptr_a, GFY_ERR_INVALID, "gfy_pairwise_record_scores: ptr_a is NULL");
  if (const int rc = check_record_call("gfy_pairwise_record_scores", a, n, b, m, metric, ptr_b,
                                       records_b, out_scores, "out_scores", ws))
    return rc;
  GFY_REQUIRE(records_a > 0 && records_a < INT32_MAX, GFY_ERR_INVALID,
              "gfy_pairwise_record_scores: records_a = %lld outside 1..2^31 - 2",
              (long long)records_a);
  return launch_pairwise_records(a, n, b, m, metric, ptr_a, records_a, ptr_b, records_b,
                                 out_scores, ws, ws_bytes, (hipStream_t)stream);
}

size_t gfy_pairwise_within_workspace_bytes(int64_t n, int64_t m) {
  return pairwise_within_workspace_bytes(n < 1 ? 1 : n, m < 1 ? 1 : m);
}

int gfy_pairwise_within_chunks(int64_t n, int64_t m) {
  return pairwise_within_chunks(n < 1 ? 1 : n, m < 1 ? 1 : m);
}

// what the two radius calls check behind check_pairwise_call
static int check_within_call(const char* who, int64_t n, float threshold, const int32_t* skip_lo,
                             const int32_t* skip_hi) {
  GFY_REQUIRE(n < INT32_MAX, GFY_ERR_INVALID, "%s: n = %lld outside 1..2^31 - 2", who,
              (long long)n);
  GFY_REQUIRE(__builtin_isfinite(threshold), GFY_ERR_INVALID, "%s: threshold is not finite", who);
  GFY_REQUIRE((skip_lo == nullptr) == (skip_hi == nullptr), GFY_ERR_INVALID,
              "%s: skip_lo and skip_hi go together (both NULL: no exclusion)", who);
  return GFY_OK;
}

int gfy_pairwise_within_count(const void* a, int64_t n, const void* b, int64_t m, int metric,
                              float threshold, const int32_t* skip_lo, const int32_t* skip_hi,
                              int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "gfy_pairwise_within_count";
  clear_error();
  if (const int rc = check_pairwise_call(who, a, n, b, m, metric, counts, counts, ws)) return rc;
  if (const int rc = check_within_call(who, n, threshold, skip_lo, skip_hi)) return rc;
  return launch_pairwise_within(a, n, b, m, metric, threshold, skip_lo, skip_hi, counts, nullptr,
                                nullptr, nullptr, nullptr, ws, ws_bytes, (hipStream_t)stream);
}

int gfy_pairwise_within_fill(const void* a, int64_t n, const void* b, int64_t m, int metric,
                             float threshold, const int32_t* skip_lo, const int32_t* skip_hi,
                             const int64_t* offsets, int32_t* indices, float* values,
                             int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "gfy_pairwise_within_fill";
  clear_error();
  if (const int rc = check_pairwise_call(who, a, n, b, m, metric, values, indices, ws)) return rc;
  GFY_REQUIRE(offsets && status, GFY_ERR_INVALID, "%s: offsets or status is NULL", who);
  if (const int rc = check_within_call(who, n, threshold, skip_lo, skip_hi)) return rc;
  return launch_pairwise_within(a, n, b, m, metric, threshold, skip_lo, skip_hi, nullptr, offsets,
                                indices, values, status, ws, ws_bytes, (hipStream_t)stream);
}

// The 14 values every alignment call of the ABI starts with, in the order of include/gfy.h, and
// an output pointer with the name a refusal gives it.
struct AlignAbi {
  const void* a;
  int64_t n;
  const int32_t* ptr_a;
  int64_t records_a;
  const void* b;
  int64_t m;
  const int32_t* ptr_b;
  int64_t records_b;
  const int32_t* pairs;
  int64_t P;
  float match_scale, match_shift, gap_open, gap_extend;
};
struct NamedOutput {
  const void* pointer;
  const char* name;
  bool has = true;   // the call has this pointer at all
};

// The argument rules every alignment call (gfy_align_local to gfy_align_global_trace_box) shares, in one
// order (the outputs in the order given), and the call record the launchers take: `call` gets
// every field that comes from the 14 values; the outputs are the entry point's, carry and cap the
// launcher's.
static int checked_align_call(const char* who, const AlignAbi& v,
                              const NamedOutput* outputs, size_t count, const void* ws,
                              AlignArgs* call, bool has_workspace = true) {
  GFY_REQUIRE(v.a, GFY_ERR_INVALID, "%s: a is NULL", who);
  GFY_REQUIRE(v.b, GFY_ERR_INVALID, "%s: b is NULL", who);
  GFY_REQUIRE(v.ptr_a, GFY_ERR_INVALID, "%s: ptr_a is NULL", who);
  GFY_REQUIRE(v.ptr_b, GFY_ERR_INVALID, "%s: ptr_b is NULL", who);
  GFY_REQUIRE(v.pairs, GFY_ERR_INVALID, "%s: pairs is NULL", who);
  for (const NamedOutput* out = outputs; out != outputs + count; ++out)
    GFY_REQUIRE(out->pointer || !out->has, GFY_ERR_INVALID, "%s: %s is NULL", who, out->name);
  GFY_REQUIRE(ws || !has_workspace, GFY_ERR_INVALID, "%s: workspace is NULL", who);
  GFY_REQUIRE(v.n > 0 && v.m > 0 && v.n < INT32_MAX && v.m < INT32_MAX, GFY_ERR_INVALID,
              "%s: bad arguments: n = %lld, m = %lld", who, (long long)v.n, (long long)v.m);
  GFY_REQUIRE(v.records_a > 0 && v.records_a < INT32_MAX && v.records_b > 0 &&
                  v.records_b < INT32_MAX,
              GFY_ERR_INVALID, "%s: records_a = %lld, records_b = %lld outside 1..2^31 - 2", who,
              (long long)v.records_a, (long long)v.records_b);
  GFY_REQUIRE(v.P >= 1 && v.P <= INT32_MAX, GFY_ERR_INVALID, "%s: P = %lld outside 1..2^31 - 1",
              who, (long long)v.P);
  GFY_REQUIRE(std::isfinite(v.match_scale) && std::isfinite(v.match_shift) &&
                  std::isfinite(v.gap_open) && std::isfinite(v.gap_extend),
              GFY_ERR_INVALID, "%s: match_scale, match_shift, gap_open and gap_extend must be finite",
              who);
  GFY_REQUIRE(0.0f <= v.gap_extend && v.gap_extend <= v.gap_open, GFY_ERR_INVALID,
              "%s: 0 <= gap_extend <= gap_open required, got gap_open = %g, gap_extend = %g", who,
              (double)v.gap_open, (double)v.gap_extend);
  *call = AlignArgs{};
  call->a = (const f16*)v.a;
  call->b = (const f16*)v.b;
  call->ptr_a = v.ptr_a;
  call->ptr_b = v.ptr_b;
  call->pairs = v.pairs;
  call->n = v.n;
  call->m = v.m;
  call->P = v.P;
  call->records_a = (int)v.records_a;
  call->records_b = (int)v.records_b;
  call->match_scale = v.match_scale;
  call->match_shift = v.match_shift;
  call->gap_open = v.gap_open;
  call->gap_extend = v.gap_extend;
  return GFY_OK;
}

static int64_t clipped_align_rows(int64_t max_rows_b) {
  return max_rows_b < 0 ? 0 : max_rows_b > GFY_ALIGN_ROWS_MAX ? GFY_ALIGN_ROWS_MAX : max_rows_b;
}

size_t gfy_align_workspace_bytes(int64_t pairs, int64_t max_rows_b) {
  return align_workspace_bytes(pairs < 1 ? 1 : pairs, clipped_align_rows(max_rows_b));
}

size_t gfy_align_span_workspace_bytes(int64_t pairs, int64_t max_rows_b) {
  return align_span_workspace_bytes(pairs < 1 ? 1 : pairs, clipped_align_rows(max_rows_b));
}

size_t gfy_align_trace_workspace_bytes(int64_t pairs, int64_t max_box_rows, int64_t max_box_cols) {
  return align_trace_workspace_bytes(pairs < 1 ? 1 : pairs, clipped_align_rows(max_box_rows),
                                     clipped_align_rows(max_box_cols));
}

size_t gfy_align_global_trace_workspace_bytes(int64_t pairs, int64_t max_rows_a,
                                              int64_t max_rows_b) {
  return gfy_align_trace_workspace_bytes(pairs, max_rows_a, max_rows_b);
}

// One of the twelve launch entry points (gfy_align_local to gfy_align_global_trace_box), described:
// its name, its mode (the kernel, and which of the fields below the call has), the 14 values and
// what follows them in the signature, as given.  A field that the mode does not have stays zero.
struct AlignEntry {
  const char* who;
  unsigned mode;        // AlignMode bits
  const char* plain;    // the call without the band (kBand) or box (kBox) that this one requires,
                        // which a NULL one is told; kOrder requires neither
  AlignAbi v;
  const int32_t* bands;
  const int32_t* boxes;
  float* out_score;
  int32_t* out_end;
  AlignExtras extras;   // the trace's pointers, order and order_ptr, out_start, within, and the two
                        // maxima of a trace as given
  int64_t shuffles;
};
#define GFY_ALIGN_VALUES                                                                    \
  {a, n, ptr_a, records_a, b, m, ptr_b, records_b, pairs, P, match_scale, match_shift, gap_open, \
   gap_extend}

// Every check of such an entry point, in the one order all of them keep: the band or box that the
// call requires, the pointers a trace call names first, the shared rules (a score call's outputs
// between `pairs` and the workspace), `within`, the maxima or the shuffles; then the call record
// and the launcher, which checks the workspace's size.
static int align_entry(AlignEntry& e, void* ws, size_t ws_bytes, void* stream) {
  const char* who = e.who;
  const bool span = e.mode & kSpan, trace = e.mode & kTrace, global = e.mode & kGlobal;
  const bool order = e.mode & kOrder;
  clear_error();
  if (!order && (e.mode & kBox)) {
    GFY_REQUIRE(e.boxes, GFY_ERR_INVALID,
                "%s: boxes is NULL (int32 [P][4] of (i_lo, i_hi, j_lo, j_hi) rows in device "
                "memory; %s is the call without a box)", who, e.plain);
  } else if (!order && (e.mode & kBand)) {
    GFY_REQUIRE(e.bands, GFY_ERR_INVALID,
                "%s: bands is NULL (int32 [P][2] of (lo, hi) diagonals in device memory; %s is "
                "the call without a band)", who, e.plain);
  }
  // every pointer a call can name, in the order that all of them keep, and whether this one does
  const TraceArgs& t = e.extras.trace;
  const NamedOutput all[] = {{t.starts, "starts", trace && !global},
                             {t.ends, "ends", trace},
                             {t.op_ptr, "op_ptr", trace},
                             {t.out_ops, "out_ops", trace},
                             {t.out_len, "out_len", trace},
                             {e.extras.orders.order, "order", order},
                             {e.extras.orders.order_ptr, "order_ptr", order},
                             {e.out_score, "out_score", !trace},
                             {e.extras.out_start, "out_start", span || (trace && global)},
                             {e.out_end, "out_end", !trace && !order}};
  if (trace)
    for (const NamedOutput& named : all)
      GFY_REQUIRE(named.pointer || !named.has, GFY_ERR_INVALID, "%s: %s is NULL", who, named.name);
  AlignArgs call;   // a trace's pointers are named above: none is left to the shared check
  if (const int rc = checked_align_call(who, e.v, all, trace ? 0 : std::size(all), ws, &call))
    return rc;
  if (global)
    GFY_REQUIRE(e.extras.within == 0 || e.extras.within == 1, GFY_ERR_INVALID,
                "%s: within = %d is neither 0 nor 1", who, e.extras.within);
  if (trace)
    GFY_REQUIRE(e.extras.max_box_rows >= 0 && e.extras.max_box_cols >= 0, GFY_ERR_INVALID,
                "%s: %s = %lld, %s = %lld are negative", who,
                global ? "max_rows_a" : "max_box_rows", (long long)e.extras.max_box_rows,
                global ? "max_rows_b" : "max_box_cols", (long long)e.extras.max_box_cols);
  if (order) {
    GFY_REQUIRE(e.shuffles >= 1, GFY_ERR_INVALID, "%s: shuffles = %lld is below 1", who,
                (long long)e.shuffles);
    GFY_REQUIRE(e.shuffles <= INT32_MAX / e.v.P, GFY_ERR_INVALID,
                "%s: P * shuffles = %lld * %lld outside 1..2^31 - 1", who, (long long)e.v.P,
                (long long)e.shuffles);
    e.extras.orders.shuffles = (int)e.shuffles;
  }
  call.bands = e.bands;
  call.boxes = e.boxes;
  call.out_score = e.out_score;
  call.out_end = e.out_end;
  e.extras.max_box_rows = clipped_align_rows(e.extras.max_box_rows);
  e.extras.max_box_cols = clipped_align_rows(e.extras.max_box_cols);
  return launch_align(e.mode, call, e.extras, ws, ws_bytes, (hipStream_t)stream);
}

int gfy_align_local(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                    const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                    const int32_t* pairs, int64_t P, float match_scale, float match_shift,
                    float gap_open, float gap_extend, float* out_score, int32_t* out_end,
                    void* ws, size_t ws_bytes, void* stream) {
  AlignEntry e{"gfy_align_local", 0, nullptr, GFY_ALIGN_VALUES};
  e.out_score = out_score, e.out_end = out_end;
  return align_entry(e, ws, ws_bytes, stream);
}

int gfy_align_local_span(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                         const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                         const int32_t* pairs, int64_t P, float match_scale, float match_shift,
                         float gap_open, float gap_extend, float* out_score, int32_t* out_start,
                         int32_t* out_end, void* ws, size_t ws_bytes, void* stream) {
  AlignEntry e{"gfy_align_local_span", kSpan, nullptr, GFY_ALIGN_VALUES};
  e.out_score = out_score, e.extras.out_start = out_start, e.out_end = out_end;
  return align_entry(e, ws, ws_bytes, stream);
}

int gfy_align_trace(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                    const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                    const int32_t* pairs, int64_t P, float match_scale, float match_shift,
                    float gap_open, float gap_extend, const int32_t* starts, const int32_t* ends,
                    const int64_t* op_ptr, uint8_t* out_ops, int32_t* out_len,
                    int64_t max_box_rows, int64_t max_box_cols, void* ws, size_t ws_bytes,
                    void* stream) {
  AlignEntry e{"gfy_align_trace", kTrace, nullptr, GFY_ALIGN_VALUES};
  e.extras.trace = {starts, ends, op_ptr, out_ops, out_len};
  e.extras.max_box_rows = max_box_rows, e.extras.max_box_cols = max_box_cols;
  return align_entry(e, ws, ws_bytes, stream);
}

// The three local calls inside a band per pair: their counterpart's checks in its order, with
// `bands` named first.
int gfy_align_local_band(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                         const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                         const int32_t* pairs, int64_t P, float match_scale, float match_shift,
                         float gap_open, float gap_extend, const int32_t* bands, float* out_score,
                         int32_t* out_end, void* ws, size_t ws_bytes, void* stream) {
  AlignEntry e{"gfy_align_local_band", kBand, "gfy_align_local", GFY_ALIGN_VALUES, bands};
  e.out_score = out_score, e.out_end = out_end;
  return align_entry(e, ws, ws_bytes, stream);
}

int gfy_align_local_span_band(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                              const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                              const int32_t* pairs, int64_t P, float match_scale,
                              float match_shift, float gap_open, float gap_extend,
                              const int32_t* bands, float* out_score, int32_t* out_start,
                              int32_t* out_end, void* ws, size_t ws_bytes, void* stream) {
  AlignEntry e{"gfy_align_local_span_band", kSpan | kBand, "gfy_align_local_span",
               GFY_ALIGN_VALUES, bands};
  e.out_score = out_score, e.extras.out_start = out_start, e.out_end = out_end;
  return align_entry(e, ws, ws_bytes, stream);
}

int gfy_align_trace_band(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                         const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                         const int32_t* pairs, int64_t P, float match_scale, float match_shift,
                         float gap_open, float gap_extend, const int32_t* bands,
                         const int32_t* starts, const int32_t* ends, const int64_t* op_ptr,
                         uint8_t* out_ops, int32_t* out_len, int64_t max_box_rows,
                         int64_t max_box_cols, void* ws, size_t ws_bytes, void* stream) {
  AlignEntry e{"gfy_align_trace_band", kTrace | kBand, "gfy_align_trace", GFY_ALIGN_VALUES, bands};
  e.extras.trace = {starts, ends, op_ptr, out_ops, out_len};
  e.extras.max_box_rows = max_box_rows, e.extras.max_box_cols = max_box_cols;
  return align_entry(e, ws, ws_bytes, stream);
}

// The score and span calls inside a box of rows per pair: the banded call's checks in its order,
// with `boxes` named first and `bands` free to be NULL (no band).
int gfy_align_local_box(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                        const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                        const int32_t* pairs, int64_t P, float match_scale, float match_shift,
                        float gap_open, float gap_extend, const int32_t* bands,
                        const int32_t* boxes, float* out_score, int32_t* out_end, void* ws,
                        size_t ws_bytes, void* stream) {
  AlignEntry e{"gfy_align_local_box", kBand | kBox, "gfy_align_local_band", GFY_ALIGN_VALUES,
               bands, boxes};
  e.out_score = out_score, e.out_end = out_end;
  return align_entry(e, ws, ws_bytes, stream);
}

int gfy_align_local_span_box(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                             const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                             const int32_t* pairs, int64_t P, float match_scale,
                             float match_shift, float gap_open, float gap_extend,
                             const int32_t* bands, const int32_t* boxes, float* out_score,
                             int32_t* out_start, int32_t* out_end, void* ws, size_t ws_bytes,
                             void* stream) {
  AlignEntry e{"gfy_align_local_span_box", kSpan | kBand | kBox, "gfy_align_local_span_band",
               GFY_ALIGN_VALUES, bands, boxes};
  e.out_score = out_score, e.extras.out_start = out_start, e.out_end = out_end;
  return align_entry(e, ws, ws_bytes, stream);
}

// Null scores: the boxed score call's checks in its order with `bands` and `boxes` both free to
// be NULL, the orders named like outputs, and then what the virtual pairs add.
int gfy_align_local_null(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                         const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                         const int32_t* pairs, int64_t P, float match_scale, float match_shift,
                         float gap_open, float gap_extend, const int32_t* bands,
                         const int32_t* boxes, int64_t shuffles, const int32_t* order,
                         const int64_t* order_ptr, float* out_score, void* ws, size_t ws_bytes,
                         void* stream) {
  AlignEntry e{"gfy_align_local_null", kBand | kBox | kOrder, nullptr, GFY_ALIGN_VALUES, bands,
               boxes};
  e.shuffles = shuffles, e.extras.orders = {order, order_ptr};
  e.out_score = out_score;
  return align_entry(e, ws, ws_bytes, stream);
}

int gfy_align_global(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                     const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                     const int32_t* pairs, int64_t P, float match_scale, float match_shift,
                     float gap_open, float gap_extend, int within, float* out_score,
                     int32_t* out_end, void* ws, size_t ws_bytes, void* stream) {
  AlignEntry e{"gfy_align_global", kGlobal, nullptr, GFY_ALIGN_VALUES};
  e.extras.within = within, e.out_score = out_score, e.out_end = out_end;
  return align_entry(e, ws, ws_bytes, stream);
}

int gfy_align_global_trace(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                           const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                           const int32_t* pairs, int64_t P, float match_scale, float match_shift,
                           float gap_open, float gap_extend, int within, const int32_t* ends,
                           const int64_t* op_ptr, uint8_t* out_ops, int32_t* out_len,
                           int32_t* out_start, int64_t max_rows_a, int64_t max_rows_b, void* ws,
                           size_t ws_bytes, void* stream) {
  AlignEntry e{"gfy_align_global_trace", kTrace | kGlobal, nullptr, GFY_ALIGN_VALUES};
  e.extras.within = within, e.extras.out_start = out_start;
  e.extras.trace = {nullptr, ends, op_ptr, out_ops, out_len};
  e.extras.max_box_rows = max_rows_a, e.extras.max_box_cols = max_rows_b;
  return align_entry(e, ws, ws_bytes, stream);
}

// The two global calls inside a box of rows per pair: their counterpart's checks in its order,
// with `boxes` named first.  There is no band.
int gfy_align_global_box(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                         const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                         const int32_t* pairs, int64_t P, float match_scale, float match_shift,
                         float gap_open, float gap_extend, int within, const int32_t* boxes,
                         float* out_score, int32_t* out_end, void* ws, size_t ws_bytes,
                         void* stream) {
  AlignEntry e{"gfy_align_global_box", kGlobal | kBox, "gfy_align_global", GFY_ALIGN_VALUES,
               nullptr, boxes};
  e.extras.within = within, e.out_score = out_score, e.out_end = out_end;
  return align_entry(e, ws, ws_bytes, stream);
}

int gfy_align_global_trace_box(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                               const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                               const int32_t* pairs, int64_t P, float match_scale,
                               float match_shift, float gap_open, float gap_extend, int within,
                               const int32_t* boxes, const int32_t* ends, const int64_t* op_ptr,
                               uint8_t* out_ops, int32_t* out_len, int32_t* out_start,
                               int64_t max_rows_a, int64_t max_rows_b, void* ws, size_t ws_bytes,
                               void* stream) {
  AlignEntry e{"gfy_align_global_trace_box", kTrace | kGlobal | kBox, "gfy_align_global_trace",
               GFY_ALIGN_VALUES, nullptr, boxes};
  e.extras.within = within, e.extras.out_start = out_start;
  e.extras.trace = {nullptr, ends, op_ptr, out_ops, out_len};
  e.extras.max_box_rows = max_rows_a, e.extras.max_box_cols = max_rows_b;
  return align_entry(e, ws, ws_bytes, stream);
}

// The values of given paths (align_values.hip): the shared checks of the alignment calls, the
// pointers of its own named in its own order, and no workspace.
int gfy_align_path_values(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                          const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                          const int32_t* pairs, int64_t P, float match_scale, float match_shift,
                          float gap_open, float gap_extend, const int32_t* starts,
                          const int64_t* op_ptr, const uint8_t* ops, int64_t n_ops,
                          float* out_cosine, float* out_running, float* out_score,
                          int32_t* out_counts, double* out_cosine_sum, int64_t max_waves,
                          void* stream) {
  clear_error();
  AlignArgs call;
  const NamedOutput named[] = {
      {starts, "starts"}, {op_ptr, "op_ptr"}, {ops, "ops"}, {out_cosine, "out_cosine"},
      {out_running, "out_running"}, {out_score, "out_score"}, {out_counts, "out_counts"},
      {out_cosine_sum, "out_cosine_sum"}};
  if (const int rc = checked_align_call("gfy_align_path_values", GFY_ALIGN_VALUES, named,
                                        std::size(named), nullptr, &call, false))
    return rc;
  GFY_REQUIRE(n_ops >= 0, GFY_ERR_INVALID, "gfy_align_path_values: n_ops = %lld is negative",
              (long long)n_ops);
  GFY_REQUIRE(max_waves >= 0, GFY_ERR_INVALID,
              "gfy_align_path_values: max_waves = %lld is negative", (long long)max_waves);
  PathValueArgs values{};
  values.starts = starts;
  values.op_ptr = op_ptr;
  values.ops = ops;
  values.n_ops = n_ops;
  values.out_cosine = out_cosine;
  values.out_running = out_running;
  values.out_score = out_score;
  values.out_counts = out_counts;
  values.out_cosine_sum = out_cosine_sum;
  return launch_align_path_values(call, values, max_waves, (hipStream_t)stream);
}

}  // extern "C"
