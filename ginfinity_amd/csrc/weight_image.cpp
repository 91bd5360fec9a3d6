// What the kernels read, derived from a weight pack on the host, once per encoder
// (weight_image.h).  No HIP call.
//
// Reference behaviour reproduced here:
//   model.half()                       src/ginfinity/api.py:111-112
//   edge_lin on a one-hot row          src/ginfinity/_model.py:43   -> 10-row table
//   (1 + eps) formed in fp16           src/ginfinity/_model.py:46
//   BatchNorm1d eval affine in fp32    src/ginfinity/_model.py:35
// The rounding points follow SURVEY.md §8-A / oracle/gine_numpy.py.
// Compiled with -ffp-contract=off: alpha/shift must round after every step.
#include "weight_image.h"

#include <cmath>
#include <cstring>

namespace gfy {

void pack_b_fragments(const f16* w, int n_out, int k_in, f16* frag) {
  const int tiles = n_out / 32, ksteps = k_in / 16;
  for (int tile = 0; tile < tiles; ++tile)
    for (int ks = 0; ks < ksteps; ++ks)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j)
          frag[(((size_t)tile * ksteps + ks) * 64 + lane) * 8 + j] =
              w[(size_t)(32 * tile + (lane & 31)) * k_in + 16 * ks +
                8 * (lane >> 5) + j];
}

void pack_k_chained(const f16* w, int n_out, int k_in, f16* frag) {
  const int blocks = n_out / 32, ksteps = k_in / 16;
  for (int blk = 0; blk < blocks; ++blk)
    for (int s = 0; s < ksteps; ++s)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j)
          frag[(((size_t)blk * ksteps + s) * 64 + lane) * 8 + j] =
              w[(size_t)(32 * blk + (lane & 31)) * k_in + 16 * s + 8 * (j >> 2) +
                4 * (lane >> 5) + (j & 3)];
}

void pack_chain_fragments(const f16* w, int n_out, int k_in, f16* frag) {
  const int blocks = n_out / 32, ksteps = k_in / 16;
  for (int blk = 0; blk < blocks; ++blk)
    for (int s = 0; s < ksteps; ++s)
      for (int lane = 0; lane < 64; ++lane) {
        const int m = lane & 31, half = lane >> 5;
        const int reg = (m & 3) + 4 * (m >> 3), row_half = (m >> 2) & 1;   // C/D row m
        const int out_channel = 32 * blk + 16 * (reg >> 3) + 8 * row_half + (reg & 7);
        for (int j = 0; j < 8; ++j) {
          const int k = 16 * s + 8 * (j >> 2) + 4 * half + (j & 3);
          frag[(((size_t)blk * ksteps + s) * 64 + lane) * 8 + j] =
              w[(size_t)out_channel * k_in + k];
        }
      }
}

namespace {

constexpr int H = kHidden, M = kMlp;

inline f16 rh(float v) { return (f16)v; }  // RNE, as torch's .half()

std::vector<f16> halves(const float* w, size_t count) {
  std::vector<f16> out(count);
  for (size_t i = 0; i < count; ++i) out[i] = rh(w[i]);
  return out;
}

// put(at, c) for every channel c of `channels`, at = its position as [block][lane half][register]
// of an MFMA result
template <typename Put>
void in_gemm_result_order(int channels, Put&& put) {
  for (int blk = 0; blk < channels / 32; ++blk)
    for (int half = 0; half < 2; ++half)
      for (int reg = 0; reg < 16; ++reg)
        put((blk * 2 + half) * 16 + reg, gemm_result_channel(blk, half, reg));
}

size_t put_copy(Blob& blob, const float* src, size_t n) {
  const size_t off = blob.reserve(n * 4);
  std::memcpy(blob.at<float>(off), src, n * 4);
  return off;
}

size_t put_transposed(Blob& blob, const float* src, int rows, int cols) {   // -> [cols][rows]
  const size_t off = blob.reserve((size_t)rows * cols * 4);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c)
      blob.at<float>(off)[(size_t)c * rows + r] = src[(size_t)r * cols + c];
  return off;
}

}  // namespace

// ---- fp16 model ------------------------------------------------------------------------------
InputOff put_input_f16(Blob& blob, const PackView& pack) {
  InputOff o;
  o.w = blob.reserve((size_t)H * 8 * sizeof(f16));
  o.b = blob.reserve(H * sizeof(f16));
  for (int p = 0; p < H; ++p) {
    // stored position p holds channel stored_channel(p); packed [p & 7][p >> 3][k]: see
    // k_input_linear_f16
    const int c = stored_channel(p);
    for (int k = 0; k < kInDim; ++k)
      blob.at<f16>(o.w)[((p & 7) * 16 + (p >> 3)) * 8 + k] = rh(pack.w_in[c * kInDim + k]);
    blob.at<f16>(o.b)[p] = rh(pack.b_in[c]);
  }
  return o;
}

LayerF16Off put_layer_f16(Blob& blob, const PackLayer& layer, int edge_dim) {
  LayerF16Off o;
  o.scale = (float)rh(1.0f + (float)rh(layer.eps[0]));  // fp16 scalar (1 + eps)
  // [W0 | W1] fragments: every B operand of the layer kernel is an MFMA result (or a
  // stored row, which has the same order) used in place
  o.w01 = blob.reserve((size_t)2 * M * H * sizeof(f16));
  pack_k_chained(halves(layer.w0, (size_t)M * H).data(), M, H, blob.at<f16>(o.w01));
  pack_k_chained(halves(layer.w1, (size_t)H * M).data(), H, M, blob.at<f16>(o.w01) + (size_t)M * H);
  // LDS image of gine_layer.inc, in the order its lanes read it (layer_image.h)
  o.image = blob.reserve(kImageBytes);
  char* im = blob.at<char>(o.image);
  f16* table = reinterpret_cast<f16*>(im + kImageTable);   // [17][128], stored order
  for (int t = 0; t < edge_dim; ++t)
    for (int p = 0; p < H; ++p) {   // R(R(W[c][t]) + R(b[c]))  — one-hot Linear
      const int c = stored_channel(p);
      table[t * H + p] = rh((float)rh(layer.edge_w[c * edge_dim + t]) + (float)rh(layer.edge_b[c]));
    }
  for (int p = 0; p < H; ++p) table[kMaxEdgeTypes * H + p] = (f16)(-INFINITY);
  float* alpha_out = reinterpret_cast<float*>(im + kImageAlpha);
  float* shift_out = reinterpret_cast<float*>(im + kImageShift);
  in_gemm_result_order(M, [&](int at, int c) {
    const float g = (float)rh(layer.bn_gamma[c]), b = (float)rh(layer.bn_beta[c]);
    const float mean = (float)rh(layer.bn_mean[c]), var = (float)rh(layer.bn_var[c]);
    const float invstd = 1.0f / std::sqrt(var + 1e-5f);
    const float alpha = invstd * g;
    const float prod = mean * alpha;  // separate rounding (no fma)
    alpha_out[at] = alpha;
    shift_out[at] = b - prod;
  });
  // b0 and b1 are added on the matrix cores (gine_layer.inc, mlp_pipe_step): natural channel
  // order — row lane % 32 of A-operand block b is channel 32 b + row
  f16* b0 = reinterpret_cast<f16*>(im + kImageB0);
  f16* b1 = reinterpret_cast<f16*>(im + kImageB1);
  for (int c = 0; c < M; ++c) b0[c] = rh(layer.b0[c]);
  for (int c = 0; c < H; ++c) b1[c] = rh(layer.b1[c]);
  f16* gamma = reinterpret_cast<f16*>(im + kImageGamma);
  f16* beta = reinterpret_cast<f16*>(im + kImageBeta);
  in_gemm_result_order(H, [&](int at, int c) {
    gamma[at] = rh(layer.ln_gamma[c]);
    beta[at] = rh(layer.ln_beta[c]);
  });
  return o;
}

HeadF16Off put_head_f16(Blob& blob, const PackView& pack) {
  HeadF16Off o;
  // stand-alone head kernel: reads stored rows (k chained), writes natural rows
  o.wa = blob.reserve((size_t)H * H * sizeof(f16));
  pack_k_chained(halves(pack.wa, (size_t)H * H).data(), H, H, blob.at<f16>(o.wa));
  // fused head: head.0 k-chained, head.2 chained with its rows dealt into natural chunks
  o.w_image = blob.reserve((size_t)2 * H * H * sizeof(f16));
  std::memcpy(blob.at<f16>(o.w_image), blob.at<f16>(o.wa), (size_t)H * H * sizeof(f16));
  const std::vector<f16> wb = halves(pack.wb, (size_t)kOutDim * H);
  o.wb = blob.reserve(wb.size() * sizeof(f16));
  pack_b_fragments(wb.data(), kOutDim, H, blob.at<f16>(o.wb));
  pack_chain_fragments(wb.data(), kOutDim, H, blob.at<f16>(o.w_image) + (size_t)H * H);
  o.ba = blob.reserve(H * sizeof(f16));
  o.bb = blob.reserve(kOutDim * sizeof(f16));
  for (int c = 0; c < H; ++c) blob.at<f16>(o.ba)[c] = rh(pack.ba[c]);
  for (int c = 0; c < kOutDim; ++c) blob.at<f16>(o.bb)[c] = rh(pack.bb[c]);
  o.image = blob.reserve(kHeadImageBytes);
  f16* image_ba = reinterpret_cast<f16*>(blob.at<char>(o.image) + kHeadImageBa);
  f16* image_bb = reinterpret_cast<f16*>(blob.at<char>(o.image) + kHeadImageBb);
  in_gemm_result_order(H, [&](int at, int c) { image_ba[at] = blob.at<f16>(o.ba)[c]; });
  for (int half = 0; half < 2; ++half)
    for (int ks = 0; ks < 8; ++ks)
      for (int j = 0; j < 8; ++j)
        image_bb[(half * 8 + ks) * 8 + j] = blob.at<f16>(o.bb)[hidden_layout_channel(half, ks, j)];
  return o;
}

ImageF16 build_image_f16(Blob& blob, const PackView& pack) {
  ImageF16 o{};
  o.input = put_input_f16(blob, pack);
  for (int l = 0; l < pack.layers; ++l)
    o.layer[l] = put_layer_f16(blob, pack.layer[l], pack.edge_dim);
  o.head = put_head_f16(blob, pack);
  return o;
}

// ---- fp32 model ------------------------------------------------------------------------------
InputOff put_input_f32(Blob& blob, const PackView& pack) {
  InputOff o;
  o.w = put_transposed(blob, pack.w_in, H, kInDim);   // -> [K][N]
  o.b = put_copy(blob, pack.b_in, H);
  return o;
}

LayerF32Off put_layer_f32(Blob& blob, const PackLayer& layer, int edge_dim) {
  LayerF32Off o;
  o.one_plus_eps = 1.0f + layer.eps[0];
  o.table = blob.reserve((size_t)kMaxEdgeTypes * H * 4);
  for (int t = 0; t < edge_dim; ++t)
    for (int c = 0; c < H; ++c)
      blob.at<float>(o.table)[t * H + c] = layer.edge_w[c * edge_dim + t] + layer.edge_b[c];
  o.w0t = put_transposed(blob, layer.w0, M, H);   // -> [H][M]
  o.b0 = put_copy(blob, layer.b0, M);
  o.alpha = blob.reserve(M * 4);
  o.shift = blob.reserve(M * 4);
  for (int c = 0; c < M; ++c) {
    const float invstd = 1.0f / std::sqrt(layer.bn_var[c] + 1e-5f);
    const float alpha = invstd * layer.bn_gamma[c];
    const float prod = layer.bn_mean[c] * alpha;
    blob.at<float>(o.alpha)[c] = alpha;
    blob.at<float>(o.shift)[c] = layer.bn_beta[c] - prod;
  }
  o.w1t = put_transposed(blob, layer.w1, H, M);   // -> [M][H]
  o.b1 = put_copy(blob, layer.b1, H);
  o.ln_g = put_copy(blob, layer.ln_gamma, H);
  o.ln_b = put_copy(blob, layer.ln_beta, H);
  return o;
}

HeadF32Off put_head_f32(Blob& blob, const PackView& pack) {
  HeadF32Off o;
  o.wa_t = put_transposed(blob, pack.wa, H, H);
  o.wb_t = put_transposed(blob, pack.wb, kOutDim, H);
  o.ba = put_copy(blob, pack.ba, H);
  o.bb = put_copy(blob, pack.bb, kOutDim);
  return o;
}

ImageF32 build_image_f32(Blob& blob, const PackView& pack) {
  ImageF32 o{};
  o.input = put_input_f32(blob, pack);
  for (int l = 0; l < pack.layers; ++l)
    o.layer[l] = put_layer_f32(blob, pack.layer[l], pack.edge_dim);
  o.head = put_head_f32(blob, pack);
  return o;
}

}  // namespace gfy
