// Host-side derivation of everything the kernels read from a weight pack, laid out in one
// staging image of the device blob (weight_image.cpp).  No HIP call: gfy_encoder_create uploads
// the image and turns the offsets below into pointers; tools/weight_image_dump.cpp writes it
// to a file.  Needs _Float16 on the host (hipcc, or the clang it drives).
#pragma once

#include <cstddef>
#include <vector>

#include "layer_image.h"

namespace gfy {

typedef _Float16 f16;

// Hidden rows are stored with the channel groups 4-7 and 8-11 of every 16 swapped: 16-byte
// chunk 2 s + hq of a row is then the eight values lane half hq holds for k-step s in the
// MFMA C/D layout, so activations move between memory, LDS and MFMA operands as whole chunks.
inline int stored_channel(int position) {   // an involution: bits 2 and 3 trade places
  return (position & ~12) | ((position & 4) << 1) | ((position & 8) >> 1);
}
inline int gemm_result_channel(int block, int half, int reg) {   // 32x32 C/D layout
  return 32 * block + (reg & 3) + 8 * (reg >> 2) + 4 * half;
}
inline int hidden_layout_channel(int half, int ks, int j) { return 16 * ks + 8 * half + j; }

// W[n_out][k_in] (row-major fp16) -> fragments of the MFMA 32x32x16 A operand (out^T = W . in^T):
// frag[(block * ksteps + s) * 64 + lane][j] = W[row(block, lane & 31)][k(s, lane >> 5, j)]
//   pack_b_fragments      natural:  row = 32 block + m,  k = 16 s + 8 half + j
//   pack_k_chained        the B operand is an MFMA result used in place (gine_layer.inc):
//                         k = 16 s + 8 (j >> 2) + 4 half + (j & 3), rows natural
//   pack_chain_fragments  same k; rows dealt so that the result's registers are natural
//                         16-byte chunks of the output row (head.2 -> embedding)
void pack_b_fragments(const f16* w, int n_out, int k_in, f16* frag);
void pack_k_chained(const f16* w, int n_out, int k_in, f16* frag);
void pack_chain_fragments(const f16* w, int n_out, int k_in, f16* frag);

// bump allocator over the host staging image of the device blob: 256-byte aligned, zero-filled
struct Blob {
  std::vector<char> host;
  size_t reserve(size_t bytes) {
    const size_t at = (host.size() + 255) / 256 * 256;
    host.resize(at + bytes, 0);
    return at;
  }
  template <typename T>
  T* at(size_t off) { return reinterpret_cast<T*>(host.data() + off); }
};

// ---- where each part lies in the blob (bytes); the members follow ModelF16 / ModelF32 --------
struct InputOff { size_t w, b; };
struct LayerF16Off {
  size_t w01, image;
  float scale;           // fp16 value R(1 + R(eps)) widened to fp32
};
struct HeadF16Off { size_t wa, ba, wb, bb, w_image, image; };
struct ImageF16 {
  InputOff input;
  LayerF16Off layer[kMaxLayers];
  HeadF16Off head;
};

struct LayerF32Off {
  size_t table, w0t, b0, alpha, shift, w1t, b1, ln_g, ln_b;
  float one_plus_eps;
};
struct HeadF32Off { size_t wa_t, ba, wb_t, bb; };
struct ImageF32 {
  InputOff input;
  LayerF32Off layer[kMaxLayers];
  HeadF32Off head;
};

// fp16 model (model.half(): parameters and BatchNorm buffers rounded to fp16 first)
InputOff put_input_f16(Blob& blob, const PackView& pack);
LayerF16Off put_layer_f16(Blob& blob, const PackLayer& layer, int edge_dim);
HeadF16Off put_head_f16(Blob& blob, const PackView& pack);
// fp32 (full_precision) model
InputOff put_input_f32(Blob& blob, const PackView& pack);
LayerF32Off put_layer_f32(Blob& blob, const PackLayer& layer, int edge_dim);
HeadF32Off put_head_f32(Blob& blob, const PackView& pack);
// a whole model: input Linear, the pack's layers, head, in that order
ImageF16 build_image_f16(Blob& blob, const PackView& pack);
ImageF32 build_image_f32(Blob& blob, const PackView& pack);

}  // namespace gfy
