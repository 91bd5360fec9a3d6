// The weight pack (include/gfy.h; written by ginfinity_amd/weights.py): its header, its field
// order and every check a loader makes before it reads a float, stated ONCE for libgfy.so and
// libgfy_host.so (implementation: gfy_base.cpp).  Plain C++: the host library builds with the
// host compiler alone.
#pragma once

#include <cstddef>
#include <cstdint>

namespace gfy {

// ---- model geometry compiled into the kernels and the host loops ------------------------
constexpr int kHidden = 128;   // data/model.json:12
constexpr int kMlp = 256;      // 2 * hidden       (_model.py:34)
constexpr int kInDim = 7;      // node features    (graph.py:91-93)
constexpr int kOutDim = 128;
constexpr int kMaxEdgeTypes = 16;
constexpr int kMaxLayers = 8;

constexpr uint32_t kPackMagic = 0x31594647u;   // 'GFY1'
constexpr uint32_t kPackVersion = 1;

struct PackHeader {
  uint32_t magic, version, in_dim, hidden, layers, edge_dim, out_dim, flags;
};
static_assert(sizeof(PackHeader) == 32, "the floats start 32 bytes into the pack");

// One layer's arrays in pack order (H = hidden, M = 2 H), fp32 exactly as the checkpoint has them
struct PackLayer {
  const float* eps;                                      // [1]
  const float *edge_w, *edge_b;                          // edge_lin: [H][edge_dim], [H]
  const float *w0, *b0;                                  // mlp.0: [M][H], [M]
  const float *bn_gamma, *bn_beta, *bn_mean, *bn_var;    // mlp.1 (BatchNorm1d): [M] each
  const float *w1, *b1;                                  // mlp.4: [H][M], [H]
  const float *ln_gamma, *ln_beta;                       // norms: [H] each
};

// Named pointers into a pack the caller keeps alive; filled by read_weight_pack alone
struct PackView {
  int layers, edge_dim, residual;
  const float *w_in, *b_in;          // input Linear: [H][in_dim], [H]
  PackLayer layer[kMaxLayers];
  const float *wa, *ba, *wb, *bb;    // head.0: [H][H], [H]; head.2: [out_dim][H], [out_dim]
};

// Floats behind the header.  Computed by the walk that fills a PackView, run over no pack at
// all: the size and the field order cannot drift apart.
size_t pack_floats(uint32_t in_dim, uint32_t hidden, uint32_t layers, uint32_t edge_dim,
                   uint32_t out_dim);

// Checks a caller's pack and model dtype and fills `view`.  GFY_OK, or — with the error text
// set, prefixed by `who` — GFY_ERR_UNSUPPORTED for an architecture the kernels are not built
// for and GFY_ERR_INVALID for everything else (missing / truncated pack, magic, version, byte
// count, model dtype).
int read_weight_pack(const char* who, const void* pack, size_t bytes, int model_dtype,
                     PackView* view);

}  // namespace gfy
