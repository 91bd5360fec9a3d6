// The constant images the fp16 layer kernels copy into LDS, as byte offsets from an image's
// start: the ONE definition the host writes through (weight_image.cpp) and the kernels read
// through (gine_layer.inc: kLdsImage + offset).  Plain C++.
#pragma once

#include "weight_pack.h"

namespace gfy {

// ---- per-layer image (LayerF16::image) ---------------------------------------------------
constexpr int kImageTable = 0;                        // 17 x 256 B edge table, stored order
constexpr int kImageAlpha = kImageTable + (kMaxEdgeTypes + 1) * kHidden * 2;
                                                      // f32 [8][2][16]   MFMA result order
constexpr int kImageShift = kImageAlpha + kMlp * 4;
constexpr int kImageB0 = kImageShift + kMlp * 4;      // f16 [256]        natural channel order
                                                      //                  (bias MFMAs)
constexpr int kImageB1 = kImageB0 + kMlp * 2;         // f16 [128]        natural channel order
constexpr int kImageGamma = kImageB1 + kHidden * 2;
constexpr int kImageBeta = kImageGamma + kHidden * 2;
constexpr int kImageBytes = kImageBeta + kHidden * 2;   // 7,680

// ---- head image (HeadF16::image), in LDS right behind the layer's ------------------------
constexpr int kHeadImageBa = 0;                             // f16 [4][2][16]  MFMA result order
constexpr int kHeadImageBb = kHeadImageBa + kHidden * 2;    // f16 [2][8][8]   natural 16-B chunks
constexpr int kHeadImageBytes = kHeadImageBb + kOutDim * 2;   // 512

}  // namespace gfy
