// The device blob of an encoder, built on the host and written to a file — no HIP, no GPU:
//
//   weight_image_dump PACK f16|f32 OUT
//
// reads the weight pack PACK (ginfinity_amd/weights.py, build_weight_pack) through the
// library's own reader (weight_pack.h) and derivation (weight_image.h), writes the image
// gfy_encoder_create would upload to OUT and prints layer_image.h's figures and where every
// part lies in the blob, one "name value" per line.  Built by tools/build_tools.sh with the
// ROCm clang (which has _Float16 on the host) and the library's floating-point flags;
// tests/test_weight_image_host.py pins the images' SHA-256.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../include/gfy.h"
#include "../ginfinity_amd/csrc/weight_image.h"

using namespace gfy;

static void line(const std::string& name, size_t value) {
  std::printf("%s %zu\n", name.c_str(), value);
}

int main(int argc, char** argv) {
  const std::string dtype = argc == 4 ? argv[2] : "";
  if (dtype != "f16" && dtype != "f32") {
    std::fprintf(stderr, "usage: weight_image_dump PACK f16|f32 OUT\n");
    return 2;
  }
  std::ifstream in(argv[1], std::ios::binary);
  const std::vector<char> bytes((std::istreambuf_iterator<char>(in)),
                                std::istreambuf_iterator<char>());
  PackView pack;
  if (read_weight_pack("weight_image_dump", bytes.data(), bytes.size(),
                       dtype == "f16" ? GFY_F16 : GFY_F32, &pack) != GFY_OK) {
    std::fprintf(stderr, "%s\n", gfy_last_error());
    return 1;
  }
  line("image.table", kImageTable);
  line("image.alpha", kImageAlpha);
  line("image.shift", kImageShift);
  line("image.b0", kImageB0);
  line("image.b1", kImageB1);
  line("image.gamma", kImageGamma);
  line("image.beta", kImageBeta);
  line("image.bytes", kImageBytes);
  line("head_image.ba", kHeadImageBa);
  line("head_image.bb", kHeadImageBb);
  line("head_image.bytes", kHeadImageBytes);

  Blob blob;
  if (dtype == "f16") {
    const ImageF16 o = build_image_f16(blob, pack);
    line("input.w", o.input.w);
    line("input.b", o.input.b);
    for (int l = 0; l < pack.layers; ++l) {
      const std::string name = "layer" + std::to_string(l) + ".";
      line(name + "w01", o.layer[l].w01);
      line(name + "image", o.layer[l].image);
    }
    line("head.wa", o.head.wa);
    line("head.ba", o.head.ba);
    line("head.wb", o.head.wb);
    line("head.bb", o.head.bb);
    line("head.w_image", o.head.w_image);
    line("head.image", o.head.image);
  } else {
    const ImageF32 o = build_image_f32(blob, pack);
    line("input.w", o.input.w);
    line("input.b", o.input.b);
    for (int l = 0; l < pack.layers; ++l) {
      const std::string name = "layer" + std::to_string(l) + ".";
      const LayerF32Off& at = o.layer[l];
      line(name + "table", at.table);
      line(name + "w0t", at.w0t);
      line(name + "b0", at.b0);
      line(name + "alpha", at.alpha);
      line(name + "shift", at.shift);
      line(name + "w1t", at.w1t);
      line(name + "b1", at.b1);
      line(name + "ln_g", at.ln_g);
      line(name + "ln_b", at.ln_b);
    }
    line("head.wa_t", o.head.wa_t);
    line("head.ba", o.head.ba);
    line("head.wb_t", o.head.wb_t);
    line("head.bb", o.head.bb);
  }
  line("blob.bytes", blob.host.size());
  std::ofstream out(argv[3], std::ios::binary);
  out.write(blob.host.data(), (std::streamsize)blob.host.size());
  return out.good() ? 0 : 1;
}
