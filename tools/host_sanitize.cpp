// The library's host C++ driven from a program of its own, so that it can be built with
// -fsanitize=address,undefined or -fsanitize=thread (tests/test_host_sanitizers.py) — no HIP,
// no Python, no GPU:
//
//   host_sanitize pack|microbatch|encode|threads CASEDIR
//
// CASEDIR holds what tests/host_sanitize_cases.py wrote: `data.bin` (plain binary arrays, back
// to back) and `manifest.txt`, one case per block:
//
//   case NAME
//   int KEY VALUE            ints KEY COUNT V0 V1 ...
//   array KEY OFFSET BYTES   (a range of data.bin)
//   text KEY REST OF LINE
//   end
//
// Every case is run and every result compared with the expected bytes and status of the case:
// the sanitized build is a correctness run too.  One "ok SUBCOMMAND NAME" line per case; the
// first mismatch prints "FAIL ..." and exits 1.  Every buffer a call reads or writes is a heap
// allocation of exactly the bytes the call is entitled to (never a part of a larger arena), so
// the sanitizer's red zones start at its first and behind its last byte.
//
// Built from this file, csrc/gfy_base.cpp and csrc/gine_host.cpp with any C++17 compiler and the
// library's floating-point flags.  The image derivation (csrc/weight_image.cpp) is run under
// the same sanitizers through tools/weight_image_dump.cpp.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <sstream>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../include/gfy.h"

namespace {

struct Case {
  std::string name;
  std::map<std::string, std::vector<int64_t>> ints;
  std::map<std::string, std::pair<size_t, size_t>> arrays;   // offset, bytes in data.bin
  std::map<std::string, std::string> texts;

  bool has(const std::string& key) const { return ints.count(key) != 0; }
  int64_t get(const std::string& key, int64_t otherwise = 0) const {
    auto at = ints.find(key);
    return at == ints.end() ? otherwise : at->second.at(0);
  }
  std::string text(const std::string& key) const {
    auto at = texts.find(key);
    return at == texts.end() ? std::string() : at->second;
  }
};

std::vector<char> g_data;
std::string g_command;

[[noreturn]] void fail(const Case& c, const std::string& why) {
  std::printf("FAIL %s %s: %s\n", g_command.c_str(), c.name.c_str(), why.c_str());
  std::fflush(stdout);
  std::exit(1);
}

std::string join(std::initializer_list<std::string> parts) {
  std::string out;
  for (const auto& part : parts) out += part;
  return out;
}

// An exact heap copy of one array of the case; absent -> NULL (malloc(0) is a valid pointer
// without one accessible byte).
struct Exact {
  void* p = nullptr;
  size_t bytes = 0;
  Exact() = default;
  Exact(const Case& c, const std::string& key) {
    auto at = c.arrays.find(key);
    if (at == c.arrays.end()) return;
    bytes = at->second.second;
    p = std::malloc(bytes);
    if (bytes) std::memcpy(p, g_data.data() + at->second.first, bytes);
  }
  Exact(Exact&& other) noexcept : p(other.p), bytes(other.bytes) { other.p = nullptr; }
  Exact(const Exact&) = delete;
  Exact& operator=(const Exact&) = delete;
  ~Exact() { std::free(p); }
  template <typename T> const T* as() const { return static_cast<const T*>(p); }
};

std::vector<Case> read_manifest(const std::string& directory) {
  std::ifstream data(directory + "/data.bin", std::ios::binary);
  g_data.assign(std::istreambuf_iterator<char>(data), std::istreambuf_iterator<char>());
  std::ifstream in(directory + "/manifest.txt");
  if (!in) {
    std::fprintf(stderr, "host_sanitize: no manifest.txt in %s\n", directory.c_str());
    std::exit(2);
  }
  std::vector<Case> cases;
  std::string line;
  bool open = false;
  while (std::getline(in, line)) {
    std::istringstream words(line);
    std::string kind, key;
    words >> kind;
    if (kind.empty()) continue;
    if (kind == "case") {
      cases.emplace_back();
      words >> cases.back().name;
      open = true;
      continue;
    }
    if (!open) {
      std::fprintf(stderr, "host_sanitize: '%s' outside a case\n", line.c_str());
      std::exit(2);
    }
    Case& c = cases.back();
    if (kind == "end") {
      open = false;
    } else if (kind == "int") {
      int64_t value = 0;
      words >> key >> value;
      c.ints[key] = {value};
    } else if (kind == "ints") {
      size_t count = 0;
      words >> key >> count;
      std::vector<int64_t> values(count);
      for (auto& v : values) words >> v;
      c.ints[key] = values;
    } else if (kind == "array") {
      size_t offset = 0, bytes = 0;
      words >> key >> offset >> bytes;
      if (offset + bytes > g_data.size()) {
        std::fprintf(stderr, "host_sanitize: array %s of %s leaves data.bin\n", key.c_str(),
                     c.name.c_str());
        std::exit(2);
      }
      c.arrays[key] = {offset, bytes};
    } else if (kind == "text") {
      words >> key;
      std::string rest;
      std::getline(words, rest);
      c.texts[key] = rest.empty() ? rest : rest.substr(1);
    } else {
      std::fprintf(stderr, "host_sanitize: unknown manifest line '%s'\n", line.c_str());
      std::exit(2);
    }
    if (!words && kind != "text") {
      std::fprintf(stderr, "host_sanitize: malformed manifest line '%s'\n", line.c_str());
      std::exit(2);
    }
  }
  return cases;
}

// What every call leaves in the error channel: text on a failure (with the words the case
// names), nothing after a success.
void check_status(const Case& c, int status, const std::string& where = "") {
  const int want = (int)c.get("status");
  const std::string text = gfy_last_error();
  if (status != want)
    fail(c, join({where, "status ", std::to_string(status), ", expected ", std::to_string(want),
                  " (", text, ")"}));
  if (status == GFY_OK && !text.empty()) fail(c, join({where, "error text after a success: ", text}));
  if (status != GFY_OK && text.empty()) fail(c, join({where, "no error text with a failure"}));
  if (status != GFY_OK && text.find(c.text("error")) == std::string::npos)
    fail(c, join({where, "error text '", text, "' lacks '", c.text("error"), "'"}));
}

// ---- pack: read_weight_pack through gfy_host_encoder_create ----------------------------------
// The case's pack cut or zero-extended to `length` bytes, header word `word` set to `value`.
Exact mutated_pack(const Case& c) {
  Exact pack;
  if (c.get("null_pack")) return pack;
  const Exact whole(c, "pack");
  pack.bytes = (size_t)c.get("length", (int64_t)whole.bytes);
  pack.p = std::calloc(pack.bytes ? pack.bytes : 1, 1);
  if (!pack.bytes) {   // (calloc(0) may be NULL, and NULL is a case of its own)
    std::free(pack.p);
    pack.p = std::malloc(0);
  }
  std::memcpy(pack.p, whole.p, pack.bytes < whole.bytes ? pack.bytes : whole.bytes);
  const int64_t word = c.get("word", -1);
  if (word >= 0 && pack.bytes >= (size_t)(4 * word + 4)) {
    const uint32_t value = (uint32_t)c.get("value");
    std::memcpy(static_cast<char*>(pack.p) + 4 * word, &value, 4);
  }
  return pack;
}

void run_pack(const Case& c) {
  const Exact pack = mutated_pack(c);
  gfy_host_encoder* encoder = reinterpret_cast<gfy_host_encoder*>(0x1);   // must be overwritten
  const size_t bytes = c.get("null_pack") ? (size_t)c.get("length") : pack.bytes;
  const int status = gfy_host_encoder_create(pack.p, bytes, (int)c.get("dtype"),
                                             c.get("null_out") ? nullptr : &encoder);
  check_status(c, status);
  if (c.get("null_out")) return;
  if ((status == GFY_OK) != (encoder != nullptr)) fail(c, "encoder handle does not follow the status");
  gfy_host_encoder_destroy(encoder);
}

// ---- microbatch: gfy_pack_microbatch ------------------------------------------------------
void run_microbatch(const Case& c) {
  const Exact features(c, "node_features"), edges(c, "edge_index"), types(c, "edge_types"),
      roles(c, "node_roles"), node_ptr(c, "node_ptr"), edge_ptr(c, "edge_ptr"), want(c, "want_slot");
  const size_t slot_bytes = (size_t)c.get("slot_bytes"), lead = (size_t)c.get("misalign");
  const auto& want_offsets = c.ints.count("offsets") ? c.ints.at("offsets") : std::vector<int64_t>();
  const auto& want_counts = c.ints.count("counts") ? c.ints.at("counts") : std::vector<int64_t>();
  for (int pass = 0; pass < 2; ++pass) {   // streaming stores (the default), then memcpy
    if (pass == 0) unsetenv("GFY_PACK_STREAM");
    else setenv("GFY_PACK_STREAM", "0", 1);
    const std::string where = pass == 0 ? "[stream] " : "[GFY_PACK_STREAM=0] ";
    // the slot: exactly slot_bytes, `lead` bytes behind a 16-byte boundary (the bytes in front
    // of it keep a pattern, the allocation ends where the slot ends)
    void* block = nullptr;
    if (posix_memalign(&block, 16, lead + slot_bytes ? lead + slot_bytes : 16) != 0)
      fail(c, "out of memory");
    std::memset(block, 0, lead + slot_bytes);
    std::memset(block, 0x5A, lead);
    char* slot = static_cast<char*>(block) + lead;
    int64_t offsets[6], counts[4];
    for (auto& v : offsets) v = -77;
    for (auto& v : counts) v = -77;
    const int status = gfy_pack_microbatch(
        features.as<float>(), (int)c.get("feature_dim"), edges.as<int32_t>(), c.get("edges_total"),
        types.as<uint8_t>(), roles.as<uint8_t>(), node_ptr.as<int64_t>(), edge_ptr.as<int64_t>(),
        c.get("start"), c.get("stop"), (int)c.get("with_records"), slot, c.get("base"), offsets,
        counts);
    check_status(c, status, where);
    for (size_t i = 0; i < lead; ++i)
      if (static_cast<unsigned char*>(block)[i] != 0x5A) fail(c, where + "a byte in front of the slot changed");
    if (status == GFY_OK) {
      for (int i = 0; i < 6; ++i)
        if (offsets[i] != want_offsets.at(i))
          fail(c, join({where, "offsets[", std::to_string(i), "] = ", std::to_string(offsets[i]),
                        ", expected ", std::to_string(want_offsets.at(i))}));
      for (int i = 0; i < 4; ++i)
        if (counts[i] != want_counts.at(i))
          fail(c, join({where, "counts[", std::to_string(i), "] = ", std::to_string(counts[i]),
                        ", expected ", std::to_string(want_counts.at(i))}));
      if (want.bytes != slot_bytes) fail(c, "want_slot is not slot_bytes long");
      for (size_t i = 0; i < slot_bytes; ++i)
        if (slot[i] != want.as<char>()[i])
          fail(c, join({where, "slot byte ", std::to_string(i), " differs"}));
    }
    std::free(block);
  }
  unsetenv("GFY_PACK_STREAM");
}

// ---- encode: gfy_host_encode ----------------------------------------------------------------
double half_to_double(uint16_t h) {
  const int exp = (h >> 10) & 0x1F, man = h & 0x3FF;
  double value;
  if (exp == 0) value = std::ldexp((double)man, -24);
  else if (exp == 31) value = man ? NAN : INFINITY;
  else value = std::ldexp((double)(man | 0x400), exp - 25);
  return (h & 0x8000) ? -value : value;
}

size_t item_bytes(int dtype) { return dtype == GFY_F16 ? 2 : dtype == GFY_F32 ? 4 : 8; }

// Encoders are made once per (pack, model dtype), shared by the cases of one run and
// destroyed at its end.
std::map<std::pair<size_t, int>, gfy_host_encoder*> g_encoders;

const gfy_host_encoder* encoder_of(const Case& c) {
  auto& made = g_encoders;
  const std::pair<size_t, int> key{c.arrays.at("pack").first, (int)c.get("model_dtype")};
  auto at = made.find(key);
  if (at != made.end()) return at->second;
  const Exact pack(c, "pack");
  gfy_host_encoder* encoder = nullptr;
  if (gfy_host_encoder_create(pack.p, pack.bytes, key.second, &encoder) != GFY_OK)
    fail(c, join({"gfy_host_encoder_create: ", gfy_last_error()}));
  made[key] = encoder;
  return encoder;
}

// One call checked against the case: exact bytes (`want`), or float64 values and a tolerance
// per element (`want64`, `tol64`: the fp32 model has no bit-exact reference).
void check_rows(const Case& c, const void* out, size_t out_bytes, const Exact& want,
                const Exact& want64, const Exact& tol64, const std::string& where) {
  const int dtype = (int)c.get("out_dtype");
  if (want.p) {
    if (want.bytes != out_bytes) fail(c, "want is not as long as out");
    if (std::memcmp(out, want.p, out_bytes) != 0) {
      size_t at = 0;
      while (static_cast<const char*>(out)[at] == want.as<char>()[at]) ++at;
      fail(c, join({where, "output byte ", std::to_string(at), " differs"}));
    }
    return;
  }
  const size_t count = out_bytes / item_bytes(dtype);
  if (want64.bytes != 8 * count || tol64.bytes != 8 * count) fail(c, "want64 / tol64 do not fit out");
  for (size_t i = 0; i < count; ++i) {
    const double got = dtype == GFY_F16   ? half_to_double(static_cast<const uint16_t*>(out)[i])
                       : dtype == GFY_F32 ? (double)static_cast<const float*>(out)[i]
                                          : static_cast<const double*>(out)[i];
    const double off = std::fabs(got - want64.as<double>()[i]);
    if (!(off <= tol64.as<double>()[i])) {
      char text[160];
      std::snprintf(text, sizeof text, "element %zu: %.9g, expected %.9g within %.3g", i, got,
                    want64.as<double>()[i], tol64.as<double>()[i]);
      fail(c, where + text);
    }
  }
}

void run_encode(const Case& c) {
  const gfy_host_encoder* encoder = c.get("null_encoder") ? nullptr : encoder_of(c);
  const Exact x(c, "x"), edges(c, "edge_index"), types(c, "edge_types"), rows(c, "out_rows"),
      want(c, "want"), want64(c, "want64"), tol64(c, "tol64");
  const size_t out_bytes = (size_t)c.get("out_count") * 128 * item_bytes((int)c.get("out_dtype"));
  std::vector<char> first;
  for (int64_t threads : c.ints.at("threads")) {
    const std::string where = join({"[threads=", std::to_string(threads), "] "});
    char* out = static_cast<char*>(std::malloc(out_bytes));
    std::memset(out, 0xAB, out_bytes);
    const int status = gfy_host_encode(encoder, x.as<float>(), edges.as<int32_t>(),
                                       types.as<uint8_t>(), c.get("n"), c.get("e"),
                                       rows.as<int32_t>(), out, (int)c.get("out_dtype"),
                                       (int)c.get("normalise"), (int)threads);
    check_status(c, status, where);
    if (status == GFY_OK) {
      check_rows(c, out, out_bytes, want, want64, tol64, where);
      // the same bytes whatever the number of workers
      if (first.empty()) first.assign(out, out + out_bytes);
      else if (std::memcmp(first.data(), out, out_bytes) != 0)
        fail(c, where + "bytes differ from those of the first thread count");
    } else {
      for (size_t i = 0; i < out_bytes; ++i)
        if ((unsigned char)out[i] != 0xAB) fail(c, where + "a refused call wrote to out");
    }
    std::free(out);
  }
}

// ---- threads: the per-thread error channel, encoders of one's own and a shared one ------------
std::atomic<int> g_failures{0};
std::string g_failure_text[3];

void thread_failed(int who, const std::string& why) {
  g_failure_text[who] = why;   // (one writer per entry; read after the joins)
  g_failures.fetch_add(1);
}

// `rounds` encodes of the case's graph with three workers each; the caller's own results and an
// empty error text every time
void encode_rounds(int who, const Case& c, const gfy_host_encoder* encoder, const Exact& x,
                   const Exact& edges, const Exact& types, const Exact& want, int rounds) {
  for (int round = 0; round < rounds; ++round) {
    char* out = static_cast<char*>(std::malloc(want.bytes));
    std::memset(out, 0xAB, want.bytes);
    const int status = gfy_host_encode(encoder, x.as<float>(), edges.as<int32_t>(),
                                       types.as<uint8_t>(), c.get("n"), c.get("e"), nullptr, out,
                                       GFY_F16, 1, 3);
    const std::string text = gfy_last_error();
    const bool same = std::memcmp(out, want.p, want.bytes) == 0;
    std::free(out);
    if (status != GFY_OK || !text.empty() || !same) {
      thread_failed(who, join({"round ", std::to_string(round), ": status ", std::to_string(status),
                               same ? "" : ", other bytes", ", error text '", text, "'"}));
      return;
    }
  }
}

void run_threads(const Case& c) {
  const Exact pack(c, "pack"), x(c, "x"), edges(c, "edge_index"), types(c, "edge_types"),
      want(c, "want");
  const int rounds = (int)c.get("rounds");
  g_failures = 0;
  if (c.get("shared")) {   // one const encoder under two encoding threads
    gfy_host_encoder* encoder = nullptr;
    if (gfy_host_encoder_create(pack.p, pack.bytes, GFY_F16, &encoder) != GFY_OK)
      fail(c, join({"gfy_host_encoder_create: ", gfy_last_error()}));
    const gfy_host_encoder* shared = encoder;
    std::thread a([&] { encode_rounds(0, c, shared, x, edges, types, want, rounds); });
    std::thread b([&] { encode_rounds(1, c, shared, x, edges, types, want, rounds); });
    a.join();
    b.join();
    gfy_host_encoder_destroy(encoder);
  } else {   // an encoder each, and a third thread that fails meanwhile
    std::atomic<int> running{2};
    auto own = [&](int who) {
      gfy_host_encoder* encoder = nullptr;
      // each thread parses a pack of its own (exact allocation)
      const Exact mine(c, "pack");
      if (gfy_host_encoder_create(mine.p, mine.bytes, GFY_F16, &encoder) != GFY_OK) {
        thread_failed(who, join({"gfy_host_encoder_create: ", gfy_last_error()}));
      } else {
        encode_rounds(who, c, encoder, x, edges, types, want, rounds);
        gfy_host_encoder_destroy(encoder);
      }
      running.fetch_sub(1);
    };
    std::thread a(own, 0), b(own, 1);
    std::thread refused([&] {
      const size_t cut = (size_t)c.get("bad_length");
      void* truncated = std::malloc(cut);
      std::memcpy(truncated, pack.p, cut);
      int calls = 0;
      while (running.load() > 0 || calls < 3) {
        gfy_host_encoder* encoder = reinterpret_cast<gfy_host_encoder*>(0x1);
        const int status = gfy_host_encoder_create(truncated, cut, GFY_F16, &encoder);
        const std::string text = gfy_last_error();
        ++calls;
        if (status != GFY_ERR_INVALID || encoder != nullptr ||
            text.find(c.text("error")) == std::string::npos) {
          thread_failed(2, join({"call ", std::to_string(calls), ": status ",
                                 std::to_string(status), ", error text '", text, "'"}));
          break;
        }
        std::this_thread::yield();
      }
      std::free(truncated);
    });
    a.join();
    b.join();
    refused.join();
  }
  if (g_failures.load() != 0)
    for (int who = 0; who < 3; ++who)
      if (!g_failure_text[who].empty())
        fail(c, join({"thread ", std::to_string(who), ": ", g_failure_text[who]}));
  if (std::string(gfy_last_error()) != "") fail(c, "the main thread sees another thread's error text");
}

}   // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: host_sanitize pack|microbatch|encode|threads CASEDIR\n");
    return 2;
  }
  g_command = argv[1];
  void (*run)(const Case&) = g_command == "pack"         ? run_pack
                             : g_command == "microbatch" ? run_microbatch
                             : g_command == "encode"     ? run_encode
                             : g_command == "threads"    ? run_threads
                                                         : nullptr;
  if (!run) {
    std::fprintf(stderr, "host_sanitize: unknown sub-command %s\n", argv[1]);
    return 2;
  }
  for (const Case& c : read_manifest(argv[2])) {
    run(c);
    std::printf("ok %s %s\n", g_command.c_str(), c.name.c_str());
    std::fflush(stdout);
  }
  for (auto& entry : g_encoders) gfy_host_encoder_destroy(entry.second);
  return 0;
}
