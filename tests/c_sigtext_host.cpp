// c_sigtext_host.cpp -- the shared core of signature JSON written on the device (sourmash-rust_amd/csrc/sigtext_core.hpp: the
// digit count, the formatter, MD5 with its padding, the layout walk and the serial driver) and the one string writer
// (sigjson.hpp's json_escape) as a plain host program, for tests/test_sigtext_host.py: built with g++ and the address and
// undefined-behaviour sanitizers, no HIP header, no library.
//   c_sigtext_host CASES RESULTS
// CASES:   u32 cases, then per case u32 n, u32 has_abunds, u32 has_doc_starts, u32 n_docs, (n_docs + 1) u32 doc_starts when it has
//          them, then per node u32 num, u32 ksize, u64 seed, u64 max_hash, u32 molecule, i32 name length (-1: null), the name,
//          i32 filename length (-1: null), the filename, u64 count, the hashes (u64), the abundances (u32) with has_abunds
// RESULTS: per case u64 length, the text, u32 entries, that many u64 document offsets, 16 n digest bytes
// Every node's values sit in heap blocks of exactly their size, so one element read past an end is reported.  Every value is
// also formatted on its own and checked against snprintf, digit count included.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "sigjson.hpp"
#include "sigtext_core.hpp"

using namespace smh;

static const char* kMolecules[4] = {"DNA", "protein", "dayhoff", "hp"};

template <class T> static T get(FILE* f) {
  T v;
  if (fread(&v, sizeof v, 1, f) != 1) { fprintf(stderr, "short read\n"); exit(2); }
  return v;
}
static std::string get_bytes(FILE* f, size_t n) {
  std::string s(n, '\0');
  if (n && fread(&s[0], 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
  return s;
}
template <class T> static void put(FILE* f, const T& v) { fwrite(&v, sizeof v, 1, f); }

static bool check_value(uint64_t v, bool narrow) {
  char want[32];
  const int n = snprintf(want, sizeof want, "%llu", (unsigned long long)v);
  std::vector<uint8_t> got((size_t)n);   // exactly the digits: a byte too many is reported
  const uint32_t k = narrow ? sigtext::format_u32((uint32_t)v, got.data()) : sigtext::format_u64(v, got.data());
  const uint32_t d = narrow ? sigtext::digits_u32((uint32_t)v) : sigtext::digits_u64(v);
  return k == (uint32_t)n && d == k && memcmp(got.data(), want, (size_t)n) == 0;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: c_sigtext_host CASES RESULTS\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
  const uint32_t cases = get<uint32_t>(in);
  for (uint32_t c = 0; c < cases; c++) {
    const uint32_t n = get<uint32_t>(in), has_abunds = get<uint32_t>(in), has_docs = get<uint32_t>(in), n_docs = get<uint32_t>(in);
    std::vector<uint32_t> doc_starts;
    for (uint32_t d = 0; has_docs && d <= n_docs; d++) doc_starts.push_back(get<uint32_t>(in));
    std::vector<sigtext::NodeText> nodes;
    std::vector<uint32_t> ksizes;
    std::vector<uint64_t> offsets(1, 0);
    std::vector<std::vector<uint64_t>> hashes(n);
    std::vector<std::vector<uint32_t>> abunds(n);
    for (uint32_t v = 0; v < n; v++) {
      sigtext::NodeParams p;
      p.num = get<uint32_t>(in); p.ksize = get<uint32_t>(in); p.seed = get<uint64_t>(in); p.max_hash = get<uint64_t>(in);
      const uint32_t molecule = get<uint32_t>(in);
      if (molecule > 3) { fprintf(stderr, "bad molecule\n"); return 2; }
      p.molecule = kMolecules[molecule];
      std::string json[2];   // name, filename
      for (int k = 0; k < 2; k++) {
        const int32_t len = get<int32_t>(in);
        if (len < 0) json[k] = "null"; else json_escape(json[k], get_bytes(in, (size_t)len));
      }
      nodes.push_back(sigtext::node_text(p, json[1], json[0], has_abunds != 0));
      ksizes.push_back(p.ksize);
      const uint64_t count = get<uint64_t>(in);
      hashes[v].resize(count);
      for (uint64_t i = 0; i < count; i++) hashes[v][i] = get<uint64_t>(in);
      if (has_abunds) { abunds[v].resize(count); for (uint64_t i = 0; i < count; i++) abunds[v][i] = get<uint32_t>(in); }
      offsets.push_back(offsets.back() + count);
      for (uint64_t h : hashes[v]) if (!check_value(h, false)) { printf("FAILED: value %llu\n", (unsigned long long)h); return 1; }
      for (uint32_t a : abunds[v]) if (!check_value(a, true)) { printf("FAILED: abundance %u\n", a); return 1; }
    }
    // the CSR, in blocks of exactly its size
    std::vector<uint64_t> flat_h;
    std::vector<uint32_t> flat_a;
    for (uint32_t v = 0; v < n; v++) { flat_h.insert(flat_h.end(), hashes[v].begin(), hashes[v].end()); flat_a.insert(flat_a.end(), abunds[v].begin(), abunds[v].end()); }
    flat_h.shrink_to_fit(); flat_a.shrink_to_fit();
    static const uint32_t none32 = 0;
    std::string text;
    std::vector<uint64_t> doc_offsets;
    std::vector<uint8_t> md5;
    sigtext::write_serial(n, offsets.data(), flat_h.data(), has_abunds ? (flat_a.empty() ? &none32 : flat_a.data()) : nullptr, ksizes.data(),
                          nodes.data(), has_docs ? doc_starts.data() : nullptr, n_docs, &text, &doc_offsets, &md5);
    put<uint64_t>(out, text.size());
    fwrite(text.data(), 1, text.size(), out);
    put<uint32_t>(out, (uint32_t)doc_offsets.size());
    for (uint64_t o : doc_offsets) put<uint64_t>(out, o);
    if (!md5.empty()) fwrite(md5.data(), 1, md5.size(), out);
  }
  fclose(in);
  if (fclose(out) != 0) { fprintf(stderr, "cannot write the results\n"); return 2; }
  printf("c sigtext host ok: %u cases\n", cases);
  return 0;
}
