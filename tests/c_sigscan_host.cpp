// c_sigscan_host.cpp -- the shared core of the signature scan (sourmash-rust_amd/csrc/sigscan_core.hpp: its serial driver)
// and the JSON parser with holes (sigjson.hpp) as a plain host program, for tests/test_sigscan_host.py: built with g++ and the
// address and undefined-behaviour sanitizers, no HIP header, no library.
//   c_sigscan_host CASES RESULTS
// CASES:   u32 n, then per case u32 n_docs, (n_docs + 1) u64 doc offsets, u64 len, the text
// RESULTS: per case
//            u32 holes verdict (0 accepted, 1 refused, 2 refused as a float split in two), u32 its failing document,
//            u32 plain verdict (0 accepted, 1 refused), u32 its failing document,
//            u32 agree (both accepted: the sketches of both routes are equal field for field, hashes and abundances included),
//            u32 sketches (holes route, when accepted),
//            u64 skeleton length, the skeleton, u64 spans, per span u64 start, end, first_token, n_tokens, bad_off, u32 status,
//            u64 values, the values
// The text of every case sits in a heap block of exactly its size, so one byte read past an end is reported.  The plain route
// is what the host loader does: the same parser without holes on the document's own bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "sigjson.hpp"

using namespace smh;

struct Sketch {
  uint32_t signature, sketch, num, ksize;
  uint64_t seed, max_hash;
  uint8_t molecule;
  bool has_abunds, has_name = false, has_filename = false;
  std::string md5, name, filename, license, klass;
  std::vector<uint64_t> mins, abunds;
  bool operator==(const Sketch& o) const {
    return signature == o.signature && sketch == o.sketch && num == o.num && ksize == o.ksize && seed == o.seed && max_hash == o.max_hash &&
           molecule == o.molecule && has_abunds == o.has_abunds && has_name == o.has_name && has_filename == o.has_filename && md5 == o.md5 &&
           name == o.name && filename == o.filename && license == o.license && klass == o.klass && mins == o.mins && abunds == o.abunds;
  }
};

// one document through the shared walk; holes null: the plain route.  Returns 0, 1 or 2.
static int read_document(const char* data, size_t len, const Holes* holes, const std::vector<uint64_t>& values, uint32_t doc,
                         std::vector<Sketch>* out) {
  (void)doc;
  try {
    JVal root;
    parse_document(data, len, holes, &root);
    std::vector<Sketch> pending;
    auto numbers = [&](const JVal& arr) {
      std::vector<uint64_t> v;
      if (holes) {
        const sigscan::SpanRow& r = holes->rows[arr.span];
        for (uint64_t i = 0; i < r.n_tokens; i++) v.push_back(values.at(r.first_token + i));
      } else {
        for (auto& e : arr.arr) v.push_back(e.u);
      }
      return v;
    };
    walk_document(root, holes,
                  [&](size_t i, size_t k, const SketchFields& f) {
                    Sketch s;
                    s.signature = (uint32_t)i; s.sketch = (uint32_t)k; s.num = f.num; s.ksize = f.ksize; s.seed = f.seed; s.max_hash = f.max_hash;
                    s.molecule = f.molecule; s.has_abunds = f.has_abunds; s.md5 = f.md5sum;
                    s.mins = numbers(*f.mins);
                    if (f.has_abunds) s.abunds = numbers(*f.abunds);
                    pending.push_back(s);
                  },
                  [&](size_t, const SignatureFields& f) {
                    for (Sketch& s : pending) {
                      s.name = f.name; s.has_name = f.has_name; s.filename = f.filename; s.has_filename = f.has_filename;
                      s.license = f.license; s.klass = f.klass;
                      out->push_back(s);
                    }
                    pending.clear();
                  });
    return 0;
  } catch (const JsonError& e) {
    return e.split_float ? 2 : 1;
  }
}

static uint64_t rd(FILE* f, int bytes) {
  uint8_t b[8] = {0};
  if (fread(b, 1, (size_t)bytes, f) != (size_t)bytes) { fprintf(stderr, "cases file cut short\n"); exit(2); }
  uint64_t v = 0;
  for (int i = 0; i < bytes; i++) v |= (uint64_t)b[i] << (8 * i);
  return v;
}
static void wr(FILE* f, uint64_t v, int bytes) {
  uint8_t b[8];
  for (int i = 0; i < bytes; i++) b[i] = (uint8_t)(v >> (8 * i));
  fwrite(b, 1, (size_t)bytes, f);
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: c_sigscan_host CASES RESULTS\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* res = fopen(argv[2], "wb");
  if (!in || !res) { fprintf(stderr, "cannot open the files\n"); return 2; }
  const uint32_t n = (uint32_t)rd(in, 4);
  for (uint32_t c = 0; c < n; c++) {
    const uint32_t n_docs = (uint32_t)rd(in, 4);
    std::vector<uint64_t> off(n_docs + 1);
    for (auto& o : off) o = rd(in, 8);
    const uint64_t len = rd(in, 8);
    uint8_t* text = (uint8_t*)malloc(len ? len : 1);
    if (len && fread(text, 1, len, in) != len) { fprintf(stderr, "cases file cut short\n"); return 2; }

    std::string skeleton;
    std::vector<sigscan::SpanRow> spans;
    std::vector<uint64_t> values;
    sigscan::scan_serial(text, len, &skeleton, &spans, &values);
    const std::vector<uint64_t> removed = removed_prefix(spans);

    uint32_t vh = 0, dh = 0, vp = 0, dp = 0;
    std::vector<Sketch> by_holes, by_plain;
    for (uint32_t d = 0; d < n_docs && vh == 0; d++) {
      const DocSlice s = slice_document(spans, removed, off[d], off[d + 1]);
      // the document's skeleton in a block of its own size
      const size_t sl = (size_t)(s.skel_end - s.skel_begin);
      char* doc = (char*)malloc(sl ? sl : 1);
      memcpy(doc, skeleton.data() + s.skel_begin, sl);
      vh = (uint32_t)read_document(doc, sl, &s.holes, values, d, &by_holes);
      dh = d;
      free(doc);
    }
    for (uint32_t d = 0; d < n_docs && vp == 0; d++) {
      const size_t dl = (size_t)(off[d + 1] - off[d]);
      char* doc = (char*)malloc(dl ? dl : 1);
      memcpy(doc, text + off[d], dl);
      vp = (uint32_t)read_document(doc, dl, nullptr, values, d, &by_plain);
      dp = d;
      free(doc);
    }
    const uint32_t agree = (vh == 0 && vp == 0) ? (by_holes == by_plain ? 1u : 0u) : 1u;
    wr(res, vh, 4); wr(res, dh, 4); wr(res, vp, 4); wr(res, dp, 4); wr(res, agree, 4); wr(res, vh == 0 ? by_holes.size() : 0, 4);
    wr(res, skeleton.size(), 8);
    fwrite(skeleton.data(), 1, skeleton.size(), res);
    wr(res, spans.size(), 8);
    for (const auto& r : spans) { wr(res, r.start, 8); wr(res, r.end, 8); wr(res, r.first_token, 8); wr(res, r.n_tokens, 8); wr(res, r.bad_off, 8); wr(res, r.status, 4); }
    wr(res, values.size(), 8);
    for (uint64_t v : values) wr(res, v, 8);
    free(text);
  }
  fclose(in);
  if (fclose(res) != 0) { fprintf(stderr, "cannot write the results\n"); return 2; }
  printf("c sigscan host ok: %u cases\n", n);
  return 0;
}
