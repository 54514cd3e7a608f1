// c_archive_host.cpp -- the zip scan and the chunked CRC fold (sourmash-rust_amd/csrc/archive_core.hpp) with the shared DEFLATE
// decoder (inflate_core.hpp) as a plain host program, for tests/test_archive_host.py: built with g++ and the address and
// undefined-behaviour sanitizers, no HIP header, no library.
//   c_archive_host CASES RESULTS
// CASES:   u32 n, then per case u32 len, the archive's bytes
// RESULTS: per case u32 accepted; refused: u32 len, the message; accepted: u32 entries, then per entry
//            u32 len, name; u32 len, reason; u32 method, flags, crc32, kind, device_ok, text_size, text_crc;
//            u64 comp_size, size, header_off, data_off, payload_off, payload_len;
//            u32 status with the CRC verified, u32 status without, u32 produced, the produced text
//          status 255: the entry is not for the device, or its announced text is above 16 MiB (not run here)
// Every archive and every output sits in a heap block of exactly its size, so one byte read or written past an end is reported.
// The CRC is taken the way the kernels take it -- per chunk in 64 slices, then folded by 64 lanes striding over the chunks --
// and compared with the serial CRC on every case; every chunk is looked up in the chunk prefix as the kernel looks it up.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "archive_core.hpp"

namespace inf = smh::inflate;
namespace arc = smh::archive;

struct HostSink {
  uint8_t* out;
  void lit(uint32_t pos, uint8_t b) { out[pos] = b; }
  void copy(uint32_t pos, uint32_t dist, uint32_t len) { for (uint32_t i = 0; i < len; i++) out[pos + i] = out[pos - dist + i]; }
  void stored(uint32_t pos, const uint8_t* src, uint32_t n) { memcpy(out + pos, src, n); }
  void flush() {}
};

static uint32_t rd32(FILE* f) {
  uint8_t b[4];
  if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "cases file cut short\n"); exit(2); }
  return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}
static void wr32(FILE* f, uint32_t v) {
  const uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
  fwrite(b, 1, 4, f);
}
static void wr64(FILE* f, uint64_t v) { wr32(f, (uint32_t)v); wr32(f, (uint32_t)(v >> 32)); }
static void wrstr(FILE* f, const std::string& s) { wr32(f, (uint32_t)s.size()); fwrite(s.data(), 1, s.size(), f); }

constexpr uint32_t kNotRun = 255, kCap = 1u << 24;

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: c_archive_host CASES RESULTS\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* res = fopen(argv[2], "wb");
  if (!in || !res) { fprintf(stderr, "cannot open the files\n"); return 2; }
  uint32_t* crc_table = (uint32_t*)malloc(256 * 4);
  for (uint32_t i = 0; i < 256; i++) crc_table[i] = inf::crc_table_entry(i);
  inf::Tables t;
  t.lens = (uint8_t*)malloc(inf::kLensBytes);
  t.lsym = (uint16_t*)malloc(inf::kLitSyms * 2);
  t.dsym = (uint16_t*)malloc(inf::kDistSyms * 2);
  t.work = (uint16_t*)malloc(inf::kWorkWords * 2);
  const uint32_t n = rd32(in);
  uint64_t folds = 0;
  for (uint32_t c = 0; c < n; c++) {
    const uint32_t len = rd32(in);
    uint8_t* data = (uint8_t*)malloc(len);
    if (len && fread(data, 1, len, in) != len) { fprintf(stderr, "cases file cut short\n"); return 2; }
    arc::Archive a;
    std::string msg;
    if (!arc::scan(&a, data, len, &msg)) {
      wr32(res, 0);
      wrstr(res, msg);
      free(data);
      continue;
    }
    wr32(res, 1);
    wr32(res, (uint32_t)a.entries.size());
    // the chunk prefix of the entries the device would take, and every chunk looked up in it
    std::vector<uint64_t> prefix(1, 0);
    std::vector<uint32_t> sizes;
    for (const arc::Entry& e : a.entries) {
      const uint32_t size = (e.device_ok && e.text_size <= kCap) ? e.text_size : 0;
      sizes.push_back(size);
      prefix.push_back(prefix.back() + arc::chunks_of(size));
    }
    for (size_t m = 0; m < sizes.size(); m++)
      for (uint64_t w = prefix[m]; w < prefix[m + 1]; w++)
        if (arc::member_of_chunk(prefix.data(), sizes.size(), w) != m) { fprintf(stderr, "case %u: chunk %llu is not member %zu's\n", c, (unsigned long long)w, m); return 3; }
    for (const arc::Entry& e : a.entries) {
      wrstr(res, e.name); wrstr(res, e.reason);
      wr32(res, e.method); wr32(res, e.flags); wr32(res, e.crc32); wr32(res, e.kind); wr32(res, e.device_ok ? 1 : 0);
      wr32(res, e.text_size); wr32(res, e.text_crc);
      wr64(res, e.comp_size); wr64(res, e.size); wr64(res, e.header_off); wr64(res, e.data_off); wr64(res, e.payload_off); wr64(res, e.payload_len);
      if (!e.device_ok || e.text_size > kCap) { wr32(res, kNotRun); wr32(res, kNotRun); wr32(res, 0); continue; }
      // the payload in a block of its own size: a read past the stream is a read past the block
      uint8_t* payload = (uint8_t*)malloc(e.payload_len);
      if (e.payload_len) memcpy(payload, data + e.payload_off, e.payload_len);
      uint8_t* out = (uint8_t*)malloc(e.text_size);
      uint32_t produced = 0;
      uint8_t r = inf::kOk;
      if (e.kind == arc::kDeflate || e.kind == arc::kGzip) {
        HostSink sink{out};
        r = inf::inflate_member(payload, (uint32_t)e.payload_len, e.text_size, t, sink, &produced);
      } else {
        if (e.text_size) memcpy(out, payload, e.text_size);   // (stored: payload_len == text_size)
        produced = e.text_size;
      }
      uint8_t verified = r;
      if (r == inf::kOk) {
        const uint64_t n_chunks = arc::chunks_of(e.text_size);
        uint32_t* terms = (uint32_t*)malloc(n_chunks * 4);
        for (uint64_t k = 0; k < n_chunks; k++) {
          const uint32_t lo = arc::chunk_begin(e.text_size, k), hi = arc::chunk_begin(e.text_size, k + 1);
          uint32_t x = 0;
          for (uint32_t lane = 0; lane < 64; lane++) x ^= arc::chunk_lane_term(out + lo, hi - lo, 64, lane, crc_table);
          terms[k] = x;
        }
        uint32_t x = 0;
        for (uint32_t lane = 0; lane < 64; lane++) x ^= arc::fold_lane_term(terms, n_chunks, e.text_size, 64, lane);
        free(terms);
        if (~x != ~inf::crc_run(0xffffffffu, out, e.text_size, crc_table)) { fprintf(stderr, "case %u: the folded CRC differs from the serial one\n", c); return 3; }
        if (~x != e.text_crc) verified = inf::kCrc;
        folds++;
      }
      wr32(res, verified); wr32(res, r); wr32(res, produced);
      fwrite(out, 1, produced, res);
      free(out); free(payload);
    }
    free(data);
  }
  free(t.lens); free(t.lsym); free(t.dsym); free(t.work);
  free(crc_table);
  fclose(in);
  if (fclose(res) != 0) return 2;
  printf("c archive host ok: %u cases, %llu folds\n", n, (unsigned long long)folds);
  return 0;
}
