// c_inflate_host.cpp -- the shared DEFLATE decoder (sourmash-rust_amd/csrc/inflate_core.hpp) as a plain host program, for
// tests/test_inflate_host.py: built with g++ and the address and undefined-behaviour sanitizers, no HIP header, no library.
//   c_inflate_host CASES RESULTS
// CASES:   u32 n, then per case u32 payload_len, u32 isize, u32 crc, u32 verify, payload bytes
// RESULTS: per case u32 status, u32 out_len, out bytes (isize bytes for status 0, else what was produced)
// Every payload, output and table sits in a heap block of exactly its size, so one byte read or written past an end is
// reported.  The CRC is taken the way the kernel takes it: 64 slices, shifted and XOR-ed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "inflate_core.hpp"

namespace inf = smh::inflate;

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

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: c_inflate_host CASES RESULTS\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* res = fopen(argv[2], "wb");
  if (!in || !res) { fprintf(stderr, "cannot open the files\n"); return 2; }
  uint32_t* crc_table = (uint32_t*)malloc(256 * 4);
  for (uint32_t i = 0; i < 256; i++) crc_table[i] = inf::crc_table_entry(i);
  const uint32_t n = rd32(in);
  for (uint32_t c = 0; c < n; c++) {
    const uint32_t plen = rd32(in), isize = rd32(in), crc = rd32(in), verify = rd32(in);
    if (isize > inf::kMaxMember) { fprintf(stderr, "case %u: ISIZE above 65536\n", c); return 2; }
    uint8_t* payload = (uint8_t*)malloc(plen ? plen : 1);
    if (plen && fread(payload, 1, plen, in) != plen) { fprintf(stderr, "cases file cut short\n"); return 2; }
    if (!plen) { free(payload); payload = (uint8_t*)malloc(0); }
    uint8_t* out = (uint8_t*)malloc(isize);
    inf::Tables t;
    t.lens = (uint8_t*)malloc(inf::kLensBytes);
    t.lsym = (uint16_t*)malloc(inf::kLitSyms * 2);
    t.dsym = (uint16_t*)malloc(inf::kDistSyms * 2);
    t.work = (uint16_t*)malloc(inf::kWorkWords * 2);
    HostSink sink{out};
    uint32_t produced = 0;
    uint8_t r = inf::inflate_member(payload, plen, isize, t, sink, &produced);
    if (r == inf::kOk && verify) {
      uint32_t x = 0;
      for (uint32_t lane = 0; lane < 64; lane++) x ^= inf::crc_lane_term(out, isize, 64, lane, crc_table);
      if (~x != crc) r = inf::kCrc;
      if (~inf::crc_run(0xffffffffu, out, isize, crc_table) != ~x) { fprintf(stderr, "case %u: the folded CRC differs from the serial one\n", c); return 3; }
    }
    wr32(res, r);
    wr32(res, produced);
    fwrite(out, 1, produced, res);
    free(t.lens); free(t.lsym); free(t.dsym); free(t.work);
    free(out); free(payload);
  }
  free(crc_table);
  fclose(in);
  if (fclose(res) != 0) return 2;
  printf("c inflate host ok: %u cases\n", n);
  return 0;
}
