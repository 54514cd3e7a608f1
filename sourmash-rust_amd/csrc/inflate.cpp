// inflate.cpp -- blocked gzip (BGZF): the member scan on the host and the host side of inflate_kernels.hip.
#include <string>
#include <vector>

#include "inflate_core.hpp"
#include "kernels.hpp"

namespace smh {

namespace {

std::string at_member(uint64_t index, uint64_t off) { return " (member " + std::to_string(index) + " at byte " + std::to_string(off) + ")"; }

const char* reason_text(uint32_t r) {
  static const char* const text[inflate::kReasons] = {
      "ok",
      "reserved block type",
      "stored block whose LEN is not the complement of NLEN",
      "more than 286 literal/length codes or more than 30 distance codes",
      "code-length repeat with nothing to repeat or running past the announced lengths",
      "over-subscribed code set",
      "incomplete code set",
      "no end-of-block code",
      "invalid literal/length or distance symbol",
      "distance reaching in front of the member's output",
      "input exhausted",
      "output would pass ISIZE",
      "stream ends with output below ISIZE",
      "payload bytes left over after the final block",
      "CRC-32 mismatch",
  };
  return r < inflate::kReasons ? text[r] : "unknown reason";
}

uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
uint32_t le32(const uint8_t* p) { return le16(p) | le16(p + 2) << 16; }

}  // namespace

const char* inflate_reason_text(uint32_t reason) { return reason_text(reason); }

void gzip_scan(Gzip* g, const uint8_t* data, uint64_t len) {
  g->members.clear(); g->header_off.clear();
  g->len = len; g->inflated = 0;
  uint64_t off = 0;
  while (off < len) {
    const uint64_t index = g->members.size(), left = len - off;
    const uint8_t* h = data + off;
    const std::string where = at_member(index, off);
    const bool magic = left >= 2 ? (h[0] == 0x1f && h[1] == 0x8b) : (h[0] == 0x1f);
    if (!magic || (left >= 3 && h[2] != 8)) {
      if (index == 0) throw Error(kMsg, "gzip: the bytes are not gzip" + where);
      throw Error(kMsg, "gzip: bytes trail after the last member" + where);
    }
    const auto cut = [&]() -> Error { return Error(kMsg, "gzip: a member's header is cut short" + where); };
    if (left < 10) throw cut();
    const uint32_t flg = h[3];
    uint64_t at = 10;   // relative to the member
    bool have_bc = false;
    uint32_t bsize = 0;
    if (flg & 4) {      // FEXTRA
      if (left < at + 2) throw cut();
      const uint64_t xlen = le16(h + at);
      at += 2;
      if (left < at + xlen) throw cut();
      uint64_t sub = at;
      const uint64_t end = at + xlen;
      while (sub < end) {
        if (end - sub < 4) throw cut();
        const uint64_t slen = le16(h + sub + 2);
        if (end - sub - 4 < slen) throw cut();
        if (h[sub] == 'B' && h[sub + 1] == 'C' && slen == 2 && !have_bc) { have_bc = true; bsize = le16(h + sub + 4); }
        sub += 4 + slen;
      }
      at = end;
    }
    for (uint32_t bit = 8; bit <= 16; bit <<= 1) {   // FNAME, FCOMMENT: up to and with a NUL
      if (!(flg & bit)) continue;
      while (at < left && h[at] != 0) at++;
      if (at >= left) throw cut();
      at++;
    }
    if (flg & 2) at += 2;   // FHCRC
    if (at > left) throw cut();
    if (!have_bc) throw Error(kMsg, "gzip: not blocked gzip: a member without the BC subfield" + where);
    const uint64_t total = (uint64_t)bsize + 1;
    if (total > left) throw Error(kMsg, "gzip: BSIZE runs past the end of the bytes" + where);
    if (at + 8 > total) throw cut();
    InflateMember m;
    m.payload_off = off + at;
    m.payload_len = (uint32_t)(total - at - 8);
    m.crc = le32(h + total - 8);
    m.isize = le32(h + total - 4);
    m.out_off = g->inflated;
    m.pad = 0;
    if (m.isize > inflate::kMaxMember) throw Error(kMsg, "gzip: ISIZE above 65536" + where);
    g->members.push_back(m);
    g->header_off.push_back(off);
    g->inflated += m.isize;
    off += total;
  }
}

void gzip_inflate_dev(const Gzip& g, const uint8_t* data_dev, uint64_t len, uint8_t* out_dev, uint64_t out_cap, bool verify_crc,
                      uint8_t* status_out, hipStream_t s, Device& dev) {
  if (len != g.len) throw Error(kMsg, "gzip: the member table was scanned from " + std::to_string(g.len) + " bytes, not " + std::to_string(len));
  if (out_cap < g.inflated) throw Error(kMsg, "gzip: the output holds " + std::to_string(out_cap) + " bytes, the text has " + std::to_string(g.inflated));
  const uint64_t n = g.members.size();
  if (n == 0) return;
  require(data_dev, "data_dev");
  if (g.inflated) require(out_dev, "out_dev");
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  Workspace ws(s);
  InflateMember* members = ws.take<InflateMember>(n);
  uint8_t* status = ws.take<uint8_t>(n);
  unsigned long long* err = ws.take<unsigned long long>(1);
  unsigned long long low = ~0ull;
  HIP_CHECK(hipMemcpyAsync(members, g.members.data(), n * sizeof(InflateMember), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(err, 0xff, 8, s));
  dev.prof_begin(s);
  launch_inflate(data_dev, members, n, out_dev, verify_crc, status, err, dev, s);
  dev.prof_end("inflate", s);
  HIP_CHECK(hipMemcpyAsync(&low, err, 8, hipMemcpyDeviceToHost, s));
  if (status_out) HIP_CHECK(hipMemcpyAsync(status_out, status, n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (low != ~0ull) {
    const uint64_t m = low >> 8;
    throw Error(kMsg, std::string("gzip: ") + reason_text((uint32_t)(low & 0xff)) + at_member(m, m < n ? g.header_off[m] : 0));
  }
}

void gzip_inflate_host(const uint8_t* data, uint64_t len, uint8_t* out_dev, uint64_t out_cap, bool verify_crc, uint8_t* status_out,
                       Device& dev) {
  Gzip g;
  gzip_scan(&g, data, len);
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  Workspace ws(s);
  uint8_t* data_dev = ws.take<uint8_t>(len);
  if (len) HIP_CHECK(hipMemcpyAsync(data_dev, data, len, hipMemcpyHostToDevice, s));
  gzip_inflate_dev(g, data_dev, len, out_dev, out_cap, verify_crc, status_out, s, dev);
}

}  // namespace smh
