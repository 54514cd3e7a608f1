// archive_core.hpp -- zip collections (the rules are in include/sourmash_amd.h, "Zip collections"), as one
// source for the library (archive.cpp, archive_kernels.hip) and for a plain host build (tests/c_archive_host.cpp):
//   * the arithmetic the kernels share with the host: how a member's text is cut into chunks, which member a chunk belongs
//     to, a chunk's CRC register from state 0 and the fold of the chunk registers into the member's CRC-32 (SMH_HD);
//   * the scan of the container: end record, zip64 records, central directory, local headers, each entry's kind (host only;
//     no device is touched and no HIP header is needed).
// Every comparison of an offset with a length is written as a subtraction from the larger side, so that no sum of two
// numbers taken from the file can wrap.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "inflate_core.hpp"

namespace smh {
namespace archive {

// --- chunks and the fold ----------------------------------------------------------------------------------------------
// A member's text [0, size) is cut into chunks of kChunk bytes, the last one shorter; a text of 0 bytes has no chunk.  One
// wave takes one chunk and leaves run(0, chunk), the CRC register after the chunk's bytes from state 0.  With the identity
// of inflate_core.hpp, crc = ~(shift(~0, size) ^ XOR_c shift(run(0, chunk c), bytes behind chunk c)).
constexpr uint32_t kChunk = 16384;

SMH_HD inline uint64_t chunks_of(uint32_t size) { return ((uint64_t)size + kChunk - 1) / kChunk; }
SMH_HD inline uint32_t chunk_begin(uint32_t size, uint64_t c) {   // chunk c is [chunk_begin(c), chunk_begin(c + 1))
  const uint64_t at = c * kChunk;
  return at < size ? (uint32_t)at : size;
}
// prefix[m] = chunks of the members in front of m, n + 1 entries; w < prefix[n].  The member of chunk w is the LAST m with
// prefix[m] <= w: members without a chunk share their successor's entry and are stepped over.
SMH_HD inline uint64_t member_of_chunk(const uint64_t* prefix, uint64_t n, uint64_t w) {
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (prefix[mid] <= w) lo = mid; else hi = mid;
  }
  return lo;
}
// lane i's share of run(0, p[0, n)): its slice run from 0 and shifted over the bytes behind it; the XOR over the lanes is
// the chunk's register
SMH_HD inline uint32_t chunk_lane_term(const uint8_t* p, uint32_t n, uint32_t lanes, uint32_t i, const uint32_t* table) {
  const uint32_t lo = inflate::crc_slice_begin(n, lanes, i), hi = inflate::crc_slice_begin(n, lanes, i + 1);
  return inflate::crc_shift(inflate::crc_run(0, p + lo, hi - lo, table), n - hi);
}
// lane i's share of the fold over a member's chunk registers (the lanes stride over the chunks); crc = ~XOR over the lanes
SMH_HD inline uint32_t fold_lane_term(const uint32_t* terms, uint64_t n_chunks, uint32_t size, uint32_t lanes, uint32_t i) {
  uint32_t x = i == 0 ? inflate::crc_shift(0xffffffffu, size) : 0;
  for (uint64_t c = i; c < n_chunks; c += lanes) x ^= inflate::crc_shift(terms[c], size - chunk_begin(size, c + 1));
  return x;
}

// --- the scan ---------------------------------------------------------------------------------------------------------
enum Kind : uint32_t { kStored = 0, kDeflate = 1, kGzip = 2, kDirectory = 3, kOther = 4 };

struct Entry {
  std::string name;
  std::string reason;            // why device_ok is false ("" otherwise)
  uint32_t method = 0, flags = 0, crc32 = 0, kind = kStored;
  bool device_ok = true;
  uint64_t comp_size = 0, size = 0;      // as the central directory (or its zip64 extra field) has them
  uint64_t header_off = 0, data_off = 0; // the local header; the entry's bytes are data[data_off, data_off + comp_size)
  // what a device inflate reads and writes (device_ok only): the DEFLATE stream of a deflate or gzip entry, the bytes of a
  // stored one; the size and CRC-32 of the text (gzip: ISIZE and CRC of the trailer)
  uint64_t payload_off = 0, payload_len = 0;
  uint32_t text_size = 0, text_crc = 0;
};

struct Archive {
  std::vector<Entry> entries;
  uint64_t len = 0;              // the bytes that were scanned
};

inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t le32(const uint8_t* p) { return le16(p) | le16(p + 2) << 16; }
inline uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | (uint64_t)le32(p + 4) << 32; }
inline bool sig_at(const uint8_t* p, uint8_t a, uint8_t b) { return p[0] == 'P' && p[1] == 'K' && p[2] == a && p[3] == b; }

// The RFC 1952 header of h[0, left), which begins 1f 8b 08, as gzip_scan reads it, without the BC requirement.  *at = the
// first byte behind the header.  False: the header, or the 8 bytes of the trailer behind it, do not fit.
inline bool gzip_header(const uint8_t* h, uint64_t left, uint64_t* at_out) {
  if (left < 10) return false;
  const uint32_t flg = h[3];
  uint64_t at = 10;
  if (flg & 4) {                 // FEXTRA
    if (left - at < 2) return false;
    const uint64_t xlen = le16(h + at);
    at += 2;
    if (left - at < xlen) return false;
    uint64_t sub = at;
    const uint64_t end = at + xlen;
    while (sub < end) {
      if (end - sub < 4) return false;
      const uint64_t slen = le16(h + sub + 2);
      if (end - sub - 4 < slen) return false;
      sub += 4 + slen;
    }
    at = end;
  }
  for (uint32_t bit = 8; bit <= 16; bit <<= 1) {   // FNAME, FCOMMENT: up to and with a NUL
    if (!(flg & bit)) continue;
    while (at < left && h[at] != 0) at++;
    if (at >= left) return false;
    at++;
  }
  if (flg & 2) at += 2;          // FHCRC
  if (at > left || left - at < 8) return false;
  *at_out = at;
  return true;
}

inline std::string at_byte(uint64_t off) { return " (at byte " + std::to_string(off) + ")"; }
inline std::string at_entry(uint64_t i, uint64_t off) { return " (entry " + std::to_string(i) + " at byte " + std::to_string(off) + ")"; }

// kind, device_ok and what the device reads, from the entry's fields and its first bytes
inline void classify(Entry* e, const uint8_t* d) {
  const uint8_t* p = d + e->data_off;
  if (!e->name.empty() && e->name.back() == '/' && e->size == 0) e->kind = kDirectory;
  else if (e->method == 8) e->kind = kDeflate;
  else if (e->method == 0) e->kind = (e->comp_size >= 3 && p[0] == 0x1f && p[1] == 0x8b && p[2] == 8) ? kGzip : kStored;
  else e->kind = kOther;
  const auto refuse = [&](const std::string& why) { e->device_ok = false; e->reason = why; };
  e->device_ok = true;
  e->payload_off = e->data_off; e->payload_len = 0; e->text_size = 0; e->text_crc = e->crc32;
  if (e->flags & 1) return refuse("encrypted entry");
  if (e->kind == kOther) return refuse("compression method " + std::to_string(e->method));
  if (e->comp_size >> 32 || e->size >> 32) return refuse("size of 2^32 or more");
  if (e->kind == kDirectory) return;
  if (e->method == 0 && e->comp_size != e->size) return refuse("stored entry whose sizes differ");
  if (e->kind == kGzip) {
    uint64_t at;
    if (!gzip_header(p, e->comp_size, &at)) return refuse("gzip entry shorter than its header and trailer");
    e->payload_off = e->data_off + at;
    e->payload_len = e->comp_size - at - 8;
    e->text_crc = le32(p + e->comp_size - 8);
    e->text_size = le32(p + e->comp_size - 4);
    return;
  }
  e->payload_len = e->comp_size;
  e->text_size = (uint32_t)e->size;
}

// Fills *a from data[0, len).  False: the archive is refused and *msg says why ("archive: ...").
inline bool scan(Archive* a, const uint8_t* d, uint64_t len, std::string* msg) {
  a->entries.clear();
  a->len = len;
  const auto refuse = [&](const std::string& why) { *msg = "archive: " + why; a->entries.clear(); return false; };
  // the end record: the LOWEST place in the last 22 + 65535 bytes where the signature stands and the comment length leads
  // exactly to the end of the data -- a record inside the true record's comment stands behind it
  if (len < 22) return refuse("no end-of-central-directory record" + at_byte(len));
  uint64_t p = len - 22, eocd = ~0ull;
  for (;;) {
    if (sig_at(d + p, 5, 6) && le16(d + p + 20) == len - 22 - p) eocd = p;
    if (p == 0 || len - 22 - p == 65535) break;
    p--;
  }
  if (eocd == ~0ull) return refuse("no end-of-central-directory record" + at_byte(len));
  uint64_t disk = le16(d + eocd + 4), cd_disk = le16(d + eocd + 6), n_here = le16(d + eocd + 8), n = le16(d + eocd + 10);
  uint64_t cd_size = le32(d + eocd + 12), cd_off = le32(d + eocd + 16), limit = eocd;
  if (eocd >= 20 && sig_at(d + eocd - 20, 6, 7)) {   // the zip64 locator, and the zip64 end record it points to
    const uint8_t* l = d + eocd - 20;
    if (le32(l + 4) != 0 || le32(l + 16) > 1) return refuse("multi-disk archive" + at_byte(eocd - 20));
    const uint64_t z = le64(l + 8);
    if (z > len || len - z < 56 || !sig_at(d + z, 6, 6)) return refuse("zip64 end record outside the data or without its signature" + at_byte(z));
    disk = le32(d + z + 16); cd_disk = le32(d + z + 20); n_here = le64(d + z + 24); n = le64(d + z + 32);
    cd_size = le64(d + z + 40); cd_off = le64(d + z + 48); limit = z;
  }
  if (disk != 0 || cd_disk != 0 || n_here != n) return refuse("multi-disk archive" + at_byte(eocd));
  if (cd_off > limit || cd_size > limit - cd_off) return refuse("central directory outside the data" + at_byte(cd_off));
  const uint64_t cd_end = cd_off + cd_size;
  uint64_t at = cd_off;
  for (uint64_t i = 0; i < n; i++) {
    if (cd_end - at < 46) return refuse("truncated central directory" + at_entry(i, at));
    const uint8_t* c = d + at;
    if (!sig_at(c, 1, 2)) return refuse("central directory entry without its signature" + at_entry(i, at));
    const uint64_t nlen = le16(c + 28), xlen = le16(c + 30), clen = le16(c + 32);
    if (cd_end - at - 46 < nlen + xlen + clen) return refuse("truncated central directory" + at_entry(i, at));
    Entry e;
    e.flags = le16(c + 8); e.method = le16(c + 10); e.crc32 = le32(c + 16);
    e.comp_size = le32(c + 20); e.size = le32(c + 24); e.header_off = le32(c + 42);
    uint64_t disk_start = le16(c + 34);
    e.name.assign(reinterpret_cast<const char*>(c + 46), nlen);
    // the zip64 extra field: the 8-byte size, compressed size and offset and the 4-byte disk, each present only when the
    // fixed field is all ones, in this order
    const bool want = e.size == 0xffffffffu || e.comp_size == 0xffffffffu || e.header_off == 0xffffffffu || disk_start == 0xffff;
    if (want) {
      const uint8_t* x = c + 46 + nlen;
      uint64_t k = 0;
      bool found = false;
      while (xlen - k >= 4) {
        const uint64_t id = le16(x + k), sz = le16(x + k + 2);
        if (sz > xlen - k - 4) break;
        if (id == 1) {
          uint64_t q = k + 4, left = sz;
          found = true;
          if (e.size == 0xffffffffu) { if (left < 8) { found = false; break; } e.size = le64(x + q); q += 8; left -= 8; }
          if (e.comp_size == 0xffffffffu) { if (left < 8) { found = false; break; } e.comp_size = le64(x + q); q += 8; left -= 8; }
          if (e.header_off == 0xffffffffu) { if (left < 8) { found = false; break; } e.header_off = le64(x + q); q += 8; left -= 8; }
          if (disk_start == 0xffff) { if (left < 4) { found = false; break; } disk_start = le32(x + q); }
          break;
        }
        k += 4 + sz;
      }
      if (!found) return refuse("zip64 extra field missing or cut short" + at_entry(i, at));
    }
    if (disk_start != 0) return refuse("multi-disk archive" + at_entry(i, at));
    const uint64_t lh = e.header_off;
    if (lh > len || len - lh < 30) return refuse("local header outside the data" + at_entry(i, lh));
    if (!sig_at(d + lh, 3, 4)) return refuse("local header without its signature" + at_entry(i, lh));
    e.data_off = lh + 30 + le16(d + lh + 26) + le16(d + lh + 28);   // the local header's own lengths
    if (e.data_off > len || e.comp_size > len - e.data_off) return refuse("entry data outside the data" + at_entry(i, e.data_off));
    classify(&e, d);
    a->entries.push_back(std::move(e));
    at += 46 + nlen + xlen + clen;
  }
  return true;
}

}  // namespace archive
}  // namespace smh
