// signature.cpp -- the Signature container and its JSON wire format (".sig" v0.4).
//
// Host only.  Restates reference src/lib.rs:62-139 (KmerMinHash Serialize / Deserialize incl.
// the md5sum of ksize + decimal mins), 546-675 (Signature, load_signatures, PartialEq).  The
// writer reproduces serde_json's compact output (field order of the Serialize impls, no spaces).
#include "signature.hpp"
#include "sigjson.hpp"

#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>

namespace smh {

// ------------------------------------------------------------------------------------
// MD5 (RFC 1321) -- only for the md5sum field of serialised sketches (src/lib.rs:72-77,86)
namespace {

struct Md5 {
  uint32_t a = 0x67452301, b = 0xefcdab89, c = 0x98badcfe, d = 0x10325476;
  uint64_t total = 0;
  uint8_t buf[64];
  size_t fill = 0;

  static uint32_t rol(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }

  void block(const uint8_t* p) {
    static const uint32_t K[64] = {
        0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501,
        0x698098d8, 0x8b44f7af, 0xffff5bb1, 0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821,
        0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453, 0xd8a1e681, 0xe7d3fbc8,
        0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a,
        0xfffa3942, 0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70,
        0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05, 0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665,
        0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d, 0x85845dd1,
        0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391};
    static const int S[64] = {7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22,
                              5, 9,  14, 20, 5, 9,  14, 20, 5, 9,  14, 20, 5, 9,  14, 20,
                              4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23,
                              6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21};
    uint32_t M[16];
    for (int i = 0; i < 16; i++)
      M[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
             ((uint32_t)p[4 * i + 3] << 24);
    uint32_t A = a, B = b, C = c, D = d;
    for (int i = 0; i < 64; i++) {
      uint32_t F;
      int g;
      if (i < 16) { F = (B & C) | (~B & D); g = i; }
      else if (i < 32) { F = (D & B) | (~D & C); g = (5 * i + 1) & 15; }
      else if (i < 48) { F = B ^ C ^ D; g = (3 * i + 5) & 15; }
      else { F = C ^ (B | ~D); g = (7 * i) & 15; }
      F = F + A + K[i] + M[g];
      A = D; D = C; C = B;
      B = B + rol(F, S[i]);
    }
    a += A; b += B; c += C; d += D;
  }

  void update(const void* data, size_t n) {
    const uint8_t* p = (const uint8_t*)data;
    total += n;
    while (n) {
      size_t take = std::min(n, (size_t)64 - fill);
      memcpy(buf + fill, p, take);
      fill += take; p += take; n -= take;
      if (fill == 64) { block(buf); fill = 0; }
    }
  }

  std::string hex() {
    uint64_t bits = total * 8;
    uint8_t pad = 0x80;
    update(&pad, 1);
    uint8_t z = 0;
    while (fill != 56) update(&z, 1);
    uint8_t len[8];
    for (int i = 0; i < 8; i++) len[i] = (uint8_t)(bits >> (8 * i));
    update(len, 8);
    uint32_t w[4] = {a, b, c, d};
    char out[33];
    for (int i = 0; i < 16; i++) snprintf(out + 2 * i, 3, "%02x", (w[i / 4] >> (8 * (i % 4))) & 0xff);
    return std::string(out, 32);
  }
};

}  // namespace

std::string sketch_md5(const KmerMinHash& mh) {
  mh.materialize();
  Md5 m;
  std::string k = std::to_string(mh.ksize);
  m.update(k.data(), k.size());
  char tmp[24];
  for (uint64_t v : mh.mins) {
    int n = snprintf(tmp, sizeof tmp, "%llu", (unsigned long long)v);
    m.update(tmp, (size_t)n);
  }
  return m.hex();
}

// ------------------------------------------------------------------------------------
// the JSON document model, its parser and the fields of a document: sigjson.hpp (shared with the device route, sigscan.cpp)
namespace {

[[noreturn]] void rethrow(const JsonError& e) { throw Error(kSerdeError, e.message); }

std::vector<uint64_t> u64_elements(const JVal& v) {
  std::vector<uint64_t> out;
  out.reserve(v.arr.size());
  for (auto& e : v.arr) out.push_back(e.u);
  return out;
}

// reference src/lib.rs:104-139
KmerMinHash sketch_from_fields(const SketchFields& f) {
  static_assert(kMoleculeDNA == 0 && kMoleculeProtein == 1 && kMoleculeDayhoff == 2 && kMoleculeHp == 3, "sigjson.hpp's molecule numbers");
  KmerMinHash mh;
  mh.ksize = f.ksize;
  mh.seed = f.seed;
  mh.max_hash = f.max_hash;
  mh.mins = u64_elements(*f.mins);
  mh.has_abunds = f.has_abunds;
  if (f.has_abunds) mh.abunds = u64_elements(*f.abunds);
  else mh.abunds.clear();
  mh.molecule = f.molecule;
  mh.is_protein = mh.molecule != kMoleculeDNA;
  mh.num = f.num;
  return mh;
}

void json_escape(std::string& out, const std::string& s) {
  out.push_back('"');
  for (unsigned char c : s) {
    switch (c) {
      case '"': out += "\\\""; break;
      case '\\': out += "\\\\"; break;
      case '\b': out += "\\b"; break;
      case '\f': out += "\\f"; break;
      case '\n': out += "\\n"; break;
      case '\r': out += "\\r"; break;
      case '\t': out += "\\t"; break;
      default:
        if (c < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", c); out += b; }
        else out.push_back((char)c);
    }
  }
  out.push_back('"');
}

// shortest decimal that round-trips, in serde_json's (ryu) style for the values a version takes
std::string f64_to_json(double v) {
  if (!std::isfinite(v)) return "null";
  char b[40];
  for (int prec = 1; prec <= 17; prec++) {
    snprintf(b, sizeof b, "%.*g", prec, v);
    if (strtod(b, nullptr) == v) break;
  }
  std::string s(b);
  if (s.find_first_of(".eEn") == std::string::npos) s += ".0";
  return s;
}

void u64_array(std::string& out, const std::vector<uint64_t>& v) {
  out.push_back('[');
  char tmp[24];
  for (size_t i = 0; i < v.size(); i++) {
    if (i) out.push_back(',');
    int n = snprintf(tmp, sizeof tmp, "%llu", (unsigned long long)v[i]);
    out.append(tmp, (size_t)n);
  }
  out.push_back(']');
}

// reference src/lib.rs:62-102
void sketch_to_json(std::string& out, const KmerMinHash& mh) {
  mh.materialize();
  out += "{\"num\":" + std::to_string(mh.num);
  out += ",\"ksize\":" + std::to_string(mh.ksize);
  out += ",\"seed\":" + std::to_string(mh.seed);
  out += ",\"max_hash\":" + std::to_string(mh.max_hash);
  out += ",\"mins\":";
  u64_array(out, mh.mins);
  out += ",\"md5sum\":\"" + sketch_md5(mh) + "\"";
  if (mh.has_abunds) { out += ",\"abundances\":"; u64_array(out, mh.abunds); }
  out += std::string(",\"molecule\":\"") + molecule_name(mh.molecule) + "\"}";
}

}  // namespace

bool sketch_equal(const KmerMinHash& a, const KmerMinHash& b) {
  a.materialize();
  b.materialize();
  return a.num == b.num && a.ksize == b.ksize && a.molecule == b.molecule && a.seed == b.seed &&
         a.max_hash == b.max_hash && a.mins.get() == b.mins.get() && a.has_abunds == b.has_abunds &&
         (!a.has_abunds || a.abunds == b.abunds);
}

// derive(Serialize) field order of reference src/lib.rs:546-565
void signature_to_json(std::string& out, const Signature& s) {
  out += "{\"class\":"; json_escape(out, s.klass);
  out += ",\"email\":"; json_escape(out, s.email);
  out += ",\"hash_function\":"; json_escape(out, s.hash_function);
  out += ",\"filename\":"; if (s.has_filename) json_escape(out, s.filename); else out += "null";
  out += ",\"name\":"; if (s.has_name) json_escape(out, s.name); else out += "null";
  out += ",\"license\":"; json_escape(out, s.license);
  out += ",\"signatures\":[";
  for (size_t i = 0; i < s.signatures.size(); i++) {
    if (i) out.push_back(',');
    sketch_to_json(out, s.signatures[i]);
  }
  out += "],\"version\":" + f64_to_json(s.version) + "}";
}

std::string signatures_to_json(const std::vector<const Signature*>& v) {
  std::string out = "[";
  for (size_t i = 0; i < v.size(); i++) {
    if (i) out.push_back(',');
    signature_to_json(out, *v[i]);
  }
  out.push_back(']');
  return out;
}

// reference src/lib.rs:585-591 from_reader: a JSON array of signatures
std::vector<Signature> signatures_from_json(const char* data, size_t len) {
  try {
    JVal root;
    parse_document(data, len, nullptr, &root);
    std::vector<Signature> out;
    out.reserve(root.arr.size());
    std::vector<KmerMinHash> sketches;
    walk_document(root, nullptr,
                  [&](size_t, size_t, const SketchFields& f) { sketches.push_back(sketch_from_fields(f)); },
                  [&](size_t, const SignatureFields& f) {   // reference src/lib.rs:546-577
                    Signature s;
                    s.klass = f.klass; s.email = f.email; s.hash_function = f.hash_function;
                    s.has_filename = f.has_filename; s.filename = f.filename;
                    s.has_name = f.has_name; s.name = f.name;
                    s.license = f.license; s.version = f.version;
                    s.signatures = std::move(sketches);
                    sketches.clear();
                    out.push_back(std::move(s));
                  });
    return out;
  } catch (const JsonError& e) { rethrow(e); }
}

// reference src/lib.rs:593-645 load_signatures: one Signature per sketch, filtered
std::vector<Signature> load_signatures(const char* data, size_t len, size_t ksize, const char* moltype) {
  std::vector<Signature> orig = signatures_from_json(data, len);
  std::string mt;
  if (moltype) for (const char* c = moltype; *c; c++) mt.push_back((char)tolower((unsigned char)*c));
  std::vector<Signature> out;
  for (auto& s : orig) {
    for (auto& mh : s.signatures) {
      if (!(ksize == 0 || ksize == (size_t)mh.ksize)) continue;
      if (moltype && !((mt == "dna" && mh.molecule == kMoleculeDNA) || (mt == "protein" && mh.molecule == kMoleculeProtein) ||
                        (mt == "dayhoff" && mh.molecule == kMoleculeDayhoff) || (mt == "hp" && mh.molecule == kMoleculeHp))) continue;
      Signature one = s;
      one.signatures.clear();
      one.signatures.push_back(mh);
      out.push_back(std::move(one));
    }
  }
  return out;
}

bool signature_equal(const Signature& a, const Signature& b) {
  // reference src/lib.rs:663-675: metadata + first sketch; indexing an empty list panics
  if (a.signatures.empty() || b.signatures.empty()) throw_panic("index out of bounds: the len is 0 but the index is 0");
  bool meta = a.klass == b.klass && a.email == b.email && a.hash_function == b.hash_function &&
              a.has_filename == b.has_filename && (!a.has_filename || a.filename == b.filename) &&
              a.has_name == b.has_name && (!a.has_name || a.name == b.name);
  return meta && sketch_equal(a.signatures[0], b.signatures[0]);
}

SbtJson sbt_json_from(const char* data, size_t len) {
  try {
    JParser ps{data, data + len};
    JVal root;
    ps.parse_value(root);
    ps.ws();
    if (ps.p != ps.end) serde_error("JSON error: trailing characters");
    if (root.kind != JVal::Obj) serde_error("invalid type: expected struct SBTInfo");
    SbtJson out;
    out.d = (uint32_t)want_uint(root.get("d"), "d", UINT32_MAX);
    out.version = (uint32_t)want_uint(root.get("version"), "version", UINT32_MAX);
    const JVal* st = root.get("storage");
    if (!st || st->kind != JVal::Obj) serde_error("missing field `storage`");
    const JVal* args = st->get("args");
    if (!args || args->kind != JVal::Obj) serde_error("missing field `args`");
    out.storage_path = want_str(args->get("path"), "path");
    const JVal* fac = root.get("factory");
    if (!fac || fac->kind != JVal::Obj) serde_error("missing field `factory`");
    out.factory_args = u64_elements(want_u64_array(fac->get("args"), "args", nullptr));
    auto entries = [&](const char* field, std::vector<SbtJsonEntry>& v, bool node) {
      const JVal* m = root.get(field);
      if (!m) serde_error(std::string("missing field `") + field + "`");
      if (m->kind != JVal::Obj) serde_error(std::string("invalid type for field `") + field + "`: expected a map");
      for (auto& kv : m->obj) {
        SbtJsonEntry e;
        char* endp = nullptr;
        if (kv.first.empty() || !isdigit((unsigned char)kv.first[0])) serde_error("invalid map key: expected u64");
        e.pos = strtoull(kv.first.c_str(), &endp, 10);
        if (*endp) serde_error("invalid map key: expected u64");
        e.filename = want_str(kv.second.get("filename"), "filename");
        e.name = want_str(kv.second.get("name"), "name");
        if (node) {
          const JVal* md = kv.second.get("metadata");
          if (!md || md->kind != JVal::Obj) serde_error("invalid type for field `metadata`: expected a map");
          if (const JVal* mn = md->get("min_n_below")) {
            e.has_min_n_below = true;
            e.min_n_below = want_uint(mn, "min_n_below", UINT64_MAX);
          }
        }
        v.push_back(std::move(e));
      }
    };
    entries("nodes", out.nodes, true);
    entries("leaves", out.leaves, false);
    return out;
  } catch (const JsonError& e) { rethrow(e); }
}

std::string read_file(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw Error(kIo, "No such file or directory (os error 2)");
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

}  // namespace smh
