// signature.cpp -- the Signature container and its JSON wire format (".sig" v0.4).
//
// Host only.  Restates reference src/lib.rs:62-139 (KmerMinHash Serialize / Deserialize incl.
// the md5sum of ksize + decimal mins), 546-675 (Signature, load_signatures, PartialEq).  The
// writer reproduces serde_json's compact output (field order of the Serialize impls, no spaces).
#include "signature.hpp"
#include "sigjson.hpp"
#include "sigtext_core.hpp"

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
// the md5sum field of serialised sketches (src/lib.rs:72-77,86): MD5 itself is sigtext_core.hpp's, shared with the device
// writer
std::string sketch_md5(const KmerMinHash& mh) {
  mh.materialize();
  sigtext::Md5 m;
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
