// sigjson.hpp -- the JSON document model and parser of the signature wire format (what serde_json accepts for these types),
// and what a signature document says, field by field.  Host only and free of HIP, so that tests/c_sigscan_host.cpp builds it
// with a plain compiler; signature.cpp (the host loader) and sigscan.cpp (the device route) both read
// documents through it, so the object semantics -- keys, nulls, defaults, Q9, unknown fields, escapes -- exist once.
//
// The parser has two modes.  Plain: the text is the document.  With holes (JParser::holes set): the text is a SKELETON, the
// document with the bytes of every number span removed (sigscan_core.hpp), and the k-th '[' stands for an array whose leading
// elements are span k's tokens; they are never made into values.  The rules by which the rest of the array must follow are
// in include/sourmash_amd.h, "Signature JSON on the device".
#pragma once
#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <utility>
#include <vector>

#include "sigscan_core.hpp"

namespace smh {

// what a document is refused with; split_float: the one deliberate deviation of the device route (a message of its own)
// (A std::exception, so that a landing pad that knows nothing of this header still catches it; the two routes turn it into
// the library's Error with the code that fits.)
struct JsonError : std::exception {
  std::string message;
  bool split_float = false;
  uint64_t at = 0;   // holes mode: byte offset in the document's text
  JsonError(std::string m, bool split, uint64_t where) : message(std::move(m)), split_float(split), at(where) {}
  const char* what() const noexcept override { return message.c_str(); }
};

struct JVal {
  enum Kind { Null, Bool, UInt, NegInt, Float, Str, Arr, Obj } kind = Null;
  bool b = false;
  uint64_t u = 0;     // UInt: value; NegInt: magnitude
  double f = 0.0;
  int64_t span = -1;  // Arr, holes mode: the span whose tokens are the array's leading elements
  std::string s;
  std::vector<JVal> arr;
  std::vector<std::pair<std::string, JVal>> obj;
  const JVal* get(const char* key) const {
    const JVal* found = nullptr;
    for (auto& kv : obj) if (kv.first == key) found = &kv.second;  // serde: duplicate -> error; keep last
    return found;
  }
};

[[noreturn]] inline void serde_error(const std::string& m) { throw JsonError{m, false, 0}; }

// a string as serde_json writes it: quoted, with the short escapes and \u00xx for the other control bytes; everything from
// 0x20 on, UTF-8 included, as it is.  The one writer of strings: signature.cpp and the device route (sigtext.cpp) both use it.
inline void json_escape(std::string& out, const std::string& s) {
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

// The spans of one document, for a parse with holes.  rows[first .. first + n) are the document's own; doc_begin / doc_end are
// its bounds in the text the spans were cut from.
struct Holes {
  const sigscan::SpanRow* rows = nullptr;
  uint64_t n = 0;
  uint64_t doc_begin = 0, doc_end = 0;
};

struct JParser {
  const char* p;
  const char* end;
  int depth = 0;
  const Holes* holes = nullptr;
  uint64_t next_span = 0;
  const char* begin = nullptr;
  uint64_t removed = 0;        // holes mode: span bytes in front of p
  void ws() { while (p < end && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) p++; }
  // holes mode: where p stands in the document's own text
  uint64_t text_offset() const { return begin ? (uint64_t)(p - begin) + removed : 0; }
  [[noreturn]] void fail(const char* what) { throw JsonError{std::string("JSON error: ") + what, false, text_offset()}; }

  void parse_string(std::string& out) {
    if (p >= end || *p != '"') fail("expected string");
    p++;
    while (true) {
      if (p >= end) fail("EOF while parsing a string");
      unsigned char c = (unsigned char)*p++;
      if (c == '"') break;
      if (c < 0x20) fail("control character in string");
      if (c != '\\') { out.push_back((char)c); continue; }
      if (p >= end) fail("EOF in escape");
      char e = *p++;
      switch (e) {
        case '"': out.push_back('"'); break;
        case '\\': out.push_back('\\'); break;
        case '/': out.push_back('/'); break;
        case 'b': out.push_back('\b'); break;
        case 'f': out.push_back('\f'); break;
        case 'n': out.push_back('\n'); break;
        case 'r': out.push_back('\r'); break;
        case 't': out.push_back('\t'); break;
        case 'u': {
          auto hex4 = [&]() {
            if (end - p < 4) fail("EOF in \\u escape");
            uint32_t v = 0;
            for (int i = 0; i < 4; i++) {
              char h = *p++;
              v <<= 4;
              if (h >= '0' && h <= '9') v |= h - '0';
              else if (h >= 'a' && h <= 'f') v |= h - 'a' + 10;
              else if (h >= 'A' && h <= 'F') v |= h - 'A' + 10;
              else fail("invalid escape");
            }
            return v;
          };
          uint32_t cp = hex4();
          if (cp >= 0xD800 && cp <= 0xDBFF) {
            if (end - p < 2 || p[0] != '\\' || p[1] != 'u') fail("lone surrogate");
            p += 2;
            uint32_t lo = hex4();
            if (lo < 0xDC00 || lo > 0xDFFF) fail("lone surrogate");
            cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
          } else if (cp >= 0xDC00 && cp <= 0xDFFF) fail("lone surrogate");
          if (cp < 0x80) out.push_back((char)cp);
          else if (cp < 0x800) { out.push_back((char)(0xC0 | (cp >> 6))); out.push_back((char)(0x80 | (cp & 0x3F))); }
          else if (cp < 0x10000) {
            out.push_back((char)(0xE0 | (cp >> 12))); out.push_back((char)(0x80 | ((cp >> 6) & 0x3F)));
            out.push_back((char)(0x80 | (cp & 0x3F)));
          } else {
            out.push_back((char)(0xF0 | (cp >> 18))); out.push_back((char)(0x80 | ((cp >> 12) & 0x3F)));
            out.push_back((char)(0x80 | ((cp >> 6) & 0x3F))); out.push_back((char)(0x80 | (cp & 0x3F)));
          }
          break;
        }
        default: fail("invalid escape");
      }
    }
  }

  void parse_number(JVal& v) {
    const char* s = p;
    bool neg = false;
    if (*p == '-') { neg = true; p++; }
    if (p >= end || !isdigit((unsigned char)*p)) fail("invalid number");
    bool is_float = false, overflow = false;
    uint64_t acc = 0;
    if (*p == '0') { p++; }
    else while (p < end && isdigit((unsigned char)*p)) {
      uint64_t d = (uint64_t)(*p - '0');
      if (acc > (UINT64_MAX - d) / 10) overflow = true; else acc = acc * 10 + d;
      p++;
    }
    if (p < end && *p == '.') { is_float = true; p++; if (p >= end || !isdigit((unsigned char)*p)) fail("invalid number"); while (p < end && isdigit((unsigned char)*p)) p++; }
    if (p < end && (*p == 'e' || *p == 'E')) {
      is_float = true; p++;
      if (p < end && (*p == '+' || *p == '-')) p++;
      if (p >= end || !isdigit((unsigned char)*p)) fail("invalid number");
      while (p < end && isdigit((unsigned char)*p)) p++;
    }
    if (is_float || overflow) { v.kind = JVal::Float; v.f = strtod(std::string(s, p).c_str(), nullptr); }
    else if (neg) { v.kind = JVal::NegInt; v.u = acc; v.f = -(double)acc; }
    else { v.kind = JVal::UInt; v.u = acc; v.f = (double)acc; }
  }

  // Holes mode, p behind a '[': takes the array's span and says how the array must go on -- 0: either way (']' or a value),
  // 1: with a value, 2: with ']'.
  int take_span(JVal& v) {
    if (next_span >= holes->n) fail("more arrays than spans");   // (not for a text scanned from its first byte: both sides count the same brackets)
    const sigscan::SpanRow& r = holes->rows[next_span];
    v.span = (int64_t)next_span++;
    if (r.end >= holes->doc_end) fail("EOF while parsing a list");
    removed += r.end - r.start;
    if (r.status == sigscan::kBadSyntax) {
      throw JsonError{"JSON error: malformed number or separator in an array", false, r.bad_off - holes->doc_begin};
    }
    if (r.last_state == sigscan::kSpanTok && p < end && (*p == '.' || *p == 'e' || *p == 'E'))
      throw JsonError{"a number with a fraction or an exponent inside an array", true, r.end - holes->doc_begin};
    if (r.n_tokens && depth + 1 > 128) fail("recursion limit exceeded");   // (each number is a value one level down)
    if (r.status == sigscan::kOpen) return 1;
    return r.n_tokens ? 2 : 0;
  }

  void parse_value(JVal& v) {
    ws();
    if (p >= end) fail("EOF while parsing a value");
    if (++depth > 128) fail("recursion limit exceeded");
    char c = *p;
    if (c == '{') {
      v.kind = JVal::Obj; p++; ws();
      if (p < end && *p == '}') { p++; }
      else while (true) {
        ws();
        std::string k; parse_string(k);
        ws();
        if (p >= end || *p != ':') fail("expected ':'");
        p++;
        v.obj.emplace_back(std::move(k), JVal());
        parse_value(v.obj.back().second);
        ws();
        if (p < end && *p == ',') { p++; continue; }
        if (p < end && *p == '}') { p++; break; }
        fail("expected ',' or '}'");
      }
    } else if (c == '[') {
      v.kind = JVal::Arr; p++;
      const int how = holes ? take_span(v) : 0;
      ws();
      if (how == 2) {
        if (p < end && *p == ']') p++;
        else fail("expected ',' or ']'");
      } else if (how == 0 && p < end && *p == ']') { p++; }
      else while (true) {
        v.arr.emplace_back();
        parse_value(v.arr.back());
        ws();
        if (p < end && *p == ',') { p++; continue; }
        if (p < end && *p == ']') { p++; break; }
        fail("expected ',' or ']'");
      }
    } else if (c == '"') { v.kind = JVal::Str; parse_string(v.s); }
    else if (c == 't' && end - p >= 4 && !memcmp(p, "true", 4)) { v.kind = JVal::Bool; v.b = true; p += 4; }
    else if (c == 'f' && end - p >= 5 && !memcmp(p, "false", 5)) { v.kind = JVal::Bool; v.b = false; p += 5; }
    else if (c == 'n' && end - p >= 4 && !memcmp(p, "null", 4)) { v.kind = JVal::Null; p += 4; }
    else if (c == '-' || isdigit((unsigned char)c)) parse_number(v);
    else fail("expected value");
    depth--;
  }
};

inline uint64_t want_uint(const JVal* v, const char* field, uint64_t maxv) {
  if (!v) serde_error(std::string("missing field `") + field + "`");
  if (v->kind != JVal::UInt || v->u > maxv) serde_error(std::string("invalid type for field `") + field + "`");
  return v->u;
}
inline const std::string& want_str(const JVal* v, const char* field) {
  if (!v) serde_error(std::string("missing field `") + field + "`");
  if (v->kind != JVal::Str) serde_error(std::string("invalid type for field `") + field + "`: expected a string");
  return v->s;
}
// An array read as u64.  Plain: every element is one.  With holes: the array is its span alone and no token is above 2^64 - 1.
inline const JVal& want_u64_array(const JVal* v, const char* field, const Holes* holes) {
  if (!v) serde_error(std::string("missing field `") + field + "`");
  if (v->kind != JVal::Arr) serde_error(std::string("invalid type for field `") + field + "`: expected a sequence");
  for (auto& e : v->arr)
    if (holes || e.kind != JVal::UInt) serde_error(std::string("invalid type in `") + field + "`: expected u64");
  if (holes && holes->rows[v->span].status == sigscan::kOverflow) serde_error(std::string("invalid type in `") + field + "`: expected u64");
  return *v;
}

// What one sketch of a document says (reference src/lib.rs:104-139).  molecule: 0 DNA, 1 protein, 2 dayhoff, 3 hp.
struct SketchFields {
  uint32_t num = 0, ksize = 0;
  uint64_t seed = 0, max_hash = 0;
  std::string md5sum;
  uint8_t molecule = 0;
  bool has_abunds = false;
  const JVal* mins = nullptr;     // the arrays themselves: their elements (plain) or their span (holes)
  const JVal* abunds = nullptr;   // null unless has_abunds
};

inline SketchFields sketch_fields(const JVal& v, const Holes* holes) {
  if (v.kind != JVal::Obj) serde_error("invalid type: expected struct TempSig");
  SketchFields f;
  const uint32_t num = (uint32_t)want_uint(v.get("num"), "num", UINT32_MAX);
  f.ksize = (uint32_t)want_uint(v.get("ksize"), "ksize", UINT32_MAX);
  f.seed = want_uint(v.get("seed"), "seed", UINT64_MAX);
  f.max_hash = want_uint(v.get("max_hash"), "max_hash", UINT64_MAX);
  f.md5sum = want_str(v.get("md5sum"), "md5sum");
  f.mins = &want_u64_array(v.get("mins"), "mins", holes);
  const JVal* ab = v.get("abundances");
  if (ab && ab->kind != JVal::Null) { f.has_abunds = true; f.abunds = &want_u64_array(ab, "abundances", holes); }
  const std::string& mol = want_str(v.get("molecule"), "molecule");
  // anything else reads as DNA (Q9); dayhoff / hp are this library's own (include/sourmash_amd.h "alphabets")
  f.molecule = mol == "protein" ? 1 : mol == "dayhoff" ? 2 : mol == "hp" ? 3 : 0;
  f.num = f.max_hash != 0 ? 0 : num;          // Q9
  return f;
}

// What one signature of a document says (reference src/lib.rs:546-577), without its sketches.
struct SignatureFields {
  std::string klass = "sourmash_signature", email, hash_function, filename, name, license = "CC0";
  bool has_filename = false, has_name = false;
  double version = 0.4;
  const JVal* sketches = nullptr;   // the `signatures` array
};

inline SignatureFields signature_fields(const JVal& v) {
  if (v.kind != JVal::Obj) serde_error("invalid type: expected struct Signature");
  SignatureFields s;
  if (const JVal* c = v.get("class")) s.klass = want_str(c, "class");
  if (const JVal* e = v.get("email")) s.email = want_str(e, "email");
  s.hash_function = want_str(v.get("hash_function"), "hash_function");
  if (const JVal* f = v.get("filename")) { if (f->kind != JVal::Null) { s.has_filename = true; s.filename = want_str(f, "filename"); } }
  if (const JVal* n = v.get("name")) { if (n->kind != JVal::Null) { s.has_name = true; s.name = want_str(n, "name"); } }
  if (const JVal* l = v.get("license")) s.license = want_str(l, "license");
  const JVal* sk = v.get("signatures");
  if (!sk) serde_error("missing field `signatures`");
  if (sk->kind != JVal::Arr) serde_error("invalid type for field `signatures`: expected a sequence");
  s.sketches = sk;
  return s;
}
// (the version is read behind the sketches, as the derive does)
inline double signature_version(const JVal& v, double dflt) {
  if (const JVal* ver = v.get("version")) {
    if (ver->kind == JVal::UInt || ver->kind == JVal::NegInt || ver->kind == JVal::Float) return ver->f;
    serde_error("invalid type for field `version`: expected f64");
  }
  return dflt;
}

// One document parsed whole (reference src/lib.rs:585-591 from_reader: a JSON array of signatures): *root receives it.
inline void parse_document(const char* data, size_t len, const Holes* holes, JVal* root) {
  JParser ps{data, data + len};
  ps.holes = holes;
  ps.begin = holes ? data : nullptr;
  ps.parse_value(*root);
  ps.ws();
  if (ps.p != ps.end) ps.fail("trailing characters");
  if (root->kind != JVal::Arr) serde_error("invalid type: expected a sequence");
}

// Document d of a text = text[b, e): its part of the skeleton and its spans.  spans: the whole text's table;
// removed[k] = the span bytes in front of span k (spans.size() + 1 entries, removed_prefix).
inline std::vector<uint64_t> removed_prefix(const std::vector<sigscan::SpanRow>& spans) {
  std::vector<uint64_t> removed(spans.size() + 1, 0);
  for (size_t k = 0; k < spans.size(); k++) removed[k + 1] = removed[k] + (spans[k].end - spans[k].start);
  return removed;
}
struct DocSlice {
  Holes holes;
  uint64_t first_span = 0;             // the document's first row in the whole table
  uint64_t skel_begin = 0, skel_end = 0;
};
inline DocSlice slice_document(const std::vector<sigscan::SpanRow>& spans, const std::vector<uint64_t>& removed, uint64_t b, uint64_t e) {
  auto spans_upto = [&](uint64_t t) {   // the spans whose '[' lies in front of text offset t
    size_t lo = 0, hi = spans.size();
    while (lo < hi) { const size_t mid = (lo + hi) / 2; if (spans[mid].start <= t) lo = mid + 1; else hi = mid; }
    return (uint64_t)lo;
  };
  auto kept_before = [&](uint64_t t) {  // skeleton bytes in front of text offset t
    size_t lo = 0, hi = spans.size();
    while (lo < hi) { const size_t mid = (lo + hi) / 2; if (spans[mid].start < t) lo = mid + 1; else hi = mid; }
    uint64_t gone = removed[lo];
    if (lo && spans[lo - 1].end > t) gone -= spans[lo - 1].end - t;   // a span that crosses t
    return t - gone;
  };
  DocSlice s;
  s.first_span = spans_upto(b);
  s.holes.rows = spans.data() + s.first_span;
  s.holes.n = spans_upto(e) - s.first_span;
  s.holes.doc_begin = b; s.holes.doc_end = e;
  s.skel_begin = kept_before(b); s.skel_end = kept_before(e);
  return s;
}

// The walk both routes share: of every signature of a parsed document first its sketches, in order, then the signature itself
// (its version is read last, as the derive does).  With holes a number where a signature or a sketch should stand is a token.
template <class OnSketch, class OnSignature>
inline void walk_document(const JVal& root, const Holes* holes, OnSketch&& on_sketch, OnSignature&& on_signature) {
  if (holes && holes->rows[root.span].n_tokens) serde_error("invalid type: expected struct Signature");
  for (size_t i = 0; i < root.arr.size(); i++) {
    const JVal& sv = root.arr[i];
    SignatureFields s = signature_fields(sv);
    if (holes && holes->rows[s.sketches->span].n_tokens) serde_error("invalid type: expected struct TempSig");
    for (size_t k = 0; k < s.sketches->arr.size(); k++) on_sketch(i, k, sketch_fields(s.sketches->arr[k], holes));
    s.version = signature_version(sv, s.version);
    on_signature(i, s);
  }
}

}  // namespace smh
