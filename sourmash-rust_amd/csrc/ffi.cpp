// ffi.cpp -- the C ABI: every symbol of include/sourmash.h (the reference's surface, restating
// src/ffi.rs and src/utils.rs) and the additive MI355X entry points of include/sourmash_amd.h.
#include <cstddef>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <set>
#include <vector>

#include "../../include/sourmash_amd.h"
#include "minhash.hpp"
#include "sbt.hpp"
#include "signature.hpp"

using smh::Error;

struct KmerMinHash : smh::KmerMinHash {
  using smh::KmerMinHash::KmerMinHash;
  KmerMinHash() = default;
  KmerMinHash(const smh::KmerMinHash& o) : smh::KmerMinHash(o) {}
};
struct Signature : smh::Signature {
  Signature() = default;
  Signature(const smh::Signature& o) : smh::Signature(o) {}
};

namespace {

bool g_panic_hook = false;  // sourmash_init() installs the hook that records panics (utils.rs:100-104)

void set_last_error(const Error& e) {
  // utils.rs:154-166: an Err is always stored; a panic only reaches the slot through the hook
  if (e.code == smh::kPanic && !g_panic_hook) return;
  auto& slot = smh::last_error();
  slot.set = true;
  slot.code = e.code;
  slot.message = e.message;
}

// landing pad: run f, on failure fill the slot and hand back an all-zero value
template <class R, class F>
R pad(F&& f) {
  try {
    return f();
  } catch (const Error& e) {
    set_last_error(e);
  } catch (const std::bad_alloc&) {
    set_last_error(Error(smh::kPanic, "sourmash panicked: memory allocation failed"));
  } catch (const std::exception& e) {
    set_last_error(Error(smh::kPanic, std::string("sourmash panicked: ") + e.what()));
  }
  R zero;
  memset(&zero, 0, sizeof zero);
  return zero;
}
template <class F>
void pad_void(F&& f) {
  (void)pad<int>([&] { f(); return 0; });
}
// additive ABI: 0 on success, else the error code (slot also set)
template <class F>
int pad_code(F&& f) {
  try {
    f();
    return 0;
  } catch (const Error& e) {
    auto& slot = smh::last_error();
    slot.set = true; slot.code = e.code; slot.message = e.message;
    return (int)e.code;
  } catch (const std::exception& e) {
    auto& slot = smh::last_error();
    slot.set = true; slot.code = smh::kPanic; slot.message = std::string("sourmash panicked: ") + e.what();
    return (int)smh::kPanic;
  }
}

void require(const void* p, const char* what) {
  if (!p) smh::throw_panic(std::string("assertion failed: !") + what + ".is_null()");
}

SourmashStr str_from_string(const std::string& s) {  // utils.rs:201-210 from_string: owned copy
  SourmashStr r;
  r.len = s.size();
  r.data = (char*)malloc(s.size() ? s.size() : 1);
  if (s.size()) memcpy(r.data, s.data(), s.size());
  r.owned = true;
  return r;
}

bool utf8_cstr_ok(const char* s) {
  const unsigned char* p = (const unsigned char*)s;
  while (*p) {
    unsigned char c = *p;
    int need;
    if (c < 0x80) { p++; continue; }
    else if (c >= 0xC2 && c <= 0xDF) need = 1;
    else if (c >= 0xE0 && c <= 0xEF) need = 2;
    else if (c >= 0xF0 && c <= 0xF4) need = 3;
    else return false;
    unsigned char lo = 0x80, hi = 0xBF;
    if (c == 0xE0) lo = 0xA0; else if (c == 0xED) hi = 0x9F; else if (c == 0xF0) lo = 0x90; else if (c == 0xF4) hi = 0x8F;
    if (p[1] < lo || p[1] > hi) return false;
    for (int j = 2; j <= need; j++) if (p[j] < 0x80 || p[j] > 0xBF) return false;
    p += need + 1;
  }
  return true;
}

template <class T>
T** leak_array(std::vector<T*>& v, uintptr_t* size) {
  T** arr = (T**)malloc((v.size() ? v.size() : 1) * sizeof(T*));
  for (size_t i = 0; i < v.size(); i++) arr[i] = v[i];
  *size = v.size();
  return arr;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ hashing / sketching

uint64_t hash_murmur(const char* kmer, uint64_t seed) {
  return pad<uint64_t>([&] {
    require(kmer, "kmer");
    const uint64_t off[2] = {0, (uint64_t)strlen(kmer)};
    uint64_t h = 0;
    smh::Engine::get().hash_words((const uint8_t*)kmer, off, 1, seed, &h);
    return h;
  });
}

KmerMinHash* kmerminhash_new(uint32_t n, uint32_t k, bool prot, uint64_t seed, uint64_t mx, bool track_abundance) {
  return pad<KmerMinHash*>([&] { return new KmerMinHash(n, k, prot, seed, mx, track_abundance); });
}

void kmerminhash_free(KmerMinHash* ptr) { delete ptr; }

void kmerminhash_add_sequence(KmerMinHash* ptr, const char* sequence, bool force) {
  pad_void([&] {
    require(ptr, "ptr");
    require(sequence, "sequence");
    ptr->add_sequence((const uint8_t*)sequence, strlen(sequence), force);
  });
}

void kmerminhash_add_hash(KmerMinHash* ptr, uint64_t h) {
  pad_void([&] { require(ptr, "ptr"); ptr->add_hash(h); });
}

void kmerminhash_add_word(KmerMinHash* ptr, const char* word) {
  pad_void([&] {
    require(ptr, "ptr");
    require(word, "word");
    ptr->add_word((const uint8_t*)word, strlen(word));
  });
}

void kmerminhash_add_from(KmerMinHash* ptr, const KmerMinHash* other) {
  pad_void([&] { require(ptr, "ptr"); require(other, "other"); ptr->add_from(*other); });
}

void kmerminhash_merge(KmerMinHash* ptr, const KmerMinHash* other) {
  pad_void([&] { require(ptr, "ptr"); require(other, "other"); ptr->merge(*other); });
}

// ------------------------------------------------------------------ comparing

double kmerminhash_compare(KmerMinHash* ptr, const KmerMinHash* other) {
  return pad<double>([&] { require(ptr, "ptr"); require(other, "other"); return ptr->compare(*other); });
}

uint64_t kmerminhash_count_common(KmerMinHash* ptr, const KmerMinHash* other) {
  return pad<uint64_t>([&] { require(ptr, "ptr"); require(other, "other"); return ptr->count_common(*other); });
}

uint64_t kmerminhash_intersection(KmerMinHash* ptr, const KmerMinHash* other) {
  // src/ffi.rs:304-307: the SIZE of the combined sketch; any Err of intersection() reads as 0
  return pad<uint64_t>([&] {
    require(ptr, "ptr");
    require(other, "other");
    try {
      uint64_t common = 0, size = 0;
      ptr->intersection_size(*other, &common, &size);
      return size;
    } catch (const Error& e) {
      if (e.code == smh::kPanic || e.code == smh::kInternal) throw;
      return (uint64_t)0;
    }
  });
}

// ------------------------------------------------------------------ accessors

const uint64_t* kmerminhash_get_mins(KmerMinHash* ptr) {
  return pad<const uint64_t*>([&] {
    require(ptr, "ptr"); ptr->materialize();
    uint64_t* out = (uint64_t*)malloc((ptr->mins.size() ? ptr->mins.size() : 1) * sizeof(uint64_t));
    if (!ptr->mins.empty()) memcpy(out, ptr->mins.data(), ptr->mins.size() * sizeof(uint64_t));
    return (const uint64_t*)out;
  });
}

uintptr_t kmerminhash_get_mins_size(KmerMinHash* ptr) {
  return pad<uintptr_t>([&] { require(ptr, "ptr"); return (uintptr_t)ptr->size(); });
}

uint64_t kmerminhash_get_min_idx(KmerMinHash* ptr, uint64_t idx) {
  return pad<uint64_t>([&] {
    require(ptr, "ptr"); ptr->materialize();
    if (idx >= ptr->mins.size()) smh::throw_panic("index out of bounds");
    return ptr->mins[idx];
  });
}

void kmerminhash_mins_push(KmerMinHash* ptr, uint64_t val) {
  pad_void([&] { require(ptr, "ptr"); ptr->materialize(); ptr->mins.w().push_back(val); });
}

const uint64_t* kmerminhash_get_abunds(KmerMinHash* ptr) {
  return pad<const uint64_t*>([&] {
    require(ptr, "ptr"); ptr->materialize();
    if (!ptr->has_abunds) return (const uint64_t*)nullptr;
    uint64_t* out = (uint64_t*)malloc((ptr->abunds.size() ? ptr->abunds.size() : 1) * sizeof(uint64_t));
    if (!ptr->abunds.empty()) memcpy(out, ptr->abunds.data(), ptr->abunds.size() * sizeof(uint64_t));
    return (const uint64_t*)out;
  });
}

uintptr_t kmerminhash_get_abunds_size(KmerMinHash* ptr) {
  return pad<uintptr_t>([&] { require(ptr, "ptr"); ptr->materialize(); return (uintptr_t)(ptr->has_abunds ? ptr->abunds.size() : 0); });
}

uint64_t kmerminhash_get_abund_idx(KmerMinHash* ptr, uint64_t idx) {
  return pad<uint64_t>([&] {
    require(ptr, "ptr"); ptr->materialize();
    if (!ptr->has_abunds) return (uint64_t)0;
    if (idx >= ptr->abunds.size()) smh::throw_panic("index out of bounds");
    return ptr->abunds[idx];
  });
}

void kmerminhash_abunds_push(KmerMinHash* ptr, uint64_t val) {
  pad_void([&] { require(ptr, "ptr"); ptr->materialize(); if (ptr->has_abunds) ptr->abunds.push_back(val); });
}

bool kmerminhash_is_protein(KmerMinHash* ptr) { return pad<bool>([&] { require(ptr, "ptr"); return ptr->is_protein; }); }
uint64_t kmerminhash_seed(KmerMinHash* ptr) { return pad<uint64_t>([&] { require(ptr, "ptr"); return ptr->seed; }); }
bool kmerminhash_track_abundance(KmerMinHash* ptr) { return pad<bool>([&] { require(ptr, "ptr"); return ptr->has_abunds; }); }
uint32_t kmerminhash_num(KmerMinHash* ptr) { return pad<uint32_t>([&] { require(ptr, "ptr"); return ptr->num; }); }
uint32_t kmerminhash_ksize(KmerMinHash* ptr) { return pad<uint32_t>([&] { require(ptr, "ptr"); return ptr->ksize; }); }
uint64_t kmerminhash_max_hash(KmerMinHash* ptr) { return pad<uint64_t>([&] { require(ptr, "ptr"); return ptr->max_hash; }); }

// ------------------------------------------------------------------ Signature

Signature* signature_new(void) { return pad<Signature*>([&] { return new Signature(); }); }
void signature_free(Signature* ptr) { delete ptr; }

void signature_set_name(Signature* ptr, const char* name) {
  pad_void([&] {
    require(ptr, "ptr"); require(name, "name");
    if (utf8_cstr_ok(name)) { ptr->has_name = true; ptr->name = name; }  // ffi.rs:357-359: silently ignored otherwise
  });
}
void signature_set_filename(Signature* ptr, const char* name) {
  pad_void([&] {
    require(ptr, "ptr"); require(name, "name");
    if (utf8_cstr_ok(name)) { ptr->has_filename = true; ptr->filename = name; }
  });
}
void signature_push_mh(Signature* ptr, const KmerMinHash* other) {
  pad_void([&] { require(ptr, "ptr"); require(other, "other"); ptr->signatures.push_back(*other); });
}
void signature_set_mh(Signature* ptr, const KmerMinHash* other) {
  pad_void([&] { require(ptr, "ptr"); require(other, "other"); ptr->signatures.assign(1, *other); });
}
SourmashStr signature_get_name(Signature* ptr) {
  return pad<SourmashStr>([&] { require(ptr, "ptr"); return str_from_string(ptr->has_name ? ptr->name : ""); });
}
SourmashStr signature_get_filename(Signature* ptr) {
  return pad<SourmashStr>([&] { require(ptr, "ptr"); return str_from_string(ptr->has_filename ? ptr->filename : ""); });
}
SourmashStr signature_get_license(Signature* ptr) {
  return pad<SourmashStr>([&] { require(ptr, "ptr"); return str_from_string(ptr->license); });
}
KmerMinHash* signature_first_mh(Signature* ptr) {
  return pad<KmerMinHash*>([&] {
    require(ptr, "ptr");
    if (!ptr->signatures.empty()) return new KmerMinHash(ptr->signatures[0]);
    return new KmerMinHash();  // ffi.rs:468-471 "this is totally wrong": a Default sketch
  });
}
bool signature_eq(Signature* ptr, Signature* other) {
  return pad<bool>([&] { require(ptr, "ptr"); require(other, "other"); return smh::signature_equal(*ptr, *other); });
}
SourmashStr signature_save_json(Signature* ptr) {
  return pad<SourmashStr>([&] {
    require(ptr, "ptr");
    std::string out;
    smh::signature_to_json(out, *ptr);
    return str_from_string(out);
  });
}
KmerMinHash** signature_get_mhs(Signature* ptr, uintptr_t* size) {
  return pad<KmerMinHash**>([&] {
    require(ptr, "ptr");
    require(size, "size");
    std::vector<KmerMinHash*> v;
    for (auto& mh : ptr->signatures) v.push_back(new KmerMinHash(mh));
    return leak_array(v, size);
  });
}
SourmashStr signatures_save_buffer(Signature** ptr, uintptr_t size) {
  return pad<SourmashStr>([&] {
    require(ptr, "ptr");
    std::vector<const smh::Signature*> v;
    for (uintptr_t i = 0; i < size; i++) {
      if (!ptr[i]) smh::throw_panic("called `Option::unwrap()` on a `None` value");
      v.push_back(ptr[i]);
    }
    return str_from_string(smh::signatures_to_json(v));
  });
}

static Signature** load_common(const std::string& data, uintptr_t ksize, const char* select_moltype, uintptr_t* size) {
  require(size, "size");
  if (select_moltype && !utf8_cstr_ok(select_moltype)) throw Error(smh::kUtf8Error, "invalid utf-8 sequence");
  std::vector<smh::Signature> sigs = smh::load_signatures(data.data(), data.size(), ksize, select_moltype);
  std::vector<Signature*> v;
  for (auto& s : sigs) v.push_back(new Signature(s));
  return leak_array(v, size);
}

Signature** signatures_load_path(const char* ptr, bool ignore_md5sum, uintptr_t ksize, const char* select_moltype,
                                 uintptr_t* size) {
  (void)ignore_md5sum;  // ffi.rs:555 "TODO: implement ignore_md5sum"
  return pad<Signature**>([&] {
    require(ptr, "ptr");
    if (!utf8_cstr_ok(ptr)) throw Error(smh::kUtf8Error, "invalid utf-8 sequence");
    return load_common(smh::read_file(ptr), ksize, select_moltype, size);
  });
}

Signature** signatures_load_buffer(const char* ptr, uintptr_t insize, bool ignore_md5sum, uintptr_t ksize,
                                   const char* select_moltype, uintptr_t* size) {
  (void)ignore_md5sum;
  return pad<Signature**>([&] {
    require(ptr, "ptr");
    return load_common(std::string(ptr, insize), ksize, select_moltype, size);
  });
}

// ------------------------------------------------------------------ errors and strings

void sourmash_err_clear(void) {
  auto& s = smh::last_error();
  s.set = false; s.code = 0; s.message.clear();
}

SourmashStr sourmash_err_get_backtrace(void) {
  SourmashStr r = {nullptr, 0, false};  // no backtrace is captured: the reference returns Default then
  return r;
}

SourmashErrorCode sourmash_err_get_last_code(void) {
  auto& s = smh::last_error();
  return s.set ? s.code : SOURMASH_ERROR_CODE_NO_ERROR;
}

SourmashStr sourmash_err_get_last_message(void) {
  auto& s = smh::last_error();
  if (!s.set) { SourmashStr r = {nullptr, 0, false}; return r; }
  return str_from_string(s.message);
}

void sourmash_init(void) { g_panic_hook = true; }

void sourmash_str_free(SourmashStr* s) {
  if (s && s->owned) {
    free(s->data);
    s->data = nullptr; s->len = 0; s->owned = false;
  }
}

SourmashStr sourmash_str_from_cstr(const char* s) {
  // utils.rs:220-234: borrows the bytes but marks them owned; the caller clears `owned` if it
  // keeps the memory
  return pad<SourmashStr>([&] {
    if (!s || !utf8_cstr_ok(s)) throw Error(smh::kUtf8Error, "invalid utf-8 sequence");
    SourmashStr r;
    r.data = (char*)s; r.len = strlen(s); r.owned = true;
    return r;
  });
}

// ================================================================== additive MI355X ABI

int smh_device_available(void) { return smh::Device::available() ? 1 : 0; }

int smh_device_info(int* device, int* compute_units) {
  return pad_code([&] {
    auto& d = smh::Device::get();
    if (device) *device = d.id();
    if (compute_units) *compute_units = d.cu_count();
  });
}

int smh_add_sequence_len(KmerMinHash* ptr, const char* seq, uint64_t len, bool force) {
  return pad_code([&] { require(ptr, "ptr"); require(seq, "seq"); ptr->add_sequence((const uint8_t*)seq, len, force); });
}

int smh_add_sequences(KmerMinHash* ptr, const char* seq, const uint64_t* offsets, uint32_t n_records, bool force) {
  return pad_code([&] {
    require(ptr, "ptr"); require(seq, "seq"); require(offsets, "offsets");
    if (n_records == 0) return;
    const uint64_t base = offsets[0], total = offsets[n_records] - base;
    std::vector<uint64_t> rel(n_records + 1);
    for (uint32_t i = 0; i <= n_records; i++) rel[i] = offsets[i] - base;
    ptr->add_sequences_host((const uint8_t*)seq + base, total, rel.data(), n_records, force);
  });
}

int smh_add_sequences_dev(KmerMinHash* ptr, const void* seq_dev, uint64_t total_len, const uint64_t* offsets,
                          uint32_t n_records, bool force, void* stream) {
  return pad_code([&] {
    require(ptr, "ptr"); require(seq_dev, "seq_dev"); require(offsets, "offsets");
    ptr->add_sequences_device((const uint8_t*)seq_dev, total_len, offsets, n_records, force,
                              smh::Device::get().user_stream(stream), nullptr);
  });
}

int smh_add_sequences_grouped(KmerMinHash* const* sketches, uint32_t n_sketches, const char* seq, const uint64_t* offsets,
                              const uint32_t* groups, uint32_t n_records, bool force) {
  return pad_code([&] {
    if (n_records == 0) return;
    require(sketches, "sketches"); require(seq, "seq"); require(offsets, "offsets"); require(groups, "groups");
    for (uint32_t g = 0; g < n_sketches; g++) require(sketches[g], "sketches[g]");
    auto& dev = smh::Device::get();
    auto& E = smh::Engine::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    const uint64_t base = offsets[0], total = offsets[n_records] - base;
    std::vector<uint64_t> rel(n_records + 1);
    for (uint32_t i = 0; i <= n_records; i++) rel[i] = offsets[i] - base;
    E.seqbuf.ensure(total + 64);
    if (total) HIP_CHECK(hipMemcpyAsync(E.seqbuf.ptr, seq + base, total, hipMemcpyHostToDevice, dev.stream()));
    std::vector<smh::KmerMinHash*> mhs(sketches, sketches + n_sketches);
    smh::add_sequences_grouped(mhs.data(), n_sketches, E.seqbuf.as<uint8_t>(), total, rel.data(), groups, n_records, force,
                               dev.stream(), nullptr);
  });
}

int smh_add_sequences_grouped_dev(KmerMinHash* const* sketches, uint32_t n_sketches, const void* seq_dev, uint64_t total_len,
                                  const uint64_t* offsets, const uint32_t* groups, uint32_t n_records, bool force,
                                  void* stream) {
  return pad_code([&] {
    if (n_records == 0) return;
    require(sketches, "sketches"); require(seq_dev, "seq_dev"); require(offsets, "offsets"); require(groups, "groups");
    for (uint32_t g = 0; g < n_sketches; g++) require(sketches[g], "sketches[g]");
    std::vector<smh::KmerMinHash*> mhs(sketches, sketches + n_sketches);
    smh::add_sequences_grouped(mhs.data(), n_sketches, (const uint8_t*)seq_dev, total_len, offsets, groups, n_records, force,
                               smh::Device::get().user_stream(stream), nullptr);
  });
}

// ------------------------------------------------------------------ records parsed on the device

}  // extern "C"

// The records of one FASTA / FASTQ text: the compacted sequence bytes and the name spans in HBM, the offsets on the host
// (page-locked: the sketching paths walk them and upload them again).  Holds no reference to the text.
struct SmhRecords {
  void* seq = nullptr; size_t seq_cap = 0;          // total + 64 bytes, from the block pool
  void* names = nullptr; size_t names_cap = 0;      // name_start[n], name_end[n]
  uint64_t* offsets = nullptr;                      // n + 1, hipHostMalloc
  uint32_t n = 0;
  uint64_t total = 0;
  int format = 0;
  ~SmhRecords() {
    if (seq) smh::device_pool_free(seq, seq_cap, true);
    if (names) smh::device_pool_free(names, names_cap, true);
    if (offsets) (void)hipHostFree(offsets);
  }
};

namespace {

struct PoolBlock {      // a transient device block
  void* ptr = nullptr; size_t cap = 0;
  explicit PoolBlock(size_t need) { ptr = smh::device_pool_alloc(need, &cap); }
  ~PoolBlock() { if (ptr) smh::device_pool_free(ptr, cap, true); }
  PoolBlock(const PoolBlock&) = delete;
  PoolBlock& operator=(const PoolBlock&) = delete;
};

SmhRecords* parse_records(const uint8_t* text, uint64_t len, int format, hipStream_t s) {
  if (format != smh::kFormatAuto && format != smh::kFormatFasta && format != smh::kFormatFastq)
    throw Error(smh::kMsg, "unknown sequence file format " + std::to_string(format));
  auto rec = std::make_unique<SmhRecords>();
  PoolBlock small(256);
  auto* totals_dev = static_cast<smh::ParseTotals*>(small.ptr);
  if (format == smh::kFormatAuto) {
    uint64_t first = ~0ull;
    if (len) {
      auto* first_dev = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(small.ptr) + 128);
      smh::launch_first_content(text, len, first_dev, s);
      HIP_CHECK(hipMemcpyAsync(&first, first_dev, 8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
    if (first == ~0ull || first == '>') format = smh::kFormatFasta;      // a text without content holds no records
    else if (first == '@') format = smh::kFormatFastq;
    else throw Error(smh::kMsg, "neither FASTA nor FASTQ: the first non-empty line starts with byte " + std::to_string(first));
  }
  rec->format = format;
  smh::ParseTotals tot{0, 0, 0, 0, ~0ull};
  if (len) {
    PoolBlock ws(smh::parse_workspace_bytes(text, len));
    const smh::ParseTileIn first{0, 0, 0, 0, 0};
    auto& dev = smh::Device::get();
    dev.prof_begin(s);
    smh::launch_parse_scan(format, text, len, first, ws.ptr, totals_dev, s);
    dev.prof_end("parse_scan", s);
    HIP_CHECK(hipMemcpyAsync(&tot, totals_dev, sizeof tot, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (tot.n_records > 0xffffffffull) throw Error(smh::kMsg, "more than 2^32 - 1 records in one text");
    if (tot.total > len) smh::throw_internal("parse: more sequence bytes than text");
    const uint64_t n = tot.n_records;
    rec->seq = smh::device_pool_alloc(tot.total + 64, &rec->seq_cap);
    rec->names = smh::device_pool_alloc(n * 16 + 16, &rec->names_cap);
    PoolBlock offs(n * 8 + 8);
    auto* names = static_cast<uint64_t*>(rec->names);
    if (n) HIP_CHECK(hipMemsetAsync(rec->names, 0, n * 16, s));
    dev.prof_begin(s);
    smh::launch_parse_compact(format, text, len, ws.ptr, tot, static_cast<uint8_t*>(rec->seq), static_cast<uint64_t*>(offs.ptr),
                              names, names + n, totals_dev, s);
    dev.prof_end("parse_compact", s);
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&rec->offsets), (n + 1) * 8, hipHostMallocDefault));
    if (n) HIP_CHECK(hipMemcpyAsync(rec->offsets, offs.ptr, n * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&tot.err, &totals_dev->err, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    rec->offsets[n] = tot.total;
  } else {
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&rec->offsets), 8, hipHostMallocDefault));
    rec->offsets[0] = 0;
  }
  if (tot.err != ~0ull) {
    if (format == smh::kFormatFasta)
      throw Error(smh::kMsg, "FASTA: sequence data in front of the first header at byte " + std::to_string(tot.err));
    throw Error(smh::kMsg, "FASTQ: malformed record " + std::to_string(tot.err) +
                               " (no '@', no '+', quality and sequence lengths differ, or the record is cut short)");
  }
  rec->n = (uint32_t)tot.n_records;
  rec->total = tot.total;
  return rec.release();
}

}  // namespace

extern "C" {

SmhRecords* smh_records_parse_dev(const void* text_dev, uint64_t len, int format, void* stream) {
  return pad<SmhRecords*>([&] {
    auto& dev = smh::Device::get();
    if (len) require(text_dev, "text_dev");
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    return parse_records(static_cast<const uint8_t*>(text_dev), len, format, dev.user_stream(stream));
  });
}

SmhRecords* smh_records_parse(const char* text, uint64_t len, int format) {
  return pad<SmhRecords*>([&] {
    auto& dev = smh::Device::get();
    if (len) require(text, "text");
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    PoolBlock up(len + 64);
    if (len) HIP_CHECK(hipMemcpyAsync(up.ptr, text, len, hipMemcpyHostToDevice, s));
    return parse_records(static_cast<const uint8_t*>(up.ptr), len, format, s);
  });
}

void smh_records_free(SmhRecords* r) { delete r; }
uint32_t smh_records_len(const SmhRecords* r) { return r ? r->n : 0; }
uint64_t smh_records_total(const SmhRecords* r) { return r ? r->total : 0; }
int smh_records_format(const SmhRecords* r) { return r ? r->format : 0; }
const void* smh_records_seq_dev(const SmhRecords* r) { return r ? r->seq : nullptr; }
const uint64_t* smh_records_offsets(const SmhRecords* r) { return r ? r->offsets : nullptr; }
uint32_t smh_records_tile_bytes(void) { return smh::kParseTileBytes; }

int smh_records_names(const SmhRecords* r, uint64_t* start_out, uint32_t* len_out) {
  return pad_code([&] {
    require(r, "r");
    if (r->n == 0) return;
    require(start_out, "start_out"); require(len_out, "len_out");
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    std::vector<uint64_t> ends(r->n);
    const uint64_t* names = static_cast<const uint64_t*>(r->names);
    HIP_CHECK(hipMemcpyAsync(start_out, names, (size_t)r->n * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(ends.data(), names + r->n, (size_t)r->n * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < r->n; i++) {
      const uint64_t l = ends[i] >= start_out[i] ? ends[i] - start_out[i] : 0;
      if (l > 0xffffffffull) throw Error(smh::kMsg, "a record name longer than 2^32 - 1 bytes");
      len_out[i] = (uint32_t)l;
    }
  });
}

int smh_add_records(KmerMinHash* ptr, const SmhRecords* r, bool force) {
  return pad_code([&] {
    require(ptr, "ptr"); require(r, "r");
    ptr->add_sequences_device(static_cast<const uint8_t*>(r->seq), r->total, r->offsets, r->n, force,
                              smh::Device::get().user_stream(nullptr), nullptr);
  });
}

int smh_add_records_grouped(KmerMinHash* const* sketches, uint32_t n_sketches, const SmhRecords* r, const uint32_t* groups,
                            bool force) {
  return pad_code([&] {
    require(r, "r");
    if (r->n == 0) return;
    require(sketches, "sketches");
    for (uint32_t g = 0; g < n_sketches; g++) require(sketches[g], "sketches[g]");
    std::vector<uint32_t> own;
    if (!groups) {
      if (n_sketches != r->n) smh::throw_internal("one sketch per record needs as many sketches as records");
      own.resize(r->n);
      for (uint32_t i = 0; i < r->n; i++) own[i] = i;
      groups = own.data();
    }
    std::vector<smh::KmerMinHash*> mhs(sketches, sketches + n_sketches);
    smh::add_sequences_grouped(mhs.data(), n_sketches, static_cast<const uint8_t*>(r->seq), r->total, r->offsets, groups, r->n,
                               force, smh::Device::get().user_stream(nullptr), nullptr);
  });
}

int smh_add_many(KmerMinHash* ptr, const uint64_t* hashes, uint64_t n) {
  return pad_code([&] { require(ptr, "ptr"); if (n) require(hashes, "hashes"); ptr->materialize(); ptr->add_many(hashes, n); });
}

int smh_add_many_with_abund(KmerMinHash* ptr, const uint64_t* hashes, const uint64_t* abunds, uint64_t n) {
  return pad_code([&] {
    require(ptr, "ptr");
    if (n) { require(hashes, "hashes"); require(abunds, "abunds"); }
    ptr->add_many_with_abund(hashes, abunds, n);
  });
}

int smh_check_compatible(const KmerMinHash* ptr, const KmerMinHash* other) {
  return pad_code([&] { require(ptr, "ptr"); require(other, "other"); ptr->check_compatible(*other); });
}

int smh_intersection(const KmerMinHash* ptr, const KmerMinHash* other, uint64_t** common_out, uint64_t* n_common,
                     uint64_t* union_size) {
  return pad_code([&] {
    require(ptr, "ptr"); require(other, "other"); require(common_out, "common_out"); require(n_common, "n_common");
    std::vector<uint64_t> common;
    uint64_t size = 0;
    ptr->intersection(*other, &common, &size);
    uint64_t* out = (uint64_t*)malloc((common.empty() ? 1 : common.size()) * sizeof(uint64_t));
    if (!out) smh::throw_internal("out of memory");
    if (!common.empty()) memcpy(out, common.data(), common.size() * sizeof(uint64_t));
    *common_out = out; *n_common = common.size();
    if (union_size) *union_size = size;
  });
}

int smh_hash_words(const char* bytes, const uint64_t* offsets, uint32_t n, uint64_t seed, uint64_t* out) {
  return pad_code([&] {
    require(offsets, "offsets"); require(out, "out");
    smh::Engine::get().hash_words((const uint8_t*)bytes, offsets, n, seed, out);
  });
}

int smh_compare_block(KmerMinHash* const* rows, uint32_t n_rows, KmerMinHash* const* cols, uint32_t n_cols,
                      double* jaccard, uint64_t* common, uint64_t* size, uint64_t* count_common,
                      double* containment) {
  return pad_code([&] {
    if (n_rows == 0 || n_cols == 0) return;
    require(rows, "rows"); require(cols, "cols");
    std::vector<const smh::KmerMinHash*> R(n_rows), C(n_cols);
    std::vector<uint32_t> nums(n_rows);
    for (uint32_t i = 0; i < n_rows; i++) { require(rows[i], "rows[i]"); R[i] = rows[i]; nums[i] = rows[i]->num; }
    for (uint32_t j = 0; j < n_cols; j++) { require(cols[j], "cols[j]"); C[j] = cols[j]; }
    for (uint32_t i = 0; i < n_rows; i++)
      for (uint32_t j = 0; j < n_cols; j++) R[i]->check_compatible(*C[j]);
    smh::Engine::get().compare_host(R, C, nums.data(), 0, common, size, jaccard, count_common, containment);
  });
}

int smh_compare_block_dev(const uint64_t* row_hashes_dev, const uint64_t* row_offsets, uint32_t n_rows,
                          const uint64_t* col_hashes_dev, const uint64_t* col_offsets, uint32_t n_cols,
                          uint32_t num, double* jaccard_dev, uint64_t* common_dev, uint64_t* size_dev,
                          uint64_t* count_common_dev, double* containment_dev, void* stream) {
  return pad_code([&] {
    if (n_rows == 0 || n_cols == 0) return;
    require(row_offsets, "row_offsets"); require(col_offsets, "col_offsets");
    auto& dev = smh::Device::get();
    auto& E = smh::Engine::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.user_stream(stream);
    uint32_t mr = 0, mc = 0;
    for (uint32_t i = 0; i < n_rows; i++) mr = std::max<uint32_t>(mr, (uint32_t)(row_offsets[i + 1] - row_offsets[i]));
    for (uint32_t j = 0; j < n_cols; j++) mc = std::max<uint32_t>(mc, (uint32_t)(col_offsets[j + 1] - col_offsets[j]));
    E.cmp_oa.ensure((size_t)(n_rows + 1) * 8);
    E.cmp_ob.ensure((size_t)(n_cols + 1) * 8);
    HIP_CHECK(hipMemcpyAsync(E.cmp_oa.ptr, row_offsets, (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(E.cmp_ob.ptr, col_offsets, (size_t)(n_cols + 1) * 8, hipMemcpyHostToDevice, s));
    smh::SketchSet R, C;
    R.hashes = row_hashes_dev; R.offsets = E.cmp_oa.as<uint64_t>(); R.n = n_rows; R.h_offsets = row_offsets;
    C.hashes = col_hashes_dev; C.offsets = E.cmp_ob.as<uint64_t>(); C.n = n_cols; C.h_offsets = col_offsets;
    smh::CompareOut o;
    o.jaccard = jaccard_dev; o.common = common_dev; o.size = size_dev; o.count_common = count_common_dev;
    o.containment = containment_dev;
    const bool same_sets = row_hashes_dev == col_hashes_dev && n_rows == n_cols &&
                           std::memcmp(row_offsets, col_offsets, (size_t)(n_rows + 1) * 8) == 0;
    smh::launch_compare_block(R, C, num, nullptr, o, dev, s, mr, mc, row_offsets[n_rows] - row_offsets[0],
                              col_offsets[n_cols] - col_offsets[0], same_sets);
    HIP_CHECK(hipStreamSynchronize(s));  // the offset staging buffers are reused by the next call
  });
}

int smh_find(KmerMinHash* const* nodes, uint32_t n_nodes, const KmerMinHash* query, double threshold,
             bool containment, uint32_t* out_indices, uint32_t* out_count) {
  return pad_code([&] {
    require(out_count, "out_count");
    *out_count = 0;
    if (n_nodes == 0) return;
    require(nodes, "nodes"); require(query, "query"); require(out_indices, "out_indices");
    std::vector<const smh::KmerMinHash*> R(n_nodes), C(1, query);
    std::vector<uint32_t> nums(n_nodes);
    for (uint32_t i = 0; i < n_nodes; i++) {
      require(nodes[i], "nodes[i]");
      R[i] = nodes[i]; nums[i] = nodes[i]->num;
      R[i]->check_compatible(*query);   // Leaf::similarity unwraps compare(): an Err is fatal there too
    }
    std::vector<double> val(n_nodes);
    if (containment) smh::Engine::get().compare_host(R, C, nums.data(), 0, nullptr, nullptr, nullptr, nullptr, val.data());
    else smh::Engine::get().compare_host(R, C, nums.data(), 0, nullptr, nullptr, val.data(), nullptr, nullptr);
    uint32_t k = 0;
    for (uint32_t i = 0; i < n_nodes; i++)
      if (val[i] > threshold) out_indices[k++] = i;   // NaN (empty node, containment) is never > threshold
    *out_count = k;
  });
}

int smh_most_common(const KmerMinHash* leaf, KmerMinHash* const* candidates, uint32_t n, uint32_t* best_pos,
                    uint64_t* best_common) {
  return pad_code([&] {
    if (best_pos) *best_pos = 0;
    if (best_common) *best_common = 0;
    if (n == 0) return;
    require(leaf, "leaf"); require(candidates, "candidates");
    std::vector<const smh::KmerMinHash*> R(1, leaf), C(n);
    for (uint32_t j = 0; j < n; j++) { require(candidates[j], "candidates[j]"); C[j] = candidates[j]; leaf->check_compatible(*C[j]); }
    std::vector<uint64_t> cc(n);
    smh::Engine::get().compare_host(R, C, nullptr, leaf->num, nullptr, nullptr, nullptr, cc.data(), nullptr);
    uint32_t pos = 0;
    uint64_t mx = 0;
    for (uint32_t j = 0; j < n; j++)
      if (cc[j] > mx) { mx = cc[j]; pos = j; }
    if (best_pos) *best_pos = pos;
    if (best_common) *best_common = mx;
  });
}

// ------------------------------------------------------------------ resident index

struct SmhIndex {
  smh::DeviceBuffer hashes, offsets, nums;
  std::vector<uint64_t> h_offsets;
  std::vector<uint32_t> h_nums;
  std::vector<smh::KmerMinHash> params;   // parameters only (mins cleared): check_compatible per node
  uint32_t max_len = 0;
  uint32_t n = 0;
  // what gather asks of the whole set, decided once: every node has the parameters of node 0 (the query is then checked
  // against that one block), and whether any node is a bottom-`num` sketch
  bool uniform = true;
  bool any_num = false;
  // the dictionary of the resident set (dense ranks, components, frequent hashes), built by the first all-vs-all compare
  // of the index with itself and kept: later ones skip the pre-pass (the nodes of an index never change)
  smh::CollectionDict* dict = nullptr;
  uint32_t dict_split = 0;      // the frequent-hash setting the dictionary was built under
  // angular similarity.  has_abunds: EVERY node tracks abundances and every abundance vector matches its
  // hashes; h_abunds then holds them narrowed to u32 (a copy, like the hashes) until the first angular call uploads them
  // and computes the norms -- an index nobody asks pays no HBM.  bad_node: the lowest node whose norm2 does not fit 64 bits.
  bool has_abunds = false;
  std::vector<uint32_t> h_abunds;
  uint32_t wide_node = smh::kAngularNoError;   // the first node holding an abundance of 2^32 or more
  bool angular_ready = false;
  uint32_t bad_node = smh::kAngularNoError;
  smh::DeviceBuffer abunds_dev, norm2_dev;
  std::vector<uint64_t> h_norm2;
  SmhIndex() { std::lock_guard<std::mutex> g(registry_mu()); registry().insert(this); }
  ~SmhIndex() {
    { std::lock_guard<std::mutex> g(registry_mu()); registry().erase(this); }
    if (dict) smh::collection_free(dict);
  }
  void drop_dict() { if (dict) { smh::collection_free(dict); dict = nullptr; } }
  // the live indexes: smh_release_workspace() drops their cached dictionaries (memory no other allocator can see)
  static std::set<SmhIndex*>& registry() { static auto* r = new std::set<SmhIndex*>(); return *r; }
  static std::mutex& registry_mu() { static auto* m = new std::mutex(); return *m; }
};

SmhIndex* smh_index_new(KmerMinHash* const* nodes, uint32_t n_nodes) {
  return pad<SmhIndex*>([&] {
    if (n_nodes) require(nodes, "nodes");
    auto idx = std::make_unique<SmhIndex>();
    idx->n = n_nodes;
    idx->h_nums.resize(n_nodes);
    std::vector<const smh::KmerMinHash*> v(n_nodes);
    for (uint32_t i = 0; i < n_nodes; i++) {
      require(nodes[i], "nodes[i]");
      v[i] = nodes[i];
      idx->h_nums[i] = nodes[i]->num;
      smh::KmerMinHash p(nodes[i]->num, nodes[i]->ksize, nodes[i]->is_protein, nodes[i]->seed, nodes[i]->max_hash, false);
      idx->params.push_back(p);
      const smh::KmerMinHash& p0 = idx->params[0];
      idx->uniform &= p.ksize == p0.ksize && p.is_protein == p0.is_protein && p.max_hash == p0.max_hash && p.seed == p0.seed;
      idx->any_num |= p.num != 0;
    }
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    smh::SketchSet set;
    smh::Engine::get().pack_sketches(v, idx->hashes, idx->offsets, &set, &idx->max_len, &idx->h_offsets, s);
    // (pack_sketches has brought every node to the host)
    idx->has_abunds = true;
    for (uint32_t i = 0; i < n_nodes; i++) idx->has_abunds &= v[i]->has_abunds && v[i]->abunds.size() == v[i]->mins.size();
    if (idx->has_abunds) {
      idx->h_abunds.reserve(idx->h_offsets.back());
      for (uint32_t i = 0; i < n_nodes; i++)
        for (uint64_t a : v[i]->abunds) {
          if (a >> 32) { idx->wide_node = std::min(idx->wide_node, i); a = 0xffffffffull; }
          idx->h_abunds.push_back((uint32_t)a);
        }
    }
    idx->nums.ensure((size_t)n_nodes * 4 + 4);
    if (n_nodes) HIP_CHECK(hipMemcpyAsync(idx->nums.ptr, idx->h_nums.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return idx.release();
  });
}

void smh_index_free(SmhIndex* index) { delete index; }
void smh_index_drop_dictionary(SmhIndex* index) {
  if (!index) return;
  (void)pad_code([&] {
    std::lock_guard<std::recursive_mutex> lock(smh::Device::get().mutex());
    index->drop_dict();
  });
}
uint32_t smh_index_len(const SmhIndex* index) { return index ? index->n : 0; }

namespace {
// rows = resident index, cols = one host sketch: N x 1 block on the device, values back on the host
void index_vs_one(SmhIndex* index, const smh::KmerMinHash* q, bool q_is_row, double* jac, double* cont, uint64_t* cc) {
  auto& dev = smh::Device::get();
  auto& E = smh::Engine::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  q->materialize();
  const uint32_t n = index->n;
  const uint64_t qoff[2] = {0, (uint64_t)q->mins.size()};
  E.cmp_b.ensure(q->mins.size() * 8 + 8);
  E.cmp_ob.ensure(16);
  E.cmp_out.ensure((size_t)n * 8 * 3 + 64);
  if (!q->mins.empty())
    HIP_CHECK(hipMemcpyAsync(E.cmp_b.ptr, q->mins.data(), q->mins.size() * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(E.cmp_ob.ptr, qoff, 16, hipMemcpyHostToDevice, s));
  smh::SketchSet I, Q;
  I.hashes = index->hashes.as<uint64_t>(); I.offsets = index->offsets.as<uint64_t>(); I.n = n;
  Q.hashes = E.cmp_b.as<uint64_t>(); Q.offsets = E.cmp_ob.as<uint64_t>(); Q.n = 1;
  double* d_j = E.cmp_out.as<double>();
  double* d_c = d_j + n;
  uint64_t* d_cc = reinterpret_cast<uint64_t*>(d_c + n);
  smh::CompareOut o;
  o.jaccard = jac ? d_j : nullptr; o.containment = cont ? d_c : nullptr; o.count_common = cc ? d_cc : nullptr;
  if (!q_is_row)
    smh::launch_compare_block(I, Q, 0, index->nums.as<uint32_t>(), o, dev, s, index->max_len, (uint32_t)q->mins.size(),
                              index->h_offsets.back(), q->mins.size());
  else
    smh::launch_compare_block(Q, I, q->num, nullptr, o, dev, s, (uint32_t)q->mins.size(), index->max_len, q->mins.size(),
                              index->h_offsets.back());
  if (jac) HIP_CHECK(hipMemcpyAsync(jac, d_j, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  if (cont) HIP_CHECK(hipMemcpyAsync(cont, d_c, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  if (cc) HIP_CHECK(hipMemcpyAsync(cc, d_cc, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}
}  // namespace

int smh_index_find(SmhIndex* index, const KmerMinHash* query, double threshold, bool containment, uint32_t* out_indices,
                   uint32_t* out_count) {
  return pad_code([&] {
    require(index, "index"); require(query, "query"); require(out_count, "out_count");
    *out_count = 0;
    if (index->n == 0) return;
    require(out_indices, "out_indices");
    for (auto& p : index->params) p.check_compatible(*query);
    std::vector<double> val(index->n);
    index_vs_one(index, query, false, containment ? nullptr : val.data(), containment ? val.data() : nullptr, nullptr);
    uint32_t k = 0;
    for (uint32_t i = 0; i < index->n; i++)
      if (val[i] > threshold) out_indices[k++] = i;
    *out_count = k;
  });
}

int smh_index_most_common(SmhIndex* index, const KmerMinHash* leaf, uint32_t* best_pos, uint64_t* best_common) {
  return pad_code([&] {
    require(index, "index"); require(leaf, "leaf");
    if (best_pos) *best_pos = 0;
    if (best_common) *best_common = 0;
    if (index->n == 0) return;
    for (auto& p : index->params) leaf->check_compatible(p);
    std::vector<uint64_t> cc(index->n);
    index_vs_one(index, leaf, true, nullptr, nullptr, cc.data());
    uint32_t pos = 0; uint64_t mx = 0;
    for (uint32_t j = 0; j < index->n; j++) if (cc[j] > mx) { mx = cc[j]; pos = j; }
    if (best_pos) *best_pos = pos;
    if (best_common) *best_common = mx;
  });
}

static_assert(sizeof(SmhGatherRow) == 24 && sizeof(smh::GatherRow) == 24, "SmhGatherRow is 24 bytes");
static_assert(offsetof(SmhGatherRow, abund_sum) == 16 && offsetof(smh::GatherRow, abund_sum) == 16, "SmhGatherRow layout");

int smh_index_gather(SmhIndex* index, const KmerMinHash* query, uint32_t threshold_common, SmhGatherRow* rows,
                     uint32_t rows_capacity, uint32_t* n_rows, uint32_t* assigned) {
  return pad_code([&] {
    auto& dev = smh::Device::get();   // first: without a device the call says so, whatever it was handed
    require(index, "index"); require(query, "query"); require(n_rows, "n_rows");
    *n_rows = 0;
    if (rows_capacity) require(rows, "rows");
    if (query->num != 0) throw Error(smh::kMsg, "gather: the query is a num sketch; only scaled sketches (num == 0) can be gathered");
    if (index->any_num) throw Error(smh::kMsg, "gather: the index holds a num sketch; only scaled sketches (num == 0) can be gathered");
    if (index->n) {
      if (index->uniform) index->params[0].check_compatible(*query);
      else for (auto& p : index->params) p.check_compatible(*query);   // nodes that differ: one of them refuses the query
    }
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    query->flush_pending();
    // the query where it lives: a state in HBM is read there (uniq + counts or run starts), a host state is uploaded once
    smh::GatherQuery q;
    smh::DeviceBuffer up;
    uint64_t lq = 0;
    if (query->dev) {
      const smh::DeviceSketch& S = *query->dev;
      lq = S.n;
      q.hashes = S.uniq.as<uint64_t>();
      if (query->has_abunds) {
        if (S.has_counts) q.counts = S.counts.as<uint64_t>();
        else if (S.has_runs) { q.starts = S.starts.as<uint32_t>(); q.total = (uint32_t)S.total; }
        else smh::throw_internal("gather: the query's device state carries no abundances");
      }
    } else {
      lq = query->mins.size();
      if (query->has_abunds && query->abunds.size() != lq)
        smh::throw_internal("gather: the query's abundance vector does not match its hashes (quirks Q5/Q6)");
      if (lq) {
        up.ensure(lq * 8 * (query->has_abunds ? 2 : 1));
        HIP_CHECK(hipMemcpyAsync(up.ptr, query->mins.data(), lq * 8, hipMemcpyHostToDevice, s));
        q.hashes = up.as<uint64_t>();
        if (query->has_abunds) {
          HIP_CHECK(hipMemcpyAsync(up.as<uint64_t>() + lq, query->abunds.data(), lq * 8, hipMemcpyHostToDevice, s));
          q.counts = up.as<uint64_t>() + lq;
        }
      }
    }
    if (lq >= 0xffffffffull) smh::throw_internal("gather: a query of 2^32 - 1 or more hashes");
    q.n = (uint32_t)lq;
    if (index->n == 0 || lq == 0) {
      if (assigned && lq) std::fill(assigned, assigned + lq, 0xffffffffu);
      return;
    }
    smh::SketchSet I;
    I.hashes = index->hashes.as<uint64_t>(); I.offsets = index->offsets.as<uint64_t>(); I.n = index->n;
    I.h_offsets = index->h_offsets.data();
    *n_rows = smh::gather_run(I, index->max_len, q, threshold_common, reinterpret_cast<smh::GatherRow*>(rows), rows_capacity,
                              assigned, dev, s);
    up.release_after_sync();   // gather_run returns with the stream idle
  });
}
uint32_t smh_gather_rounds_per_sync(void) { return smh::kGatherRoundsPerSync; }

int smh_index_compare(SmhIndex* rows, SmhIndex* cols, double* jaccard, uint64_t* common, uint64_t* size,
                      uint64_t* count_common, double* containment) {
  return pad_code([&] {
    require(rows, "rows"); require(cols, "cols");
    const size_t np = (size_t)rows->n * cols->n;
    if (np == 0) return;
    for (auto& r : rows->params) for (auto& c : cols->params) r.check_compatible(c);
    auto& dev = smh::Device::get();
    auto& E = smh::Engine::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    E.cmp_out.ensure(np * 8 * 5 + 64);
    uint64_t* d_common = E.cmp_out.as<uint64_t>();
    uint64_t* d_size = d_common + np;
    double* d_jac = reinterpret_cast<double*>(d_size + np);
    uint64_t* d_cc = reinterpret_cast<uint64_t*>(d_jac + np);
    double* d_cont = reinterpret_cast<double*>(d_cc + np);
    smh::SketchSet R, C;
    R.hashes = rows->hashes.as<uint64_t>(); R.offsets = rows->offsets.as<uint64_t>(); R.n = rows->n;
    C.hashes = cols->hashes.as<uint64_t>(); C.offsets = cols->offsets.as<uint64_t>(); C.n = cols->n;
    R.h_offsets = rows->h_offsets.data(); C.h_offsets = cols->h_offsets.data();
    smh::CompareOut o;
    o.common = common ? d_common : nullptr; o.size = size ? d_size : nullptr; o.jaccard = jaccard ? d_jac : nullptr;
    o.count_common = count_common ? d_cc : nullptr; o.containment = containment ? d_cont : nullptr;
    // one num for every row: pass it as the launch-wide value (lets an index against itself use symmetry)
    bool uniform = true;
    for (uint32_t v : rows->h_nums) uniform &= v == rows->h_nums[0];
    const smh::CompareTuning tune = smh::compare_get_tuning();
    const bool block_route = tune.route == smh::kRouteAuto ? (np >= 4096 && rows->n >= 16) : (tune.route == smh::kRouteComponents || tune.route == smh::kRouteTiled);
    if (rows == cols && block_route && rows->h_offsets.back() > 0) {
      // an index against itself: its dictionary is built once and reused (the pre-pass is most of a sparse matrix's time)
      if (rows->dict && rows->dict_split != tune.split_frequent) { smh::collection_free(rows->dict); rows->dict = nullptr; }
      if (!rows->dict) {
        rows->dict = smh::collection_begin(R.hashes, R.offsets, rows->h_offsets.data(), rows->n, 1, 0, dev, s);
        smh::collection_finish(rows->dict, nullptr, dev, s);
        rows->dict_split = tune.split_frequent;
      }
      smh::collection_compare(rows->dict, 0, rows->n, 0, rows->n, uniform ? rows->h_nums[0] : 0,
                              uniform ? nullptr : rows->nums.as<uint32_t>(), 1, o, dev, s);
    } else
    smh::launch_compare_block(R, C, uniform ? rows->h_nums[0] : 0, uniform ? nullptr : rows->nums.as<uint32_t>(), o, dev, s,
                              rows->max_len, cols->max_len, rows->h_offsets.back(), cols->h_offsets.back(), rows == cols);
    if (common) HIP_CHECK(hipMemcpyAsync(common, d_common, np * 8, hipMemcpyDeviceToHost, s));
    if (size) HIP_CHECK(hipMemcpyAsync(size, d_size, np * 8, hipMemcpyDeviceToHost, s));
    if (jaccard) HIP_CHECK(hipMemcpyAsync(jaccard, d_jac, np * 8, hipMemcpyDeviceToHost, s));
    if (count_common) HIP_CHECK(hipMemcpyAsync(count_common, d_cc, np * 8, hipMemcpyDeviceToHost, s));
    if (containment) HIP_CHECK(hipMemcpyAsync(containment, d_cont, np * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

// ------------------------------------------------------------------ angular similarity on abundances

}  // extern "C" (the helpers below hold templates)

namespace {

// a block of the device pool for the length of one call
struct CallBlock {
  void* ptr = nullptr;
  size_t cap = 0;
  bool synced = false;   // the stream was waited for: nothing can still be using the block
  explicit CallBlock(size_t bytes) { ptr = smh::device_pool_alloc(bytes ? bytes : 1, &cap); }
  CallBlock(const CallBlock&) = delete;
  CallBlock& operator=(const CallBlock&) = delete;
  ~CallBlock() { smh::device_pool_free(ptr, cap, !synced); }
  template <class T> T* as() const { return reinterpret_cast<T*>(ptr); }
};

// From this many pairs on smh_index_angular first runs the block compare for count_common and walks only the pairs that
// share a hash.  Chosen from tools/bench_angular.py's sweep ("The prune threshold").
constexpr uint64_t kAngularPruneMinPairs = 4096;
uint64_t g_angular_prune_min_pairs = kAngularPruneMinPairs;
uint64_t g_angular_walked = 0, g_angular_skipped = 0;

void angular_require_tracking(const smh::KmerMinHash* mh, const char* what) {
  if (!mh->has_abunds) throw Error(smh::kMsg, std::string("angular: ") + what + " does not track abundances");
}
[[noreturn]] void angular_throw_norm(const std::string& who) {
  throw Error(smh::kMsg, "angular: norm2 of " + who + " does not fit 64 bits (an abundance of 2^32 or more, or too many large ones)");
}
// what can be said about a sketch without the device: a host state whose abundance vector does not match its hashes
void angular_check_host_state(const smh::KmerMinHash* mh, const char* what) {
  if (!mh->dev && mh->pend_seq.empty() && mh->pend_words.empty() && mh->abunds.size() != mh->mins.size())
    throw Error(smh::kMsg, std::string("angular: the abundance vector of ") + what + " does not match its hashes (quirks Q5/Q6)");
}

// One sketch in the form the kernels read: hashes and u32 abundances in device memory, offsets {0, n}, its norm2.  A state
// that lives in HBM is read there (its abundances are narrowed by a kernel); a host state is uploaded.
struct AngularOperand {
  const uint64_t* hashes = nullptr;
  const uint32_t* abunds = nullptr;
  uint32_t n = 0;
  std::unique_ptr<CallBlock> store, small;   // small: offsets (2 x u64), norm2 (u64), error word (u32)
  std::vector<uint32_t> staged;
  uint64_t off[2] = {0, 0};
  uint64_t* offsets_dev() const { return small->as<uint64_t>(); }
  uint64_t* norm2_dev() const { return small->as<uint64_t>() + 2; }
  uint32_t* err_dev() const { return reinterpret_cast<uint32_t*>(small->as<uint64_t>() + 3); }
  void done() { if (store) store->synced = true; if (small) small->synced = true; }
};

// queues the operand's upload / narrowing and its norm; the caller synchronises and then reads h_norm2 / h_err
void angular_prepare(AngularOperand& op, const smh::KmerMinHash* mh, const char* what, uint64_t* h_norm2, uint32_t* h_err, hipStream_t s) {
  mh->flush_pending();
  op.small = std::make_unique<CallBlock>(32);
  HIP_CHECK(hipMemsetAsync(op.err_dev(), 0xff, 4, s));
  uint64_t n = 0;
  if (mh->dev) {
    const smh::DeviceSketch& S = *mh->dev;
    n = S.n;
    if (n >= 0xffffffffull) smh::throw_internal("angular: a sketch of 2^32 - 1 or more hashes");
    if (n && !S.has_counts && !S.has_runs) smh::throw_internal("angular: the sketch's device state carries no abundances");
    op.store = std::make_unique<CallBlock>(n * 4);
    op.hashes = S.uniq.as<uint64_t>();
    op.abunds = op.store->as<uint32_t>();
    smh::launch_angular_narrow(S.has_counts ? S.counts.as<uint64_t>() : nullptr, S.has_counts ? nullptr : S.starts.as<uint32_t>(),
                               (uint32_t)S.total, (uint32_t)n, op.store->as<uint32_t>(), op.err_dev(), 0, s);
  } else {
    n = mh->mins.size();
    if (mh->abunds.size() != n)
      throw Error(smh::kMsg, std::string("angular: the abundance vector of ") + what + " does not match its hashes (quirks Q5/Q6)");
    if (n >= 0xffffffffull) smh::throw_internal("angular: a sketch of 2^32 - 1 or more hashes");
    op.staged.resize(n);
    for (uint64_t i = 0; i < n; i++) {
      if (mh->abunds[i] >> 32) angular_throw_norm(what);
      op.staged[i] = (uint32_t)mh->abunds[i];
    }
    op.store = std::make_unique<CallBlock>(n * 12);
    if (n) {
      HIP_CHECK(hipMemcpyAsync(op.store->ptr, mh->mins.data(), n * 8, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(op.store->as<uint64_t>() + n, op.staged.data(), n * 4, hipMemcpyHostToDevice, s));
    }
    op.hashes = op.store->as<uint64_t>();
    op.abunds = reinterpret_cast<const uint32_t*>(op.store->as<uint64_t>() + n);
  }
  op.n = (uint32_t)n;
  op.off[1] = n;
  HIP_CHECK(hipMemcpyAsync(op.offsets_dev(), op.off, 16, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(op.norm2_dev(), 0, 8, s));
  smh::launch_angular_norms(op.abunds, op.offsets_dev(), 1, op.norm2_dev(), op.err_dev(), s);
  HIP_CHECK(hipMemcpyAsync(h_norm2, op.norm2_dev(), 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(h_err, op.err_dev(), 4, hipMemcpyDeviceToHost, s));
}

smh::AngularSet angular_set(const AngularOperand& op) {
  smh::AngularSet a;
  a.hashes = op.hashes; a.abunds = op.abunds; a.offsets = op.offsets_dev(); a.norm2 = op.norm2_dev(); a.n = 1;
  return a;
}

// the first angular call on an index: abundances to HBM, norms computed and read back
void angular_ensure_index(SmhIndex* index, const char* what, hipStream_t s) {
  if (!index->angular_ready) {
    const uint32_t n = index->n;
    index->abunds_dev.ensure(index->h_abunds.size() * 4 + 4);
    index->norm2_dev.ensure((size_t)n * 8 + 8);
    index->h_norm2.assign(n, 0);
    uint32_t err = smh::kAngularNoError;
    if (n) {
      CallBlock e(4);
      HIP_CHECK(hipMemsetAsync(e.ptr, 0xff, 4, s));
      if (!index->h_abunds.empty())
        HIP_CHECK(hipMemcpyAsync(index->abunds_dev.ptr, index->h_abunds.data(), index->h_abunds.size() * 4, hipMemcpyHostToDevice, s));
      smh::launch_angular_norms(index->abunds_dev.as<uint32_t>(), index->offsets.as<uint64_t>(), n, index->norm2_dev.as<uint64_t>(),
                                e.as<uint32_t>(), s);
      HIP_CHECK(hipMemcpyAsync(index->h_norm2.data(), index->norm2_dev.ptr, (size_t)n * 8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(&err, e.ptr, 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      e.synced = true;
    }
    index->bad_node = std::min(index->wide_node, err);
    std::vector<uint32_t>().swap(index->h_abunds);   // they live in HBM now
    index->angular_ready = true;
  }
  if (index->bad_node != smh::kAngularNoError) angular_throw_norm(std::string(what) + " " + std::to_string(index->bad_node));
}

void angular_require_index(const SmhIndex* index, const char* what) {
  if (!index->has_abunds)
    throw Error(smh::kMsg, std::string("angular: ") + what + " holds a node that does not track abundances, or whose abundance "
                "vector does not match its hashes (quirks Q5/Q6)");
}

smh::AngularSet angular_set(const SmhIndex* index) {
  smh::AngularSet a;
  a.hashes = index->hashes.as<uint64_t>(); a.abunds = index->abunds_dev.as<uint32_t>(); a.offsets = index->offsets.as<uint64_t>();
  a.norm2 = index->norm2_dev.as<uint64_t>(); a.n = index->n;
  return a;
}

// count_common of rows x cols into d_cc (np entries): the route smh_index_compare takes, the cached dictionary included
void angular_count_common(SmhIndex* rows, SmhIndex* cols, uint64_t* d_cc, smh::Device& dev, hipStream_t s) {
  const size_t np = (size_t)rows->n * cols->n;
  smh::SketchSet R, C;
  R.hashes = rows->hashes.as<uint64_t>(); R.offsets = rows->offsets.as<uint64_t>(); R.n = rows->n;
  C.hashes = cols->hashes.as<uint64_t>(); C.offsets = cols->offsets.as<uint64_t>(); C.n = cols->n;
  R.h_offsets = rows->h_offsets.data(); C.h_offsets = cols->h_offsets.data();
  smh::CompareOut o;
  o.count_common = d_cc;
  bool uniform = true;
  for (uint32_t v : rows->h_nums) uniform &= v == rows->h_nums[0];
  const smh::CompareTuning tune = smh::compare_get_tuning();
  const bool block_route = tune.route == smh::kRouteAuto ? (np >= 4096 && rows->n >= 16) : (tune.route == smh::kRouteComponents || tune.route == smh::kRouteTiled);
  if (rows == cols && block_route && rows->h_offsets.back() > 0) {
    if (rows->dict && rows->dict_split != tune.split_frequent) { smh::collection_free(rows->dict); rows->dict = nullptr; }
    if (!rows->dict) {
      rows->dict = smh::collection_begin(R.hashes, R.offsets, rows->h_offsets.data(), rows->n, 1, 0, dev, s);
      smh::collection_finish(rows->dict, nullptr, dev, s);
      rows->dict_split = tune.split_frequent;
    }
    smh::collection_compare(rows->dict, 0, rows->n, 0, rows->n, uniform ? rows->h_nums[0] : 0,
                            uniform ? nullptr : rows->nums.as<uint32_t>(), 1, o, dev, s);
  } else {
    smh::launch_compare_block(R, C, uniform ? rows->h_nums[0] : 0, uniform ? nullptr : rows->nums.as<uint32_t>(), o, dev, s,
                              rows->max_len, cols->max_len, rows->h_offsets.back(), cols->h_offsets.back(), rows == cols);
  }
}

// runs the block kernel into pool memory and brings the wanted outputs and the two counters back; the stream is idle after
void angular_run_host(const smh::AngularSet& R, const smh::AngularSet& C, const uint64_t* prune_dev, bool symmetric, uint64_t* dot,
                      double* cosine, double* angular, smh::Device& dev, hipStream_t s) {
  const size_t np = (size_t)R.n * C.n;
  CallBlock d_dot(dot ? np * 8 : 0), d_cos(cosine ? np * 8 : 0), d_ang(angular ? np * 8 : 0), d_cnt(16);
  smh::AngularOut o;
  o.dot = dot ? d_dot.as<uint64_t>() : nullptr; o.cosine = cosine ? d_cos.as<double>() : nullptr;
  o.angular = angular ? d_ang.as<double>() : nullptr;
  smh::launch_angular_block(R, C, prune_dev, symmetric, o, d_cnt.as<unsigned long long>(), dev, s);
  uint64_t cnt[2] = {0, 0};
  if (dot) HIP_CHECK(hipMemcpyAsync(dot, d_dot.ptr, np * 8, hipMemcpyDeviceToHost, s));
  if (cosine) HIP_CHECK(hipMemcpyAsync(cosine, d_cos.ptr, np * 8, hipMemcpyDeviceToHost, s));
  if (angular) HIP_CHECK(hipMemcpyAsync(angular, d_ang.ptr, np * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(cnt, d_cnt.ptr, 16, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  d_dot.synced = d_cos.synced = d_ang.synced = d_cnt.synced = true;
  g_angular_walked = cnt[0]; g_angular_skipped = cnt[1];
}

}  // namespace

extern "C" {

bool smh_index_has_abundances(const SmhIndex* index) { return index && index->has_abunds; }

int smh_index_norms2(SmhIndex* index, uint64_t* out) {
  return pad_code([&] {
    require(index, "index");
    angular_require_index(index, "the index");
    if (index->n == 0) return;
    require(out, "out");
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    angular_ensure_index(index, "node", dev.stream());
    std::copy(index->h_norm2.begin(), index->h_norm2.end(), out);
  });
}

int smh_index_angular(SmhIndex* rows, SmhIndex* cols, uint64_t* dot, double* cosine, double* angular) {
  return pad_code([&] {
    require(rows, "rows"); require(cols, "cols");
    angular_require_index(rows, "the row index");
    angular_require_index(cols, "the column index");
    if (rows->n && cols->n) {
      if (rows->uniform && cols->uniform) rows->params[0].check_compatible(cols->params[0]);
      else for (auto& r : rows->params) for (auto& c : cols->params) r.check_compatible(c);
    }
    const size_t np = (size_t)rows->n * cols->n;
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    g_angular_walked = g_angular_skipped = 0;
    angular_ensure_index(rows, rows == cols ? "node" : "row node", s);
    if (rows != cols) angular_ensure_index(cols, "column node", s);
    if (np == 0) return;
    std::unique_ptr<CallBlock> cc;
    if (np >= g_angular_prune_min_pairs) {
      cc = std::make_unique<CallBlock>(np * 8);
      angular_count_common(rows, cols, cc->as<uint64_t>(), dev, s);
    }
    angular_run_host(angular_set(rows), angular_set(cols), cc ? cc->as<uint64_t>() : nullptr, rows == cols, dot, cosine, angular, dev, s);
    if (cc) cc->synced = true;
  });
}

int smh_index_angular_query(SmhIndex* index, const KmerMinHash* query, uint64_t* dot, uint64_t* query_norm2, double* cosine,
                            double* angular) {
  return pad_code([&] {
    require(index, "index"); require(query, "query");
    angular_require_index(index, "the index");
    angular_require_tracking(query, "the query");
    angular_check_host_state(query, "the query");
    if (index->n) {
      if (index->uniform) index->params[0].check_compatible(*query);
      else for (auto& p : index->params) p.check_compatible(*query);
    }
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    g_angular_walked = g_angular_skipped = 0;
    angular_ensure_index(index, "node", s);
    AngularOperand q;
    uint64_t n2 = 0;
    uint32_t err = smh::kAngularNoError;
    angular_prepare(q, query, "the query", &n2, &err, s);
    HIP_CHECK(hipStreamSynchronize(s));
    if (err != smh::kAngularNoError) { q.done(); angular_throw_norm("the query"); }
    if (query_norm2) std::fill(query_norm2, query_norm2 + index->n, n2);
    if (index->n) angular_run_host(angular_set(q), angular_set(index), nullptr, false, dot, cosine, angular, dev, s);
    q.done();
  });
}

int smh_angular_similarity(const KmerMinHash* a, const KmerMinHash* b, double* angular, double* cosine, uint64_t* dot,
                           uint64_t* norm2_a, uint64_t* norm2_b) {
  return pad_code([&] {
    require(a, "a"); require(b, "b");
    angular_require_tracking(a, "the first sketch");
    angular_require_tracking(b, "the second sketch");
    a->check_compatible(*b);
    angular_check_host_state(a, "the first sketch");
    angular_check_host_state(b, "the second sketch");
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    g_angular_walked = g_angular_skipped = 0;
    AngularOperand A, B;
    uint64_t n2[2] = {0, 0};
    uint32_t err[2] = {smh::kAngularNoError, smh::kAngularNoError};
    angular_prepare(A, a, "the first sketch", &n2[0], &err[0], s);
    angular_prepare(B, b, "the second sketch", &n2[1], &err[1], s);
    HIP_CHECK(hipStreamSynchronize(s));
    if (err[0] != smh::kAngularNoError || err[1] != smh::kAngularNoError) {
      A.done(); B.done();
      angular_throw_norm(err[0] != smh::kAngularNoError ? "the first sketch" : "the second sketch");
    }
    uint64_t d = 0;
    double c = 0.0, an = 0.0;
    angular_run_host(angular_set(A), angular_set(B), nullptr, false, &d, &c, &an, dev, s);
    A.done(); B.done();
    if (angular) *angular = an;
    if (cosine) *cosine = c;
    if (dot) *dot = d;
    if (norm2_a) *norm2_a = n2[0];
    if (norm2_b) *norm2_b = n2[1];
  });
}

int smh_angular_block_dev(const uint64_t* row_hashes_dev, const uint32_t* row_abunds_dev, const uint64_t* row_offsets, uint32_t n_rows,
                          const uint64_t* col_hashes_dev, const uint32_t* col_abunds_dev, const uint64_t* col_offsets, uint32_t n_cols,
                          const uint64_t* count_common_dev, bool symmetric, uint64_t* dot_dev, uint64_t* row_norm2_dev,
                          uint64_t* col_norm2_dev, double* cosine_dev, double* angular_dev, void* stream) {
  return pad_code([&] {
    require(row_offsets, "row_offsets"); require(col_offsets, "col_offsets");
    if (symmetric && (n_rows != n_cols || std::memcmp(row_offsets, col_offsets, ((size_t)n_rows + 1) * 8) != 0))
      throw Error(smh::kMsg, "angular: a symmetric block needs the same sketches as rows and as columns");
    for (uint32_t i = 0; i < n_rows; i++)
      if (row_offsets[i + 1] < row_offsets[i] || row_offsets[i + 1] - row_offsets[i] >= 0xffffffffull)
        throw Error(smh::kMsg, "angular: row_offsets must ascend, with sketches shorter than 2^32 - 1");
    for (uint32_t j = 0; j < n_cols; j++)
      if (col_offsets[j + 1] < col_offsets[j] || col_offsets[j + 1] - col_offsets[j] >= 0xffffffffull)
        throw Error(smh::kMsg, "angular: col_offsets must ascend, with sketches shorter than 2^32 - 1");
    if (row_offsets[n_rows] > row_offsets[0]) { require(row_hashes_dev, "row_hashes_dev"); require(row_abunds_dev, "row_abunds_dev"); }
    if (col_offsets[n_cols] > col_offsets[0]) { require(col_hashes_dev, "col_hashes_dev"); require(col_abunds_dev, "col_abunds_dev"); }
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.user_stream(stream);
    g_angular_walked = g_angular_skipped = 0;
    CallBlock offs(((size_t)n_rows + n_cols + 2) * 8), norms(((size_t)n_rows + n_cols) * 8), small(32);
    uint64_t* d_ro = offs.as<uint64_t>();
    uint64_t* d_co = d_ro + n_rows + 1;
    uint64_t* d_rn = row_norm2_dev ? row_norm2_dev : norms.as<uint64_t>();
    uint64_t* d_cn = col_norm2_dev ? col_norm2_dev : norms.as<uint64_t>() + n_rows;
    unsigned long long* d_cnt = small.as<unsigned long long>();
    uint32_t* d_err = reinterpret_cast<uint32_t*>(d_cnt + 2);
    HIP_CHECK(hipMemcpyAsync(d_ro, row_offsets, ((size_t)n_rows + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_co, col_offsets, ((size_t)n_cols + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(d_err, 0xff, 8, s));
    smh::launch_angular_norms(row_abunds_dev, d_ro, n_rows, d_rn, d_err, s);
    smh::launch_angular_norms(col_abunds_dev, d_co, n_cols, d_cn, d_err + 1, s);
    uint32_t err[2] = {smh::kAngularNoError, smh::kAngularNoError};
    HIP_CHECK(hipMemcpyAsync(err, d_err, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (err[0] != smh::kAngularNoError || err[1] != smh::kAngularNoError) {
      offs.synced = norms.synced = small.synced = true;
      if (err[0] != smh::kAngularNoError) angular_throw_norm("row sketch " + std::to_string(err[0]));
      angular_throw_norm("column sketch " + std::to_string(err[1]));
    }
    smh::AngularSet R, C;
    R.hashes = row_hashes_dev; R.abunds = row_abunds_dev; R.offsets = d_ro; R.norm2 = d_rn; R.n = n_rows;
    C.hashes = col_hashes_dev; C.abunds = col_abunds_dev; C.offsets = d_co; C.norm2 = d_cn; C.n = n_cols;
    smh::AngularOut o;
    o.dot = dot_dev; o.cosine = cosine_dev; o.angular = angular_dev;
    smh::launch_angular_block(R, C, count_common_dev, symmetric, o, d_cnt, dev, s);
    uint64_t cnt[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(cnt, d_cnt, 16, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));   // the offsets and the counters live in blocks that go back to the pool now
    offs.synced = norms.synced = small.synced = true;
    g_angular_walked = cnt[0]; g_angular_skipped = cnt[1];
  });
}

void smh_angular_last_stats(uint64_t* pairs_walked, uint64_t* pairs_skipped) {
  if (pairs_walked) *pairs_walked = g_angular_walked;
  if (pairs_skipped) *pairs_skipped = g_angular_skipped;
}
uint64_t smh_angular_prune_min_pairs(void) { return g_angular_prune_min_pairs; }
void smh_angular_set_prune_min_pairs(uint64_t pairs) { g_angular_prune_min_pairs = pairs ? pairs : kAngularPruneMinPairs; }

// ---- a scaled sketch's state as device arrays: the cross-rank union of partial sketches ----
int smh_sketch_export_dev(KmerMinHash* ptr, uint64_t* mins_dev, uint64_t* abunds_dev, uint64_t capacity, uint64_t* n_out, void* stream) {
  return pad_code([&] {
    require(ptr, "ptr"); require(n_out, "n_out");
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.user_stream(stream);
    if (!(ptr->num == 0 && ptr->max_hash > 0)) smh::throw_internal("smh_sketch_export_dev: only scaled sketches (num == 0, max_hash > 0)");
    ptr->flush_pending();
    if (!ptr->dev && ptr->has_abunds && ptr->abunds.size() != ptr->mins.size())
      smh::throw_internal("smh_sketch_export_dev: the sketch's abundance vector does not match its hashes (a state the reference's merge can "
                          "leave behind, quirks Q5/Q6); it has no device form");
    ptr->to_device_state();
    const uint64_t n = ptr->dev ? ptr->dev->n : 0;
    *n_out = n;
    if (n == 0 || !mins_dev) return;
    // a buffer sized from an earlier query, and hashes added since: say so (n_out holds the size needed) -- success with an
    // unfilled buffer would be taken for an empty part
    if (capacity < n) smh::throw_internal("smh_sketch_export_dev: capacity is smaller than the sketch (*n_out holds the size needed)");
    smh::DeviceSketch& S = *ptr->dev;
    HIP_CHECK(hipMemcpyAsync(mins_dev, S.uniq.ptr, n * 8, hipMemcpyDeviceToDevice, s));
    if (abunds_dev && ptr->has_abunds) {
      if (S.has_counts) HIP_CHECK(hipMemcpyAsync(abunds_dev, S.counts.ptr, n * 8, hipMemcpyDeviceToDevice, s));
      else smh::starts_to_counts(S.starts.as<uint32_t>(), (uint32_t)n, (uint32_t)S.total, abunds_dev, s);
    }
    HIP_CHECK(hipStreamSynchronize(s));
  });
}
int smh_sketch_absorb_dev(KmerMinHash* ptr, const uint64_t* mins_dev, const uint64_t* abunds_dev, const uint64_t* part_starts,
                          const uint64_t* part_lens, uint32_t n_parts, void* stream) {
  return pad_code([&] {
    require(ptr, "ptr");
    if (n_parts == 0) return;
    require(mins_dev, "mins_dev"); require(part_starts, "part_starts"); require(part_lens, "part_lens");
    if (!(ptr->num == 0 && ptr->max_hash > 0)) smh::throw_internal("smh_sketch_absorb_dev: only scaled sketches (num == 0, max_hash > 0)");
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.user_stream(stream);
    ptr->to_device_state();
    for (uint32_t k = 0; k < n_parts; k++)
      smh::Engine::get().union_arrays_into_device_sketch(*ptr, mins_dev + part_starts[k], abunds_dev ? abunds_dev + part_starts[k] : nullptr,
                                                         part_lens[k], s);
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

// ---- SmhCollection: the dictionary of one collection (all-vs-all, shareable among ranks) ----
struct SmhCollection {
  smh::CollectionDict* d = nullptr;
  ~SmhCollection() { if (d) smh::collection_free(d); }
};

SmhCollection* smh_collection_begin(const uint64_t* hashes_dev, const uint64_t* offsets, uint32_t n, uint32_t world, uint32_t rank,
                                    void* stream) {
  SmhCollection* out = nullptr;
  (void)pad_code([&] {
    require(hashes_dev, "hashes_dev"); require(offsets, "offsets");
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.user_stream(stream);
    std::unique_ptr<SmhCollection> c(new SmhCollection());
    c->d = smh::collection_begin(hashes_dev, nullptr, offsets, n, world, rank, dev, s);
    // the share is complete when the call returns (the caller all-gathers it next); a single owner has nobody to hand it
    // to: its work is left open on the stream, and every later entry point -- on any stream -- is ordered behind it
    // (Device::leave_open: the shared scratch buffers it still reads are not rewritten under it)
    if (world > 1) HIP_CHECK(hipStreamSynchronize(s));
    else dev.leave_open(s);
    out = c.release();
  });
  return out;
}
void smh_collection_free(SmhCollection* c) {
  if (!c) return;
  (void)pad_code([&] {
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    delete c;
  });
}
uint64_t smh_collection_share_bytes(const SmhCollection* c) { return c && c->d ? smh::collection_share_bytes(c->d) : 0; }
const void* smh_collection_share(const SmhCollection* c) { return c && c->d ? smh::collection_share(c->d) : nullptr; }
int smh_collection_share_to(const SmhCollection* c, void* dst_dev, void* stream) {
  return pad_code([&] {
    require(c, "collection"); require(dst_dev, "dst_dev");
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.user_stream(stream);
    HIP_CHECK(hipMemcpyAsync(dst_dev, smh::collection_share(c->d), smh::collection_share_bytes(c->d), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
  });
}
int smh_collection_finish(SmhCollection* c, const void* gathered_dev, void* stream) {
  return pad_code([&] {
    require(c, "collection");
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.user_stream(stream);
    smh::collection_finish(c->d, gathered_dev, dev, s);
    if (gathered_dev) HIP_CHECK(hipStreamSynchronize(s));   // the gathered buffer may be released by the caller now
    else dev.leave_open(s);                                  // (a single owner: ordered, not waited for -- see smh_collection_begin)
  });
}
int smh_collection_compare(SmhCollection* c, uint32_t row_lo, uint32_t row_hi, uint32_t num, uint32_t ownership,
                           double* jaccard_dev, uint64_t* common_dev, uint64_t* size_dev, uint64_t* count_common_dev,
                           double* containment_dev, void* stream) {
  return pad_code([&] {
    require(c, "collection");
    if (ownership > 2) smh::throw_internal("smh_collection_compare: ownership must be 0, 1 or 2");
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.user_stream(stream);
    smh::CompareOut o;
    o.jaccard = jaccard_dev; o.common = common_dev; o.size = size_dev; o.count_common = count_common_dev;
    o.containment = containment_dev;
    smh::collection_compare(c->d, row_lo, row_hi, 0, smh::collection_len(c->d), num, nullptr, ownership, o, dev, s);
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

int smh_mirror_pack(const void* out_dev, uint32_t n_local, uint32_t n_total, const uint32_t* col_lo, const uint32_t* col_hi,
                    uint32_t n_blocks, void* packed_dev, void* stream) {
  return pad_code([&] {
    if (n_blocks == 0) return;
    require(out_dev, "out_dev"); require(col_lo, "col_lo"); require(col_hi, "col_hi"); require(packed_dev, "packed_dev");
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.user_stream(stream);
    uint64_t at = 0;
    for (uint32_t b = 0; b < n_blocks; b++) {
      if (col_hi[b] < col_lo[b] || col_hi[b] > n_total) smh::throw_internal("smh_mirror_pack: block outside the matrix");
      smh::launch_mirror_pack(out_dev, n_local, n_total, col_lo[b], col_hi[b], (uint64_t*)packed_dev + at, s);
      at += (uint64_t)(col_hi[b] - col_lo[b]) * n_local;
    }
    HIP_CHECK(hipStreamSynchronize(s));
  });
}
int smh_mirror_apply(void* out_dev, uint32_t row_lo, uint32_t n_local, uint32_t n_total, const uint32_t* peer_lo, const uint32_t* peer_hi,
                     uint32_t n_blocks, const void* recv_dev, void* stream) {
  return pad_code([&] {
    if (n_blocks == 0) return;
    require(out_dev, "out_dev"); require(peer_lo, "peer_lo"); require(peer_hi, "peer_hi"); require(recv_dev, "recv_dev");
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.user_stream(stream);
    uint64_t at = 0;
    for (uint32_t b = 0; b < n_blocks; b++) {
      if (peer_hi[b] < peer_lo[b] || peer_hi[b] > n_total) smh::throw_internal("smh_mirror_apply: block outside the matrix");
      smh::launch_mirror_apply(out_dev, row_lo, n_local, n_total, peer_lo[b], peer_hi[b], (const uint64_t*)recv_dev + at, s);
      at += (uint64_t)(peer_hi[b] - peer_lo[b]) * n_local;
    }
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

int smh_synth_dna_dev(void* out_dev, uint64_t start, uint64_t len, uint64_t seed, uint64_t n_every, void* stream) {
  return pad_code([&] {
    require(out_dev, "out_dev");
    auto& dev = smh::Device::get();
    hipStream_t s = dev.user_stream(stream);
    smh::launch_synth_dna((uint8_t*)out_dev, start, len, seed, n_every, s);
    if (!stream) HIP_CHECK(hipStreamSynchronize(s));   // own stream: the buffer is complete on return
  });
}

int smh_sort_u64(uint64_t* keys, uint32_t* payload, uintptr_t n) {
  return pad_code([&] {
    if (n == 0) return;
    require(keys, "keys");
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    smh::DeviceBuffer k[2], v[2];
    for (int i = 0; i < 2; i++) { k[i].ensure(n * 8); if (payload) v[i].ensure(n * 4); }
    HIP_CHECK(hipMemcpyAsync(k[0].ptr, keys, n * 8, hipMemcpyHostToDevice, s));
    if (payload) HIP_CHECK(hipMemcpyAsync(v[0].ptr, payload, n * 4, hipMemcpyHostToDevice, s));
    int cur;
    if (payload) cur = smh::radix_sort_u64_v32(k[0].as<uint64_t>(), k[1].as<uint64_t>(), v[0].as<uint32_t>(), v[1].as<uint32_t>(), n,
                                               dev.scratch, s);
    else cur = smh::radix_sort_u64(k[0].as<uint64_t>(), k[1].as<uint64_t>(), nullptr, nullptr, n, dev.scratch, s);
    HIP_CHECK(hipMemcpyAsync(keys, k[cur].ptr, n * 8, hipMemcpyDeviceToHost, s));
    if (payload) HIP_CHECK(hipMemcpyAsync(payload, v[cur].ptr, n * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

void smh_compare_last_stats(SmhCompareStats* out) {
  if (!out) return;
  const smh::CompareStats st = smh::compare_last_stats();
  out->route = st.route; out->rows_per_tile = st.rows_per_tile;
  out->tiles_visited = st.tiles_visited; out->tiles_total = st.tiles_total; out->pairs_per_tile = st.pairs_per_tile;
  out->lds_overflow_steps = st.lds_overflow_steps;
  out->frequent_hashes = st.frequent_hashes;
  out->pipelined = st.pipelined;
  out->span_halvings = st.span_halvings;
  out->prefetched_after_halving = st.prefetched_after_halving;
}
uint32_t smh_compare_last_range_masks(void) { return smh::compare_last_stats().range_masks; }
void smh_compare_get_tuning(SmhCompareTuning* out) {
  if (!out) return;
  const smh::CompareTuning t = smh::compare_get_tuning();
  out->route = t.route; out->visit_all_tiles = t.visit_all_tiles; out->use_symmetry = t.use_symmetry;
  out->comp_pairs_limit = t.comp_pairs_limit; out->split_frequent = t.split_frequent; out->dictionary = t.dictionary;
  out->no_range_masks = t.no_range_masks;
}
int smh_compare_set_tuning(const SmhCompareTuning* in) {
  return pad_code([&] {
    smh::CompareTuning t;   // NULL = defaults
    if (in) {
      if (in->route > smh::kRouteTiled) smh::throw_internal("smh_compare_set_tuning: unknown route");
      t.route = in->route; t.visit_all_tiles = in->visit_all_tiles; t.use_symmetry = in->use_symmetry;
      t.comp_pairs_limit = in->comp_pairs_limit; t.split_frequent = in->split_frequent;
      if (in->dictionary > 1) smh::throw_internal("smh_compare_set_tuning: unknown dictionary build");
      t.dictionary = in->dictionary;
      t.no_range_masks = in->no_range_masks ? 1u : 0u;
    }
    smh::compare_set_tuning(t);
  });
}

// test hook (host only, no device): the compare block's tile planning
int smh_release_workspace(void) {
  return pad_code([&] {
    {
      // the dictionaries resident indexes cached for their all-vs-all compares (ranks, roots, the partition table: up to
      // hundreds of MB for 10 000 long sketches); the next smh_index_compare of an index with itself rebuilds its own
      std::lock_guard<std::recursive_mutex> lock(smh::Device::get().mutex());
      std::lock_guard<std::mutex> g(SmhIndex::registry_mu());
      for (SmhIndex* i : SmhIndex::registry()) i->drop_dict();
    }
    smh::Engine::get().release_workspace();
  });
}

void smh_pool_set_limit(uint64_t bytes) { (void)pad_code([&] { smh::device_pool_set_limit((size_t)bytes); }); }
uint64_t smh_pool_bytes(void) { return (uint64_t)smh::device_pool_bytes(); }

void smh_profile_enable(int on) {
  (void)pad_code([&] { smh::Device::get().profile_enable(on != 0); });
}
void smh_profile_reset(void) {
  (void)pad_code([&] { smh::Device::get().prof_reset(); });
}
int smh_profile_get(const char* name, double* total_ms, uint64_t* launches) {
  return pad_code([&] {
    require(name, "name");
    auto t = smh::Device::get().prof_get(name);
    if (total_ms) *total_ms = t.ms;
    if (launches) *launches = t.launches;
  });
}

// ------------------------------------------------------------------ Nodegraph / SBT

struct SmhNodegraph : smh::Nodegraph {
  using smh::Nodegraph::Nodegraph;
  SmhNodegraph(smh::Nodegraph&& o) : smh::Nodegraph(std::move(o)) {}
};
struct SmhSbt {
  std::unique_ptr<smh::Sbt> t;
  std::vector<uint64_t> offsets, positions;   // the last find_many's results (smh_sbt_find_many hands out a pointer)
};

SmhNodegraph* smh_nodegraph_new(const uint64_t* tablesizes, uint32_t n_tables, uint32_t ksize) {
  return pad<SmhNodegraph*>([&] {
    if (n_tables) require(tablesizes, "tablesizes");
    return new SmhNodegraph(std::vector<uint64_t>(tablesizes, tablesizes + n_tables), ksize);
  });
}
void smh_nodegraph_free(SmhNodegraph* ng) { delete ng; }
SmhNodegraph* smh_nodegraph_load_buffer(const char* data, uint64_t len) {
  return pad<SmhNodegraph*>([&] {
    if (len) require(data, "data");
    return new SmhNodegraph(smh::Nodegraph::load(data, (size_t)len));
  });
}
SmhNodegraph* smh_nodegraph_load_path(const char* path) {
  return pad<SmhNodegraph*>([&] {
    require(path, "path");
    const std::string raw = smh::read_file(path);
    return new SmhNodegraph(smh::Nodegraph::load(raw.data(), raw.size()));
  });
}
SourmashStr smh_nodegraph_save_buffer(const SmhNodegraph* ng) {
  return pad<SourmashStr>([&] { require(ng, "ng"); return str_from_string(ng->save()); });
}
bool smh_nodegraph_count(SmhNodegraph* ng, uint64_t hash) {
  return pad<bool>([&] { require(ng, "ng"); return ng->count(hash); });
}
int smh_nodegraph_count_many(SmhNodegraph* ng, const uint64_t* hashes, uint64_t n, uint8_t* out_new) {
  return pad_code([&] {
    require(ng, "ng");
    if (n) require(hashes, "hashes");
    ng->count_many(hashes, n, out_new);
  });
}
uint32_t smh_nodegraph_get(const SmhNodegraph* ng, uint64_t hash) {
  return pad<uint32_t>([&] { require(ng, "ng"); return ng->get(hash); });
}
int smh_nodegraph_get_many(const SmhNodegraph* ng, const uint64_t* hashes, uint64_t n, uint8_t* out) {
  return pad_code([&] {
    require(ng, "ng");
    if (n) { require(hashes, "hashes"); require(out, "out"); }
    ng->get_many(hashes, n, out);
  });
}
int smh_nodegraph_update(SmhNodegraph* ng, const SmhNodegraph* other) {
  return pad_code([&] { require(ng, "ng"); require(other, "other"); ng->update(*other); });
}
double smh_nodegraph_similarity(const SmhNodegraph* ng, const SmhNodegraph* other) {
  return pad<double>([&] { require(ng, "ng"); require(other, "other"); return ng->similarity(*other); });
}
double smh_nodegraph_containment(const SmhNodegraph* ng, const SmhNodegraph* other) {
  return pad<double>([&] { require(ng, "ng"); require(other, "other"); return ng->containment(*other); });
}
uint32_t smh_nodegraph_tablesizes(const SmhNodegraph* ng, uint64_t* out) {
  if (!ng) return 0;
  if (out) for (uint32_t t = 0; t < ng->L.n_tables(); t++) out[t] = ng->L.sizes[t];
  return ng->L.n_tables();
}
uint64_t smh_nodegraph_n_occupied_bins(const SmhNodegraph* ng) { return ng ? ng->occupied_bins : 0; }
uint64_t smh_nodegraph_unique_kmers(const SmhNodegraph* ng) { return ng ? ng->unique_kmers : 0; }
int smh_nodegraph_bins(const uint64_t* tablesizes, uint32_t n_tables, const uint64_t* hashes, uint64_t n, uint32_t* out) {
  return pad_code([&] {
    if (n == 0 || n_tables == 0) return;
    require(tablesizes, "tablesizes"); require(hashes, "hashes"); require(out, "out");
    smh::TableLayout L;
    L.init(std::vector<uint64_t>(tablesizes, tablesizes + n_tables));
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    smh::DeviceLayout DL;
    DL.upload(L, s);
    smh::DeviceBuffer dh, db;
    dh.ensure(n * 8); db.ensure(n * n_tables * 4);
    HIP_CHECK(hipMemcpyAsync(dh.ptr, hashes, n * 8, hipMemcpyHostToDevice, s));
    smh::launch_sbt_bins(dh.as<uint64_t>(), n, DL, db.as<uint32_t>(), s);
    HIP_CHECK(hipMemcpyAsync(out, db.ptr, n * n_tables * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

SmhSbt* smh_sbt_load_path(const char* json_path) {
  return pad<SmhSbt*>([&] {
    require(json_path, "json_path");
    std::unique_ptr<SmhSbt> o(new SmhSbt());
    o->t.reset(smh::Sbt::load(json_path));
    return o.release();
  });
}
SmhSbt* smh_sbt_build(uint32_t d, const uint64_t* positions, KmerMinHash* const* leaves, uint32_t n_leaves,
                      const uint64_t* tablesizes, uint32_t n_tables, uint32_t ksize) {
  return pad<SmhSbt*>([&] {
    if (n_leaves) { require(positions, "positions"); require(leaves, "leaves"); }
    if (n_tables) require(tablesizes, "tablesizes");
    std::vector<const smh::KmerMinHash*> v(n_leaves);
    for (uint32_t i = 0; i < n_leaves; i++) { require(leaves[i], "leaves[i]"); v[i] = leaves[i]; }
    std::unique_ptr<SmhSbt> o(new SmhSbt());
    o->t.reset(smh::Sbt::build(d, std::vector<uint64_t>(positions, positions + n_leaves), v,
                               std::vector<uint64_t>(tablesizes, tablesizes + n_tables), ksize));
    return o.release();
  });
}
int smh_sbt_save(const SmhSbt* sbt, const char* json_path) {
  return pad_code([&] { require(sbt, "sbt"); require(json_path, "json_path"); sbt->t->save(json_path); });
}
void smh_sbt_free(SmhSbt* sbt) {
  if (!sbt) return;
  (void)pad_code([&] {
    std::lock_guard<std::recursive_mutex> lock(smh::Device::get().mutex());
    delete sbt;
  });
}
uint32_t smh_sbt_n_nodes(const SmhSbt* sbt) { return sbt ? sbt->t->n_nodes() : 0; }
uint32_t smh_sbt_n_leaves(const SmhSbt* sbt) { return sbt ? sbt->t->n_leaves() : 0; }
int smh_sbt_leaf_positions(const SmhSbt* sbt, uint64_t* out) {
  return pad_code([&] {
    require(sbt, "sbt");
    const auto& p = sbt->t->leaf_positions();
    if (!p.empty()) { require(out, "out"); std::copy(p.begin(), p.end(), out); }
  });
}
KmerMinHash* smh_sbt_leaf_sketch(const SmhSbt* sbt, uint32_t i) {
  return pad<KmerMinHash*>([&] {
    require(sbt, "sbt");
    if (i >= sbt->t->n_leaves()) smh::throw_panic("index out of bounds: leaf");
    return new KmerMinHash(sbt->t->leaf_sketch(i));
  });
}
int smh_sbt_find_many(SmhSbt* sbt, KmerMinHash* const* queries, uint32_t n, double threshold, bool containment,
                      uint64_t* out_offsets, const uint64_t** out_positions) {
  return pad_code([&] {
    require(sbt, "sbt"); require(out_offsets, "out_offsets"); require(out_positions, "out_positions");
    *out_positions = nullptr;
    std::fill(out_offsets, out_offsets + n + 1, 0);
    if (n) require(queries, "queries");
    std::vector<const smh::KmerMinHash*> q(n);
    for (uint32_t i = 0; i < n; i++) { require(queries[i], "queries[i]"); q[i] = queries[i]; }
    sbt->t->find_many(q, threshold, containment, sbt->offsets, sbt->positions);
    std::copy(sbt->offsets.begin(), sbt->offsets.end(), out_offsets);
    *out_positions = sbt->positions.data();
  });
}
int smh_sbt_find(SmhSbt* sbt, const KmerMinHash* query, double threshold, bool containment, uint64_t* out_positions,
                 uint32_t* out_count) {
  return pad_code([&] {
    require(sbt, "sbt"); require(query, "query"); require(out_count, "out_count");
    *out_count = 0;
    std::vector<const smh::KmerMinHash*> q(1, query);
    sbt->t->find_many(q, threshold, containment, sbt->offsets, sbt->positions);
    if (!sbt->positions.empty()) { require(out_positions, "out_positions"); std::copy(sbt->positions.begin(), sbt->positions.end(), out_positions); }
    *out_count = (uint32_t)sbt->positions.size();
  });
}

}  // extern "C"
