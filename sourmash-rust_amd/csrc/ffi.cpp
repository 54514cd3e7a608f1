// ffi.cpp -- the C ABI: every symbol of include/sourmash.h (the reference's surface, restating
// src/ffi.rs and src/utils.rs) and the additive MI355X entry points of include/sourmash_amd.h.
#include <cstddef>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/sourmash_amd.h"
#include "archive_core.hpp"
#include "index.hpp"
#include "sbt.hpp"
#include "signature.hpp"
#include "sigscan.hpp"
#include "sigtext.hpp"

using smh::Error;
using smh::require;

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

// the queries of a batch call as the checked array the index takes
std::vector<const smh::KmerMinHash*> require_queries(const KmerMinHash* const* queries, uint32_t n) {
  if (n) require(queries, "queries");
  std::vector<const smh::KmerMinHash*> v(n);
  for (uint32_t q = 0; q < n; q++) { require(queries[q], "queries[q]"); v[q] = queries[q]; }
  return v;
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

KmerMinHash* smh_kmerminhash_new_molecule(uint32_t n, uint32_t k, int molecule, uint64_t seed, uint64_t mx, bool track_abundance) {
  return pad<KmerMinHash*>([&] {
    if (molecule < SMH_MOLECULE_DNA || molecule > SMH_MOLECULE_HP) throw Error(smh::kMsg, "unknown molecule");
    return new KmerMinHash(n, k, (smh::Molecule)molecule, seed, mx, track_abundance);
  });
}
int smh_kmerminhash_molecule(const KmerMinHash* ptr) { return pad<int>([&] { require(ptr, "ptr"); return (int)ptr->molecule; }); }

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

// ------------------------------------------------------------------ amino-acid input

int smh_add_protein(KmerMinHash* ptr, const char* seq, uint64_t len) {
  return pad_code([&] {
    require(ptr, "ptr");
    ptr->check_amino_input();
    if (len) require(seq, "seq");
    const uint64_t off[2] = {0, len};
    ptr->add_proteins_host((const uint8_t*)seq, len, off, 1);
  });
}

int smh_add_proteins(KmerMinHash* ptr, const char* seq, const uint64_t* offsets, uint32_t n_records) {
  return pad_code([&] {
    require(ptr, "ptr");
    ptr->check_amino_input();
    require(offsets, "offsets");
    if (n_records == 0) { (void)smh::Device::get(); return; }
    const uint64_t base = offsets[0], total = offsets[n_records] - base;
    if (total) require(seq, "seq");
    std::vector<uint64_t> rel(n_records + 1);
    for (uint32_t i = 0; i <= n_records; i++) rel[i] = offsets[i] - base;
    ptr->add_proteins_host((const uint8_t*)seq + base, total, rel.data(), n_records);
  });
}

int smh_add_proteins_dev(KmerMinHash* ptr, const void* seq_dev, uint64_t total_len, const uint64_t* offsets, uint32_t n_records,
                         void* stream) {
  return pad_code([&] {
    require(ptr, "ptr");
    ptr->check_amino_input();
    require(offsets, "offsets");
    if (total_len) require(seq_dev, "seq_dev");
    ptr->add_proteins_device((const uint8_t*)seq_dev, total_len, offsets, n_records, smh::Device::get().user_stream(stream));
  });
}

void smh_amino_geometry(uint64_t total_len, uint32_t win, uint32_t* tile_positions, uint32_t* run) {
  smh::amino_geometry(total_len, win, tile_positions, run);
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

// ------------------------------------------------------------------ records parsed on the device (records.cpp)

struct SmhRecords : smh::Records {};

static SmhRecords* records_parse(const void* text, const char* what, bool on_host, uint64_t len, int format, void* stream) {
  return pad<SmhRecords*>([&] {
    auto& dev = smh::Device::get();
    if (len) require(text, what);
    auto rec = std::make_unique<SmhRecords>();
    smh::parse_records(rec.get(), text, on_host, len, format, stream, dev);
    return rec.release();
  });
}
SmhRecords* smh_records_parse_dev(const void* text_dev, uint64_t len, int format, void* stream) {
  return records_parse(text_dev, "text_dev", false, len, format, stream);
}
SmhRecords* smh_records_parse(const char* text, uint64_t len, int format) { return records_parse(text, "text", true, len, format, nullptr); }
void smh_records_free(SmhRecords* r) { delete r; }
uint32_t smh_records_len(const SmhRecords* r) { return r ? r->n : 0; }
uint64_t smh_records_total(const SmhRecords* r) { return r ? r->total : 0; }
int smh_records_format(const SmhRecords* r) { return r ? r->format : 0; }
const void* smh_records_seq_dev(const SmhRecords* r) { return r ? r->seq_dev() : nullptr; }
const uint64_t* smh_records_offsets(const SmhRecords* r) { return r ? r->offsets : nullptr; }
uint32_t smh_records_tile_bytes(void) { return smh::kParseTileBytes; }

int smh_records_names(const SmhRecords* r, uint64_t* start_out, uint32_t* len_out) {
  return pad_code([&] {
    require(r, "r");
    if (r->n == 0) return;
    require(start_out, "start_out"); require(len_out, "len_out");
    r->name_spans(start_out, len_out);
  });
}

// ------------------------------------------------------------------ blocked gzip (inflate.cpp)

struct SmhGzip : smh::Gzip {};

SmhGzip* smh_gzip_scan(const void* data, uint64_t len) {
  return pad<SmhGzip*>([&] {
    if (len) require(data, "data");
    auto g = std::make_unique<SmhGzip>();
    smh::gzip_scan(g.get(), static_cast<const uint8_t*>(data), len);
    return g.release();
  });
}
void smh_gzip_free(SmhGzip* g) { delete g; }
uint64_t smh_gzip_members(const SmhGzip* g) { return g ? g->members.size() : 0; }
uint64_t smh_gzip_inflated_len(const SmhGzip* g) { return g ? g->inflated : 0; }
int smh_gzip_member(const SmhGzip* g, uint64_t i, uint64_t* payload_off, uint32_t* payload_len, uint32_t* isize, uint32_t* crc) {
  return pad_code([&] {
    require(g, "g");
    if (i >= g->members.size()) throw Error(smh::kMsg, "gzip: member " + std::to_string(i) + " of " + std::to_string(g->members.size()));
    const smh::InflateMember& m = g->members[i];
    if (payload_off) *payload_off = m.payload_off;
    if (payload_len) *payload_len = m.payload_len;
    if (isize) *isize = m.isize;
    if (crc) *crc = m.crc;
  });
}
int smh_gzip_inflate_dev(const SmhGzip* g, const void* data_dev, uint64_t len, void* out_dev, uint64_t out_cap, int verify_crc,
                         uint8_t* status_out, void* stream) {
  return pad_code([&] {
    auto& dev = smh::Device::get();
    require(g, "g");
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    smh::gzip_inflate_dev(*g, static_cast<const uint8_t*>(data_dev), len, static_cast<uint8_t*>(out_dev), out_cap, verify_crc != 0, status_out,
                          dev.user_stream(stream), dev);
  });
}
int smh_gzip_inflate(const void* data, uint64_t len, void* out_dev, uint64_t out_cap, int verify_crc, uint8_t* status_out) {
  return pad_code([&] {
    auto& dev = smh::Device::get();
    if (len) require(data, "data");
    smh::gzip_inflate_host(static_cast<const uint8_t*>(data), len, static_cast<uint8_t*>(out_dev), out_cap, verify_crc != 0, status_out, dev);
  });
}

// ------------------------------------------------------------------ zip collections (archive.cpp)

struct SmhArchive : smh::archive::Archive {};
static_assert(SMH_ARCHIVE_STORED == smh::archive::kStored && SMH_ARCHIVE_DEFLATE == smh::archive::kDeflate &&
              SMH_ARCHIVE_GZIP == smh::archive::kGzip && SMH_ARCHIVE_DIRECTORY == smh::archive::kDirectory &&
              SMH_ARCHIVE_OTHER == smh::archive::kOther, "the kinds of the header are archive_core.hpp's");

SmhArchive* smh_archive_scan(const void* data, uint64_t len) {
  return pad<SmhArchive*>([&] {
    if (len) require(data, "data");
    auto a = std::make_unique<SmhArchive>();
    smh::archive_scan(a.get(), static_cast<const uint8_t*>(data), len);
    return a.release();
  });
}
void smh_archive_free(SmhArchive* a) { delete a; }
uint64_t smh_archive_entries(const SmhArchive* a) { return a ? a->entries.size() : 0; }
int smh_archive_entry(const SmhArchive* a, uint64_t i, SmhArchiveEntry* out) {
  return pad_code([&] {
    require(a, "a"); require(out, "out");
    if (i >= a->entries.size()) throw Error(smh::kMsg, "archive: entry " + std::to_string(i) + " of " + std::to_string(a->entries.size()));
    const smh::archive::Entry& e = a->entries[i];
    memset(out, 0, sizeof *out);
    out->name = e.name.c_str(); out->reason = e.reason.c_str();
    out->method = e.method; out->flags = e.flags; out->crc32 = e.crc32; out->kind = e.kind;
    out->device_ok = e.device_ok ? 1 : 0; out->text_size = e.text_size; out->text_crc = e.text_crc;
    out->comp_size = e.comp_size; out->size = e.size; out->header_off = e.header_off; out->data_off = e.data_off;
    out->payload_off = e.payload_off; out->payload_len = e.payload_len;
  });
}
int smh_archive_inflate_dev(const SmhArchive* a, const void* data_dev, uint64_t len, const uint32_t* ids, const uint64_t* out_offs, uint64_t n_ids,
                            void* out_dev, uint64_t out_cap, int verify, uint8_t* status_out, void* stream) {
  return pad_code([&] {
    auto& dev = smh::Device::get();
    require(a, "a");
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    smh::archive_inflate_dev(*a, static_cast<const uint8_t*>(data_dev), len, ids, out_offs, n_ids, static_cast<uint8_t*>(out_dev), out_cap,
                             verify != 0, status_out, dev.user_stream(stream), dev);
  });
}
int smh_archive_inflate(const SmhArchive* a, const void* data, uint64_t len, const uint32_t* ids, const uint64_t* out_offs, uint64_t n_ids,
                        void* out_dev, uint64_t out_cap, int verify, uint8_t* status_out) {
  return pad_code([&] {
    auto& dev = smh::Device::get();
    require(a, "a");
    if (len) require(data, "data");
    smh::archive_inflate_host(*a, static_cast<const uint8_t*>(data), len, ids, out_offs, n_ids, static_cast<uint8_t*>(out_dev), out_cap,
                              verify != 0, status_out, dev);
  });
}
void smh_archive_geometry(uint32_t* chunk_bytes, uint32_t* threads) {
  if (chunk_bytes) *chunk_bytes = smh::archive::kChunk;
  if (threads) *threads = smh::kInflateThreads;
}
void smh_archive_set_sorted(int sorted) { smh::g_archive_sorted = sorted != 0; }
int smh_archive_sorted(void) { return smh::g_archive_sorted ? 1 : 0; }

int smh_add_records(KmerMinHash* ptr, const SmhRecords* r, bool force) {
  return pad_code([&] {
    require(ptr, "ptr"); require(r, "r");
    ptr->add_sequences_device(r->seq_dev(), r->total, r->offsets, r->n, force,
                              smh::Device::get().user_stream(nullptr), nullptr);
  });
}

int smh_add_records_protein(KmerMinHash* ptr, const SmhRecords* r) {
  return pad_code([&] {
    require(ptr, "ptr");
    ptr->check_amino_input();
    require(r, "r");
    ptr->add_proteins_device(r->seq_dev(), r->total, r->offsets, r->n, smh::Device::get().user_stream(nullptr));
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
    smh::add_sequences_grouped(mhs.data(), n_sketches, r->seq_dev(), r->total, r->offsets, groups, r->n,
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
    smh::Engine::get().compare_block_dev(row_hashes_dev, row_offsets, n_rows, col_hashes_dev, col_offsets, n_cols, num,
                                         {common_dev, size_dev, jaccard_dev, count_common_dev, containment_dev}, stream);
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
    *out_count = smh::indices_above(val.data(), n_nodes, threshold, out_indices);
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
    smh::arg_max(cc.data(), n, best_pos, best_common);
  });
}

// ------------------------------------------------------------------ resident index (index.cpp, angular.cpp)

struct SmhIndex : smh::ResidentIndex { using smh::ResidentIndex::ResidentIndex; };

SmhIndex* smh_index_new(KmerMinHash* const* nodes, uint32_t n_nodes) {
  return pad<SmhIndex*>([&] {
    if (n_nodes) require(nodes, "nodes");
    std::vector<const smh::KmerMinHash*> v(n_nodes);
    for (uint32_t i = 0; i < n_nodes; i++) { require(nodes[i], "nodes[i]"); v[i] = nodes[i]; }
    return new SmhIndex(v);
  });
}
void smh_index_free(SmhIndex* index) { delete index; }
void smh_index_drop_dictionary(SmhIndex* index) {
  if (index) (void)pad_code([&] { std::lock_guard<std::recursive_mutex> lock(smh::Device::get().mutex()); index->drop_dict(); });
}
uint32_t smh_index_len(const SmhIndex* index) { return index ? index->n : 0; }

int smh_index_find(SmhIndex* index, const KmerMinHash* query, double threshold, bool containment, uint32_t* out_indices,
                   uint32_t* out_count) {
  return pad_code([&] {
    require(index, "index"); require(query, "query"); require(out_count, "out_count");
    *out_count = 0;
    if (index->n == 0) return;
    require(out_indices, "out_indices");
    *out_count = index->find(*query, threshold, containment, out_indices);
  });
}
int smh_index_most_common(SmhIndex* index, const KmerMinHash* leaf, uint32_t* best_pos, uint64_t* best_common) {
  return pad_code([&] {
    require(index, "index"); require(leaf, "leaf");
    if (best_pos) *best_pos = 0;
    if (best_common) *best_common = 0;
    if (index->n == 0) return;
    index->most_common(*leaf, best_pos, best_common);
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
    *n_rows = index->gather(*query, threshold_common, reinterpret_cast<smh::GatherRow*>(rows), rows_capacity, assigned, dev);
  });
}
uint32_t smh_gather_rounds_per_sync(void) { return smh::kGatherRoundsPerSync; }

namespace {
// a CSR carries no parameters: the index must speak for itself with one voice
void require_uniform_scaled(const SmhIndex* index, const char* op) {
  if (!(index->uniform && index->all_scaled))
    throw Error(smh::kMsg, std::string(op) + ": the device form needs an index whose nodes are scaled sketches with the same ksize, molecule, "
                                             "seed and max_hash");
}
// the rows handed out the way match hands out hit_hashes: malloc'ed, one element at least
void gather_many_rows_out(const std::vector<smh::GatherRow>& got, SmhGatherRow** rows) {
  SmhGatherRow* out = (SmhGatherRow*)malloc((got.empty() ? 1 : got.size()) * sizeof(SmhGatherRow));
  if (!out) smh::throw_internal("out of memory");
  if (!got.empty()) memcpy(out, got.data(), got.size() * sizeof(SmhGatherRow));
  *rows = out;
}
}  // namespace

int smh_index_gather_many(SmhIndex* index, const KmerMinHash* const* queries, uint32_t n_queries, uint32_t threshold_common,
                          uint32_t rows_capacity, uint64_t* row_offsets, SmhGatherRow** rows, uint64_t* query_offsets, uint32_t* assigned) {
  return pad_code([&] {
    auto& dev = smh::Device::get();   // first: without a device the call says so, whatever it was handed
    require(index, "index"); require(row_offsets, "row_offsets"); require(rows, "rows");
    const std::vector<const smh::KmerMinHash*> v = require_queries(queries, n_queries);
    std::vector<smh::GatherRow> got;
    index->gather_many(v.data(), n_queries, threshold_common, rows_capacity, row_offsets, &got, query_offsets, assigned, dev);
    gather_many_rows_out(got, rows);
  });
}

int smh_index_gather_block_dev(SmhIndex* index, const uint64_t* q_hashes_dev, const uint64_t* q_abunds_dev, const uint64_t* q_offsets,
                               uint32_t n_queries, uint32_t threshold_common, uint32_t rows_capacity, uint64_t* row_offsets,
                               SmhGatherRow** rows, uint32_t* assigned, void* stream) {
  return pad_code([&] {
    auto& dev = smh::Device::get();
    require(index, "index"); require(row_offsets, "row_offsets"); require(rows, "rows"); require(q_offsets, "q_offsets");
    require_uniform_scaled(index, "gather_many");
    if (n_queries && q_offsets[n_queries] != q_offsets[0]) require(q_hashes_dev, "q_hashes_dev");
    std::vector<smh::GatherRow> got;
    index->gather_many_dev(q_hashes_dev, q_abunds_dev, q_offsets, n_queries, threshold_common, rows_capacity, row_offsets, &got, assigned,
                           dev, dev.user_stream(stream));
    gather_many_rows_out(got, rows);
  });
}

void smh_gather_many_set_budget(uint64_t pairs) { smh::g_gather_many_budget = pairs ? pairs : smh::kGatherManyBudget; }
uint64_t smh_gather_many_budget(void) { return smh::g_gather_many_budget; }

static_assert(sizeof(SmhSearchRow) == 16 && sizeof(smh::SearchRow) == 16, "SmhSearchRow is 16 bytes");
static_assert(offsetof(SmhSearchRow, query_size) == 12 && offsetof(smh::SearchRow, query_size) == 12, "SmhSearchRow layout");
static_assert(SMH_SEARCH_JACCARD == smh::kSearchJaccard && SMH_SEARCH_CONTAINMENT_NODE == smh::kSearchContainmentNode &&
                  SMH_SEARCH_CONTAINMENT_QUERY == smh::kSearchContainmentQuery && SMH_SEARCH_MAX_CONTAINMENT == smh::kSearchMaxContainment,
              "the metrics of the header are the kernels'");

namespace {
// what every search call refuses before it looks at anything else -- and before the device: these need none
void search_require(uint32_t metric, double threshold, uint64_t* row_offsets, SmhSearchRow** rows) {
  require(row_offsets, "row_offsets"); require(rows, "rows");
  smh::check_search(metric, threshold);
}
}  // namespace

int smh_index_search_many(SmhIndex* index, const KmerMinHash* const* queries, uint32_t n_queries, uint32_t metric, double threshold,
                          uint32_t threshold_common, uint64_t* row_offsets, SmhSearchRow** rows) {
  return pad_code([&] {
    search_require(metric, threshold, row_offsets, rows);
    auto& dev = smh::Device::get();
    require(index, "index");
    const std::vector<const smh::KmerMinHash*> v = require_queries(queries, n_queries);
    *rows = reinterpret_cast<SmhSearchRow*>(index->search_many(v.data(), n_queries, metric, threshold, threshold_common, row_offsets, dev));
  });
}

int smh_index_search_block_dev(SmhIndex* index, const uint64_t* q_hashes_dev, const uint64_t* q_offsets, uint32_t n_queries, uint32_t metric,
                               double threshold, uint32_t threshold_common, uint64_t* row_offsets, SmhSearchRow** rows, void* stream) {
  return pad_code([&] {
    search_require(metric, threshold, row_offsets, rows);
    auto& dev = smh::Device::get();
    require(index, "index"); require(q_offsets, "q_offsets");
    require_uniform_scaled(index, "search_many");
    if (n_queries && q_offsets[n_queries] != q_offsets[0]) require(q_hashes_dev, "q_hashes_dev");
    *rows = reinterpret_cast<SmhSearchRow*>(index->search_many_dev(q_hashes_dev, q_offsets, n_queries, metric, threshold, threshold_common,
                                                                   smh::kSearchNotSelf, row_offsets, dev, dev.user_stream(stream)));
  });
}

int smh_index_search_self(SmhIndex* index, uint32_t metric, double threshold, uint32_t threshold_common, bool upper_only,
                          uint64_t* row_offsets, SmhSearchRow** rows) {
  return pad_code([&] {
    search_require(metric, threshold, row_offsets, rows);
    auto& dev = smh::Device::get();
    require(index, "index");
    *rows = reinterpret_cast<SmhSearchRow*>(index->search_self(metric, threshold, threshold_common, upper_only, row_offsets, dev));
  });
}

void smh_search_many_set_budget(uint64_t pairs) { smh::g_search_many_budget = pairs ? pairs : smh::kSearchManyBudget; }
uint64_t smh_search_many_budget(void) { return smh::g_search_many_budget; }
void smh_search_geometry(uint32_t* short_owners, uint32_t* node_tile, uint32_t* max_queries) {
  smh::search_geometry(short_owners, node_tile, max_queries);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Nearest neighbours: the best k of those pairs per query (additive ABI)

int smh_index_nearest_many(SmhIndex* index, const KmerMinHash* const* queries, uint32_t n_queries, uint32_t k, uint32_t metric,
                           double threshold, uint32_t threshold_common, uint64_t* row_offsets, SmhSearchRow** rows) {
  return pad_code([&] {
    search_require(metric, threshold, row_offsets, rows);
    smh::check_nearest_k(k);
    auto& dev = smh::Device::get();
    require(index, "index");
    const std::vector<const smh::KmerMinHash*> v = require_queries(queries, n_queries);
    *rows = reinterpret_cast<SmhSearchRow*>(index->nearest_many(v.data(), n_queries, k, metric, threshold, threshold_common, row_offsets, dev));
  });
}

int smh_index_nearest_block_dev(SmhIndex* index, const uint64_t* q_hashes_dev, const uint64_t* q_offsets, uint32_t n_queries, uint32_t k,
                                uint32_t metric, double threshold, uint32_t threshold_common, uint64_t* row_offsets, SmhSearchRow** rows,
                                void* stream) {
  return pad_code([&] {
    search_require(metric, threshold, row_offsets, rows);
    smh::check_nearest_k(k);
    auto& dev = smh::Device::get();
    require(index, "index"); require(q_offsets, "q_offsets");
    require_uniform_scaled(index, "nearest_many");
    if (n_queries && q_offsets[n_queries] != q_offsets[0]) require(q_hashes_dev, "q_hashes_dev");
    *rows = reinterpret_cast<SmhSearchRow*>(index->nearest_dev(q_hashes_dev, q_offsets, n_queries, k, metric, threshold, threshold_common,
                                                               smh::kSearchNotSelf, row_offsets, dev, dev.user_stream(stream)));
  });
}

int smh_index_nearest_self(SmhIndex* index, uint32_t k, uint32_t metric, double threshold, uint32_t threshold_common, uint64_t* row_offsets,
                           SmhSearchRow** rows) {
  return pad_code([&] {
    search_require(metric, threshold, row_offsets, rows);
    smh::check_nearest_k(k);
    auto& dev = smh::Device::get();
    require(index, "index");
    *rows = reinterpret_cast<SmhSearchRow*>(index->nearest_self(k, metric, threshold, threshold_common, row_offsets, dev));
  });
}

void smh_nearest_geometry(uint32_t* max_k, uint32_t* node_tile, uint32_t* merge_slots) { smh::nearest_geometry(max_k, node_tile, merge_slots); }

static_assert(SMH_CLUSTER_COMPONENTS == smh::kClusterComponents && SMH_CLUSTER_GREEDY == smh::kClusterGreedy, "the linkages of the header are the kernels'");

int smh_index_cluster(SmhIndex* index, uint32_t metric, double threshold, uint32_t threshold_common, uint32_t linkage, const uint32_t* scores,
                      uint32_t* cluster, uint32_t* representative, uint32_t* rep_common, uint32_t* n_clusters) {
  return pad_code([&] {
    // refused before the index or the device is looked at: these need neither
    require(cluster, "cluster"); require(representative, "representative"); require(n_clusters, "n_clusters");
    smh::check_cluster(metric, threshold, linkage, rep_common != nullptr);
    auto& dev = smh::Device::get();
    require(index, "index");
    index->cluster(metric, threshold, threshold_common, linkage, scores, cluster, representative, rep_common, n_clusters, dev);
  });
}

void smh_cluster_set_pair_budget(uint64_t entries) { smh::g_cluster_pair_budget = entries ? entries : smh::kClusterPairBudget; }
uint64_t smh_cluster_pair_budget(void) { return smh::g_cluster_pair_budget; }
void smh_cluster_set_rounds(uint32_t rounds) { smh::g_cluster_rounds = rounds ? rounds : smh::kClusterRoundsPerSync; }
uint32_t smh_cluster_rounds(void) { return smh::g_cluster_rounds; }
void smh_cluster_geometry(uint32_t* lane_max, uint32_t* node_tile) { smh::cluster_geometry(lane_max, node_tile); }
int smh_index_sizes(const SmhIndex* index, uint32_t* sizes) {
  return pad_code([&] {
    require(index, "index");
    if (index->n) require(sizes, "sizes");
    for (uint32_t v = 0; v < index->n; v++) sizes[v] = (uint32_t)(index->h_offsets[v + 1] - index->h_offsets[v]);
  });
}

// ------------------------------------------------------------------ collapsing by groups, the read-back (collapse.cpp)

SmhIndex* smh_index_collapse(SmhIndex* index, const uint32_t* group, uint32_t n_groups, uint32_t min_count, double min_fraction,
                             uint32_t abund) {
  return pad<SmhIndex*>([&] {
    // refused before the index or the device is looked at: these need neither
    smh::check_collapse(n_groups, min_fraction, abund);
    (void)smh::Device::get();
    if (!index) throw Error(smh::kMsg, "collapse: index is NULL");   // (MSG like every refusal of this call; group: in the constructor)
    return new SmhIndex(*index, group, n_groups, min_count, min_fraction, abund);
  });
}
void smh_collapse_geometry(uint32_t* lane_max, uint32_t* wave_max, uint32_t* group_tile) {
  smh::collapse_geometry(lane_max, wave_max, group_tile);
}
int smh_index_read(SmhIndex* index, uint64_t* offsets, uint64_t* hashes, uint32_t* abunds) {
  return pad_code([&] {
    (void)smh::Device::get();
    require(index, "index");
    index->read(offsets, hashes, abunds);
  });
}

// ------------------------------------------------------------------ building an index from records, concat (index_build.cpp)

static_assert(SMH_INPUT_NUCLEOTIDE == smh::kBuildNucleotide && SMH_INPUT_AMINO == smh::kBuildAmino, "the inputs of the header are index_build's");

SmhIndex* smh_index_from_sequences(const KmerMinHash* like, int input, const char* seq, const uint64_t* offsets, const uint32_t* groups,
                                   uint32_t n_records, uint32_t n_groups) {
  return pad<SmhIndex*>([&] {
    // every refusal of the arguments first: they need no device
    // (host memory has no total_len: the offsets themselves say how far the batch reaches)
    const uint64_t reach = offsets ? offsets[n_records] : 0;
    smh::check_index_build(like, input, seq != nullptr || (offsets && reach == offsets[0]), reach, offsets, groups, n_records, n_groups);
    const uint64_t base = offsets[0], total = reach - base;
    std::vector<uint64_t> rel((size_t)n_records + 1, 0);
    for (uint32_t i = 0; i <= n_records; i++) rel[i] = offsets[i] - base;
    auto& dev = smh::Device::get();
    auto& E = smh::Engine::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    E.seqbuf.ensure(total + 64);
    if (total) HIP_CHECK(hipMemcpyAsync(E.seqbuf.ptr, seq + base, total, hipMemcpyHostToDevice, dev.stream()));
    return new SmhIndex(*like, input, E.seqbuf.as<uint8_t>(), total, rel.data(), groups, n_records, n_groups, dev.stream());
  });
}
SmhIndex* smh_index_from_sequences_dev(const KmerMinHash* like, int input, const void* seq_dev, uint64_t total_len, const uint64_t* offsets,
                                       const uint32_t* groups, uint32_t n_records, uint32_t n_groups, void* stream) {
  return pad<SmhIndex*>([&] {
    smh::check_index_build(like, input, seq_dev != nullptr, total_len, offsets, groups, n_records, n_groups);
    auto& dev = smh::Device::get();
    return new SmhIndex(*like, input, (const uint8_t*)seq_dev, total_len, offsets, groups, n_records, n_groups, dev.user_stream(stream));
  });
}
SmhIndex* smh_index_from_records(const KmerMinHash* like, int input, const SmhRecords* r, const uint32_t* groups, uint32_t n_groups) {
  return pad<SmhIndex*>([&] {
    if (!r) throw Error(smh::kMsg, "index build: records is NULL");
    static const uint64_t none = 0;   // (a handle without records may hold no offsets)
    const uint64_t* offsets = r->offsets || r->n ? r->offsets : &none;
    smh::check_index_build(like, input, r->seq_dev() != nullptr, r->total, offsets, groups, r->n, n_groups);
    auto& dev = smh::Device::get();
    return new SmhIndex(*like, input, r->seq_dev(), r->total, offsets, groups, r->n, n_groups, dev.user_stream(nullptr));
  });
}
SmhIndex* smh_index_concat(SmhIndex* const* parts, uint32_t n_parts) {
  return pad<SmhIndex*>([&] {
    std::vector<smh::ResidentIndex*> v;
    if (n_parts && !parts) throw Error(smh::kMsg, "index concat: parts is NULL");
    for (uint32_t p = 0; p < n_parts; p++) v.push_back(parts[p]);
    smh::check_index_concat(v.data(), n_parts);
    (void)smh::Device::get();
    return new SmhIndex(v.data(), n_parts);
  });
}
void smh_index_build_set_budget(uint64_t candidates) { smh::g_index_build_budget = candidates ? candidates : smh::kIndexBuildBudget; }
uint64_t smh_index_build_budget(void) { return smh::g_index_build_budget; }
void smh_index_build_geometry(uint32_t* tile_elems, uint32_t* threads) { smh::index_build_geometry(tile_elems, threads); }

// ------------------------------------------------------------------ filtering an index, taking a subset of its nodes (filter.cpp)

static_assert(SMH_FILTER_OPERAND_NONE == smh::kFilterOperandNone && SMH_FILTER_KEEP_IN == smh::kFilterKeepIn &&
              SMH_FILTER_DROP_IN == smh::kFilterDropIn && SMH_FILTER_ABUND_OWN == smh::kFilterAbundOwn &&
              SMH_FILTER_ABUND_FLAT == smh::kFilterAbundFlat && SMH_FILTER_ABUND_OPERAND == smh::kFilterAbundOperand,
              "the modes of the header are filter's");
static_assert(sizeof(SmhFilter) == 24 && sizeof(smh::FilterRule) == sizeof(SmhFilter), "SmhFilter is FilterRule: six u32");

SmhIndex* smh_index_filter(SmhIndex* index, const KmerMinHash* operand, const SmhFilter* rule) {
  return pad<SmhIndex*>([&] {
    // the rule's own refusals before the index or the device is looked at: they need neither
    smh::check_filter_rule(reinterpret_cast<const smh::FilterRule*>(rule));
    (void)smh::Device::get();
    if (!index) throw Error(smh::kMsg, "filter: index is NULL");   // (MSG like every refusal of this call)
    const smh::FilterRule r{rule->operand_mode, rule->abund_out, rule->min_abund, rule->max_abund, rule->min_owners, rule->max_owners};
    return new SmhIndex(*index, operand, r);
  });
}
SmhIndex* smh_index_select(SmhIndex* index, const uint32_t* ids, uint32_t n_ids) {
  return pad<SmhIndex*>([&] {
    (void)smh::Device::get();
    if (!index) throw Error(smh::kMsg, "select: index is NULL");
    return new SmhIndex(*index, ids, n_ids);
  });
}
void smh_filter_geometry(uint32_t* tile, uint32_t* operand_samples, uint32_t* threads) { smh::filter_geometry(tile, operand_samples, threads); }

// ------------------------------------------------------------------ signature JSON on the device (sigscan.cpp)

struct SmhSignatures : smh::Signatures {};
static_assert(SMH_SIGSPAN_CLOSED == smh::sigscan::kClosed && SMH_SIGSPAN_OPEN == smh::sigscan::kOpen &&
              SMH_SIGSPAN_OVERFLOW == smh::sigscan::kOverflow && SMH_SIGSPAN_BAD_SYNTAX == smh::sigscan::kBadSyntax,
              "the statuses of the header are sigscan_core.hpp's");

static SmhSignatures* signatures_parse(const void* text, const char* what, bool on_host, uint64_t len, const uint64_t* doc_offsets,
                                       uint32_t n_docs, void* stream) {
  return pad<SmhSignatures*>([&] {
    auto& dev = smh::Device::get();
    if (len) require(text, what);
    auto sigs = std::make_unique<SmhSignatures>();
    smh::parse_signatures(sigs.get(), text, on_host, len, doc_offsets, n_docs, stream, dev);
    return sigs.release();
  });
}
SmhSignatures* smh_signatures_parse(const char* text, uint64_t len, const uint64_t* doc_offsets, uint32_t n_docs) {
  return signatures_parse(text, "text", true, len, doc_offsets, n_docs, nullptr);
}
SmhSignatures* smh_signatures_parse_dev(const void* text_dev, uint64_t len, const uint64_t* doc_offsets, uint32_t n_docs, void* stream) {
  return signatures_parse(text_dev, "text_dev", false, len, doc_offsets, n_docs, stream);
}
void smh_signatures_free(SmhSignatures* sigs) { delete sigs; }
uint32_t smh_signatures_len(const SmhSignatures* sigs) { return sigs ? (uint32_t)sigs->entries.size() : 0; }
uint64_t smh_signatures_spans(const SmhSignatures* sigs) { return sigs ? sigs->spans.size() : 0; }
uint64_t smh_signatures_tokens(const SmhSignatures* sigs) { return sigs ? sigs->n_tokens : 0; }
const uint64_t* smh_signatures_values_dev(const SmhSignatures* sigs) { return sigs ? sigs->values_dev() : nullptr; }

int smh_signatures_entry(const SmhSignatures* sigs, uint32_t i, SmhSigEntry* out) {
  return pad_code([&] {
    require(sigs, "sigs"); require(out, "out");
    if (i >= sigs->entries.size()) throw Error(smh::kMsg, "signatures: entry " + std::to_string(i) + " of " + std::to_string(sigs->entries.size()));
    const smh::SigEntry& e = sigs->entries[i];
    memset(out, 0, sizeof *out);
    out->document = e.document; out->signature = e.signature; out->sketch = e.sketch;
    out->num = e.num; out->ksize = e.ksize; out->seed = e.seed; out->max_hash = e.max_hash; out->molecule = e.molecule;
    out->name_is_null = !e.has_name; out->filename_is_null = !e.has_filename; out->has_abundances = e.has_abunds;
    out->name = e.name.c_str(); out->filename = e.filename.c_str(); out->license = e.license.c_str();
    out->sig_class = e.klass.c_str(); out->md5sum = e.md5sum.c_str();
    out->n_mins = e.n_mins; out->n_abundances = e.n_abunds; out->mins_span = e.mins_span; out->abundances_span = e.abunds_span;
  });
}

int smh_signatures_span(const SmhSignatures* sigs, uint64_t k, uint64_t* start, uint64_t* end, uint64_t* first_token, uint64_t* n_tokens,
                        uint32_t* status, uint64_t* bad_offset) {
  return pad_code([&] {
    require(sigs, "sigs");
    if (k >= sigs->spans.size()) throw Error(smh::kMsg, "signatures: span " + std::to_string(k) + " of " + std::to_string(sigs->spans.size()));
    const smh::sigscan::SpanRow& r = sigs->spans[k];
    if (start) *start = r.start;
    if (end) *end = r.end;
    if (first_token) *first_token = r.first_token;
    if (n_tokens) *n_tokens = r.n_tokens;
    if (status) *status = r.status;
    if (bad_offset) *bad_offset = r.bad_off;
  });
}

SmhIndex* smh_signatures_index(const SmhSignatures* sigs, const uint32_t* ids, uint32_t n_ids) {
  return pad<SmhIndex*>([&] {
    (void)smh::Device::get();
    if (!sigs) throw Error(smh::kMsg, "index from signatures: sigs is NULL");
    return new SmhIndex(*sigs, ids, n_ids);   // (ids == NULL: every entry, n_ids is not read)
  });
}
uint32_t smh_signatures_filter(const SmhSignatures* sigs, uint64_t ksize, const char* moltype, uint32_t* ids_out) {
  return pad<uint32_t>([&] {
    require(sigs, "sigs");
    const std::vector<uint32_t> ids = smh::signatures_filter(*sigs, (size_t)ksize, moltype);
    if (ids_out) std::copy(ids.begin(), ids.end(), ids_out);
    return (uint32_t)ids.size();
  });
}
SmhIndex* smh_signatures_index_filtered(const SmhSignatures* sigs, uint64_t ksize, const char* moltype) {
  return pad<SmhIndex*>([&] {
    (void)smh::Device::get();
    if (!sigs) throw Error(smh::kMsg, "index from signatures: sigs is NULL");
    const std::vector<uint32_t> ids = smh::signatures_filter(*sigs, (size_t)ksize, moltype);
    static const uint32_t none = 0;
    return new SmhIndex(*sigs, ids.empty() ? &none : ids.data(), (uint32_t)ids.size());
  });
}
void smh_sigscan_geometry(uint32_t* tile_bytes, uint32_t* threads) { smh::sigscan_geometry(tile_bytes, threads); }

// ------------------------------------------------------------------ signature JSON written on the device (sigtext.cpp)

struct SmhSigText : smh::SigText {};

SmhSigText* smh_index_sigtext(SmhIndex* index, const char* const* names, const char* const* filenames, const uint32_t* doc_starts,
                              uint32_t n_docs) {
  return pad<SmhSigText*>([&] {
    auto& dev = smh::Device::get();
    if (!index) throw Error(smh::kMsg, "sigtext: index is NULL");   // (MSG like every refusal of this call)
    auto t = std::make_unique<SmhSigText>();
    smh::index_sigtext(t.get(), *index, names, filenames, doc_starts, n_docs, dev);
    return t.release();
  });
}
uint64_t smh_sigtext_len(const SmhSigText* t) { return t ? t->len : 0; }
uint32_t smh_sigtext_documents(const SmhSigText* t) { return t && !t->doc_offsets.empty() ? (uint32_t)(t->doc_offsets.size() - 1) : 0; }
int smh_sigtext_doc_offsets(const SmhSigText* t, uint64_t* out) {
  return pad_code([&] {
    require(t, "text"); require(out, "out");
    std::copy(t->doc_offsets.begin(), t->doc_offsets.end(), out);
  });
}
const void* smh_sigtext_dev(const SmhSigText* t) { return t ? t->text_dev() : nullptr; }
int smh_sigtext_read(const SmhSigText* t, uint64_t offset, uint64_t len, char* out) {
  return pad_code([&] {
    require(t, "text");
    if (offset > t->len || len > t->len - offset)
      throw Error(smh::kMsg, "sigtext: bytes " + std::to_string(offset) + " + " + std::to_string(len) + " of a text of " + std::to_string(t->len));
    if (!len) return;
    require(out, "out");
    auto& dev = smh::Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    HIP_CHECK(hipMemcpyAsync(out, t->text_dev() + offset, len, hipMemcpyDeviceToHost, dev.stream()));
    HIP_CHECK(hipStreamSynchronize(dev.stream()));
  });
}
void smh_sigtext_free(SmhSigText* t) { delete t; }
int smh_index_md5(SmhIndex* index, uint8_t* out) {
  return pad_code([&] {
    auto& dev = smh::Device::get();
    if (!index) throw Error(smh::kMsg, "sigtext: index is NULL");
    if (index->n) require(out, "out");
    smh::index_md5(*index, out, dev);
  });
}
void smh_sigtext_geometry(uint32_t* values_per_tile, uint32_t* threads, uint32_t* md5_values_per_step) {
  smh::sigtext_geometry(values_per_tile, threads, md5_values_per_step);
}

int smh_index_compare(SmhIndex* rows, SmhIndex* cols, double* jaccard, uint64_t* common, uint64_t* size,
                      uint64_t* count_common, double* containment) {
  return pad_code([&] { require(rows, "rows"); require(cols, "cols"); rows->compare(*cols, jaccard, common, size, count_common, containment); });
}

// ------------------------------------------------------------------ angular similarity on abundances

bool smh_index_has_abundances(const SmhIndex* index) { return index && index->has_abunds; }

int smh_index_norms2(SmhIndex* index, uint64_t* out) { return pad_code([&] { require(index, "index"); index->norms2(out); }); }
int smh_index_angular(SmhIndex* rows, SmhIndex* cols, uint64_t* dot, double* cosine, double* angular) {
  return pad_code([&] { require(rows, "rows"); require(cols, "cols"); rows->angular(*cols, dot, cosine, angular); });
}
int smh_index_angular_query(SmhIndex* index, const KmerMinHash* query, uint64_t* dot, uint64_t* query_norm2, double* cosine,
                            double* angular) {
  return pad_code([&] { require(index, "index"); require(query, "query"); index->angular_query(*query, dot, query_norm2, cosine, angular); });
}
int smh_angular_similarity(const KmerMinHash* a, const KmerMinHash* b, double* angular, double* cosine, uint64_t* dot,
                           uint64_t* norm2_a, uint64_t* norm2_b) {
  return pad_code([&] { require(a, "a"); require(b, "b"); smh::angular_similarity(*a, *b, angular, cosine, dot, norm2_a, norm2_b); });
}
int smh_angular_block_dev(const uint64_t* row_hashes_dev, const uint32_t* row_abunds_dev, const uint64_t* row_offsets, uint32_t n_rows,
                          const uint64_t* col_hashes_dev, const uint32_t* col_abunds_dev, const uint64_t* col_offsets, uint32_t n_cols,
                          const uint64_t* count_common_dev, bool symmetric, uint64_t* dot_dev, uint64_t* row_norm2_dev,
                          uint64_t* col_norm2_dev, double* cosine_dev, double* angular_dev, void* stream) {
  return pad_code([&] {
    require(row_offsets, "row_offsets"); require(col_offsets, "col_offsets");
    smh::angular_block_dev({row_hashes_dev, row_abunds_dev, nullptr, nullptr, n_rows}, row_offsets,
                           {col_hashes_dev, col_abunds_dev, nullptr, nullptr, n_cols}, col_offsets, count_common_dev, symmetric,
                           {dot_dev, cosine_dev, angular_dev}, row_norm2_dev, col_norm2_dev, stream);
  });
}
void smh_angular_last_stats(uint64_t* pairs_walked, uint64_t* pairs_skipped) {
  if (pairs_walked) *pairs_walked = smh::g_angular_walked;
  if (pairs_skipped) *pairs_skipped = smh::g_angular_skipped;
}
uint64_t smh_angular_prune_min_pairs(void) { return smh::g_angular_prune_min_pairs; }
void smh_angular_set_prune_min_pairs(uint64_t pairs) { smh::g_angular_prune_min_pairs = pairs ? pairs : smh::kAngularPruneMinPairs; }

// ------------------------------------------------------------------ downsampling (downsample.cpp, index.cpp)

KmerMinHash* smh_kmerminhash_downsample_max_hash(const KmerMinHash* ptr, uint64_t max_hash) {
  return pad<KmerMinHash*>([&] {
    require(ptr, "ptr");
    std::unique_ptr<KmerMinHash> out(new KmerMinHash());
    smh::downsample_max_hash(*ptr, max_hash, *out);
    return out.release();
  });
}
KmerMinHash* smh_kmerminhash_downsample_num(const KmerMinHash* ptr, uint32_t num) {
  return pad<KmerMinHash*>([&] {
    require(ptr, "ptr");
    std::unique_ptr<KmerMinHash> out(new KmerMinHash());
    smh::downsample_num(*ptr, num, *out);
    return out.release();
  });
}
SmhIndex* smh_index_downsample(SmhIndex* index, uint64_t max_hash) {
  return pad<SmhIndex*>([&] { require(index, "index"); return new SmhIndex(*index, max_hash); });
}
int smh_index_max_hash_range(const SmhIndex* index, uint64_t* lo, uint64_t* hi) {
  return pad_code([&] { require(index, "index"); index->max_hash_range(lo, hi); });
}
int smh_downsample_block_dev(const uint64_t* hashes_dev, const uint32_t* abunds_dev, const uint64_t* offsets, uint32_t n, uint64_t max_hash,
                             uint64_t* out_hashes_dev, uint32_t* out_abunds_dev, uint64_t capacity, uint64_t* out_offsets, void* stream) {
  return pad_code([&] {
    smh::downsample_block_dev(hashes_dev, abunds_dev, offsets, n, max_hash, out_hashes_dev, out_abunds_dev, capacity, out_offsets, stream);
  });
}
bool smh_index_all_scaled(const SmhIndex* index) { return index && index->all_scaled; }
void smh_downsample_geometry(uint32_t* tile_elems, uint32_t* threads) { smh::downsample_geometry(tile_elems, threads); }

// ------------------------------------------------------------------ matching records (match.cpp)

static_assert(sizeof(SmhMatchRow) == 24 && sizeof(smh::MatchRow) == 24, "SmhMatchRow is 24 bytes");
static_assert(offsetof(SmhMatchRow, best) == 16 && offsetof(smh::MatchRow, best) == 16, "SmhMatchRow layout");

namespace {
// the checks every route shares, the call, and the hit list handed out the way smh_intersection hands out common_out
void match_call(SmhIndex* index, const uint8_t* seq_dev, uint64_t total_len, const uint64_t* offsets, uint32_t n, SmhMatchRow* rows,
                uint64_t* hit_offsets, uint64_t** hit_hashes, uint64_t* n_hits, hipStream_t s) {
  const bool want = hit_offsets || hit_hashes || n_hits;
  std::vector<uint64_t> hits;
  index->match(seq_dev, total_len, offsets, n, reinterpret_cast<smh::MatchRow*>(rows), want ? hit_offsets : nullptr, want ? &hits : nullptr, s);
  if (!want) return;
  uint64_t* out = (uint64_t*)malloc((hits.empty() ? 1 : hits.size()) * sizeof(uint64_t));
  if (!out) smh::throw_internal("out of memory");
  if (!hits.empty()) memcpy(out, hits.data(), hits.size() * sizeof(uint64_t));
  *hit_hashes = out; *n_hits = hits.size();
}
void match_require(SmhIndex* index, const uint64_t* offsets, uint32_t n, SmhMatchRow* rows, uint64_t* hit_offsets, uint64_t** hit_hashes,
                   uint64_t* n_hits) {
  require(index, "index");
  if (n) { require(offsets, "offsets"); require(rows, "rows"); }
  if (hit_offsets || hit_hashes || n_hits) { require(hit_offsets, "hit_offsets"); require(hit_hashes, "hit_hashes"); require(n_hits, "n_hits"); }
  index->check_matchable();
}
}  // namespace

int smh_index_match_sequences(SmhIndex* index, const char* seq, const uint64_t* offsets, uint32_t n_records, SmhMatchRow* rows,
                              uint64_t* hit_offsets, uint64_t** hit_hashes, uint64_t* n_hits) {
  return pad_code([&] {
    auto& dev = smh::Device::get();   // first: without a device the call says so, whatever it was handed
    match_require(index, offsets, n_records, rows, hit_offsets, hit_hashes, n_hits);
    auto& E = smh::Engine::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    const uint64_t base = n_records ? offsets[0] : 0, total = n_records ? offsets[n_records] - base : 0;
    if (n_records && offsets[n_records] < base) throw Error(smh::kMsg, "match: offsets must ascend");
    if (total) require(seq, "seq");
    std::vector<uint64_t> rel((size_t)n_records + 1, 0);
    for (uint32_t i = 0; n_records && i <= n_records; i++) rel[i] = offsets[i] - base;
    E.seqbuf.ensure(total + 64);
    if (total) HIP_CHECK(hipMemcpyAsync(E.seqbuf.ptr, seq + base, total, hipMemcpyHostToDevice, dev.stream()));
    match_call(index, E.seqbuf.as<uint8_t>(), total, rel.data(), n_records, rows, hit_offsets, hit_hashes, n_hits, dev.stream());
  });
}

int smh_index_match_sequences_dev(SmhIndex* index, const void* seq_dev, uint64_t total_len, const uint64_t* offsets, uint32_t n_records,
                                  SmhMatchRow* rows, uint64_t* hit_offsets, uint64_t** hit_hashes, uint64_t* n_hits, void* stream) {
  return pad_code([&] {
    auto& dev = smh::Device::get();
    match_require(index, offsets, n_records, rows, hit_offsets, hit_hashes, n_hits);
    if (total_len) require(seq_dev, "seq_dev");
    match_call(index, (const uint8_t*)seq_dev, total_len, offsets, n_records, rows, hit_offsets, hit_hashes, n_hits, dev.user_stream(stream));
  });
}

int smh_index_match_records(SmhIndex* index, const SmhRecords* r, SmhMatchRow* rows, uint64_t* hit_offsets, uint64_t** hit_hashes,
                            uint64_t* n_hits) {
  return pad_code([&] {
    auto& dev = smh::Device::get();
    require(r, "records");
    match_require(index, r->offsets, r->n, rows, hit_offsets, hit_hashes, n_hits);
    match_call(index, r->seq_dev(), r->total, r->offsets, r->n, rows, hit_offsets, hit_hashes, n_hits, dev.user_stream(nullptr));
  });
}

void smh_match_geometry(uint32_t* lds_pairs, uint32_t* threads_per_record, uint32_t* probe_samples) {
  smh::match_geometry(lds_pairs, threads_per_record, probe_samples);
}
void smh_match_set_pair_budget(uint64_t pairs) { smh::g_match_pair_budget = pairs ? pairs : smh::kMatchPairBudget; }
uint64_t smh_match_pair_budget(void) { return smh::g_match_pair_budget; }

// ------------------------------------------------------------------ taxonomic LCA (lca.cpp)

static_assert(sizeof(SmhLcaRow) == 24 && sizeof(smh::LcaRow) == 24, "SmhLcaRow is 24 bytes");
static_assert(offsetof(SmhLcaRow, taxon) == 16 && offsetof(smh::LcaRow, taxon) == 16, "SmhLcaRow layout");
static_assert(SMH_NO_TAXON == smh::kLcaNoTaxon, "SMH_NO_TAXON");

int smh_lca_check_taxonomy(const uint32_t* parent, uint32_t n_taxa, const uint32_t* node_taxon, uint32_t n_nodes, uint32_t index_len) {
  return pad_code([&] {
    if (n_taxa) require(parent, "parent");
    if (n_nodes) require(node_taxon, "node_taxon");
    smh::lca_check_taxonomy(parent, n_taxa, node_taxon, n_nodes, index_len);
  });
}
int smh_index_set_taxonomy(SmhIndex* index, const uint32_t* parent, uint32_t n_taxa, const uint32_t* node_taxon, uint32_t n_nodes) {
  return pad_code([&] {
    require(index, "index");
    if (n_taxa) require(parent, "parent");
    if (n_nodes) require(node_taxon, "node_taxon");
    index->set_taxonomy(parent, n_taxa, node_taxon, n_nodes);
  });
}
bool smh_index_has_taxonomy(const SmhIndex* index) { return index && index->has_taxonomy(); }

namespace {
// the pairs handed out the way gather_many hands out its rows: malloc'ed, one element at least
void lca_counts_out(const std::vector<uint32_t>& t, const std::vector<uint64_t>& c, uint32_t** taxa, uint64_t** counts) {
  const size_t k = t.empty() ? 1 : t.size();
  uint32_t* ot = (uint32_t*)malloc(k * sizeof(uint32_t));
  uint64_t* oc = (uint64_t*)malloc(k * sizeof(uint64_t));
  if (!ot || !oc) { free(ot); free(oc); smh::throw_internal("out of memory"); }
  if (!t.empty()) { memcpy(ot, t.data(), t.size() * sizeof(uint32_t)); memcpy(oc, c.data(), c.size() * sizeof(uint64_t)); }
  *taxa = ot; *counts = oc;
}
void lca_records_require(SmhIndex* index, const uint64_t* offsets, uint32_t n, SmhLcaRow* rows) {
  require(index, "index");
  if (n) { require(offsets, "offsets"); require(rows, "rows"); }
  index->check_matchable();
  if (!index->has_taxonomy()) throw Error(smh::kMsg, "lca_records: the index has no taxonomy (smh_index_set_taxonomy)");
}
}  // namespace

int smh_index_lca_many(SmhIndex* index, const KmerMinHash* const* queries, uint32_t n_queries, uint64_t* count_offsets, uint32_t** taxa,
                       uint64_t** counts, uint64_t* query_offsets, uint32_t* hash_taxon) {
  return pad_code([&] {
    auto& dev = smh::Device::get();   // first: without a device the call says so, whatever it was handed
    require(index, "index"); require(count_offsets, "count_offsets"); require(taxa, "taxa"); require(counts, "counts");
    const std::vector<const smh::KmerMinHash*> v = require_queries(queries, n_queries);
    std::vector<uint32_t> t;
    std::vector<uint64_t> c;
    index->lca_many(v.data(), n_queries, count_offsets, &t, &c, query_offsets, hash_taxon, dev);
    lca_counts_out(t, c, taxa, counts);
  });
}

int smh_index_lca_block_dev(SmhIndex* index, const uint64_t* q_hashes_dev, const uint64_t* q_offsets, uint32_t n_queries,
                            uint64_t* count_offsets, uint32_t** taxa, uint64_t** counts, uint32_t* hash_taxon, void* stream) {
  return pad_code([&] {
    auto& dev = smh::Device::get();
    require(index, "index"); require(count_offsets, "count_offsets"); require(taxa, "taxa"); require(counts, "counts");
    require(q_offsets, "q_offsets");
    if (n_queries && q_offsets[n_queries] != q_offsets[0]) require(q_hashes_dev, "q_hashes_dev");
    std::vector<uint32_t> t;
    std::vector<uint64_t> c;
    index->lca_many_dev(q_hashes_dev, q_offsets, n_queries, count_offsets, &t, &c, hash_taxon, dev, dev.user_stream(stream));
    lca_counts_out(t, c, taxa, counts);
  });
}

int smh_index_lca_sequences(SmhIndex* index, const char* seq, const uint64_t* offsets, uint32_t n_records, SmhLcaRow* rows) {
  return pad_code([&] {
    auto& dev = smh::Device::get();   // first: without a device the call says so, whatever it was handed
    lca_records_require(index, offsets, n_records, rows);
    auto& E = smh::Engine::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    const uint64_t base = n_records ? offsets[0] : 0, total = n_records ? offsets[n_records] - base : 0;
    if (n_records && offsets[n_records] < base) throw Error(smh::kMsg, "match: offsets must ascend");
    if (total) require(seq, "seq");
    std::vector<uint64_t> rel((size_t)n_records + 1, 0);
    for (uint32_t i = 0; n_records && i <= n_records; i++) rel[i] = offsets[i] - base;
    E.seqbuf.ensure(total + 64);
    if (total) HIP_CHECK(hipMemcpyAsync(E.seqbuf.ptr, seq + base, total, hipMemcpyHostToDevice, dev.stream()));
    index->lca_records(E.seqbuf.as<uint8_t>(), total, rel.data(), n_records, reinterpret_cast<smh::LcaRow*>(rows), dev.stream());
  });
}

int smh_index_lca_sequences_dev(SmhIndex* index, const void* seq_dev, uint64_t total_len, const uint64_t* offsets, uint32_t n_records,
                                SmhLcaRow* rows, void* stream) {
  return pad_code([&] {
    auto& dev = smh::Device::get();
    lca_records_require(index, offsets, n_records, rows);
    if (total_len) require(seq_dev, "seq_dev");
    index->lca_records((const uint8_t*)seq_dev, total_len, offsets, n_records, reinterpret_cast<smh::LcaRow*>(rows), dev.user_stream(stream));
  });
}

int smh_index_lca_records(SmhIndex* index, const SmhRecords* r, SmhLcaRow* rows) {
  return pad_code([&] {
    auto& dev = smh::Device::get();
    require(r, "records");
    lca_records_require(index, r->offsets, r->n, rows);
    index->lca_records(r->seq_dev(), r->total, r->offsets, r->n, reinterpret_cast<smh::LcaRow*>(rows), dev.user_stream(nullptr));
  });
}

void smh_lca_geometry(uint32_t* owner_lane_max, uint32_t* record_lane_max, uint32_t* threads) {
  smh::lca_geometry(owner_lane_max, record_lane_max, threads);
}
void smh_lca_set_budget(uint64_t keys) { smh::g_lca_budget = keys ? keys : smh::kLcaBudget; }
uint64_t smh_lca_budget(void) { return smh::g_lca_budget; }
void smh_set_grid_cap(uint32_t workgroups) { smh::g_grid_cap = workgroups; }
uint32_t smh_grid_cap(void) { return smh::g_grid_cap; }
void smh_set_pool_fill(int32_t byte) { smh::g_pool_fill = byte >= 0 && byte <= 255 ? byte : -1; }
int32_t smh_pool_fill(void) { return smh::g_pool_fill; }

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

int smh_release_workspace(void) {
  return pad_code([&] {
    // the dictionaries resident indexes cached for their all-vs-all compares (ranks, roots, the partition table: up to
    // hundreds of MB for 10 000 long sketches); the next block of an index with itself rebuilds its own
    smh::ResidentIndex::drop_all_dictionaries();
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
