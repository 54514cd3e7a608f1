// angular.cpp -- the host half of angular similarity on abundances: staging one sketch as an operand, the
// norms of a resident index, the prune pass through ResidentIndex::compare_block, the read-back of the block kernel.
#include <algorithm>
#include <cstring>
#include <string>

#include "index.hpp"

namespace smh {

uint64_t g_angular_prune_min_pairs = kAngularPruneMinPairs, g_angular_walked = 0, g_angular_skipped = 0;

namespace {
void require_tracking(const KmerMinHash& mh, const char* what) {
  if (!mh.has_abunds) throw Error(kMsg, std::string("angular: ") + what + " does not track abundances");
}
[[noreturn]] void throw_norm(const std::string& who) {
  throw Error(kMsg, "angular: norm2 of " + who + " does not fit 64 bits (an abundance of 2^32 or more, or too many large ones)");
}
// what can be said about a sketch without the device: a host state whose abundance vector does not match its hashes
void check_host_state(const KmerMinHash& mh, const char* what) {
  if (!mh.dev && mh.pend_seq.empty() && mh.pend_words.empty() && mh.abunds.size() != mh.mins.size())
    throw Error(kMsg, std::string("angular: the abundance vector of ") + what + " does not match its hashes (quirks Q5/Q6)");
}
void require_abundances(const ResidentIndex& index, const char* what) {
  if (!index.has_abunds)
    throw Error(kMsg, std::string("angular: ") + what + " holds a node that does not track abundances, or whose abundance "
                "vector does not match its hashes (quirks Q5/Q6)");
}

// One sketch in the form the kernels read: hashes and u32 abundances in device memory, offsets {0, n}, its norm2.  A state
// that lives in HBM is read there (its abundances are narrowed by a kernel); a host state is uploaded.
struct Operand {
  const uint64_t* hashes = nullptr;
  const uint32_t* abunds = nullptr;
  uint32_t n = 0;
  std::vector<uint32_t> staged;
  uint64_t off[2] = {0, 0}, norm2 = 0;   // norm2, err: read back by prepare, valid once the stream was waited for
  uint32_t err = kAngularNoError;
  const char* what = "";
  Workspace ws;                // `small` and the store (behind what the uploads and read-backs touch: it waits for them first)
  uint64_t* small = nullptr;   // offsets (2 x u64), norm2 (u64), error word (u32)
  explicit Operand(hipStream_t s) : ws(s) {}
  uint64_t* offsets_dev() const { return small; }
  uint64_t* norm2_dev() const { return small + 2; }
  uint32_t* err_dev() const { return reinterpret_cast<uint32_t*>(small + 3); }
  AngularSet set() const { return {hashes, abunds, offsets_dev(), norm2_dev(), 1}; }
};

// queues the operand's upload / narrowing and its norm; settle() waits for them
void prepare(Operand& op, const KmerMinHash& mh, const char* what, hipStream_t s) {
  mh.flush_pending();
  op.what = what;
  op.small = op.ws.take<uint64_t>(4);
  HIP_CHECK(hipMemsetAsync(op.err_dev(), 0xff, 4, s));
  uint64_t n = 0;
  if (mh.dev) {
    const DeviceSketch& S = *mh.dev;
    n = S.n;
    if (n >= 0xffffffffull) throw_internal("angular: a sketch of 2^32 - 1 or more hashes");
    if (n && !S.has_counts && !S.has_runs) throw_internal("angular: the sketch's device state carries no abundances");
    uint32_t* narrow = op.ws.take<uint32_t>(n);
    op.hashes = S.uniq.as<uint64_t>();
    op.abunds = narrow;
    launch_angular_narrow(S.has_counts ? S.counts.as<uint64_t>() : nullptr, S.has_counts ? nullptr : S.starts.as<uint32_t>(),
                          (uint32_t)S.total, (uint32_t)n, narrow, op.err_dev(), 0, s);
  } else {
    n = mh.mins.size();
    check_host_state(mh, what);   // (nothing is pending any more)
    if (n >= 0xffffffffull) throw_internal("angular: a sketch of 2^32 - 1 or more hashes");
    op.staged.resize(n);
    for (uint64_t i = 0; i < n; i++) {
      if (mh.abunds[i] >> 32) throw_norm(what);
      op.staged[i] = (uint32_t)mh.abunds[i];
    }
    uint64_t* store = reinterpret_cast<uint64_t*>(op.ws.take<uint8_t>(n * 12));   // n hashes, then n u32 abundances
    if (n) {
      HIP_CHECK(hipMemcpyAsync(store, mh.mins.data(), n * 8, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(store + n, op.staged.data(), n * 4, hipMemcpyHostToDevice, s));
    }
    op.hashes = store;
    op.abunds = reinterpret_cast<const uint32_t*>(store + n);
  }
  op.n = (uint32_t)n;
  op.off[1] = n;
  HIP_CHECK(hipMemcpyAsync(op.offsets_dev(), op.off, 16, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(op.norm2_dev(), 0, 8, s));
  launch_angular_norms(op.abunds, op.offsets_dev(), 1, op.norm2_dev(), op.err_dev(), s);
  HIP_CHECK(hipMemcpyAsync(&op.norm2, op.norm2_dev(), 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(&op.err, op.err_dev(), 4, hipMemcpyDeviceToHost, s));
}
// waits for the prepared operands and refuses the first whose norm2 does not fit
void settle(std::initializer_list<Operand*> ops, hipStream_t s) {
  HIP_CHECK(hipStreamSynchronize(s));
  for (Operand* bad : ops)
    if (bad->err != kAngularNoError) throw_norm(bad->what);
}

// runs the block kernel into pool memory and brings the wanted outputs and the two counters back; the stream is idle after
void run_host(const AngularSet& R, const AngularSet& C, const uint64_t* prune_dev, bool symmetric, uint64_t* dot, double* cosine,
              double* angular, Device& dev, hipStream_t s) {
  const size_t np = (size_t)R.n * C.n;
  uint64_t cnt[2] = {0, 0};
  Workspace ws(s);
  uint64_t* d_dot = ws.take<uint64_t>(dot ? np : 0);   // (an output nobody wants still takes its smallest block)
  double* d_cos = ws.take<double>(cosine ? np : 0);
  double* d_ang = ws.take<double>(angular ? np : 0);
  unsigned long long* d_cnt = ws.take<unsigned long long>(2);
  const AngularOut o{dot ? d_dot : nullptr, cosine ? d_cos : nullptr, angular ? d_ang : nullptr};
  launch_angular_block(R, C, prune_dev, symmetric, o, d_cnt, dev, s);
  if (dot) HIP_CHECK(hipMemcpyAsync(dot, d_dot, np * 8, hipMemcpyDeviceToHost, s));
  if (cosine) HIP_CHECK(hipMemcpyAsync(cosine, d_cos, np * 8, hipMemcpyDeviceToHost, s));
  if (angular) HIP_CHECK(hipMemcpyAsync(angular, d_ang, np * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(cnt, d_cnt, 16, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  g_angular_walked = cnt[0]; g_angular_skipped = cnt[1];
}
}  // namespace

void ResidentIndex::angular_ensure(const char* what, hipStream_t s) {
  if (!angular_ready) {
    // (a cut made from a parent whose abundances were in HBM holds them in abunds_dev already: nothing to allocate or upload)
    if (!abunds_resident) abunds_dev.ensure(h_abunds.size() * 4 + 4);
    norm2_dev.ensure((size_t)n * 8 + 8);
    h_norm2.assign(n, 0);
    uint32_t err = kAngularNoError;
    if (n) {
      Workspace ws(s);
      uint32_t* e = ws.take<uint32_t>(1);
      HIP_CHECK(hipMemsetAsync(e, 0xff, 4, s));
      if (!abunds_resident && !h_abunds.empty())
        HIP_CHECK(hipMemcpyAsync(abunds_dev.ptr, h_abunds.data(), h_abunds.size() * 4, hipMemcpyHostToDevice, s));
      launch_angular_norms(abunds_dev.as<uint32_t>(), offsets.as<uint64_t>(), n, norm2_dev.as<uint64_t>(), e, s);
      HIP_CHECK(hipMemcpyAsync(h_norm2.data(), norm2_dev.ptr, (size_t)n * 8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(&err, e, 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
    bad_node = std::min(wide_node, err);
    std::vector<uint32_t>().swap(h_abunds);   // they live in HBM now
    angular_ready = true;
  }
  if (bad_node != kAngularNoError) throw_norm(std::string(what) + " " + std::to_string(bad_node));
}

void ResidentIndex::norms2(uint64_t* out) {
  require_abundances(*this, "the index");
  if (n == 0) return;
  require(out, "out");
  auto& dev = Device::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  angular_ensure("node", dev.stream());
  std::copy(h_norm2.begin(), h_norm2.end(), out);
}

void ResidentIndex::angular(ResidentIndex& cols, uint64_t* dot, double* cosine, double* angular) {
  const bool self = this == &cols;
  require_abundances(*this, "the row index");
  require_abundances(cols, "the column index");
  check_index(cols);
  const size_t np = (size_t)n * cols.n;
  auto& dev = Device::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  g_angular_walked = g_angular_skipped = 0;
  angular_ensure(self ? "node" : "row node", s);
  if (!self) cols.angular_ensure("column node", s);
  if (np == 0) return;
  Workspace ws(s);
  uint64_t* cc = nullptr;
  if (np >= g_angular_prune_min_pairs) {
    cc = ws.take<uint64_t>(np);
    compare_block(*this, cols, CompareOut{nullptr, nullptr, nullptr, cc, nullptr}, dev, s);
  }
  run_host(angular_set(), cols.angular_set(), cc, self, dot, cosine, angular, dev, s);
}

void ResidentIndex::angular_query(const KmerMinHash& query, uint64_t* dot, uint64_t* query_norm2, double* cosine, double* angular) {
  require_abundances(*this, "the index");
  require_tracking(query, "the query");
  check_host_state(query, "the query");
  check_sketch(query);
  auto& dev = Device::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  g_angular_walked = g_angular_skipped = 0;
  angular_ensure("node", s);
  Operand q(s);
  prepare(q, query, "the query", s);
  settle({&q}, s);
  if (query_norm2) std::fill(query_norm2, query_norm2 + n, q.norm2);
  if (n) run_host(q.set(), angular_set(), nullptr, false, dot, cosine, angular, dev, s);
}

void angular_similarity(const KmerMinHash& a, const KmerMinHash& b, double* angular, double* cosine, uint64_t* dot, uint64_t* norm2_a,
                        uint64_t* norm2_b) {
  require_tracking(a, "the first sketch");
  require_tracking(b, "the second sketch");
  a.check_compatible(b);
  check_host_state(a, "the first sketch");
  check_host_state(b, "the second sketch");
  auto& dev = Device::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  g_angular_walked = g_angular_skipped = 0;
  Operand A(s), B(s);
  prepare(A, a, "the first sketch", s);
  prepare(B, b, "the second sketch", s);
  settle({&A, &B}, s);
  uint64_t d = 0;
  double c = 0.0, an = 0.0;
  run_host(A.set(), B.set(), nullptr, false, &d, &c, &an, dev, s);
  if (angular) *angular = an;
  if (cosine) *cosine = c;
  if (dot) *dot = d;
  if (norm2_a) *norm2_a = A.norm2;
  if (norm2_b) *norm2_b = B.norm2;
}

void angular_block_dev(AngularSet R, const uint64_t* row_offsets, AngularSet C, const uint64_t* col_offsets,
                       const uint64_t* count_common_dev, bool symmetric, const AngularOut& out, uint64_t* row_norm2_dev,
                       uint64_t* col_norm2_dev, void* stream) {
  const uint32_t n_rows = R.n, n_cols = C.n;
  if (symmetric && (n_rows != n_cols || std::memcmp(row_offsets, col_offsets, ((size_t)n_rows + 1) * 8) != 0))
    throw Error(kMsg, "angular: a symmetric block needs the same sketches as rows and as columns");
  auto ascending = [](const uint64_t* off, uint32_t n, const char* name) {
    for (uint32_t i = 0; i < n; i++)
      if (off[i + 1] < off[i] || off[i + 1] - off[i] >= 0xffffffffull)
        throw Error(kMsg, std::string("angular: ") + name + " must ascend, with sketches shorter than 2^32 - 1");
  };
  ascending(row_offsets, n_rows, "row_offsets");
  ascending(col_offsets, n_cols, "col_offsets");
  if (row_offsets[n_rows] > row_offsets[0]) { require(R.hashes, "row_hashes_dev"); require(R.abunds, "row_abunds_dev"); }
  if (col_offsets[n_cols] > col_offsets[0]) { require(C.hashes, "col_hashes_dev"); require(C.abunds, "col_abunds_dev"); }
  auto& dev = Device::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.user_stream(stream);
  g_angular_walked = g_angular_skipped = 0;
  Workspace ws(s);
  uint64_t* d_ro = ws.take<uint64_t>((size_t)n_rows + n_cols + 2);
  uint64_t* norms = ws.take<uint64_t>((size_t)n_rows + n_cols);
  uint64_t* d_co = d_ro + n_rows + 1;
  uint64_t* d_rn = row_norm2_dev ? row_norm2_dev : norms;
  uint64_t* d_cn = col_norm2_dev ? col_norm2_dev : norms + n_rows;
  R.offsets = d_ro; R.norm2 = d_rn;
  C.offsets = d_co; C.norm2 = d_cn;
  unsigned long long* d_cnt = ws.take<unsigned long long>(4);
  uint32_t* d_err = reinterpret_cast<uint32_t*>(d_cnt + 2);
  HIP_CHECK(hipMemcpyAsync(d_ro, row_offsets, ((size_t)n_rows + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_co, col_offsets, ((size_t)n_cols + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(d_err, 0xff, 8, s));
  launch_angular_norms(R.abunds, d_ro, n_rows, d_rn, d_err, s);
  launch_angular_norms(C.abunds, d_co, n_cols, d_cn, d_err + 1, s);
  uint32_t err[2] = {kAngularNoError, kAngularNoError};
  HIP_CHECK(hipMemcpyAsync(err, d_err, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (err[0] != kAngularNoError) throw_norm("row sketch " + std::to_string(err[0]));
  if (err[1] != kAngularNoError) throw_norm("column sketch " + std::to_string(err[1]));
  launch_angular_block(R, C, count_common_dev, symmetric, out, d_cnt, dev, s);
  uint64_t cnt[2] = {0, 0};
  HIP_CHECK(hipMemcpyAsync(cnt, d_cnt, 16, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  g_angular_walked = cnt[0]; g_angular_skipped = cnt[1];
}

}  // namespace smh
