// index.cpp -- smh::ResidentIndex: construction (from host nodes, or as the cut of a parent made on the device), parameter
// checks, the block route and its cached dictionary, the hash directory match and gather_many share, one sketch, gather.
#include "index.hpp"

#include <algorithm>
#include <memory>
#include <set>
#include <string>

namespace smh {

namespace {
// the live indexes: drop_all_dictionaries() walks them
std::set<ResidentIndex*>& registry() { static auto* r = new std::set<ResidentIndex*>(); return *r; }
std::mutex& registry_mu() { static auto* m = new std::mutex(); return *m; }
}  // namespace

ResidentIndex::ResidentIndex(const std::vector<const KmerMinHash*>& v) {
  n = (uint32_t)v.size();
  h_nums.resize(n);
  for (uint32_t i = 0; i < n; i++) {
    h_nums[i] = v[i]->num;
    KmerMinHash p(v[i]->num, v[i]->ksize, (Molecule)v[i]->molecule, v[i]->seed, v[i]->max_hash, false);
    params.push_back(p);
    const KmerMinHash& p0 = params[0];
    uniform &= p.ksize == p0.ksize && p.molecule == p0.molecule && p.max_hash == p0.max_hash && p.seed == p0.seed;
    any_num |= p.num != 0;
    all_scaled &= p.num == 0 && p.max_hash != 0;
  }
  {
    auto& dev = Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    SketchSet packed;
    Engine::get().pack_sketches(v, hashes, offsets, &packed, &max_len, &h_offsets, s);
    // (pack_sketches has brought every node to the host)
    has_abunds = true;
    for (uint32_t i = 0; i < n; i++) has_abunds &= v[i]->has_abunds && v[i]->abunds.size() == v[i]->mins.size();
    if (has_abunds) {
      h_abunds.reserve(h_offsets.back());
      for (uint32_t i = 0; i < n; i++)
        for (uint64_t a : v[i]->abunds) {
          if (a >> 32) { wide_node = std::min(wide_node, i); wide_pos.push_back(h_abunds.size()); a = 0xffffffffull; }
          h_abunds.push_back((uint32_t)a);
        }
    }
    nums.ensure((size_t)n * 4 + 4);
    if (n) HIP_CHECK(hipMemcpyAsync(nums.ptr, h_nums.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  enroll();   // last: nothing above may leave a half-built index registered
}

void ResidentIndex::enroll() {
  std::lock_guard<std::mutex> g(registry_mu());
  registry().insert(this);
}

ResidentIndex::ResidentIndex(ResidentIndex& parent, uint64_t mx) {
  uint64_t lo = 0, hi = 0;
  parent.max_hash_range(&lo, &hi);
  for (uint32_t i = 0; i < parent.n; i++)
    if (!(parent.params[i].num == 0 && parent.params[i].max_hash != 0))
      throw Error(kMsg, "downsample: node " + std::to_string(i) + " is not a scaled sketch (num = " + std::to_string(parent.params[i].num) +
                        ", max_hash = " + std::to_string(parent.params[i].max_hash) + ")");
  if (mx == 0) throw Error(kMsg, "downsample: the new max_hash is 0");
  if (parent.n && mx > lo)
    throw Error(kMsg, "downsample: the new max_hash " + std::to_string(mx) + " exceeds the smallest max_hash of a node, " +
                      std::to_string(lo) + " (a sketch cannot be made finer)");
  n = parent.n;
  h_nums.assign(n, 0);
  params = parent.params;
  tax_parent = parent.tax_parent; tax_depth = parent.tax_depth; node_taxon = parent.node_taxon;   // same nodes, same order
  for (uint32_t i = 0; i < n; i++) {
    params[i].max_hash = mx;
    const KmerMinHash &p = params[i], &p0 = params[0];
    uniform &= p.ksize == p0.ksize && p.molecule == p0.molecule && p.seed == p0.seed;
  }
  {
    auto& dev = Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    // bounds, the kept lengths to the host, the offsets, then the copy
    max_len = downsample_bounds_host(parent.hashes.as<uint64_t>(), parent.offsets.as<uint64_t>(), n, mx, &h_offsets, dev, s);
    const uint64_t total = h_offsets.back();
    hashes.ensure(total * 8 + 8);   // (the padding of pack_sketches: the compare kernels read a little past the end)
    offsets.ensure(h_offsets.size() * 8);
    HIP_CHECK(hipMemcpyAsync(offsets.ptr, h_offsets.data(), h_offsets.size() * 8, hipMemcpyHostToDevice, s));
    has_abunds = parent.has_abunds;
    // the parent's abundances live in HBM already: the copy cuts them too (angular_ensure then finds nothing to upload)
    const bool on_device = has_abunds && (parent.angular_ready || parent.abunds_resident);
    if (on_device) { abunds_dev.ensure(total * 4 + 4); abunds_resident = true; }
    launch_downsample_copy(parent.hashes.as<uint64_t>(), on_device ? parent.abunds_dev.as<uint32_t>() : nullptr,
                           parent.offsets.as<uint64_t>(), offsets.as<uint64_t>(), n, total, hashes.as<uint64_t>(),
                           on_device ? abunds_dev.as<uint32_t>() : nullptr, dev, s);
    if (has_abunds && !on_device) {
      h_abunds.reserve(total);
      for (uint32_t i = 0; i < n; i++) {
        const uint32_t* a = parent.h_abunds.data() + parent.h_offsets[i];
        h_abunds.insert(h_abunds.end(), a, a + (h_offsets[i + 1] - h_offsets[i]));
      }
    }
    // an abundance of 2^32 or more counts only where the cut kept it
    for (uint64_t p : parent.wide_pos) {
      const uint32_t i = (uint32_t)(std::upper_bound(parent.h_offsets.begin(), parent.h_offsets.end(), p) - parent.h_offsets.begin() - 1);
      const uint64_t t = p - parent.h_offsets[i];
      if (t < h_offsets[i + 1] - h_offsets[i]) { wide_node = std::min(wide_node, i); wide_pos.push_back(h_offsets[i] + t); }
    }
    nums.ensure((size_t)n * 4 + 4);
    HIP_CHECK(hipMemsetAsync(nums.ptr, 0, (size_t)n * 4 + 4, s));
    HIP_CHECK(hipStreamSynchronize(s));
    dev.count("index_downsampled");
  }
  enroll();
}

void ResidentIndex::max_hash_range(uint64_t* lo, uint64_t* hi) const {
  uint64_t a = 0, b = 0;
  for (uint32_t i = 0; i < n; i++) {
    a = i ? std::min(a, params[i].max_hash) : params[i].max_hash;
    b = std::max(b, params[i].max_hash);
  }
  if (lo) *lo = a;
  if (hi) *hi = b;
}

ResidentIndex::~ResidentIndex() {
  { std::lock_guard<std::mutex> g(registry_mu()); registry().erase(this); }
  drop_dict();
  drop_match_dir();
}

struct MatchDir {
  DeviceBuffer U, starts, owners;
  uint32_t n_hashes = 0, n_pairs = 0;
  MatchDirectory view() const { return {U.as<uint64_t>(), starts.as<uint32_t>(), owners.as<uint32_t>(), n_hashes, n_pairs}; }
};

void ResidentIndex::drop_match_dir() { delete match_dir; match_dir = nullptr; drop_lca_dev(); }   // (hash_taxon is per rank)

void ResidentIndex::check_directory_size(const char* who) const {
  const uint64_t total = h_offsets.back() - h_offsets.front();
  if (total >= (1ull << 31))
    throw Error(kMsg, std::string(who) + ": the index holds " + std::to_string(total) + " hashes; the directory takes fewer than 2^31");
}

// sorted distinct hashes of all nodes + who holds each: owner ids, a stable sort by hash, one run-length pass
MatchDirectory ResidentIndex::ensure_directory(const char* who, Device& dev, hipStream_t s) {
  if (match_dir) return match_dir->view();
  check_directory_size(who);
  const uint64_t total = h_offsets.back() - h_offsets.front();
  auto d = std::make_unique<MatchDir>();
  d->n_pairs = (uint32_t)total;
  if (total == 0) { match_dir = d.release(); return match_dir->view(); }
  Workspace ws(s);
  uint64_t* k[2] = {ws.take<uint64_t>(total), ws.take<uint64_t>(total)};
  uint32_t* v[2] = {ws.take<uint32_t>(total), ws.take<uint32_t>(total)};
  uint64_t* uq = ws.take<uint64_t>(total);
  uint32_t* st = ws.take<uint32_t>(total + 1);
  uint32_t* cnt = ws.take<uint32_t>(1);
  HIP_CHECK(hipMemcpyAsync(k[0], hashes.as<uint64_t>() + h_offsets.front(), total * 8, hipMemcpyDeviceToDevice, s));
  launch_match_owner_ids(offsets.as<uint64_t>(), n, total, v[0], dev, s);
  const int cur = radix_sort_u64_v32(k[0], k[1], v[0], v[1], total, dev.scratch, s);
  run_length_encode_u64_async(k[cur], total, uq, st, dev.scratch, s, nullptr, nullptr, cnt, nullptr);
  uint32_t nu = 0;
  HIP_CHECK(hipMemcpyAsync(&nu, cnt, 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  d->n_hashes = nu;
  d->U.ensure((size_t)nu * 8);
  d->starts.ensure((size_t)nu * 4);
  d->owners.ensure(total * 4);
  HIP_CHECK(hipMemcpyAsync(d->U.ptr, uq, (size_t)nu * 8, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d->starts.ptr, st, (size_t)nu * 4, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d->owners.ptr, v[cur], total * 4, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));
  dev.count("match_directory_built");
  match_dir = d.release();
  return match_dir->view();
}

void ResidentIndex::drop_all_dictionaries() {
  std::lock_guard<std::recursive_mutex> lock(Device::get().mutex());
  std::lock_guard<std::mutex> g(registry_mu());
  for (ResidentIndex* i : registry()) { i->drop_dict(); i->drop_match_dir(); }
}

void ResidentIndex::check_sketch(const KmerMinHash& mh, bool sketch_is_receiver) const {
  const size_t upto = uniform ? std::min<size_t>(1, params.size()) : params.size();
  for (size_t i = 0; i < upto; i++)
    if (sketch_is_receiver) mh.check_compatible(params[i]);
    else params[i].check_compatible(mh);
}

void ResidentIndex::check_index(const ResidentIndex& cols) const {
  if (n == 0 || cols.n == 0) return;
  if (uniform && cols.uniform) { params[0].check_compatible(cols.params[0]); return; }
  for (auto& r : params) for (auto& c : cols.params) r.check_compatible(c);
}

void ResidentIndex::compare_block(ResidentIndex& rows, ResidentIndex& cols, const CompareOut& o, Device& dev, hipStream_t s) {
  const size_t np = (size_t)rows.n * cols.n;
  const SketchSet R = rows.set(), C = cols.set();
  // one num for every row: pass it as the launch-wide value (lets an index against itself use symmetry)
  bool one_num = true;
  for (uint32_t v : rows.h_nums) one_num &= v == rows.h_nums[0];
  const uint32_t num = one_num ? rows.h_nums[0] : 0;
  const uint32_t* row_nums = one_num ? nullptr : rows.nums.as<uint32_t>();
  const CompareTuning tune = compare_get_tuning();
  const bool block_route = tune.route == kRouteAuto ? (np >= 4096 && rows.n >= 16) : (tune.route == kRouteComponents || tune.route == kRouteTiled);
  if (&rows == &cols && block_route && rows.h_offsets.back() > 0) {
    // an index against itself: its dictionary is built once and reused (the pre-pass is most of a sparse matrix's time)
    if (rows.dict && rows.dict_split != tune.split_frequent) rows.drop_dict();
    if (!rows.dict) {
      rows.dict = collection_begin(R.hashes, R.offsets, R.h_offsets, rows.n, 1, 0, dev, s);
      collection_finish(rows.dict, nullptr, dev, s);
      rows.dict_split = tune.split_frequent;
      dev.count("index_dictionary_built");
    }
    collection_compare(rows.dict, 0, rows.n, 0, rows.n, num, row_nums, 1, o, dev, s);
  } else {
    launch_compare_block(R, C, num, row_nums, o, dev, s, rows.max_len, cols.max_len, rows.h_offsets.back(), cols.h_offsets.back(),
                         &rows == &cols);
  }
}

void ResidentIndex::compare(ResidentIndex& cols, double* jaccard, uint64_t* common, uint64_t* size, uint64_t* count_common,
                            double* containment) {
  const size_t np = (size_t)n * cols.n;
  if (np == 0) return;
  check_index(cols);
  auto& dev = Device::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  const HostCompareOut out(Engine::get().cmp_out, np, common, size, jaccard, count_common, containment);
  compare_block(*this, cols, out.dev_out(), dev, s);
  out.fetch(s);
  HIP_CHECK(hipStreamSynchronize(s));
}

void ResidentIndex::vs_one(const KmerMinHash& q, bool q_is_row, double* jac, double* cont, uint64_t* cc) {
  auto& dev = Device::get();
  auto& E = Engine::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  q.materialize();
  const uint64_t qoff[2] = {0, (uint64_t)q.mins.size()};
  E.cmp_b.ensure(q.mins.size() * 8 + 8);
  E.cmp_ob.ensure(16);
  const HostCompareOut out(E.cmp_out, n, nullptr, nullptr, jac, cc, cont);
  if (!q.mins.empty()) HIP_CHECK(hipMemcpyAsync(E.cmp_b.ptr, q.mins.data(), q.mins.size() * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(E.cmp_ob.ptr, qoff, 16, hipMemcpyHostToDevice, s));
  const SketchSet I = set();
  const SketchSet Q{E.cmp_b.as<uint64_t>(), E.cmp_ob.as<uint64_t>(), 1, qoff};
  if (!q_is_row)
    launch_compare_block(I, Q, 0, nums.as<uint32_t>(), out.dev_out(), dev, s, max_len, (uint32_t)q.mins.size(), h_offsets.back(),
                         q.mins.size());
  else
    launch_compare_block(Q, I, q.num, nullptr, out.dev_out(), dev, s, (uint32_t)q.mins.size(), max_len, q.mins.size(),
                         h_offsets.back());
  out.fetch(s);
  HIP_CHECK(hipStreamSynchronize(s));
}

uint32_t ResidentIndex::find(const KmerMinHash& query, double threshold, bool containment, uint32_t* out_indices) {
  check_sketch(query);
  std::vector<double> val(n);
  vs_one(query, false, containment ? nullptr : val.data(), containment ? val.data() : nullptr, nullptr);
  return indices_above(val.data(), n, threshold, out_indices);
}

void ResidentIndex::most_common(const KmerMinHash& leaf, uint32_t* best_pos, uint64_t* best_common) {
  check_sketch(leaf, true);
  std::vector<uint64_t> cc(n);
  vs_one(leaf, true, nullptr, nullptr, cc.data());
  arg_max(cc.data(), n, best_pos, best_common);
}

uint32_t ResidentIndex::gather(const KmerMinHash& query, uint32_t threshold_common, GatherRow* rows, uint32_t rows_capacity,
                               uint32_t* assigned, Device& dev) {
  if (query.num != 0) throw Error(kMsg, "gather: the query is a num sketch; only scaled sketches (num == 0) can be gathered");
  if (any_num) throw Error(kMsg, "gather: the index holds a num sketch; only scaled sketches (num == 0) can be gathered");
  check_sketch(query);   // nodes that differ: one of them refuses the query
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  query.flush_pending();
  // the query where it lives: a state in HBM is read there (uniq + counts or run starts), a host state is uploaded once
  GatherQuery q;
  Workspace ws(s);
  uint64_t lq = 0;
  if (query.dev) {
    const DeviceSketch& S = *query.dev;
    lq = S.n;
    q.hashes = S.uniq.as<uint64_t>();
    if (query.has_abunds) {
      if (S.has_counts) q.counts = S.counts.as<uint64_t>();
      else if (S.has_runs) { q.starts = S.starts.as<uint32_t>(); q.total = (uint32_t)S.total; }
      else throw_internal("gather: the query's device state carries no abundances");
    }
  } else {
    lq = query.mins.size();
    if (query.has_abunds && query.abunds.size() != lq)
      throw_internal("gather: the query's abundance vector does not match its hashes (quirks Q5/Q6)");
    if (lq) {
      uint64_t* up = ws.take<uint64_t>(lq * (query.has_abunds ? 2 : 1));
      HIP_CHECK(hipMemcpyAsync(up, query.mins.data(), lq * 8, hipMemcpyHostToDevice, s));
      q.hashes = up;
      if (query.has_abunds) {
        HIP_CHECK(hipMemcpyAsync(up + lq, query.abunds.data(), lq * 8, hipMemcpyHostToDevice, s));
        q.counts = up + lq;
      }
    }
  }
  if (lq >= 0xffffffffull) throw_internal("gather: a query of 2^32 - 1 or more hashes");
  q.n = (uint32_t)lq;
  if (assigned && lq && n == 0) std::fill(assigned, assigned + lq, 0xffffffffu);
  if (n == 0 || lq == 0) return 0;
  return gather_run(set(), max_len, q, threshold_common, rows, rows_capacity, assigned, dev, s);
}

}  // namespace smh
