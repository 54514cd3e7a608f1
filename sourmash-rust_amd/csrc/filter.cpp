// filter.cpp -- the host half of filtering a resident index and of taking a subset of its nodes (the rules are
// in include/sourmash_amd.h, "Filtering an index").  The refusals first, on the host; the operand staged where the kernels read
// it (a state in HBM in place, a host state in one upload); then the flag pass, the scan of the tile counts, the node
// boundaries, and the emit pass into the child's own arrays (filter_kernels.hip).  8 (n + 1) bytes of offsets come to the host
// -- and 4 more under OPERAND with an operand that lives in HBM, the error word of its narrowed abundances.  select() copies
// whole nodes with downsample_copy, whose contract takes any array of source starts.
#include <algorithm>
#include <string>

#include "index.hpp"

namespace smh {

namespace {
[[noreturn]] void refuse(const std::string& what) { throw Error(kMsg, "filter: " + what); }
[[noreturn]] void refuse_select(const std::string& what) { throw Error(kMsg, "select: " + what); }
constexpr uint64_t kOperandLimit = 1ull << 31;   // what the search's 32-bit window arithmetic takes
}  // namespace

void check_filter_rule(const FilterRule* rule) {
  if (!rule) refuse("rule is NULL");
  const FilterRule& r = *rule;
  if (r.operand_mode > kFilterDropIn) refuse("unknown operand mode " + std::to_string(r.operand_mode));
  if (r.abund_out > kFilterAbundOperand) refuse("unknown abundance mode " + std::to_string(r.abund_out));
  if (r.min_abund > r.max_abund)
    refuse("min_abund " + std::to_string(r.min_abund) + " exceeds max_abund " + std::to_string(r.max_abund));
  if (r.min_owners > r.max_owners)
    refuse("min_owners " + std::to_string(r.min_owners) + " exceeds max_owners " + std::to_string(r.max_owners));
  if (r.abund_out == kFilterAbundOperand && r.operand_mode != kFilterKeepIn)
    refuse("the operand's abundances can be given only to the hashes kept in it (SMH_FILTER_ABUND_OPERAND needs SMH_FILTER_KEEP_IN)");
}

void check_filter(const ResidentIndex& P, const KmerMinHash* operand, const FilterRule* rule) {
  check_filter_rule(rule);
  const FilterRule& r = *rule;
  for (uint32_t i = 0; i < P.n && !P.all_scaled; i++)
    if (!(P.params[i].num == 0 && P.params[i].max_hash != 0))
      refuse("node " + std::to_string(i) + " is not a scaled sketch (num = " + std::to_string(P.params[i].num) + ", max_hash = " +
             std::to_string(P.params[i].max_hash) + ")");
  if (r.operand_mode != kFilterOperandNone) {
    if (!operand) refuse("operand is NULL");
    if (!(operand->num == 0 && operand->max_hash != 0))
      refuse("the operand is not a scaled sketch (num = " + std::to_string(operand->num) + ", max_hash = " + std::to_string(operand->max_hash) + ")");
    P.check_sketch(*operand);   // 101-104, as every route words them
    if (r.abund_out == kFilterAbundOperand && !operand->has_abunds) refuse("the operand does not track abundances");
  }
  const bool own = r.abund_out == kFilterAbundOwn && P.has_abunds;
  if (r.abund_window() && !P.has_abunds)
    refuse("an abundance window on an index that holds a node that does not track abundances, or whose abundance vector does not match "
           "its hashes (quirks Q5/Q6)");
  if ((r.abund_window() || own) && P.wide_node != kAngularNoError)
    refuse("node " + std::to_string(P.wide_node) + " holds an abundance of 2^32 or more");
  if (r.owner_window()) P.check_directory_size("filter");
}

ResidentIndex::ResidentIndex(ResidentIndex& P, const KmerMinHash* operand, const FilterRule& rule) {
  check_filter(P, operand, &rule);
  const bool oper = rule.operand_mode != kFilterOperandNone, inflate = rule.abund_out == kFilterAbundOperand;
  const bool need_abunds = rule.abund_window() || (rule.abund_out == kFilterAbundOwn && P.has_abunds);
  n = P.n;
  h_nums.assign(n, 0);
  params = P.params;
  uniform = P.uniform;
  tax_parent = P.tax_parent; tax_depth = P.tax_depth; node_taxon = P.node_taxon;   // same nodes, same order
  has_abunds = inflate || (rule.abund_out == kFilterAbundOwn && P.has_abunds);
  h_offsets.assign((size_t)n + 1, 0);
  {
    auto& dev = Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    FilterPass f;
    f.rule = rule;
    // the operand where it lives: a state in HBM is read there, a host state goes up in one upload
    std::vector<uint64_t> stage;
    Workspace ws(s);
    if (oper) {
      operand->flush_pending();
      const uint64_t lq = operand->dev ? operand->dev->n : operand->mins.size();
      if (lq >= kOperandLimit) refuse("the operand holds " + std::to_string(lq) + " hashes; the filter takes fewer than 2^31");
      f.n_operand = (uint32_t)lq;
      if (operand->dev) {
        const DeviceSketch& S = *operand->dev;
        f.operand = S.uniq.as<uint64_t>();
        if (inflate && lq) {
          if (!S.has_counts && !S.has_runs) throw_internal("filter: the operand's device state carries no abundances");
          uint32_t* narrow = ws.take<uint32_t>(lq);
          uint32_t* err = ws.take<uint32_t>(1);
          uint32_t wide = kAngularNoError;
          HIP_CHECK(hipMemsetAsync(err, 0xff, 4, s));
          launch_angular_narrow(S.has_counts ? S.counts.as<uint64_t>() : nullptr, S.has_counts ? nullptr : S.starts.as<uint32_t>(),
                                (uint32_t)S.total, (uint32_t)lq, narrow, err, 0, s);
          HIP_CHECK(hipMemcpyAsync(&wide, err, 4, hipMemcpyDeviceToHost, s));
          HIP_CHECK(hipStreamSynchronize(s));
          if (wide != kAngularNoError) refuse("the operand holds an abundance of 2^32 or more");
          f.operand_abunds = narrow;
        }
      } else {
        if (inflate && operand->abunds.size() != lq) refuse("the operand's abundance vector does not match its hashes (quirks Q5/Q6)");
        if (inflate)
          for (uint64_t a : operand->abunds)
            if (a >> 32) refuse("the operand holds an abundance of 2^32 or more");
        if (lq) {
          const size_t words = lq + (inflate ? (lq + 1) / 2 : 0);   // [hashes | u32 abundances]
          uint64_t* up = ws.take<uint64_t>(words);
          const uint64_t* src = operand->mins.data();
          if (inflate) {
            stage.assign(words, 0);
            std::copy(operand->mins.begin(), operand->mins.end(), stage.begin());
            uint32_t* a32 = reinterpret_cast<uint32_t*>(stage.data() + lq);
            for (uint64_t k = 0; k < lq; k++) a32[k] = (uint32_t)operand->abunds[k];
            src = stage.data();
          }
          HIP_CHECK(hipMemcpyAsync(up, src, words * 8, hipMemcpyHostToDevice, s));
          f.operand = up;
          if (inflate) f.operand_abunds = reinterpret_cast<const uint32_t*>(up + lq);
        }
      }
    }
    const uint64_t base = P.h_offsets.front(), total = P.h_offsets.back() - base;
    uint64_t S = 0;
    offsets.ensure(h_offsets.size() * 8);
    if (total) {
      if (rule.owner_window()) f.dir = P.ensure_directory("filter", dev, s);
      f.hashes = P.hashes.as<uint64_t>() + base;
      f.total = total;
      // the parent's abundances: read in place when they live in HBM, else uploaded for the call
      Workspace pass(s);
      if (need_abunds) {
        if (P.angular_ready || P.abunds_resident) {
          f.abunds = P.abunds_dev.as<uint32_t>() + base;
        } else {
          uint32_t* ab = pass.take<uint32_t>(total);
          HIP_CHECK(hipMemcpyAsync(ab, P.h_abunds.data(), total * 4, hipMemcpyHostToDevice, s));
          f.abunds = ab;
        }
      }
      const uint64_t tiles = filter_tiles(total);
      f.mask = pass.take<uint64_t>(tiles * kFilterWords);
      f.tile_at = pass.take<uint64_t>(tiles + 1);
      launch_filter_flag(f, dev, s);
      launch_filter_scan(f.tile_at, tiles, s);
      launch_filter_offsets(f, P.offsets.as<uint64_t>(), n, offsets.as<uint64_t>(), dev, s);
      HIP_CHECK(hipMemcpyAsync(h_offsets.data(), offsets.ptr, h_offsets.size() * 8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      S = h_offsets.back();
      if (h_offsets.front() != 0 || S > total) throw_internal("filter: the node boundaries do not span the survivors");
      hashes.ensure(S * 8 + 8);   // (the padding of pack_sketches: the compare kernels read a little past the end)
      if (has_abunds) abunds_dev.ensure(S * 4 + 4);
      if (S) {
        launch_filter_emit(f, hashes.as<uint64_t>(), has_abunds ? abunds_dev.as<uint32_t>() : nullptr, dev, s);
        HIP_CHECK(hipStreamSynchronize(s));
      }
    } else {
      HIP_CHECK(hipMemsetAsync(offsets.ptr, 0, h_offsets.size() * 8, s));
      hashes.ensure(8);
      if (has_abunds) abunds_dev.ensure(4);
    }
    abunds_resident = has_abunds;
    for (uint32_t i = 0; i < n; i++) max_len = std::max<uint32_t>(max_len, (uint32_t)(h_offsets[i + 1] - h_offsets[i]));
    nums.ensure((size_t)n * 4 + 4);
    HIP_CHECK(hipMemsetAsync(nums.ptr, 0, (size_t)n * 4 + 4, s));
    HIP_CHECK(hipStreamSynchronize(s));
    dev.count("index_filtered");
  }
  enroll();
}

void check_index_select(const ResidentIndex& P, const uint32_t* ids, uint32_t n_ids) {
  if (n_ids && !ids) refuse_select("ids is NULL");
  if (n_ids > 0xfffffffeu) refuse_select("the ids name " + std::to_string(n_ids) + " nodes; an index takes at most 2^32 - 2");
  for (uint32_t j = 0; j < n_ids; j++)
    if (ids[j] >= P.n) refuse_select("ids[" + std::to_string(j) + "] is " + std::to_string(ids[j]) + "; the index has " + std::to_string(P.n) + " nodes");
}

ResidentIndex::ResidentIndex(ResidentIndex& P, const uint32_t* ids, uint32_t n_ids) {
  check_index_select(P, ids, n_ids);
  n = n_ids;
  h_nums.resize(n);
  h_offsets.assign((size_t)n + 1, 0);
  std::vector<uint64_t> src((size_t)n + 1, 0);   // where node j begins in the parent's arrays (the last entry is not read)
  const uint64_t pbase = P.h_offsets.front();
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t v = ids[j];
    params.push_back(P.params[v]);
    h_nums[j] = P.h_nums[v];
    src[j] = P.h_offsets[v];
    const uint64_t len = P.h_offsets[v + 1] - P.h_offsets[v];
    h_offsets[j + 1] = h_offsets[j] + len;
    max_len = std::max<uint32_t>(max_len, (uint32_t)len);
    const KmerMinHash &q = params[j], &q0 = params[0];
    uniform &= q.ksize == q0.ksize && q.molecule == q0.molecule && q.max_hash == q0.max_hash && q.seed == q0.seed;
    any_num |= q.num != 0;
    all_scaled &= q.num == 0 && q.max_hash != 0;
  }
  tax_parent = P.tax_parent; tax_depth = P.tax_depth;   // the same taxonomy, node_taxon permuted
  if (P.has_taxonomy()) {
    node_taxon.resize(n);
    for (uint32_t j = 0; j < n; j++) node_taxon[j] = P.node_taxon[ids[j]];
  }
  has_abunds = P.has_abunds;
  const uint64_t total = h_offsets.back();
  const bool on_device = has_abunds && (P.angular_ready || P.abunds_resident);
  if (has_abunds) {
    if (!on_device) h_abunds.reserve(total);
    for (uint32_t j = 0; j < n; j++) {
      const uint64_t a = P.h_offsets[ids[j]], e = P.h_offsets[ids[j] + 1];
      if (!on_device) h_abunds.insert(h_abunds.end(), P.h_abunds.begin() + (a - pbase), P.h_abunds.begin() + (e - pbase));
      // an abundance of 2^32 or more goes where its node goes
      for (auto w = std::lower_bound(P.wide_pos.begin(), P.wide_pos.end(), a); w != P.wide_pos.end() && *w < e; ++w) {
        wide_node = std::min(wide_node, j);
        wide_pos.push_back(h_offsets[j] + (*w - a));
      }
    }
  }
  {
    auto& dev = Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    hashes.ensure(total * 8 + 8);   // (the padding of pack_sketches: the compare kernels read a little past the end)
    offsets.ensure(h_offsets.size() * 8);
    nums.ensure((size_t)n * 4 + 4);
    if (on_device) { abunds_dev.ensure(total * 4 + 4); abunds_resident = true; }
    Workspace ws(s);
    uint64_t* d_src = ws.take<uint64_t>(src.size());
    HIP_CHECK(hipMemcpyAsync(d_src, src.data(), src.size() * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(offsets.ptr, h_offsets.data(), h_offsets.size() * 8, hipMemcpyHostToDevice, s));
    if (n) HIP_CHECK(hipMemcpyAsync(nums.ptr, h_nums.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    launch_downsample_copy(P.hashes.as<uint64_t>(), on_device ? P.abunds_dev.as<uint32_t>() : nullptr, d_src,
                           offsets.as<uint64_t>(), n, total, hashes.as<uint64_t>(), on_device ? abunds_dev.as<uint32_t>() : nullptr, dev, s);
    HIP_CHECK(hipStreamSynchronize(s));
    dev.count("index_selected");
  }
  enroll();
}

}  // namespace smh
