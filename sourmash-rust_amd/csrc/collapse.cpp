// collapse.cpp -- ResidentIndex collapsed by groups (the rules are in include/sourmash_amd.h, "Collapsing an
// index by groups") and ResidentIndex::read.  The checks and need_g on the host; then the count pass over the parent's hash
// directory, the scan, the emit pass, the stable partition of the survivors by group, the groups' bounds among the
// partitioned keys and the child's arrays (collapse_kernels.hip, sort.hip).  4 G + 8 bytes come to the host -- the total of
// the survivors after the scan, so every allocation behind the count pass is exact, and the G + 1 bounds at the end (and
// the error word under SUM).
#include <algorithm>
#include <cmath>
#include <string>

#include "index.hpp"

namespace smh {

namespace {
[[noreturn]] void refuse(const std::string& what) { throw Error(kMsg, "collapse: " + what); }
}  // namespace

void check_collapse(uint32_t n_groups, double min_fraction, uint32_t abund) {
  if (n_groups == 0) refuse("n_groups is 0; a collapsed index holds one sketch per group");
  if (std::isnan(min_fraction)) refuse("min_fraction is NaN");
  if (min_fraction < 0.0 || min_fraction > 1.0) refuse("min_fraction is " + std::to_string(min_fraction) + "; it lies in [0, 1]");
  if (abund > kCollapseCount) refuse("unknown abundance mode " + std::to_string(abund));
}

uint32_t collapse_need(uint32_t members, uint32_t min_count, double min_fraction) {
  const double c = std::ceil(min_fraction * (double)members);   // (at most `members`: min_fraction <= 1)
  return std::max(std::max(1u, min_count), (uint32_t)c);
}

ResidentIndex::ResidentIndex(ResidentIndex& P, const uint32_t* group, uint32_t G, uint32_t min_count, double min_fraction, uint32_t abund) {
  check_collapse(G, min_fraction, abund);
  if (P.n && !group) refuse("group is NULL");
  for (uint32_t i = 0; i < P.n && !P.all_scaled; i++)
    if (!(P.params[i].num == 0 && P.params[i].max_hash != 0))
      refuse("node " + std::to_string(i) + " is not a scaled sketch (num = " + std::to_string(P.params[i].num) + ", max_hash = " +
             std::to_string(P.params[i].max_hash) + ")");
  for (uint32_t i = 1; i < P.n && !P.uniform; i++) {
    const KmerMinHash &p = P.params[i], &p0 = P.params[0];
    if (!(p.ksize == p0.ksize && p.molecule == p0.molecule && p.seed == p0.seed && p.max_hash == p0.max_hash))
      refuse("node " + std::to_string(i) + " differs from node 0 in ksize, molecule, seed or max_hash; the nodes of a collapsed index "
             "must agree in all four (downsample brings them to one max_hash)");
  }
  if (abund == kCollapseSum) {
    if (!P.has_abunds)
      refuse("the index holds a node that does not track abundances, or whose abundance vector does not match its hashes (quirks Q5/Q6)");
    if (P.wide_node != kAngularNoError) refuse("node " + std::to_string(P.wide_node) + " holds an abundance of 2^32 or more");
  }
  P.check_directory_size("collapse");
  std::vector<uint32_t> need(G, 0);   // first m_g, then need_g
  for (uint32_t v = 0; v < P.n; v++) {
    if (group[v] == kCollapseDrop) continue;
    if (group[v] >= G) refuse("group[" + std::to_string(v) + "] is " + std::to_string(group[v]) + "; there are " + std::to_string(G) + " groups");
    need[group[v]]++;
  }
  for (uint32_t g = 0; g < G; g++) need[g] = collapse_need(need[g], min_count, min_fraction);

  n = G;
  h_nums.assign(n, 0);
  // node 0's parameters (an index without nodes has none to hand down: DNA, ksize 21, seed 42, every hash admitted)
  const KmerMinHash p0 = P.n ? KmerMinHash(0, P.params[0].ksize, (Molecule)P.params[0].molecule, P.params[0].seed, P.params[0].max_hash, false)
                             : KmerMinHash(0, 21, kMoleculeDNA, 42, ~0ull, false);
  params.assign(n, p0);
  has_abunds = abund != kCollapseFlat;
  h_offsets.assign((size_t)n + 1, 0);
  {
    auto& dev = Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    uint64_t S = 0;
    const MatchDirectory dir = P.n ? P.ensure_directory("collapse", dev, s) : MatchDirectory{};
    if (dir.n_hashes) {
      if (abund == kCollapseSum && !P.angular_ready) {
        // the abundances to HBM.  The norms that call also computes are not needed here: its refusal of a norm2 that does not
        // fit 64 bits is not a refusal of the sums, and the abundances are in HBM by then
        try {
          P.angular_ensure("node", s);
        } catch (const Error& e) {
          if (e.code != kMsg || !P.angular_ready) throw;
        }
      }
      const uint32_t nh = dir.n_hashes;
      Workspace ws(s);
      uint32_t* d_group = ws.take<uint32_t>(P.n);
      uint32_t* d_need = ws.take<uint32_t>(G);
      uint32_t* d_start = ws.take<uint32_t>((size_t)G + 1);
      CollapseFold f;
      f.d = dir;
      f.group = d_group; f.need = d_need; f.n_groups = G;
      f.cnt = ws.take<uint32_t>((size_t)nh + 1);
      f.wave_list = ws.take<uint32_t>((size_t)dir.n_pairs / (kCollapseLaneMax + 1) + 1);
      f.long_list = ws.take<uint32_t>((size_t)dir.n_pairs / (kCollapseWaveMax + 1) + 1);
      f.list_count = ws.take<uint32_t>(4); f.err = f.list_count + 2;
      HIP_CHECK(hipMemcpyAsync(d_group, group, (size_t)P.n * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(d_need, need.data(), (size_t)G * 4, hipMemcpyHostToDevice, s));
      f.abund = abund;
      launch_collapse_count(f, dev, s);
      exclusive_scan_u32_dev(f.cnt, nh, f.cnt + nh, dev.scratch, s);
      uint32_t total = 0;
      HIP_CHECK(hipMemcpyAsync(&total, f.cnt + nh, 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));   // (`need` and the caller's `group` were read by the uploads)
      S = total;
      if (S) {
        const bool vals = abund != kCollapseFlat;
        uint64_t* k[2] = {ws.take<uint64_t>(S), ws.take<uint64_t>(S)};
        uint32_t* v[2] = {nullptr, nullptr};
        if (vals) { v[0] = ws.take<uint32_t>(S); v[1] = ws.take<uint32_t>(S); }
        f.key = k[0];
        f.val = v[0];
        if (abund == kCollapseSum) {
          f.hashes = P.hashes.as<uint64_t>(); f.offsets = P.offsets.as<uint64_t>(); f.abunds = P.abunds_dev.as<uint32_t>();
          HIP_CHECK(hipMemsetAsync(f.err, 0xff, 4, s));
        }
        launch_collapse_emit(f, dev, s);
        if (abund == kCollapseSum) {
          uint32_t err = kCollapseNoError;
          HIP_CHECK(hipMemcpyAsync(&err, f.err, 4, hipMemcpyDeviceToHost, s));
          HIP_CHECK(hipStreamSynchronize(s));
          if (err != kCollapseNoError)
            refuse("group " + std::to_string(err) + " holds a hash whose abundances add up to 2^32 or more; a sketch of an index keeps 32 bits "
                   "per abundance");
        }
        // survivors lie rank-major, so a stable sort by the group's bytes alone leaves every group ascending by rank
        int cur = 0;
        dev.prof_begin(s);
        if (G > 1) {
          uint32_t mask = 0;
          for (int p = 0; p < 4; p++) if (((uint64_t)(G - 1) >> (8 * p)) != 0) mask |= 1u << (4 + p);
          cur = vals ? radix_sort_u64_v32(k[0], k[1], v[0], v[1], S, dev.scratch, s, mask) : radix_sort_u64_keys(k[0], k[1], S, dev.scratch, s, mask);
        }
        // where every group starts among the partitioned keys: the child's offsets
        std::vector<uint32_t> start((size_t)G + 1);
        launch_collapse_bounds(k[cur], (uint32_t)S, G, d_start, dev, s);
        dev.prof_end("collapse_partition", s);
        hashes.ensure(S * 8 + 8);   // (the padding of pack_sketches: the compare kernels read a little past the end)
        if (vals) { abunds_dev.ensure(S * 4 + 4); abunds_resident = true; }
        launch_collapse_finish(dir.U, k[cur], v[cur], (uint32_t)S, hashes.as<uint64_t>(), vals ? abunds_dev.as<uint32_t>() : nullptr, dev, s);
        HIP_CHECK(hipMemcpyAsync(start.data(), d_start, ((size_t)G + 1) * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (start[0] != 0 || start[G] != S) throw_internal("collapse: the group bounds do not span the survivors");
        for (uint32_t g = 0; g < G; g++) { h_offsets[g + 1] = start[g + 1]; max_len = std::max(max_len, start[g + 1] - start[g]); }
      }
      HIP_CHECK(hipStreamSynchronize(s));
    }
    hashes.ensure(S * 8 + 8);
    if (has_abunds && !abunds_resident) { abunds_dev.ensure(S * 4 + 4); abunds_resident = true; }
    offsets.ensure(h_offsets.size() * 8);
    HIP_CHECK(hipMemcpyAsync(offsets.ptr, h_offsets.data(), h_offsets.size() * 8, hipMemcpyHostToDevice, s));
    nums.ensure((size_t)n * 4 + 4);
    HIP_CHECK(hipMemsetAsync(nums.ptr, 0, (size_t)n * 4 + 4, s));
    HIP_CHECK(hipStreamSynchronize(s));
    dev.count("index_collapsed");
  }
  enroll();
}

void ResidentIndex::read(uint64_t* offsets_out, uint64_t* hashes_out, uint32_t* abunds_out) {
  if (abunds_out) {
    if (!has_abunds)
      throw Error(kMsg, "read: the index holds a node that does not track abundances, or whose abundance vector does not match its hashes "
                        "(quirks Q5/Q6)");
    if (wide_node != kAngularNoError) throw Error(kMsg, "read: node " + std::to_string(wide_node) + " holds an abundance of 2^32 or more");
  }
  const uint64_t base = h_offsets.front(), total = h_offsets.back() - base;
  if (offsets_out)
    for (size_t i = 0; i < h_offsets.size(); i++) offsets_out[i] = h_offsets[i] - base;
  const bool on_device = abunds_out && h_abunds.size() != total;   // (moved to HBM by an angular call, or made there)
  if (abunds_out && !on_device && total) std::copy(h_abunds.begin(), h_abunds.end(), abunds_out);
  if (total == 0 || !(hashes_out || on_device)) return;
  auto& dev = Device::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  if (hashes_out) HIP_CHECK(hipMemcpyAsync(hashes_out, hashes.as<uint64_t>() + base, total * 8, hipMemcpyDeviceToHost, s));
  if (on_device) HIP_CHECK(hipMemcpyAsync(abunds_out, abunds_dev.as<uint32_t>() + base, total * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace smh
