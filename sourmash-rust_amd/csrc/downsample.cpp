// downsample.cpp -- the host half of downsampling: the rules and their refusals, one sketch cut on the host or
// in HBM, the bounds pass of a CSR with its read-back, the block form for callers that hold a CSR in device memory.  The cut
// of a resident index is ResidentIndex's second constructor (index.cpp).
#include <algorithm>
#include <string>

#include "index.hpp"

namespace smh {

namespace {
[[noreturn]] void refuse(const std::string& what) { throw Error(kMsg, "downsample: " + what); }

void check_max_hash(const KmerMinHash& src, uint64_t mx) {
  if (!(src.num == 0 && src.max_hash != 0))
    refuse("not a scaled sketch (num = " + std::to_string(src.num) + ", max_hash = " + std::to_string(src.max_hash) + ")");
  if (mx == 0) refuse("the new max_hash is 0");
  if (mx > src.max_hash)
    refuse("the new max_hash " + std::to_string(mx) + " exceeds the sketch's " + std::to_string(src.max_hash) +
           " (a sketch cannot be made finer)");
}

void copy_params(const KmerMinHash& src, KmerMinHash& out) {
  out.num = src.num; out.ksize = src.ksize; out.is_protein = src.is_protein; out.molecule = src.molecule; out.seed = src.seed;
  out.max_hash = src.max_hash; out.has_abunds = src.has_abunds;
  out.mins.w().clear(); out.abunds.clear(); out.dev.reset(); out.mirror.reset();
}

void keep_prefix(const KmerMinHash& src, size_t cut, KmerMinHash& out) {
  out.mins.w().assign(src.mins.begin(), src.mins.begin() + cut);
  if (src.has_abunds) out.abunds.assign(src.abunds.begin(), src.abunds.begin() + std::min(cut, src.abunds.size()));
}
}  // namespace

void downsample_max_hash(const KmerMinHash& src, uint64_t mx, KmerMinHash& out) {
  check_max_hash(src, mx);
  src.flush_pending();
  copy_params(src, out);
  out.max_hash = mx;
  if (!src.dev) {   // a host state is cut on the host: no device needed
    keep_prefix(src, std::upper_bound(src.mins.begin(), src.mins.end(), mx) - src.mins.begin(), out);
    return;
  }
  Device& dev = Device::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  const DeviceSketch& S = *src.dev;
  const bool counts = src.has_abunds && S.has_counts, runs = src.has_abunds && !S.has_counts;
  if (runs && !S.has_runs && S.n) throw_internal("downsample: the sketch's device state carries no abundances");
  uint64_t res[2] = {0, 0};   // the cut and the total its run starts end at
  Workspace ws(s);
  uint64_t* small = ws.take<uint64_t>(2);
  launch_downsample_cut(S.uniq.as<uint64_t>(), S.n, runs ? S.starts.as<uint32_t>() : nullptr, S.total, mx, small, s);
  HIP_CHECK(hipMemcpyAsync(res, small, 16, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  const uint64_t cut = res[0];
  if (cut == 0) return;   // (an empty sketch has no device state)
  auto ds = std::make_shared<DeviceSketch>();
  ds->uniq.ensure(cut * 8 + 8);
  HIP_CHECK(hipMemcpyAsync(ds->uniq.ptr, S.uniq.ptr, cut * 8, hipMemcpyDeviceToDevice, s));
  if (counts) {
    ds->counts.ensure(cut * 8);
    HIP_CHECK(hipMemcpyAsync(ds->counts.ptr, S.counts.ptr, cut * 8, hipMemcpyDeviceToDevice, s));
    ds->has_counts = true;
  } else if (runs) {
    ds->starts.ensure(cut * 4 + 4);
    HIP_CHECK(hipMemcpyAsync(ds->starts.ptr, S.starts.ptr, cut * 4, hipMemcpyDeviceToDevice, s));
    ds->has_runs = true;
  }
  HIP_CHECK(hipStreamSynchronize(s));
  ds->n = cut;
  ds->total = runs ? res[1] : cut;
  out.dev = ds;
}

void downsample_num(const KmerMinHash& src, uint32_t num, KmerMinHash& out) {
  if (src.max_hash != 0) refuse("downsample_num on a sketch with max_hash = " + std::to_string(src.max_hash) + " (not a num sketch)");
  if (num == 0) refuse("the new num is 0");
  if (num > src.num) refuse("the new num " + std::to_string(num) + " exceeds the sketch's " + std::to_string(src.num));
  src.materialize();   // (num sketches live on the host: this only drains what is queued)
  copy_params(src, out);
  out.num = num;
  keep_prefix(src, std::min<size_t>(num, src.mins.size()), out);
}

uint32_t downsample_bounds_host(const uint64_t* hashes_dev, const uint64_t* offsets_dev, uint32_t n, uint64_t mx,
                                std::vector<uint64_t>* new_off, Device& dev, hipStream_t s) {
  new_off->assign((size_t)n + 1, 0);
  if (n == 0) return 0;
  std::vector<uint32_t> h_kept(n);
  Workspace ws(s);
  uint32_t* kept = ws.take<uint32_t>(n);
  launch_downsample_bounds(hashes_dev, offsets_dev, n, mx, kept, dev, s);
  HIP_CHECK(hipMemcpyAsync(h_kept.data(), kept, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  uint32_t max_len = 0;
  for (uint32_t i = 0; i < n; i++) {
    (*new_off)[i + 1] = (*new_off)[i] + h_kept[i];
    max_len = std::max(max_len, h_kept[i]);
  }
  return max_len;
}

void downsample_block_dev(const uint64_t* hashes_dev, const uint32_t* abunds_dev, const uint64_t* offsets, uint32_t n, uint64_t mx,
                          uint64_t* out_hashes_dev, uint32_t* out_abunds_dev, uint64_t capacity, uint64_t* out_offsets, void* stream) {
  Device& dev = Device::get();   // first: without a device the call says so, whatever it was handed
  require(offsets, "offsets"); require(out_offsets, "out_offsets");
  if (mx == 0) refuse("the new max_hash is 0");
  for (uint32_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] >= 0xffffffffull)
      refuse("offsets must ascend, with sketches shorter than 2^32 - 1");
  const uint64_t in_total = offsets[n] - offsets[0];
  if (in_total) require(hashes_dev, "hashes_dev");
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.user_stream(stream);
  std::vector<uint64_t> new_off;
  Workspace ws(s);
  uint64_t* d_src = ws.take<uint64_t>(((size_t)n + 1) * 2);
  uint64_t* d_new = d_src + n + 1;
  HIP_CHECK(hipMemcpyAsync(d_src, offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
  downsample_bounds_host(hashes_dev, d_src, n, mx, &new_off, dev, s);
  const uint64_t total = new_off[n];
  if (total > capacity)
    refuse("the kept hashes (" + std::to_string(total) + ") exceed the capacity of the output (" + std::to_string(capacity) + ")");
  if (total) {
    require(out_hashes_dev, "out_hashes_dev");
    if (abunds_dev) require(out_abunds_dev, "out_abunds_dev");
    HIP_CHECK(hipMemcpyAsync(d_new, new_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
    launch_downsample_copy(hashes_dev, abunds_dev, d_src, d_new, n, total, out_hashes_dev, out_abunds_dev, dev, s);
  }
  HIP_CHECK(hipStreamSynchronize(s));   // (`new_off` is read by the upload)
  std::copy(new_off.begin(), new_off.end(), out_offsets);
}

}  // namespace smh
