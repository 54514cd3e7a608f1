// archive.cpp -- zip collections: the host side of archive_kernels.hip.  The scan itself is
// archive_core.hpp's; here a call's ids are checked, laid out for the three kernels and launched.
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "archive_core.hpp"
#include "kernels.hpp"

namespace smh {

bool g_archive_sorted = true;

namespace {

std::string of_entry(const archive::Archive& a, uint32_t id) {
  return " (entry " + std::to_string(id) + " '" + (id < a.entries.size() ? a.entries[id].name : std::string()) + "')";
}

}  // namespace

void archive_scan(archive::Archive* a, const uint8_t* data, uint64_t len) {
  std::string msg;
  if (!archive::scan(a, data, len, &msg)) throw Error(kMsg, msg);
}

void archive_inflate_dev(const archive::Archive& a, const uint8_t* data_dev, uint64_t len, const uint32_t* ids, const uint64_t* out_offs,
                         uint64_t n_ids, uint8_t* out_dev, uint64_t out_cap, bool verify, uint8_t* status_out, hipStream_t s, Device& dev) {
  if (len != a.len) throw Error(kMsg, "archive: the entries were scanned from " + std::to_string(a.len) + " bytes, not " + std::to_string(len));
  if (n_ids == 0) return;
  require(ids, "ids"); require(out_offs, "out_offs");
  // everything is refused before anything is launched: the ids, the slices against the capacity and against each other
  std::vector<ArchiveMember> members(n_ids);
  uint64_t text = 0;
  for (uint64_t i = 0; i < n_ids; i++) {
    const uint32_t id = ids[i];
    if (id >= a.entries.size()) throw Error(kMsg, "archive: entry " + std::to_string(id) + " of " + std::to_string(a.entries.size()));
    const archive::Entry& e = a.entries[id];
    if (!e.device_ok) throw Error(kMsg, "archive: not for the device: " + e.reason + of_entry(a, id));
    if (out_offs[i] > out_cap || e.text_size > out_cap - out_offs[i])
      throw Error(kMsg, "archive: the slice at " + std::to_string(out_offs[i]) + " of " + std::to_string(e.text_size) + " bytes leaves the output of " +
                            std::to_string(out_cap) + of_entry(a, id));
    ArchiveMember& m = members[i];
    m.src_off = e.payload_off; m.src_len = (uint32_t)e.payload_len;
    m.out_off = out_offs[i]; m.size = e.text_size; m.crc = e.text_crc;
    m.inflated = (e.kind == archive::kDeflate || e.kind == archive::kGzip) ? 1 : 0;
    text += e.text_size;
  }
  {
    std::vector<uint64_t> by_off;
    by_off.reserve(n_ids);
    for (uint64_t i = 0; i < n_ids; i++) if (members[i].size) by_off.push_back(i);
    std::sort(by_off.begin(), by_off.end(), [&](uint64_t x, uint64_t y) { return members[x].out_off < members[y].out_off; });
    for (size_t k = 1; k < by_off.size(); k++) {
      const ArchiveMember& p = members[by_off[k - 1]];
      if (p.out_off + p.size > members[by_off[k]].out_off)   // (both ends are inside out_cap: no wrap)
        throw Error(kMsg, "archive: the slices of ids " + std::to_string(std::min(by_off[k - 1], by_off[k])) + " and " +
                              std::to_string(std::max(by_off[k - 1], by_off[k])) + " overlap" + of_entry(a, ids[by_off[k]]));
    }
  }
  require(data_dev, "data_dev");
  if (text) require(out_dev, "out_dev");
  // the inflated members, longest payload first (ties in id order); the chunk prefix -- without verification only the
  // stored members have chunks, which are their copies
  std::vector<uint64_t> order;
  std::vector<uint64_t> prefix(n_ids + 1, 0);
  for (uint64_t i = 0; i < n_ids; i++) {
    if (members[i].inflated) order.push_back(i);
    prefix[i + 1] = prefix[i] + ((verify || !members[i].inflated) ? archive::chunks_of(members[i].size) : 0);
  }
  if (g_archive_sorted)
    std::stable_sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) { return members[x].src_len > members[y].src_len; });
  const uint64_t n_chunks = prefix[n_ids];

  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  Workspace ws(s);
  ArchiveMember* members_dev = ws.take<ArchiveMember>(n_ids);
  uint64_t* order_dev = ws.take<uint64_t>(order.size());
  uint64_t* prefix_dev = ws.take<uint64_t>(n_ids + 1);
  uint32_t* terms = ws.take<uint32_t>(n_chunks);
  uint8_t* status = ws.take<uint8_t>(n_ids);
  // words[0]: the error word; words[1]: the ticket.  Every block of this call has been taken -- and, under the test pattern
  // of smh_set_pool_fill, filled and waited for -- before the zeroing below is queued, and none goes back before the
  // stream has been waited for: the fill cannot reach the ticket between its zeroing and the kernel's last draw.
  unsigned long long* words = ws.take<unsigned long long>(2);
  unsigned long long low = ~0ull;
  HIP_CHECK(hipMemcpyAsync(members_dev, members.data(), n_ids * sizeof(ArchiveMember), hipMemcpyHostToDevice, s));
  if (!order.empty()) HIP_CHECK(hipMemcpyAsync(order_dev, order.data(), order.size() * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(prefix_dev, prefix.data(), (n_ids + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(status, 0, n_ids, s));
  HIP_CHECK(hipMemsetAsync(words, 0xff, 8, s));
  HIP_CHECK(hipMemsetAsync(words + 1, 0, 8, s));
  dev.prof_begin(s);
  launch_inflate_queue(data_dev, members_dev, order_dev, order.size(), words + 1, out_dev, status, words, dev, s);
  dev.prof_end("archive_inflate", s);
  dev.prof_begin(s);
  launch_archive_chunks(data_dev, members_dev, prefix_dev, n_ids, n_chunks, out_dev, terms, verify, dev, s);
  dev.prof_end("archive_chunks", s);
  if (verify) {
    dev.prof_begin(s);
    launch_archive_crc(members_dev, prefix_dev, n_ids, terms, status, words, dev, s);
    dev.prof_end("archive_crc", s);
  }
  HIP_CHECK(hipMemcpyAsync(&low, words, 8, hipMemcpyDeviceToHost, s));
  if (status_out) HIP_CHECK(hipMemcpyAsync(status_out, status, n_ids, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (low != ~0ull) {
    const uint64_t pos = low >> 8;
    throw Error(kMsg, std::string("archive: ") + inflate_reason_text((uint32_t)(low & 0xff)) + of_entry(a, pos < n_ids ? ids[pos] : ~0u));
  }
}

void archive_inflate_host(const archive::Archive& a, const uint8_t* data, uint64_t len, const uint32_t* ids, const uint64_t* out_offs,
                          uint64_t n_ids, uint8_t* out_dev, uint64_t out_cap, bool verify, uint8_t* status_out, Device& dev) {
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  Workspace ws(s);
  uint8_t* data_dev = ws.take<uint8_t>(len);
  if (len) HIP_CHECK(hipMemcpyAsync(data_dev, data, len, hipMemcpyHostToDevice, s));
  archive_inflate_dev(a, data_dev, len, ids, out_offs, n_ids, out_dev, out_cap, verify, status_out, s, dev);
}

}  // namespace smh
