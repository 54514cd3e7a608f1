// records.cpp -- the records of one FASTA / FASTQ text parsed on the device: the host side of
// parse_kernels.hip.  Its transient blocks are PoolBlocks, not a Workspace's: they wait for the device when they go back to the
// pool, as the blocks a Records object keeps do.
#include <string>
#include <vector>

#include "kernels.hpp"

namespace smh {

void parse_records(Records* rec, const void* text_in, bool text_on_host, uint64_t len, int format, void* stream, Device& dev) {
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = text_on_host ? dev.stream() : dev.user_stream(stream);
  std::unique_ptr<PoolBlock> up;
  if (text_on_host) up = std::make_unique<PoolBlock>(len + 64);
  if (text_on_host && len) HIP_CHECK(hipMemcpyAsync(up->ptr, text_in, len, hipMemcpyHostToDevice, s));
  const uint8_t* text = text_on_host ? up->as<uint8_t>() : static_cast<const uint8_t*>(text_in);
  if (format != kFormatAuto && format != kFormatFasta && format != kFormatFastq)
    throw Error(kMsg, "unknown sequence file format " + std::to_string(format));
  PoolBlock small(256);
  auto* totals_dev = small.as<ParseTotals>();
  if (format == kFormatAuto) {
    uint64_t first = ~0ull;
    if (len) {
      auto* first_dev = reinterpret_cast<uint64_t*>(small.as<uint8_t>() + 128);
      launch_first_content(text, len, first_dev, s);
      HIP_CHECK(hipMemcpyAsync(&first, first_dev, 8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
    if (first == ~0ull || first == '>') format = kFormatFasta;      // a text without content holds no records
    else if (first == '@') format = kFormatFastq;
    else throw Error(kMsg, "neither FASTA nor FASTQ: the first non-empty line starts with byte " + std::to_string(first));
  }
  rec->format = format;
  ParseTotals tot{0, 0, 0, 0, ~0ull};
  if (len) {
    PoolBlock ws(parse_workspace_bytes(text, len));
    const ParseTileIn first{0, 0, 0, 0, 0};
    dev.prof_begin(s);
    launch_parse_scan(format, text, len, first, ws.ptr, totals_dev, s);
    dev.prof_end("parse_scan", s);
    HIP_CHECK(hipMemcpyAsync(&tot, totals_dev, sizeof tot, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (tot.n_records > 0xffffffffull) throw Error(kMsg, "more than 2^32 - 1 records in one text");
    if (tot.total > len) throw_internal("parse: more sequence bytes than text");
    const uint64_t n = tot.n_records;
    rec->seq = std::make_unique<PoolBlock>(tot.total + 64);
    rec->names = std::make_unique<PoolBlock>(n * 16 + 16);
    PoolBlock offs(n * 8 + 8);
    auto* names = rec->names->as<uint64_t>();
    if (n) HIP_CHECK(hipMemsetAsync(names, 0, n * 16, s));
    dev.prof_begin(s);
    launch_parse_compact(format, text, len, ws.ptr, tot, rec->seq->as<uint8_t>(), offs.as<uint64_t>(), names, names + n,
                         totals_dev, s);
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
    if (format == kFormatFasta)
      throw Error(kMsg, "FASTA: sequence data in front of the first header at byte " + std::to_string(tot.err));
    throw Error(kMsg, "FASTQ: malformed record " + std::to_string(tot.err) +
                          " (no '@', no '+', quality and sequence lengths differ, or the record is cut short)");
  }
  rec->n = (uint32_t)tot.n_records;
  rec->total = tot.total;
}

void Records::name_spans(uint64_t* start_out, uint32_t* len_out) const {
  auto& dev = Device::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  std::vector<uint64_t> ends(n);
  const uint64_t* spans = names->as<uint64_t>();
  HIP_CHECK(hipMemcpyAsync(start_out, spans, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(ends.data(), spans + n, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t l = ends[i] >= start_out[i] ? ends[i] - start_out[i] : 0;
    if (l > 0xffffffffull) throw Error(kMsg, "a record name longer than 2^32 - 1 bytes");
    len_out[i] = (uint32_t)l;
  }
}

}  // namespace smh
