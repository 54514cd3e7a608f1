// sigscan.hpp -- signature JSON read on the device: the handle that keeps the numbers of a text in HBM with
// the span table and the sketches' metadata on the host, and the index gathered from it (ResidentIndex's constructor in
// index.hpp).  The host side of sigscan_kernels.hip is sigscan.cpp.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "sigscan_core.hpp"

namespace smh {

// One sketch of the text: where it stands, what its signature and it say, and which spans hold its numbers.
struct SigEntry {
  uint32_t document = 0, signature = 0, sketch = 0;
  std::string name, filename, license, klass, md5sum;
  bool has_name = false, has_filename = false;
  uint32_t num = 0, ksize = 0;
  uint64_t seed = 0, max_hash = 0;
  uint8_t molecule = 0;
  bool has_abunds = false;
  uint64_t n_mins = 0, n_abunds = 0;
  uint64_t mins_span = 0, abunds_span = 0;   // rows of the span table (abunds_span: only with has_abunds)
};

struct Signatures {
  std::unique_ptr<PoolBlock> values;         // n_tokens u64, device (waits for the device when freed)
  std::vector<sigscan::SpanRow> spans;       // offsets are those of the whole text
  std::vector<SigEntry> entries;             // document order, then signature order, then sketch order
  uint64_t n_tokens = 0;
  const uint64_t* values_dev() const { return values ? values->as<uint64_t>() : nullptr; }
};

// Fills a new *sigs from a text in device memory (on the caller's `stream`) or in host memory (uploaded first, own stream).
// Document d is text[doc_offsets[d], doc_offsets[d + 1]), the documents tile the text (doc_offsets[0] == 0, doc_offsets[n_docs] == len,
// else kMsg); doc_offsets null: the whole text is one document.  Returns with the
// work complete.  The lowest document that fails decides: kSerdeError where the host loader refuses it too, kMsg for a number
// with a fraction or an exponent inside an array; the message begins with the document and the byte offset in it.
void parse_signatures(Signatures* sigs, const void* text, bool text_on_host, uint64_t len, const uint64_t* doc_offsets, uint32_t n_docs,
                      void* stream, Device& dev);
// the entries load_signatures' filter keeps (ksize 0: any; moltype null: any), as ids for the index constructor
std::vector<uint32_t> signatures_filter(const Signatures& sigs, size_t ksize, const char* moltype);

}  // namespace smh
