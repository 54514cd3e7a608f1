// sigtext.hpp -- signature JSON written on the device: the handle that owns the text of an index in HBM,
// and every node's md5.  The host side of sigtext_kernels.hip is sigtext.cpp.
#pragma once
#include <memory>
#include <vector>

#include "index.hpp"

namespace smh {

struct SigText {
  std::unique_ptr<PoolBlock> text;        // len bytes, device (waits for the device when freed)
  uint64_t len = 0;
  std::vector<uint64_t> doc_offsets;      // documents + 1, from 0: document d = text[doc_offsets[d], doc_offsets[d + 1])
  const uint8_t* text_dev() const { return text ? text->as<uint8_t>() : nullptr; }
};

// Every refusal that needs no device (kMsg, the message begins with "sigtext:"): doc_starts that do not begin at 0, end at n
// or ascend (the entry is named), an index that holds an abundance of 2^32 or more (the node is named).
void check_sigtext(const ResidentIndex& index, const uint32_t* doc_starts, uint32_t n_docs);
// Fills a new *out with the text signatures_save_buffer gives for the index's own sketches, each in a default Signature with
// names[v] / filenames[v] (a null array: every one null; a null element: JSON null), split into documents at doc_starts
// (null: one document).  Runs check_sigtext first.  Returns with the work complete; 16 bytes per node come to the host.
void index_sigtext(SigText* out, ResidentIndex& index, const char* const* names, const char* const* filenames, const uint32_t* doc_starts,
                   uint32_t n_docs, Device& dev);
// out[16 v ..): the md5 sourmash names node v by -- of str(ksize) followed by its decimal hashes
void index_md5(ResidentIndex& index, uint8_t* out, Device& dev);

}  // namespace smh
