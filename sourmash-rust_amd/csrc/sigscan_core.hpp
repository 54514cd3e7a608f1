// sigscan_core.hpp -- the rules by which signature JSON text is cut into number spans and a skeleton (the
// rules are in include/sourmash_amd.h, "Signature JSON on the device", and as plain Python in tests/sigscan_restatement.py),
// as one source for the device kernels (sigscan_kernels.hip) and for a plain host build (tests/c_sigscan_host.cpp): the byte
// classes, the automaton every byte steps, the digit parse with its overflow test, and the status of a span.  No HIP header
// is needed: the qualifiers sit behind SMH_HD.  scan_serial() at the end is the serial driver of these pieces, the C++ twin
// of the restatement.
//
// The automaton.  A byte is read in one of eight states; the state it leaves behind and what it causes depend on nothing else:
//   kOut, kOutEsc        outside a string; Esc: an odd run of '\' stands directly in front of the next byte
//   kStr, kStrEsc        inside a string, likewise
//   kSpanNone            inside a span that has had no digit or comma yet (only blanks, or nothing)
//   kSpanTok             inside a span, the previous byte is a digit (a token is running)
//   kSpanComma           inside a span, the previous non-blank byte is a comma
//   kSpanGap             inside a span, the previous non-blank byte is a digit and a blank has followed it
// A text is entered in kOut.  A piece of text is therefore a map of the eight states into themselves plus counts per entering
// state, and maps compose: that is the scan's monoid.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SMH_HD __host__ __device__
#else
#define SMH_HD
#endif

#if !defined(__HIP_DEVICE_COMPILE__)
#include <string>
#include <vector>
#endif

namespace smh {
namespace sigscan {

enum State : uint32_t { kOut = 0, kOutEsc = 1, kStr = 2, kStrEsc = 3, kSpanNone = 4, kSpanTok = 5, kSpanComma = 6, kSpanGap = 7 };
constexpr uint32_t kStates = 8;

// The status of a span.  The values are ABI (include/sourmash_amd.h, SMH_SIGSPAN_*).
enum Status : uint32_t { kClosed = 0, kOpen = 1, kOverflow = 2, kBadSyntax = 3 };

// what a byte causes
enum Event : uint32_t {
  kKept = 1,        // the byte belongs to the skeleton
  kOpens = 2,       // the byte is a '[' outside a string: the next span begins behind it
  kTokStart = 4,    // the byte is the first digit of a token
  kSpanEnd = 8,     // the running span ended in front of this byte
  kBad = 16,        // the byte breaks a separator rule of its span (BAD_SYNTAX)
};

constexpr uint64_t kNoOffset = ~0ull;
constexpr uint32_t kMaxDigitsRead = 21;   // a lane reads at most 21 digits of a token, however long it is

SMH_HD inline bool is_digit(uint8_t c) { return (uint8_t)(c - '0') <= 9; }
SMH_HD inline bool is_blank(uint8_t c) { return c == ' ' || c == '\n' || c == '\t' || c == '\r'; }

struct Step { uint32_t next, events; };

SMH_HD inline Step step(uint32_t st, uint8_t c) {
  uint32_t ev = 0;
  if (st >= kSpanNone) {
    if (is_digit(c)) {
      if (st == kSpanTok) return Step{kSpanTok, 0};
      return Step{kSpanTok, kTokStart | (st == kSpanGap ? (uint32_t)kBad : 0u)};   // a token behind a digit and blanks
    }
    if (c == ',') return Step{kSpanComma, (st == kSpanTok || st == kSpanGap) ? 0u : (uint32_t)kBad};   // a comma behind no digit
    if (is_blank(c)) return Step{st == kSpanTok ? (uint32_t)kSpanGap : st, 0};
    ev = kSpanEnd;
    st = kOut;
  }
  ev |= kKept;
  if (st == kStrEsc) return Step{kStr, ev};
  if (st == kStr) return Step{c == '"' ? (uint32_t)kOut : c == '\\' ? (uint32_t)kStrEsc : (uint32_t)kStr, ev};
  // outside a string; behind an odd run of '\' a quote opens nothing
  if (c == '[') return Step{kSpanNone, ev | kOpens};
  if (c == '\\') return Step{st == kOut ? (uint32_t)kOutEsc : (uint32_t)kOut, ev};
  if (c == '"' && st == kOut) return Step{kStr, ev};
  return Step{kOut, ev};
}

// A token, read from its first digit: p[0, avail) are the bytes up to the end of the text.
enum Flaw : uint32_t { kFlawNone = 0, kFlawLeadingZero = 1, kFlawOverflow = 2 };
struct Token { uint64_t value; uint32_t flaw; };

SMH_HD inline Token parse_token(const uint8_t* p, uint64_t avail) {
  if (p[0] == '0' && avail > 1 && is_digit(p[1])) return Token{0, kFlawLeadingZero};
  uint64_t v = 0;
  bool over = false;
  for (uint32_t i = 0; i < kMaxDigitsRead && i < avail && is_digit(p[i]); i++) {
    const uint64_t d = (uint64_t)(p[i] - '0');
    if (i == kMaxDigitsRead - 1 || v > (UINT64_MAX - d) / 10) { over = true; break; }
    v = v * 10 + d;
  }
  if (over) return Token{0, kFlawOverflow};
  return Token{v, kFlawNone};
}

// the status of a span from what its bytes left behind: the lowest rule broken decides
SMH_HD inline uint32_t span_status(uint64_t bad_syntax_off, uint64_t overflow_off, uint32_t last_state, uint64_t* bad_off) {
  if (bad_syntax_off != kNoOffset) { *bad_off = bad_syntax_off; return kBadSyntax; }
  if (overflow_off != kNoOffset) { *bad_off = overflow_off; return kOverflow; }
  *bad_off = kNoOffset;
  return last_state == kSpanComma ? kOpen : kClosed;
}

// One row of the span table.  [start, end): the span's bytes; its tokens are values[first_token, first_token + n_tokens).
struct SpanRow {
  uint64_t start, end, first_token, n_tokens, bad_off;
  uint32_t status;
  uint32_t last_state;   // kSpanTok: the span's last byte is a digit (what the split-float rule asks)
};

#if !defined(__HIP_DEVICE_COMPILE__)
// The serial driver: the skeleton, the span table and the values of a text.
inline void scan_serial(const uint8_t* text, uint64_t len, std::string* skeleton, std::vector<SpanRow>* spans, std::vector<uint64_t>* values) {
  uint32_t st = kOut;
  uint64_t bad_syntax = kNoOffset, overflow = kNoOffset;
  auto close = [&](uint64_t at, uint32_t last) {
    SpanRow& r = spans->back();
    r.end = at;
    r.n_tokens = values->size() - r.first_token;
    r.last_state = last;
    r.status = span_status(bad_syntax, overflow, last, &r.bad_off);
  };
  for (uint64_t i = 0; i < len; i++) {
    const uint32_t before = st;
    const Step s = step(st, text[i]);
    st = s.next;
    if (s.events & kSpanEnd) close(i, before);
    if (s.events & kKept) skeleton->push_back((char)text[i]);
    if (s.events & kOpens) {
      spans->push_back(SpanRow{i + 1, i + 1, (uint64_t)values->size(), 0, kNoOffset, kClosed, kSpanNone});
      bad_syntax = overflow = kNoOffset;
    }
    if (s.events & kBad) { if (i < bad_syntax) bad_syntax = i; }
    if (s.events & kTokStart) {
      const Token t = parse_token(text + i, len - i);
      values->push_back(t.value);
      if (t.flaw == kFlawLeadingZero && i < bad_syntax) bad_syntax = i;
      if (t.flaw == kFlawOverflow && i < overflow) overflow = i;
    }
  }
  if (st >= kSpanNone) close(len, st);
}
#endif

}  // namespace sigscan
}  // namespace smh
