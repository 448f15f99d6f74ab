// The ownership rule of the record scan (records.hip, dispatch.cpp
// run_match_records), shared with the host: rure_amd_records_units runs this
// very code over a host buffer (tests/test_records_host.py).
//
// A text of `length` bytes is cut into records by a delimiter byte: a record
// starts at 0 and after every delimiter, provided that start is < length, and
// ends before the next delimiter or at `length`.  The text is also cut into
// units of `chunk` bytes, unit u = [u * chunk, (u + 1) * chunk) (the last one
// ends at `length`), and unit u owns the records that START in it: its lane
// walks such a record to its end, however far that lies.  The first record
// start of unit u > 0 is the byte after the first delimiter at or after
// u * chunk - 1 (a delimiter on the unit's last byte starts the next unit's
// first record).  A search never crosses a delimiter, so a unit needs nothing
// from its neighbours: no speculation and no repair.
//
// The delimiter search reads whole aligned 16-byte blocks (the text is
// readable from the 16-byte block of its first byte to the one of its last,
// as every batched call's haystack is) and tests four bytes per word with
// the zero-byte word trick of dfa_device.hpp's has_byte, in its exact form:
// the positions of the hits are used here, not only whether there is one.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RURE_REC_HD __host__ __device__ __forceinline__
#else
#define RURE_REC_HD inline
#endif

namespace rure_amd {

constexpr uint64_t kRecNone = ~0ull;

RURE_REC_HD uint64_t rec_units(uint64_t length, uint64_t chunk) { return (length + chunk - 1) / chunk; }

// Bit 7 of each byte of the result: that byte of w equals the byte rep holds
// in all four (no other bit set, no false hit above a true one).
RURE_REC_HD uint32_t rec_eq_bytes(uint32_t w, uint32_t rep) {
  const uint32_t x = w ^ rep;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}

// The first delimiter of text[p..length), or `length` if there is none
// (p <= length; rep = the delimiter * 0x01010101).
RURE_REC_HD uint64_t rec_find_delim(const uint8_t *text, uint64_t length, uint64_t p, uint32_t rep) {
  while (p < length) {
    const uintptr_t a = (uintptr_t)(text + p);
    const uint32_t j = (uint32_t)(a & 15);  // the block's bytes before p do not count
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 v = *(const uint4 *)(a - j);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#else
    uint32_t w[4];
    __builtin_memcpy(w, (const void *)(a - j), 16);
#endif
    for (uint32_t k = j >> 2; k < 4; ++k) {
      uint32_t m = rec_eq_bytes(w[k], rep);
      if (4 * k < j) m &= ~0u << (8 * (j - 4 * k));
      if (m) {
        const uint64_t q = p - j + 4 * k + ((uint32_t)__builtin_ctz(m) >> 3);
        return q < length ? q : length;
      }
    }
    p += 16 - j;
  }
  return length;
}

// The first record start unit u owns, or kRecNone (u < rec_units(length, chunk)).
RURE_REC_HD uint64_t rec_first_start(const uint8_t *text, uint64_t length, uint64_t chunk, uint64_t u, uint32_t rep) {
  if (u == 0) return 0;
  const uint64_t c0 = u * chunk;
  const uint64_t c1 = length - c0 > chunk ? c0 + chunk : length;
  const uint64_t s = rec_find_delim(text, length, c0 - 1, rep) + 1;  // (length + 1 without a delimiter)
  return s < c1 ? s : kRecNone;
}

// A walk over the records unit u owns: start() is the current record's first
// byte (kRecNone: no more), end() its end; next() moves on.
struct RecWalk {
  const uint8_t *text;
  uint64_t length, c1, s, e;
  uint32_t rep;
  RURE_REC_HD RecWalk(const uint8_t *text_, uint64_t length_, uint64_t chunk, uint64_t u, uint32_t rep_)
      : text(text_), length(length_), rep(rep_) {
    const uint64_t c0 = u * chunk;
    c1 = length - c0 > chunk ? c0 + chunk : length;
    s = rec_first_start(text, length, chunk, u, rep);
    e = s == kRecNone ? 0 : rec_find_delim(text, length, s, rep);
  }
  RURE_REC_HD bool more() const { return s != kRecNone; }
  RURE_REC_HD void next() {
    s = e + 1;
    if (s >= c1) s = kRecNone;
    else e = rec_find_delim(text, length, s, rep);
  }
};

}  // namespace rure_amd
