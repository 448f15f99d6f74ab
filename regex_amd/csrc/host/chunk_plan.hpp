// The unit size of the chunked scans, in one place: pure integer functions
// (no HIP, no library), shared by the host dispatch and the geometry kernel
// of the deferred long scan.
//
// The rule: the lanes in flight (CUs x lanes per CU) are shared out over the
// haystacks, a haystack's bytes over its share; a unit is at least a floor and
// an odd number of 128-byte lines.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RURE_AMD_HD __host__ __device__
#else
#define RURE_AMD_HD
#endif

namespace rure_amd {

// From this span a haystack is "long": it is cut into units instead of being
// one lane's (or one wave's) work.
constexpr uint64_t kLongSpan = 256u << 10;

// Lanes in flight per CU (16 waves: per-lane streams need latency hiding),
// and for is_match's split of medium haystacks (about one wave per CU).
constexpr uint64_t kLanesPerCu = 1024, kSplitLanesPerCu = 64;
// The floors: the long scan, the iteration, and one line (the split, and the
// suffix paths where a test forces them at any length).
constexpr uint64_t kLongFloor = 16u << 10, kIterFloor = 4096, kLineFloor = 128;

// Chunk sizes are an odd number of 128-byte lines: lanes that scan chunks in
// lockstep then read addresses with different low bits, instead of hammering
// the few HBM channels a power-of-two chunk would map them all to.
RURE_AMD_HD inline uint64_t odd_lines(uint64_t bytes) {
  uint64_t lines = (bytes + 127) / 128;
  if ((lines & 1) == 0) ++lines;
  return lines * 128;
}

// How a haystack's bytes are divided by its share of the lanes.
enum class Share { RoundUp, RoundDown };

// The unit size for `count` haystacks of `bytes` each (or, with count = 1, a
// batch of `bytes` in all) over `lanes` lanes in flight: at least `floor`,
// odd lines if `odd`.
RURE_AMD_HD inline uint64_t unit_bytes(uint64_t bytes, uint64_t count, uint64_t lanes, uint64_t floor, bool odd = true,
                                       Share share = Share::RoundUp) {
  const uint64_t per_h = (lanes + count - 1) / count;  // a haystack's share of the lanes
  uint64_t c = share == Share::RoundUp ? (bytes + per_h - 1) / per_h : bytes / per_h;
  if (c < floor) c = floor;
  return odd ? odd_lines(c) : c;
}

// is_match's split of `count` medium haystacks of `span` bytes: 0 where a unit
// would be the whole haystack (nothing to split).
RURE_AMD_HD inline uint64_t split_unit_bytes(uint64_t span, uint64_t count, uint64_t cus) {
  const uint64_t c = unit_bytes(span, count, cus * kSplitLanesPerCu, kLineFloor);
  return c < span ? c : 0;
}

}  // namespace rure_amd
