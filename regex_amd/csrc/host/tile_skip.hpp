// Host analysis behind the tile kernel's skip rule
// (kernels/tile_skip_device.hpp): whether a regex is, over ASCII text, one
// fixed sequence of byte classes whose windows are the only way out of the
// packed forward DFA's hot rows, and the anchors that find those windows.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "syntax.hpp"

namespace rure_amd {

struct AsciiSet {
  uint64_t w[2] = {0, 0};
  bool has(uint32_t b) const { return (w[b >> 6] >> (b & 63)) & 1; }
  void add(uint32_t b) { w[b >> 6] |= 1ull << (b & 63); }
  bool empty() const { return !(w[0] | w[1]); }
};

struct TileSkip {
  bool ok = false;             // eligible: the rule is proved for the regex
  bool use = false;            // and the anchors are rare enough for the kernel to use it
  std::string why;             // the reason it is not (diagnostics)
  uint32_t m = 0;
  std::vector<AsciiSet> seq;   // the ASCII-restricted classes, position by position
  uint32_t pa = 0, pb = 0;     // anchor positions (pa == pb: one anchor)
  uint8_t a_lo = 0, a_hi = 0, b_lo = 0, b_hi = 0;  // their byte ranges
  uint32_t s0 = 0;
  uint64_t reach = 0;
  uint16_t sa[128] = {0};      // Shift-And masks: bit j of sa[b] = b is in seq[j]
};

// The device form of an eligible regex's rule (sa: where the kernel finds the
// Shift-And masks).
struct TileSkipDev;
void tile_skip_dev(const TileSkip &k, const uint16_t *sa, TileSkipDev *out);

// The syntax check: e as seq[0..m), or false with the reason.
bool tile_skip_sequence(const Expr &e, std::vector<AsciiSet> *seq, std::string *why);

// The whole analysis.  lds: the packed hot table ((hot + 1) rows of kRow
// bytes, entry == hot: the step leaves the hot rows), ustart1: 1 + the start
// state of every reachable flag set, or 0 (PackedFwd).
void tile_skip_analyse(const Expr &e, const uint8_t *lds, uint32_t hot, uint32_t ustart1, TileSkip *out);

// One haystack walked the way a lane of the tile kernel walks it with the
// skip rule (a wave of one lane), and plainly: the states after each whole
// 128-byte tile both ways, and whether the tile was dirty.  lds, hot: the
// packed hot table, full: the whole table (nstates x 256); n_match_end: the first state id past the match
// states (FwdDfaDev).  Returns the number of tiles.
size_t tile_skip_simulate(const TileSkip &k, const uint8_t *lds, uint32_t hot, const uint16_t *full,
                          uint32_t n_match_end, const uint8_t *hay, size_t len, uint32_t *states_skip,
                          uint32_t *states_exact, uint8_t *dirty);

}  // namespace rure_amd
