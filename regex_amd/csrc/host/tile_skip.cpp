// Eligibility analysis and host simulation of the tile kernel's skip rule.
#include "tile_skip.hpp"

#include <algorithm>
#include <cstring>
#include <set>
#include <unordered_set>

#include "../kernels/dfa_scan.hpp"
#include "byte_freq.h"

namespace rure_amd {

namespace {

constexpr uint32_t kMaxPos = 16;

AsciiSet from_cranges(const std::vector<CRange> &r) {
  AsciiSet s;
  for (const CRange &x : r)
    for (uint32_t c = x.lo; c <= x.hi && c < 128; ++c) s.add(c);
  return s;
}

AsciiSet from_branges(const std::vector<BRange> &r) {
  AsciiSet s;
  for (const BRange &x : r)
    for (uint32_t c = x.lo; c <= x.hi && c < 128; ++c) s.add(c);
  return s;
}

bool push(std::vector<AsciiSet> *seq, const AsciiSet &s, std::string *why) {
  if (s.empty()) { *why = "a position's class has no ASCII byte"; return false; }
  if (seq->size() >= kMaxPos) { *why = "more than 16 positions"; return false; }
  seq->push_back(s);
  return true;
}

bool items(const Expr &e, std::vector<AsciiSet> *seq, std::string *why) {
  switch (e.kind) {
    case EK::Literal:
      for (uint32_t c : e.chars)
        if (!push(seq, from_cranges(e.casei ? class_case_fold({{c, c}}) : std::vector<CRange>{{c, c}}), why))
          return false;
      return !e.chars.empty();
    case EK::LiteralBytes:
      for (uint8_t b : e.bytes)
        if (!push(seq, from_branges(e.casei ? bclass_case_fold({{b, b}}) : std::vector<BRange>{{b, b}}), why))
          return false;
      return !e.bytes.empty();
    case EK::AnyChar:
    case EK::AnyByte: return push(seq, from_branges({{0, 127}}), why);
    case EK::AnyCharNoNL:
    case EK::AnyByteNoNL: return push(seq, from_branges({{0, 9}, {11, 127}}), why);
    case EK::Class: return push(seq, from_cranges(e.casei ? class_case_fold(e.cls) : e.cls), why);
    case EK::ClassBytes: return push(seq, from_branges(e.casei ? bclass_case_fold(e.bcls) : e.bcls), why);
    case EK::Group: return e.subs.size() == 1 && items(e.subs[0], seq, why);
    case EK::Repeat: {
      if (e.rep != Rep::Range || !e.has_max || e.rmin != e.rmax || e.rmin == 0 || e.subs.size() != 1) {
        *why = "a repeat that is not a fixed count";
        return false;
      }
      std::vector<AsciiSet> one;
      if (!items(e.subs[0], &one, why)) return false;
      if ((uint64_t)one.size() * e.rmin > kMaxPos) { *why = "more than 16 positions"; return false; }
      for (uint32_t i = 0; i < e.rmin; ++i)
        for (const AsciiSet &s : one)
          if (!push(seq, s, why)) return false;
      return true;
    }
    case EK::Concat:
      for (const Expr &s : e.subs)
        if (!items(s, seq, why)) return false;
      return !e.subs.empty();
    default:
      if (why->empty()) *why = "alternation, look-around, an anchor or an empty item";
      return false;
  }
}

// [lo, hi] if the set is one byte range
bool single_range(const AsciiSet &s, uint8_t *lo, uint8_t *hi) {
  int a = -1, b = -1;
  for (int c = 0; c < 128; ++c)
    if (s.has(c)) { if (a < 0) a = c; b = c; }
  if (a < 0) return false;
  for (int c = a; c <= b; ++c)
    if (!s.has(c)) return false;
  *lo = (uint8_t)a;
  *hi = (uint8_t)b;
  return true;
}

double range_freq(uint8_t lo, uint8_t hi) {
  uint64_t all = 0, in = 0;
  for (int c = 0; c < 128; ++c) {
    all += kByteFreq[c];
    if (c >= lo && c <= hi) in += kByteFreq[c];
  }
  return (double)in / (double)all;
}

}  // namespace

bool tile_skip_sequence(const Expr &e, std::vector<AsciiSet> *seq, std::string *why) {
  seq->clear();
  why->clear();
  if (!items(e, seq, why)) {
    if (why->empty()) *why = "not a sequence of single positions";
    return false;
  }
  if (seq->size() < 2) { *why = "fewer than 2 positions"; return false; }
  return true;
}

void tile_skip_analyse(const Expr &e, const uint8_t *lds, uint32_t hot, uint32_t ustart1, TileSkip *out) {
  TileSkip k;
  auto fail = [&](const std::string &w) { k.ok = false; k.why = w; *out = k; };
  if (!tile_skip_sequence(e, &k.seq, &k.why)) return fail(k.why);
  const uint32_t m = k.m = (uint32_t)k.seq.size();
  for (uint32_t b = 0; b < 128; ++b)
    for (uint32_t j = 0; j < m; ++j)
      if (k.seq[j].has(b)) k.sa[b] |= (uint16_t)(1u << j);
  // anchors: the one or two rarest positions whose class is one byte range
  struct Cand { double p; uint32_t pos; uint8_t lo, hi; };
  std::vector<Cand> cs;
  for (uint32_t j = 0; j < m; ++j) {
    uint8_t lo, hi;
    if (single_range(k.seq[j], &lo, &hi)) cs.push_back({range_freq(lo, hi), j, lo, hi});
  }
  if (cs.empty()) return fail("no position is a single byte range");
  std::stable_sort(cs.begin(), cs.end(), [](const Cand &x, const Cand &y) { return x.p < y.p; });
  Cand a = cs[0], b = cs.size() > 1 ? cs[1] : cs[0];
  if (a.pos > b.pos) std::swap(a, b);
  // Expected candidates by the frequency table.  Past one per lane and tile
  // the regex is not eligible at all.  The kernel uses the rule only below
  // one per wave and tile (k.use): measured on the C2 text, the one-anchor
  // [0-9a-f]{8}-[0-9a-f]{4} (31 per wave-tile by the table) ran 1.97 ms under
  // the rule against 0.77 ms without, the wave waiting on its lane with the
  // most candidates, while the date regex (0.12) and (?i)id=[A-Z]{3}-\d{4}
  // (0.04) gained.
  const double rate = 128.0 * a.p * (a.pos == b.pos ? 1.0 : b.p);
  if (rate >= 1.0) return fail("the anchors are too frequent");
  k.use = 64.0 * rate < 1.0;
  k.pa = a.pos; k.pb = b.pos;
  k.a_lo = a.lo; k.a_hi = a.hi; k.b_lo = b.lo; k.b_hi = b.hi;
  // (S) one hot start state
  if (hot == 0 || hot > 63) return fail("no hot table of at most 63 rows");
  if (!ustart1) return fail("(S) the start state depends on the flags");
  k.s0 = ustart1 - 1;
  if (k.s0 >= hot) return fail("(S) the start state is not hot");
  auto step = [&](uint32_t s, uint32_t c) { return (uint32_t)lds[(size_t)s * kRow + c]; };
  // (A) product walk with the Shift-And automaton of seq: (state, D, a
  // window ended at the byte before)
  const uint32_t fin = 1u << (m - 1);
  // (keys: state << 17 | D << 1 | pc; the product of an eligible regex is a
  // few thousand triples, so a larger one is given up early)
  constexpr size_t kMaxProduct = 1 << 15;
  std::unordered_set<uint32_t> seen;
  std::vector<uint32_t> work;
  seen.insert(k.s0 << 17);
  work.push_back(k.s0 << 17);
  while (!work.empty()) {
    const uint32_t key = work.back(), s = key >> 17, D = (key >> 1) & 0xFFFFu, pc = key & 1u;
    work.pop_back();
    k.reach |= 1ull << s;
    for (uint32_t c = 0; c < 128; ++c) {
      const uint32_t D2 = ((D << 1) | 1u) & k.sa[c];
      const uint32_t comp = (D2 & fin) ? 1u : 0u;
      const uint32_t t = step(s, c);
      if (t == hot) {
        if (!comp && !pc) return fail("(A) the hot rows are left without a window of the sequence");
        continue;
      }
      const uint32_t key2 = (t << 17) | (D2 << 1) | comp;
      if (seen.insert(key2).second) {
        if (seen.size() > kMaxProduct) return fail("(A) the product automaton is too large");
        work.push_back(key2);
      }
    }
  }
  // (B) 16 ASCII bytes inside the hot rows from any reachable state end
  // where they end from s0 (which stays inside the hot rows too)
  std::set<std::pair<uint32_t, uint32_t>> level;
  for (uint32_t s = 0; s < hot; ++s)
    if ((k.reach >> s) & 1) level.insert({s, k.s0});
  for (int depth = 0; depth < 16; ++depth) {
    std::set<std::pair<uint32_t, uint32_t>> next;
    for (const auto &pq : level)
      for (uint32_t c = 0; c < 128; ++c) {
        const uint32_t p2 = step(pq.first, c);
        if (p2 == hot) continue;
        const uint32_t q2 = step(pq.second, c);
        if (q2 == hot) return fail("(B) the run from the start state leaves the hot rows first");
        next.insert({p2, q2});
      }
    level.swap(next);
  }
  for (const auto &pq : level)
    if (pq.first != pq.second) return fail("(B) the state after 16 bytes depends on the state before them");
  k.ok = true;
  *out = k;
}

void tile_skip_dev(const TileSkip &k, const uint16_t *sa, TileSkipDev *out) {
  TileSkipDev d{};
  const uint32_t rep = 0x01010101u;
  d.on = k.use ? 1 : 0; d.m = k.m; d.pa = k.pa; d.pb = k.pb; d.s0 = k.s0; d.reach = k.reach;
  d.gt_a = (0x7Fu - k.a_hi) * rep; d.lt_a = (0x7Fu + k.a_lo) * rep;
  d.gt_b = (0x7Fu - k.b_hi) * rep; d.lt_b = (0x7Fu + k.b_lo) * rep;
  d.eq_a = k.a_lo * rep; d.eq_b = k.b_lo * rep;
  d.single = k.a_lo == k.a_hi && k.b_lo == k.b_hi;
  d.sa = sa;
  *out = d;
}

namespace {

struct HostSrc {
  const uint8_t *p;
  uint4 row(int r) const {
    uint4 v;
    memcpy(&v, p + 16 * r, 16);
    return v;
  }
  uint32_t byte(uint32_t i) const { return p[i]; }
};

}  // namespace

size_t tile_skip_simulate(const TileSkip &k, const uint8_t *lds, uint32_t hot, const uint16_t *full,
                          uint32_t n_match_end, const uint8_t *hay, size_t len, uint32_t *states_skip,
                          uint32_t *states_exact, uint8_t *dirty) {
  TileSkipDev kd;
  tile_skip_dev(k, k.sa, &kd);
  kd.on = 1;
  const size_t ntiles = len / 128;
  // a find lane: a match state is walked on, the dead and quit states end it
  auto over = [&](uint32_t s) { return s >= n_match_end; };
  TileSkipLane ln{};
  uint32_t s = k.s0, x = k.s0;
  bool done = over(s);
  for (size_t t = 0; t < ntiles; ++t) {
    const uint8_t *p = hay + 128 * t;
    HostSrc src{p};
    const uint32_t f = done ? 0u : tile_skip_dirty(kd, k.sa, src, ln, s);
    const bool d = (f & kSkipDirty) != 0;
    dirty[t] = d ? 1 : 0;
    if (!done) {
      if (!d) {  // the clean path: chain16(s0, the last 16 bytes) through the hot table
        uint32_t c = k.s0;
        for (int j = 112; j < 128; ++j) c = lds[(size_t)c * kRow + p[j]];
        s = c;
        ln.prev_dirty = 0;
      } else {   // the exact walk
        bool left = s >= hot;
        for (int j = 0; j < 128 && !done; ++j) {
          s = full[(size_t)s * 256 + p[j]];
          left = left || s >= hot;
          done = over(s);
        }
        ln.prev_dirty = (f & kSkipOwn) || left;
      }
    }
    states_skip[t] = s;
    for (int j = 0; j < 128 && !over(x); ++j) x = full[(size_t)x * 256 + p[j]];
    states_exact[t] = x;
  }
  return ntiles;
}

}  // namespace rure_amd
