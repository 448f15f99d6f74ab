// The tile kernel's skip rule (dfa_scan.hip dfa_fwd_tile_kernel<.., SKIP>),
// shared with the host: host/tile_skip.cpp proves a regex eligible and
// simulates a lane with this very code (rure_amd_tile_skip_simulate).
//
// An eligible regex is, over ASCII text, one fixed sequence seq[0..m) of byte
// classes (2 <= m <= 16), and the host has checked on the packed forward DFA
// that (S) every search starts in one hot state s0, (A) a run over ASCII bytes
// from s0 leaves the hot rows only at, or one byte after, the end of a window
// of seq, and (B) after 16 ASCII bytes inside the hot rows the state depends
// on those bytes alone.  So a lane whose 128-byte tile holds no byte >= 0x80
// and ends no window of seq need not walk it: its state afterwards is
// chain16(s0, the tile's last 16 bytes).
//
// A tile is dirty for a lane for a reason of its own (kSkipOwn) when it holds
// a byte >= 0x80, when the lane's state at its start is not a hot state
// reachable from s0, or when a verified window of seq ends inside it; and it
// is dirty when the tile before it was dirty for a reason of its own or the
// lane left the hot rows in it.  Dirt does not spread further: a walked
// all-ASCII tile that began in a reachable state and stayed inside the hot
// rows ends, by (B), in chain16(s0, its last 16 bytes) like a skipped one.  Windows are found from one or two
// anchor positions whose class is a single byte range (SWAR range tests, the
// hits gathered into a bit per byte), then verified byte by byte against the
// Shift-And masks sa[b] (bit j: b is in seq[j]).  The last 16 bytes of the
// tile before are carried in registers, so a window that straddles the cut
// is verified like any other.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rure_amd {

struct TileSkipDev {
  uint32_t on;               // the regex is eligible and its anchors rare: the kernel uses the rule
  uint32_t m;                // positions of seq
  uint32_t pa, pb;           // anchor positions, pa <= pb (pa == pb: one anchor)
  // range constants of the anchors, replicated into the four bytes: for a
  // byte b < 0x80, bit 7 of b + gt is set iff b > hi, of lt - b iff b < lo
  uint32_t gt_a, lt_a, gt_b, lt_b;
  uint32_t eq_a, eq_b;       // single: the anchors' bytes, replicated
  uint32_t single;           // both anchor ranges are one byte
  uint32_t s0;               // the start state (S)
  uint64_t reach;            // bit s: hot state s is reachable from s0 over ASCII bytes inside the hot rows
  const uint16_t *sa;        // 128 Shift-And masks (device copy; staged in LDS)
};

// What a lane carries from tile to tile (all zero before the first).
struct TileSkipLane {
  uint32_t c0, c1, c2, c3;  // the last 16 bytes of the tile before
  uint32_t cflags;          // their anchor hits: a in bits 0..15, b in bits 16..31
  uint32_t prev_dirty;
};

// Bit 7 of each byte of x (the other bits clear) gathered, in byte order, into
// bits sh + 7 .. sh + 10.
__host__ __device__ __forceinline__ uint32_t skip_gather4(uint32_t x, uint32_t acc, int sh) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_udot4(x, 0x08040201u << sh, acc, false);
#else
  return acc + (((((x >> 7) * 0x00204081u) >> 21) & 0xFu) << (sh + 7));
#endif
}

// Bit 7 of the result's bytes: the byte of w (< 0x80) is NOT in the anchor's
// range.  SINGLE: the range is one byte (eq: that byte in all four), else
// [lo, hi] through gt and lt.
template <bool SINGLE>
__host__ __device__ __forceinline__ uint32_t skip_miss(uint32_t w, uint32_t eq, uint32_t gt, uint32_t lt) {
  return (SINGLE ? (w ^ eq) + 0x7F7F7F7Fu : ((w + gt) | (lt - w))) & 0x80808080u;
}

// The 16 bytes of a row NOT in the anchor's range, one bit each.
template <bool SINGLE>
__host__ __device__ __forceinline__ uint32_t skip_row_misses(const uint4 &v, uint32_t eq, uint32_t gt, uint32_t lt) {
  uint32_t lo8 = skip_gather4(skip_miss<SINGLE>(v.x, eq, gt, lt), 0, 0);
  lo8 = skip_gather4(skip_miss<SINGLE>(v.y, eq, gt, lt), lo8, 4);
  uint32_t hi8 = skip_gather4(skip_miss<SINGLE>(v.z, eq, gt, lt), 0, 0);
  hi8 = skip_gather4(skip_miss<SINGLE>(v.w, eq, gt, lt), hi8, 4);
  return (lo8 | (hi8 << 8)) >> 7;
}

__host__ __device__ __forceinline__ uint32_t skip_carry_byte(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                             uint32_t i) {
  const uint32_t w = (i & 8) ? ((i & 4) ? c3 : c2) : ((i & 4) ? c1 : c0);
  return (w >> ((i & 3) * 8)) & 0xFF;
}

constexpr uint32_t kSkipDirty = 1, kSkipOwn = 2;

// Whether the tile behind `src` is dirty for the lane whose state at its
// start is s (kSkipDirty), and whether for a reason of its own (kSkipOwn);
// updates the lane's carry (not prev_dirty: the caller sets it to kSkipOwn
// or "the lane walked the tile and left the hot rows").
// Src: row(r) = bytes [16 r, 16 r + 16) of the tile as a uint4 (r < 8),
// byte(p) = byte p of the tile (p < 128).
// SINGLE, SAME: both anchor ranges are one byte / the same range.
template <bool SINGLE, bool SAME, class Src>
__host__ __device__ __forceinline__ uint32_t tile_skip_dirty_as(const TileSkipDev &k, const uint16_t *sa, const Src &src,
                                                            TileSkipLane &ln, uint32_t s) {
  const uint32_t d = k.pb - k.pa, tail = k.m - 1 - k.pb;
  const uint32_t o0 = ln.c0, o1 = ln.c1, o2 = ln.c2, o3 = ln.c3;
  // cand[i] bit t: a window whose b anchor is byte 32 i + t - 16 of the tile
  // (bits 0..15 of cand[0]: the carried bytes) may end inside the tile
  uint32_t cand[5] = {0, 0, 0, 0, 0};
  uint32_t ha = ln.cflags << 16;  // a hits of the row before (low half) and of this row (high half)
  cand[0] = (ln.cflags >> 16) & (ha >> (16 - d)) & (0xFFFFu << (16 - tail)) & 0xFFFFu;
  uint32_t high = 0, fa = 0, fb = 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint4 v = src.row(r);
    high |= v.x | v.y | v.z | v.w;
    fa = ~skip_row_misses<SINGLE>(v, k.eq_a, k.gt_a, k.lt_a) & 0xFFFFu;
    fb = SAME ? fa : (~skip_row_misses<SINGLE>(v, k.eq_b, k.gt_b, k.lt_b) & 0xFFFFu);
    ha = (ha >> 16) | (fa << 16);
    uint32_t c = fb & (ha >> (16 - d)) & 0xFFFFu;
    if (r == 7) {
      c &= 0xFFFFu >> tail;  // a later window ends in the next tile
      ln.c0 = v.x; ln.c1 = v.y; ln.c2 = v.z; ln.c3 = v.w;
    }
    cand[(r + 1) >> 1] |= c << (16 * ((r + 1) & 1));
  }
  ln.cflags = fa | (fb << 16);
  bool dirty = (high & 0x80808080u) != 0 || s >= 64 || !((k.reach >> s) & 1);
  if (!dirty && (cand[0] | cand[1] | cand[2] | cand[3] | cand[4])) {
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      uint32_t cm = cand[i];
      while (cm && !dirty) {
        const int t = __builtin_ctz(cm);
        cm &= cm - 1;
        const int q = 32 * i + t - 16 - (int)k.pb;  // the window's first byte (>= -15)
        uint32_t ok = 1;
        for (uint32_t j = 0; j < k.m; ++j) {
          const int p = q + (int)j;
          const uint32_t b = p < 0 ? skip_carry_byte(o0, o1, o2, o3, (uint32_t)(p + 16)) : src.byte((uint32_t)(p < 0 ? 0 : p));
          ok &= (uint32_t)sa[b & 127] >> j;
        }
        dirty = ok & 1;
      }
    }
  }
  return dirty ? (kSkipDirty | kSkipOwn) : (ln.prev_dirty ? kSkipDirty : 0u);
}

template <class Src>
__host__ __device__ __forceinline__ uint32_t tile_skip_dirty(const TileSkipDev &k, const uint16_t *sa, const Src &src,
                                                         TileSkipLane &ln, uint32_t s) {
  const bool same = k.gt_a == k.gt_b && k.lt_a == k.lt_b;
  if (k.single) return same ? tile_skip_dirty_as<true, true>(k, sa, src, ln, s)
                            : tile_skip_dirty_as<true, false>(k, sa, src, ln, s);
  return same ? tile_skip_dirty_as<false, true>(k, sa, src, ln, s)
              : tile_skip_dirty_as<false, false>(k, sa, src, ln, s);
}

}  // namespace rure_amd
