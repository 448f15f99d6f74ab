// Batched replacen with a `$`-expanding template (gfx950).
//
// Reference: bytes::Regex::replacen's captures path (re_bytes.rs:513-535: the
// text between matches is copied, each of the first `limit` matches becomes
// the template expanded over its groups) and expand_bytes (expand.rs:50-91).
// The template is compiled on the host (capi.cpp compile_template) into
// pieces (kind, a, b): (0, offset into the literal pool, length) or
// (1, group, 0); the groups of match g are row g of the captures_iter rows
// (nfa_scan.hip caps_iter_kernel), ns u64 per row, ~0 = unset.
//
// Plan: seg[g] = (s_g - end of the previous match) + the expansion's length
// for a replaced match, else 0; S = exclusive scan of seg over nm + 1
// entries; a haystack's output = its segments + the tail after its last
// replaced match, prefix-summed into out_offsets.
//
// Write, in two kernels.  The expansions are match-driven: a wave per
// replaced match copies the literal pieces from the pool and the group pieces
// from the haystack, lanes across bytes.  The text between matches and the
// tail are input-driven: the text is cut into units of kUnit bytes, a wave
// per unit, so that no wave moves more than kUnit bytes however far apart the
// matches lie (one match at the end of a 1 GiB haystack is 262144 units).
// Nothing is written at or past the output capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dfa_scan.hpp"
#include "iter_device.hpp"  // owner_of

namespace rure_amd {

namespace {

constexpr uint64_t kUnset = ~0ull;
constexpr uint32_t kUnit = 4096;      // text bytes per wave of the gap / tail copy
constexpr uint32_t kLaneStretch = 32; // from this many stretches in a unit: a lane per stretch

__device__ __forceinline__ void hay_at(const BatchDev &bt, uint64_t h, const uint8_t **base, uint64_t *len) {
  if (bt.offs) {
    const uint64_t o0 = bt.offs[h];
    *base = bt.hay + o0;
    *len = bt.offs[h + 1] - o0;
  } else {
    *base = bt.hay + h * bt.stride;
    *len = bt.length;
  }
}

__device__ __forceinline__ uint64_t min_u64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t max_u64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// Group `grp` of a row as a byte range of its haystack: false where the group
// is unset (or the template names a group the row does not hold).
__device__ __forceinline__ bool group_span(const uint64_t *row, uint32_t ns, uint32_t grp, uint64_t len, uint64_t *gs,
                                           uint64_t *cnt) {
  if (2 * grp + 1 >= ns) return false;
  const uint64_t a = row[2 * grp], b = row[2 * grp + 1];
  if (a == kUnset || b == kUnset || b < a || b > len) return false;
  *gs = a;
  *cnt = b - a;
  return true;
}

// seg[g], one thread per match (entry nm = 0).
__global__ __launch_bounds__(256) void expand_seg_kernel(BatchDev bt, const uint64_t *moff, const uint64_t *m,
                                                         uint64_t nm, uint64_t limit, const uint64_t *rows, uint32_t ns,
                                                         ExpandTpl tp, uint64_t *seg) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g > nm) return;
  uint64_t v = 0;
  if (g < nm) {
    const uint64_t h = owner_of(moff, bt.count, g), idx = g - moff[h];
    if (idx < limit) {
      const uint8_t *base;
      uint64_t len, gs, cnt;
      hay_at(bt, h, &base, &len);
      v = m[2 * g] - (idx ? m[2 * g - 1] : 0) + tp.lit_total;
      for (uint32_t p = 0; p < tp.npieces; ++p)
        if (tp.pieces[3 * p] == 1 && group_span(rows + g * ns, ns, tp.pieces[3 * p + 1], len, &gs, &cnt)) v += cnt;
    }
  }
  seg[g] = v;
}

// Output length per haystack, one thread per haystack (entry n = 0).
__global__ __launch_bounds__(256) void expand_olen_kernel(BatchDev bt, const uint64_t *counts, const uint64_t *moff,
                                                          const uint64_t *m, uint64_t limit, const uint64_t *S,
                                                          uint64_t *olen) {
  const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h > bt.count) return;
  uint64_t v = 0;
  if (h < bt.count) {
    const uint8_t *base;
    uint64_t len;
    hay_at(bt, h, &base, &len);
    const uint64_t k = min_u64(counts[h], limit), g0 = moff[h];
    const uint64_t last = k ? m[2 * (g0 + k - 1) + 1] : 0;
    v = (S[g0 + k] - S[g0]) + (len - last);
  }
  olen[h] = v;
}

// Units of text per haystack of an offset batch (entry n = 0).
__global__ __launch_bounds__(256) void expand_units_kernel(BatchDev bt, uint64_t *units) {
  const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h > bt.count) return;
  units[h] = h < bt.count ? (bt.offs[h + 1] - bt.offs[h] + kUnit - 1) / kUnit : 0;
}

struct WriteCtx {
  BatchDev bt;
  const uint64_t *counts, *moff, *m, *S, *ooff;
  uint64_t nm, limit;
  uint8_t *out;
  uint64_t cap;
};

// The expansions: a wave per replaced match.
__global__ __launch_bounds__(256) void expand_write_kernel(WriteCtx c, const uint64_t *rows, uint32_t ns,
                                                           ExpandTpl tp) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  for (uint64_t g = wave; g < c.nm; g += nwaves) {
    const uint64_t h = owner_of(c.moff, c.bt.count, g), g0 = c.moff[h], idx = g - g0;
    if (idx >= c.limit) continue;
    const uint8_t *base;
    uint64_t len;
    hay_at(c.bt, h, &base, &len);
    uint64_t x = c.ooff[h] + (c.S[g] - c.S[g0]) + (c.m[2 * g] - (idx ? c.m[2 * g - 1] : 0));
    const uint64_t *row = rows + g * ns;
    for (uint32_t p = 0; p < tp.npieces; ++p) {
      const uint32_t kind = tp.pieces[3 * p], a = tp.pieces[3 * p + 1];
      const uint8_t *src;
      uint64_t cnt;
      if (kind == 0) {
        src = tp.lits + a;
        cnt = tp.pieces[3 * p + 2];
      } else {
        uint64_t gs;
        if (!group_span(row, ns, a, len, &gs, &cnt)) continue;
        src = base + gs;
      }
      for (uint64_t i = lane; i < cnt && x + i < c.cap; i += 64) c.out[x + i] = src[i];
      x += cnt;
    }
  }
}

// Stretch t of haystack h (t = -1: the text before its first match, else the
// text after replaced match t up to the next replaced match or the end) cut
// to the unit [lo, hi): source range and output position of its first byte.
struct Stretch {
  uint64_t lo, hi, dst;
};
__device__ __forceinline__ Stretch stretch_of(const uint64_t *mb, const uint64_t *Sb, uint64_t k, uint64_t obase,
                                              int64_t t, uint64_t lo, uint64_t hi) {
  Stretch s;
  s.hi = (uint64_t)(t + 1) < k ? min_u64(hi, mb[2 * (t + 1)]) : hi;
  if (t < 0) {
    s.lo = lo;
    s.dst = obase + lo;
  } else {
    const uint64_t e = mb[2 * t + 1];
    s.lo = max_u64(lo, e);
    s.dst = obase + (Sb[t + 1] - Sb[0]) + (s.lo - e);
  }
  return s;
}

// The text between the replaced matches and the tail: a wave per unit.
__global__ __launch_bounds__(256) void expand_text_kernel(WriteCtx c, const uint64_t *uoff, uint64_t upu,
                                                          uint64_t nunits_strided) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const uint64_t nunits = uoff ? uoff[c.bt.count] : nunits_strided;
  for (uint64_t w = wave; w < nunits; w += nwaves) {
    uint64_t h, u;
    if (uoff) {
      h = owner_of(uoff, c.bt.count, w);
      u = w - uoff[h];
    } else {
      h = w / upu;
      u = w - h * upu;
    }
    const uint8_t *base;
    uint64_t len;
    hay_at(c.bt, h, &base, &len);
    const uint64_t lo = u * kUnit, hi = min_u64(len, lo + kUnit);
    if (lo >= hi) continue;
    const uint64_t k = min_u64(c.counts[h], c.limit), g0 = c.moff[h];
    const uint64_t *mb = c.m + 2 * g0, *Sb = c.S + g0;
    const uint64_t obase = c.ooff[h];
    // ja = replaced matches starting at or before lo, jb = starting before hi
    uint64_t a = 0, b = k;
    while (a < b) {
      const uint64_t mid = (a + b) >> 1;
      if (mb[2 * mid] <= lo) a = mid + 1; else b = mid;
    }
    const uint64_t ja = a;
    b = k;
    while (a < b) {
      const uint64_t mid = (a + b) >> 1;
      if (mb[2 * mid] < hi) a = mid + 1; else b = mid;
    }
    const uint64_t jb = a;
    // stretches ja - 1 .. jb - 1 meet the unit (the earlier ones end at or before lo)
    const uint64_t nst = jb - ja + 1;
    const int64_t t0 = (int64_t)ja - 1;
    if (nst >= kLaneStretch) {
      for (uint64_t i = lane; i < nst; i += 64) {
        const Stretch s = stretch_of(mb, Sb, k, obase, t0 + (int64_t)i, lo, hi);
        for (uint64_t p = s.lo; p < s.hi; ++p) {
          const uint64_t d = s.dst + (p - s.lo);
          if (d < c.cap) c.out[d] = base[p];
        }
      }
    } else {
      for (uint64_t i = 0; i < nst; ++i) {
        const Stretch s = stretch_of(mb, Sb, k, obase, t0 + (int64_t)i, lo, hi);
        for (uint64_t p = s.lo + lane; p < s.hi; p += 64) {
          const uint64_t d = s.dst + (p - s.lo);
          if (d < c.cap) c.out[d] = base[p];
        }
      }
    }
  }
}

inline int blocks_for(uint64_t items, int cus, int per_cu) {
  const uint64_t want = (items + 255) / 256;
  return (int)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)cus * per_cu));
}

}  // namespace

hipError_t launch_expand_plan(const BatchDev &b, const uint64_t *counts, const uint64_t *moff, const uint64_t *m,
                              uint64_t nm, uint64_t limit, const uint64_t *rows, uint32_t ns, const ExpandTpl &tp,
                              uint64_t *seg, uint64_t *S, uint64_t *olen, uint64_t *out_offsets, hipStream_t st) {
  hipLaunchKernelGGL(expand_seg_kernel, dim3((unsigned)((nm + 1 + 255) / 256)), dim3(256), 0, st, b, moff, m, nm, limit,
                     rows, ns, tp, seg);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = exclusive_scan_u64(seg, S, nm + 1, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(expand_olen_kernel, dim3((unsigned)((b.count + 1 + 255) / 256)), dim3(256), 0, st, b, counts, moff,
                     m, limit, S, olen);
  e = hipGetLastError();
  if (e == hipSuccess) e = exclusive_scan_u64(olen, out_offsets, b.count + 1, st);
  return e;
}

hipError_t launch_expand_write(const BatchDev &b, const uint64_t *counts, const uint64_t *moff, const uint64_t *m,
                               uint64_t nm, uint64_t limit, const uint64_t *rows, uint32_t ns, const ExpandTpl &tp,
                               const uint64_t *S, const uint64_t *out_offsets, uint64_t *units, uint64_t *uoff,
                               uint8_t *out, uint64_t cap, hipStream_t st, int cus) {
  WriteCtx c{b, counts, moff, m, S, out_offsets, nm, limit, out, cap};
  hipError_t e = hipSuccess;
  if (nm && tp.npieces) {
    // 4 waves per block, a wave per match
    hipLaunchKernelGGL(expand_write_kernel, dim3(blocks_for(nm * 64, cus, 16)), dim3(256), 0, st, c, rows, ns, tp);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  uint64_t upu = 0, nunits = 0;
  if (b.offs) {
    hipLaunchKernelGGL(expand_units_kernel, dim3((unsigned)((b.count + 1 + 255) / 256)), dim3(256), 0, st, b, units);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = exclusive_scan_u64(units, uoff, b.count + 1, st)) != hipSuccess) return e;
    nunits = (uint64_t)cus * 16 * 4;  // the kernel reads the count from uoff; this sizes the grid
  } else {
    upu = (b.length + kUnit - 1) / kUnit;
    nunits = upu * b.count;
    if (nunits == 0) return hipSuccess;
  }
  hipLaunchKernelGGL(expand_text_kernel, dim3(blocks_for(nunits * 64, cus, 16)), dim3(256), 0, st, c,
                     b.offs ? uoff : nullptr, upu, nunits);
  return hipGetLastError();
}

}  // namespace rure_amd
