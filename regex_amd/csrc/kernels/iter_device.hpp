// Unit geometry and LDS staging shared by the chunked kernels: find_iter
// (iter_scan.hip) and the long scan (long_scan.hip).
#pragma once
#include "dfa_device.hpp"

namespace rure_amd {
namespace {  // internal linkage: included by several kernel files

// Unit -> (haystack, chunk).  Uniform (uoff null): every haystack has nk
// units, unit u is chunk u % nk of haystack u / nk.  Ragged (offset batches
// with a long haystack, iter_ragged_units): haystack h owns the units
// [uoff[h], uoff[h + 1]), at least one each, so uoff is strictly increasing
// and a unit's owner is unique; uoff[count] = the number of units.
struct Geo {
  uint64_t nk;      // units per haystack (uniform)
  uint64_t chunk;   // bytes per unit
  uint64_t end;     // cut of the last unit (~0: the haystack end; a span's hi)
  uint32_t slots;   // speculative matches stored per unit
  const uint64_t *uoff = nullptr;  // ragged: count + 1 exclusive sums of the units per haystack (device)
};

// The last i in [0, n] with a[i] <= x (a non-decreasing, n + 1 entries, a[0] <= x).
__device__ __forceinline__ uint64_t owner_of(const uint64_t *a, uint64_t n, uint64_t x) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (a[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// What the passes ask of a unit: its haystack and bounds (unit_bounds), and
// whether it is that haystack's first / last unit.  g.uoff is the same for
// every lane, so the ragged form costs the uniform one a single wave-uniform
// branch; its search is a short chain of loads per unit, never per byte.
__device__ __forceinline__ bool unit_head(const Geo &g, const BatchDev &b, uint64_t u) {
  return g.uoff ? g.uoff[owner_of(g.uoff, b.count, u)] == u : u % g.nk == 0;
}
__device__ __forceinline__ bool unit_tail(const Geo &g, const BatchDev &b, uint64_t u) {
  return g.uoff ? g.uoff[owner_of(g.uoff, b.count, u) + 1] == u + 1 : (u + 1) % g.nk == 0;
}

// RAGGED = false: a kernel instance that is only launched in the uniform form
// (the long scan; the per-lane Shift-And kernel: with the ragged branch
// compiled in, its uniform form took 147 VGPRs for 117 and lost a wave per
// SIMD).
template <bool RAGGED = true>
__device__ __forceinline__ void unit_bounds(const BatchDev &b, const Geo &g, uint64_t u, uint64_t *h,
                                            const uint8_t **base, uint64_t *len, uint64_t *c0, uint64_t *c1) {
  uint64_t k;
  bool tail;
  if (RAGGED && g.uoff) {
    *h = owner_of(g.uoff, b.count, u);
    k = u - g.uoff[*h];
    tail = g.uoff[*h + 1] == u + 1;
  } else {
    *h = u / g.nk;
    k = u % g.nk;
    tail = k + 1 == g.nk;
  }
  if (b.offs) {
    const uint64_t o0 = b.offs[*h], o1 = b.offs[*h + 1];
    *base = b.hay + o0;
    *len = o1 - o0;
  } else {
    *base = b.hay + *h * b.stride;
    *len = b.length;
  }
  *c0 = b.start + k * g.chunk;
  *c1 = tail ? g.end : b.start + (k + 1) * g.chunk;
}

// Dynamic LDS of the DFA kernels here: forward hot table, then the reverse
// one (offset rev_lds_offset).
__host__ __device__ inline uint32_t rev_lds_offset(uint32_t fwd_bytes) { return (fwd_bytes + 15) & ~15u; }
inline size_t iter_lds_bytes(const FwdDfaDev &f, const RevDfaDev &r) { return rev_lds_offset(f.lds_bytes) + r.lds_bytes; }

__device__ __forceinline__ const uint8_t *stage_tables(const FwdDfaDev &f, const RevDfaDev &r, uint8_t *lds) {
  for (uint32_t i = threadIdx.x * 16; i < f.lds_bytes; i += blockDim.x * 16)
    *(uint4 *)(lds + i) = *(const uint4 *)(f.lds_image + i);
  uint8_t *rl = lds + rev_lds_offset(f.lds_bytes);
  for (uint32_t i = threadIdx.x * 16; i < r.lds_bytes; i += blockDim.x * 16)
    *(uint4 *)(rl + i) = *(const uint4 *)(r.lds_image + i);
  __syncthreads();
  return r.lds_bytes ? rl : nullptr;
}

// Dynamic LDS beyond 64 KiB must be opted into per kernel (a gfx950
// workgroup may use all 160 KiB).
template <typename K>
hipError_t allow_lds(K kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// Blocks for `items` at `threads` each, at most per_cu per compute unit.
inline int grid_cap(uint64_t items, int threads, int cus, int per_cu) {
  uint64_t g = (items + threads - 1) / threads;
  uint64_t cap = (uint64_t)cus * per_cu;
  if (g > cap) g = cap;
  return (int)(g < 1 ? 1 : g);
}

}  // namespace
}  // namespace rure_amd
