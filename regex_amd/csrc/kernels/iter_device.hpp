// Unit geometry and LDS staging shared by the chunked kernels: find_iter
// (iter_scan.hip) and the long scan (long_scan.hip).
#pragma once
#include "dfa_device.hpp"

namespace rure_amd {
namespace {  // internal linkage: included by several kernel files

struct Geo {  // unit -> (haystack, chunk) for fixed-stride batches
  uint64_t nk;      // units per haystack
  uint64_t chunk;   // bytes per unit
  uint64_t end;     // cut of the last unit (~0: the haystack end; a span's hi)
  uint32_t slots;   // speculative matches stored per unit
};

__device__ __forceinline__ void unit_bounds(const BatchDev &b, const Geo &g, uint64_t u, uint64_t *h,
                                            const uint8_t **base, uint64_t *len, uint64_t *c0, uint64_t *c1) {
  *h = u / g.nk;
  const uint64_t k = u % g.nk;
  if (b.offs) {
    const uint64_t o0 = b.offs[*h], o1 = b.offs[*h + 1];
    *base = b.hay + o0;
    *len = o1 - o0;
  } else {
    *base = b.hay + *h * b.stride;
    *len = b.length;
  }
  *c0 = b.start + k * g.chunk;
  *c1 = (k + 1 == g.nk) ? g.end : b.start + (k + 1) * g.chunk;
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
