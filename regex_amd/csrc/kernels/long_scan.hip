// One search over long haystacks for gfx950.
//
// find / is_match / shortest_match (exec.rs:473-514, 382-420) when a batch
// holds few, long haystacks: every unit scans its chunk with the cut-bounded
// search (threads started in [c0, c1) only).  The leftmost-first match lives
// in the first unit whose threads reach a match state: its forward end equals
// the unrestricted search's (the earlier-started threads never match and the
// later-started ones are cut by the match or never outrank it), and the
// reverse pass runs over text[start..end] as the reference's does.  The
// earliest match end (shortest_match) is the minimum over units.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "iter_device.hpp"

namespace rure_amd {

namespace {

// Unit u: the search of text[start..len) cut to the threads started in
// [c0, c1).  A match goes to slot `slot` of best: is_match stores a byte,
// shortest_match takes the minimum end (best = the output itself for both),
// find keeps the unit's (start, end) in ures and the minimum unit in best.
template <int MODE, bool PFX>
__device__ __forceinline__ void long_unit(uint64_t start, const FwdDfaDev &f, const RevDfaDev &r, const uint8_t *lds,
                                          const uint8_t *rlds, const uint8_t *base, uint64_t len, uint64_t c0,
                                          uint64_t c1, uint64_t u, uint64_t slot, uint64_t *ures,
                                          unsigned long long *best) {
  LaneState L;
  lane_start(L, f, base, len, c0);
  if (c1 > c0 && c1 - 1 <= len) {
    fwd_range<MODE, PFX>(L, f, lds, base, c0, c1 - 1);
    if (!L.done) {
      L.s = f.strip[L.s];
      if (L.s == f.dead) L.done = true;
    }
    fwd_range<MODE>(L, f, lds, base, c1 - 1, len);
  } else {
    fwd_range<MODE, PFX>(L, f, lds, base, c0, len);
  }
  if (!L.done && f.eof[L.s]) L.last = len;
  if (L.last == NONE) return;
  if (MODE == MODE_ISMATCH) {
    ((uint8_t *)best)[slot] = 1;
  } else if (MODE == MODE_SHORTEST) {
    atomicMin(&best[slot], (unsigned long long)L.last);
  } else {
    uint64_t ms, me = L.last;
    if (me == start) ms = me;  // exec.rs:647
    else {
      const uint64_t rs = rev_scan(r, rlds, base, len, start, me);
      ms = rs;
      if (rs == NONE) me = NONE;  // reverse NoMatch -> the search has no match
    }
    ures[2 * u] = ms;
    ures[2 * u + 1] = me;
    atomicMin(&best[slot], (unsigned long long)u);
  }
}

template <int MODE, bool PFX>
__global__ __launch_bounds__(256) void long_scan_kernel(BatchDev b, Geo g, uint64_t nunits, FwdDfaDev f, RevDfaDev r,
                                                        uint64_t *ures, unsigned long long *best) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const uint8_t *rlds = stage_tables(f, r, lds);
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < nunits; u += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t h, len, c0, c1;
    const uint8_t *base;
    unit_bounds<false>(b, g, u, &h, &base, &len, &c0, &c1);
    // best = the output itself for is_match / shortest_match (long_scan_m)
    long_unit<MODE, PFX>(b.start, f, r, lds, rlds, base, len, c0, c1, u, h, ures, best);
  }
}

// ------------------------------------------------- deferred long haystacks
// Offset batches (launch_long_ragged): the lane kernels leave the haystacks
// over the threshold on a device list (dfa_device.hpp defer_long);
// nothing of it is known to the host, so the geometry is made here and the
// scan runs a fixed grid over the units the header tells.
//
// Device block (u64 words; n = the list's capacity): header, list (n), lu
// (n + 1: the exclusive sums of the units per listed haystack), best (n),
// done (n: find's units finished per listed haystack), ures (find: 2 per
// unit).  Units <= listed + total / chunk <= n + lanes, as chunk >=
// total / lanes: the block's size never depends on the offsets.
__host__ __device__ inline size_t ragged_lu_off(uint64_t n) { return kDeferList + n; }
__host__ __device__ inline size_t ragged_best_off(uint64_t n) { return ragged_lu_off(n) + n + 1; }
__host__ __device__ inline size_t ragged_done_off(uint64_t n) { return ragged_best_off(n) + n; }
__host__ __device__ inline size_t ragged_ures_off(uint64_t n) { return (ragged_done_off(n) + n + 1) & ~(size_t)1; }

__device__ __forceinline__ uint64_t ragged_span(const BatchDev &b, uint64_t h) {
  const uint64_t len = b.offs[h + 1] - b.offs[h];
  return len > b.start ? len - b.start : 0;
}

// One block: the chunk from the deferred bytes (long_batch's rule over their
// sum: at least `floor`, lanes-in-flight units in all; round: odd_lines), the
// units per listed haystack, their exclusive sums, best = none, done = 0.
// rec (pinned host memory, or null): receives the haystacks, the chunk and
// the units for rure_amd_last_long_units, so that no copy is enqueued.
__global__ __launch_bounds__(1024) void long_geometry_kernel(BatchDev b, uint64_t cap, uint64_t floor, uint32_t round,
                                                             uint64_t lanes, uint64_t *rec) {
  __shared__ uint64_t part[1024];
  unsigned long long *D = b.defer;
  const uint64_t tried = D[kDeferTried];
  const uint64_t n = tried < cap ? tried : cap;
  if (n == 0) {  // (the header's count, chunk and units stay 0)
    if (rec && threadIdx.x < 3) rec[threadIdx.x] = 0;
    return;
  }
  const uint64_t total = D[kDeferTotal];
  const uint64_t c = unit_bytes(total, 1, lanes, floor, round != 0);
  const unsigned long long *list = D + kDeferList;
  unsigned long long *lu = D + ragged_lu_off(cap), *best = D + ragged_best_off(cap);
  unsigned long long *done = D + ragged_done_off(cap);
  const uint32_t tid = threadIdx.x;
  const uint64_t per = (n + 1023) / 1024;
  const uint64_t lo = std::min<uint64_t>(n, tid * per), hi = std::min<uint64_t>(n, lo + per);
  uint64_t sum = 0;
  for (uint64_t j = lo; j < hi; ++j) sum += std::max<uint64_t>(1, (ragged_span(b, list[j]) + c - 1) / c);
  part[tid] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < 1024; off <<= 1) {
    const uint64_t v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  uint64_t at = part[tid] - sum;
  for (uint64_t j = lo; j < hi; ++j) {
    lu[j] = at;
    best[j] = ~0ull;
    done[j] = 0;
    at += std::max<uint64_t>(1, (ragged_span(b, list[j]) + c - 1) / c);
  }
  if (tid == 1023) {
    lu[n] = part[1023];
    D[kDeferCount] = n;
    D[kDeferChunk] = c;
    D[kDeferUnits] = part[1023];
    if (rec) {
      rec[0] = n;
      rec[1] = c;
      rec[2] = part[1023];
    }
  }
}

// long_scan_kernel over the listed haystacks: unit u is chunk u - lu[j] of
// haystack list[j], j its owner in lu.  is_match / shortest_match write the
// output (which the lane kernel set to "no match").  find keeps best per
// listed haystack, and the unit that finishes last of its haystack's writes
// the winner out (a count of finished units behind a fence, the
// last-block-done pattern: no finish kernel to launch).  No unit: nothing
// staged.
template <int MODE, bool PFX>
__global__ __launch_bounds__(256) void long_ragged_kernel(BatchDev b, uint64_t cap, FwdDfaDev f, RevDfaDev r,
                                                          void *out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const unsigned long long *D = b.defer;
  const uint64_t nunits = D[kDeferUnits];
  if (nunits == 0) return;
  const uint64_t n = D[kDeferCount], chunk = D[kDeferChunk];
  const uint8_t *rlds = stage_tables(f, r, lds);
  const unsigned long long *list = D + kDeferList, *lu = D + ragged_lu_off(cap);
  uint64_t *ures = (uint64_t *)(b.defer + ragged_ures_off(cap));
  unsigned long long *best = MODE == MODE_FIND ? b.defer + ragged_best_off(cap) : (unsigned long long *)out;
  unsigned long long *done = b.defer + ragged_done_off(cap);
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < nunits; u += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t j = owner_of((const uint64_t *)lu, n, u);
    const uint64_t h = list[j], k = u - lu[j];
    const uint64_t o0 = b.offs[h], len = b.offs[h + 1] - o0;
    const uint64_t c0 = b.start + k * chunk;
    const uint64_t c1 = lu[j + 1] == u + 1 ? ~0ull : c0 + chunk;
    long_unit<MODE, PFX>(b.start, f, r, lds, rlds, b.hay + o0, len, c0, c1, u, MODE == MODE_FIND ? j : h, ures, best);
    if (MODE == MODE_FIND) {
      // this unit's ures / best are visible before its count is
      __threadfence();
      const unsigned long long nk = lu[j + 1] - lu[j];
      if (atomicAdd(&done[j], 1ull) + 1 != nk) continue;
      // the last unit of haystack j: every other unit's results are written
      __threadfence();
      const unsigned long long v = atomicMin(&best[j], ~0ull);  // (an atomic read)
      uint64_t ms = NONE, me = NONE;
      if (v != ~0ull) {
        ms = __hip_atomic_load(&ures[2 * v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        me = __hip_atomic_load(&ures[2 * v + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      ((uint64_t *)out)[2 * h] = ms;
      ((uint64_t *)out)[2 * h + 1] = me;
    }
  }
}

template <int MODE>
__global__ void long_finish_kernel(uint64_t count, const uint64_t *ures, const unsigned long long *best, void *out) {
  for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < count; h += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long v = best[h];
    if (MODE == MODE_ISMATCH) {
      ((uint8_t *)out)[h] = v == 1 ? 1 : 0;
    } else if (MODE == MODE_SHORTEST) {
      ((uint64_t *)out)[h] = v;
    } else {
      ((uint64_t *)out)[2 * h] = v == ~0ull ? NONE : ures[2 * v];
      ((uint64_t *)out)[2 * h + 1] = v == ~0ull ? NONE : ures[2 * v + 1];
    }
  }
}

template <int MODE>
hipError_t long_scan_m(const BatchDev &b, const FwdDfaDev &f, const RevDfaDev &r, uint64_t chunk, void *out,
                       hipStream_t st, int cus) {
  Geo g;
  g.chunk = chunk;
  g.end = ~0ull;
  g.slots = 0;
  const uint64_t span = b.length > b.start ? b.length - b.start : 0;
  g.nk = span <= chunk ? 1 : (span + chunk - 1) / chunk;
  const uint64_t nunits = b.count * g.nk;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  // is_match / shortest_match write the output directly (a byte store / an
  // atomic min per haystack): no scratch and no finish pass — the scratch
  // cache's event per call had cost the latency-bound C1 step ~5 us
  const size_t sz_u = MODE == MODE_FIND ? nunits * 16 : 0, sz_b = MODE == MODE_FIND ? b.count * 8 : 0;
  uint8_t *buf = nullptr;
  hipError_t e = MODE == MODE_FIND ? scratch_malloc((void **)&buf, al(sz_u) + al(sz_b), st) : hipSuccess;
  if (e != hipSuccess) return e;
  uint64_t *ures = (uint64_t *)buf;
  unsigned long long *best = MODE == MODE_FIND ? (unsigned long long *)(buf + al(sz_u)) : (unsigned long long *)out;
  do {
    if (MODE == MODE_FIND)
      e = hipMemsetAsync(best, 0xFF, sz_b, st);
    else
      e = hipMemsetAsync(out, MODE == MODE_ISMATCH ? 0 : 0xFF, b.count * (MODE == MODE_ISMATCH ? 1 : 8), st);
    if (e != hipSuccess) break;
    const int per_cu = std::max<int>(1, std::min<int>(8, (int)((160u * 1024u) / std::max<size_t>(iter_lds_bytes(f, r), 1))));
    const dim3 lg(grid_cap(nunits, 256, cus, per_cu));
    // the start-state prefix skip (fwd_range<MODE, true>) for one prefix
    // first byte: measured faster there (Sherlock\s+\w+ 1.76 -> 1.54 ms per
    // GiB, >[^\n]*\n 1.10 -> 0.31) and slower with two ((?i)holmes\w*:
    // 1.46 -> 1.73 ms; profiles/r03_prefix_ab.jsonl)
    if (f.pfx_n == 1 || f.rare_on) {
      if ((e = allow_lds(long_scan_kernel<MODE, true>, iter_lds_bytes(f, r))) != hipSuccess) break;
      hipLaunchKernelGGL((long_scan_kernel<MODE, true>), lg, dim3(256), iter_lds_bytes(f, r), st, b, g, nunits, f, r,
                         ures, best);
    } else {
      if ((e = allow_lds(long_scan_kernel<MODE, false>, iter_lds_bytes(f, r))) != hipSuccess) break;
      hipLaunchKernelGGL((long_scan_kernel<MODE, false>), lg, dim3(256), iter_lds_bytes(f, r), st, b, g, nunits, f, r,
                         ures, best);
    }
    if ((e = hipGetLastError()) != hipSuccess) break;
    if (MODE == MODE_FIND) {
      hipLaunchKernelGGL(long_finish_kernel<MODE>, dim3(grid_cap(b.count, 256, cus, 4)), dim3(256), 0, st, b.count,
                         (const uint64_t *)ures, (const unsigned long long *)best, out);
      e = hipGetLastError();
    }
  } while (false);
  hipError_t e2 = buf ? scratch_free(buf, st) : hipSuccess;
  return e != hipSuccess ? e : e2;
}

template <int MODE>
hipError_t long_ragged_m(const BatchDev &b, uint64_t cap, const FwdDfaDev &f, const RevDfaDev &r, uint64_t floor,
                         bool round, uint64_t lanes, uint64_t *rec, void *out, hipStream_t st, int cus) {
  hipLaunchKernelGGL(long_geometry_kernel, dim3(1), dim3(1024), 0, st, b, cap, floor, round ? 1u : 0u, lanes, rec);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the grid of the most units there can be (the header tells how many there are)
  const size_t lds = iter_lds_bytes(f, r);
  const int per_cu = std::max<int>(1, std::min<int>(8, (int)((160u * 1024u) / std::max<size_t>(lds, 1))));
  const dim3 lg(grid_cap(cap + lanes, 256, cus, per_cu));
  if (f.pfx_n == 1 || f.rare_on) {  // as long_scan_m
    if ((e = allow_lds(long_ragged_kernel<MODE, true>, lds)) != hipSuccess) return e;
    hipLaunchKernelGGL((long_ragged_kernel<MODE, true>), lg, dim3(256), lds, st, b, cap, f, r, out);
  } else {
    if ((e = allow_lds(long_ragged_kernel<MODE, false>, lds)) != hipSuccess) return e;
    hipLaunchKernelGGL((long_ragged_kernel<MODE, false>), lg, dim3(256), lds, st, b, cap, f, r, out);
  }
  return hipGetLastError();
}

}  // namespace

size_t long_ragged_bytes(int mode, uint64_t cap, uint64_t lanes) {
  return 8 * (ragged_ures_off(cap) + (mode == MODE_FIND ? 2 * (cap + lanes) : 0));
}

// The header before the lane kernel runs: nothing asked, nothing listed.
__global__ void long_defer_init_kernel(unsigned long long *defer, uint64_t cap) {
  if (threadIdx.x < kDeferList) defer[threadIdx.x] = threadIdx.x == kDeferCap ? cap : 0;
}

hipError_t launch_long_defer_init(unsigned long long *defer, uint64_t cap, hipStream_t st) {
  hipLaunchKernelGGL(long_defer_init_kernel, dim3(1), dim3(64), 0, st, defer, cap);
  return hipGetLastError();
}

hipError_t launch_long_ragged(int mode, const BatchDev &b, uint64_t cap, const FwdDfaDev &f, const RevDfaDev &r,
                              uint64_t floor, bool round, uint64_t lanes, uint64_t *rec, void *out, hipStream_t st,
                              int cus) {
  if (!b.offs || !b.defer || !f.strip || lanes == 0 || floor == 0 || cap == 0) return hipErrorInvalidValue;
  switch (mode) {
    case MODE_FIND: return long_ragged_m<MODE_FIND>(b, cap, f, r, floor, round, lanes, rec, out, st, cus);
    case MODE_ISMATCH: return long_ragged_m<MODE_ISMATCH>(b, cap, f, r, floor, round, lanes, rec, out, st, cus);
    default: return long_ragged_m<MODE_SHORTEST>(b, cap, f, r, floor, round, lanes, rec, out, st, cus);
  }
}

hipError_t launch_long_scan(int mode, const BatchDev &b, const FwdDfaDev &f, const RevDfaDev &r, uint64_t chunk,
                            void *out, hipStream_t st, int cus) {
  note_fwd_path(RURE_AMD_PATH_LONG_SCAN);
  switch (mode) {
    case MODE_FIND: return long_scan_m<MODE_FIND>(b, f, r, chunk, out, st, cus);
    case MODE_ISMATCH: return long_scan_m<MODE_ISMATCH>(b, f, r, chunk, out, st, cus);
    default: return long_scan_m<MODE_SHORTEST>(b, f, r, chunk, out, st, cus);
  }
}

}  // namespace rure_amd
