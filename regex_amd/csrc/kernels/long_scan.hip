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

template <int MODE, bool PFX>
__global__ __launch_bounds__(256) void long_scan_kernel(BatchDev b, Geo g, uint64_t nunits, FwdDfaDev f, RevDfaDev r,
                                                        uint64_t *ures, unsigned long long *best) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const uint8_t *rlds = stage_tables(f, r, lds);
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < nunits; u += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t h, len, c0, c1;
    const uint8_t *base;
    unit_bounds<false>(b, g, u, &h, &base, &len, &c0, &c1);
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
    if (L.last == NONE) continue;
    if (MODE == MODE_ISMATCH) {
      ((uint8_t *)best)[h] = 1;  // best = the u8 output itself (long_scan_m)
    } else if (MODE == MODE_SHORTEST) {
      atomicMin(&best[h], (unsigned long long)L.last);  // the u64 output itself
    } else {
      uint64_t ms, me = L.last;
      if (me == b.start) ms = me;  // exec.rs:647
      else {
        const uint64_t rs = rev_scan(r, rlds, base, len, b.start, me);
        ms = rs;
        if (rs == NONE) me = NONE;  // reverse NoMatch -> the search has no match
      }
      ures[2 * u] = ms;
      ures[2 * u + 1] = me;
      atomicMin(&best[h], (unsigned long long)u);
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

}  // namespace

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
