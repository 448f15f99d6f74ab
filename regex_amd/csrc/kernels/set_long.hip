// RegexSet::matches over long haystacks for gfx950.
//
// many_matches_at (exec.rs:998-1038 -> dfa.rs:525-570) when a batch holds
// few, long haystacks.  A set DFA never drops a thread on a match (dfa.rs:
// 1557-1559), so the patterns matching text[start..] are the union, over
// every position p >= start, of the patterns a thread started at p matches,
// and that union splits over any partition of the start positions.  Unit
// [c0, c1) runs the set DFA from the start state at c0 (with the look-behind
// there) through c1 - 1, replaces the state by its stripped twin (no thread
// starts at or after c1) and runs on until that state is dead, can report
// nothing new, or the text ends; the unit that owns the end of the text also
// owns a start at `length`.  The units OR their patterns into the haystack's
// mask word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "iter_device.hpp"

namespace rure_amd {

namespace {

// How often a unit past its cut re-reads its haystack's mask word (bytes).
constexpr uint64_t kSetPoll = 4096;

// dfa_set_kernel's byte loop over text[at, end): an aligned head, 16-byte
// blocks through the hot rows, a careful step where the state leaves them or
// reports matches.  True: the walk is over (set_step1).
__device__ __forceinline__ bool set_range(uint32_t &s, uint64_t &mask, const SetDfaDev &f, const uint8_t *lds,
                                          const uint8_t *base, uint64_t at, uint64_t end) {
  bool quit = false, done = false;  // (this automaton has no quit state)
  while (!done && at < end && (((uintptr_t)(base + at)) & 15)) {
    done = set_step1(s, mask, f, lds, base[at], quit);
    ++at;
  }
  while (!done && at + 16 <= end) {
    const uint4 v = *(const uint4 *)(base + at);
    if (s < f.hot) {
      uint32_t t = s;
      t = fast4(t, v.x, lds); t = fast4(t, v.y, lds); t = fast4(t, v.z, lds); t = fast4(t, v.w, lds);
      if (t != f.hot) { s = t; at += 16; continue; }
    }
    const uint32_t words[4] = {v.x, v.y, v.z, v.w};
#pragma unroll 1
    for (int j = 0; j < 16 && !done; ++j)
      done = set_step1(s, mask, f, lds, (words[j >> 2] >> ((j & 3) * 8)) & 0xFF, quit);
    at += 16;
  }
  while (!done && at < end) {
    done = set_step1(s, mask, f, lds, base[at], quit);
    ++at;
  }
  return done;
}

__global__ __launch_bounds__(256) void set_long_kernel(BatchDev b, Geo g, uint64_t nunits, SetLongDev f,
                                                       unsigned long long *out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const SetDfaDev &d = f.d;
  for (uint32_t i = threadIdx.x * 16; i < d.lds_bytes; i += blockDim.x * 16)
    *(uint4 *)(lds + i) = *(const uint4 *)(d.lds_image + i);
  __syncthreads();
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < nunits; u += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t h, len, c0, c1;
    const uint8_t *base;
    unit_bounds<false>(b, g, u, &h, &base, &len, &c0, &c1);
    if (c0 > len) continue;  // a search from past the end: no pattern (the word stays 0)
    uint32_t s = d.start[fwd_flag_index(base, len, c0)];
    uint64_t mask = 0;
    bool done = s == d.dead;
    // the cut as long_unit's: unstripped through c1 - 1, strip, on from c1 - 1
    const bool cut = c1 > c0 && c1 - 1 <= len;
    uint64_t at = cut ? c1 - 1 : len;
    if (!done) done = set_range(s, mask, d, lds, base, c0, at);
    if (!done && cut) {
      s = f.strip[s];
      done = s == d.dead;
      while (!done) {
        // Everything this unit can still report is in reach[s]: once the
        // unit or another one has reported all of it, a lingering `.*`
        // thread need not drag the unit to the end of the haystack.  The
        // word is read here only, never in the per-byte chain (a stale value
        // only delays the exit: bits are never taken back).
        const uint64_t seen = mask | __hip_atomic_load(&out[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((f.reach[s] & ~seen) == 0) done = true;
        if (done || at >= len) break;
        // (to a 16-byte boundary, so that only the first stretch has a head)
        const uint64_t to = std::min<uint64_t>(len, at + kSetPoll - (((uintptr_t)(base + at)) & 15));
        done = set_range(s, mask, d, lds, base, at, to);
        at = to;
      }
    }
    if (!done) mask |= d.eof_mask[s];
    if (mask) atomicOr(&out[h], (unsigned long long)mask);
  }
}

}  // namespace

hipError_t launch_set_long(const BatchDev &b, const SetLongDev &f, uint64_t chunk, uint64_t *out, hipStream_t st,
                           int cus, uint64_t *units) {
  if (b.offs || !f.strip || !f.reach || chunk == 0 || b.count == 0) return hipErrorInvalidValue;
  Geo g;
  g.chunk = chunk;
  g.end = ~0ull;
  g.slots = 0;
  const uint64_t span = b.length > b.start ? b.length - b.start : 0;
  g.nk = span <= chunk ? 1 : (span + chunk - 1) / chunk;
  const uint64_t nunits = b.count * g.nk;
  *units = nunits;
  hipError_t e = hipMemsetAsync(out, 0, b.count * 8, st);
  if (e != hipSuccess) return e;
  const size_t lds = f.d.lds_bytes;
  const int per_cu = std::max<int>(1, std::min<int>(8, (int)((160u * 1024u) / std::max<size_t>(lds, 1))));
  if ((e = allow_lds(set_long_kernel, lds)) != hipSuccess) return e;
  hipLaunchKernelGGL(set_long_kernel, dim3(grid_cap(nunits, 256, cus, per_cu)), dim3(256), lds, st, b, g, nunits, f,
                     (unsigned long long *)out);
  return hipGetLastError();
}

}  // namespace rure_amd
