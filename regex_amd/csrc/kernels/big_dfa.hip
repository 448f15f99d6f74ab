// Batched DFA scans of automata too large for the u16 tables (BigDfaDev):
// u32 next states in column form, the hot rows in LDS, the rest read from
// global memory (L2 / Infinity Cache resident for tables of tens of MB).
//
// Reference semantics restated (src/dfa.rs): exec_at (576-764, one-byte
// delayed match flag, EOF step), exec_at_reverse (768-866, longest match
// -> leftmost start), start_flags (1415-1464); dispatch find_dfa_forward
// (exec.rs:632-662) and shortest_dfa (exec.rs:692-694).  The reference
// builds such automata lazily in a bounded cache; the host materialises them
// eagerly (dfa_build.cpp, column form) so a lane only reads tables.  Past
// that budget too, rows are built on demand between rounds of
// lazy_dfa_kernel (a regex), lazy_long_kernel (its few long haystacks, cut
// into units), lazy_iter_kernel (its find_iter; lazy_iter_long_kernel over
// few long haystacks), lazy_set_kernel (a
// RegexSet's matches) or lazy_set_long_kernel (its few long haystacks).
//
// Execution: one lane per haystack (lazy_long_kernel: per unit).  A 16-byte chunk's columns come from the
// LDS column map first (independent of the state), then the dependent chain
// is one table read per byte: LDS for hot states, global otherwise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfa_device.hpp"
#include "iter_device.hpp"

namespace rure_amd {
namespace {

constexpr uint32_t kBigLdsBytes = 64 * 1024;  // hot rows (u32)

__device__ __forceinline__ uint32_t big_next(const BigDfaDev &f, const uint32_t *hot_rows, uint32_t s, uint32_t c) {
  return s < f.hot ? hot_rows[s * f.ncol + c] : f.trans[(size_t)s * f.ncol + c];
}

// Reverse scan over text[lo..me) (rev_scan with the big reverse DFA).
__device__ uint64_t big_rev_scan(const BigDfaDev &r, const uint8_t *base, uint64_t len, uint64_t lo, uint64_t me) {
  uint32_t s = r.ustart1 ? r.ustart1 - 1 : r.start[rev_flag_index(base, lo, len, me)];
  if (s == r.dead) return NONE;
  uint64_t rs = NONE;
  for (uint64_t a = me; a > lo;) {
    --a;
    s = r.trans[(size_t)s * r.ncol + r.colmap[base[a]]];
    if (s >= r.n_normal) {
      if (s < r.n_match_end) rs = a + 1;
      else return rs;  // dead (no quit state in the big automata)
    }
  }
  if (r.eof[s]) rs = lo;
  return rs;
}

template <int MODE, bool STRIDED>
__global__ __launch_bounds__(1024) void big_dfa_kernel(BatchDev bt, BigDfaDev f, BigDfaDev r, void *out) {
  __shared__ __attribute__((aligned(16))) uint32_t hot_rows[kBigLdsBytes / 4];
  __shared__ uint8_t colmap[256];
  const uint32_t nhot = f.hot * f.ncol;
  for (uint32_t i = threadIdx.x; i < nhot; i += blockDim.x) hot_rows[i] = f.trans[i];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) colmap[i] = f.colmap[i];
  __syncthreads();
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < bt.count; h += nthreads) {
    const uint8_t *base;
    uint64_t len;
    if (STRIDED) {
      base = bt.hay + h * bt.stride;
      len = bt.length;
    } else {
      const uint64_t o0 = bt.offs[h], o1 = bt.offs[h + 1];
      base = bt.hay + o0;
      len = o1 - o0;
    }
    const uint64_t at = bt.start;
    uint64_t last = NONE;
    bool done = at > len;
    uint32_t s = f.dead;
    if (!done) {
      s = f.ustart1 ? f.ustart1 - 1 : f.start[fwd_flag_index(base, len, at)];
      done = s >= f.n_normal;  // dead start state (dfa.rs:484)
    }
    uint64_t p = at;
    // head to the 16-byte boundary, then whole chunks, then the tail
    while (!done && p < len) {
      const uintptr_t a = (uintptr_t)(base + p);
      const uint4 v = *(const uint4 *)(a & ~(uintptr_t)15);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      const uint32_t j0 = (uint32_t)(a & 15);
      const uint32_t n = (uint32_t)min<uint64_t>(16 - j0, len - p);
      uint32_t cols[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) cols[j] = colmap[(w[j >> 2] >> (8 * (j & 3))) & 0xFF];
#pragma unroll
      for (uint32_t j = 0; j < 16; ++j) {
        if (j < j0 || j >= j0 + n || done) continue;
        s = big_next(f, hot_rows, s, cols[j]);
        if (s >= f.n_normal) {
          if (s < f.n_match_end) {  // dfa.rs:658-668: Match(at - 1)
            last = p + (j - j0);
            if (MODE != MODE_FIND) done = true;  // quit_after_match
          } else {
            done = true;  // dead
          }
        }
      }
      p += n;
    }
    if (!done && f.eof[s]) last = len;  // dfa.rs:748-763
    if (MODE == MODE_ISMATCH) {
      ((uint8_t *)out)[h] = last != NONE ? 1 : 0;
      continue;
    }
    if (MODE == MODE_SHORTEST) {
      ((uint64_t *)out)[h] = last;
      continue;
    }
    uint64_t ms = NONE, me = NONE;
    if (last != NONE) {
      me = last;
      if (me == at) {
        ms = at;  // exec.rs:647
      } else {
        const uint64_t rs = big_rev_scan(r, base, len, at, me);
        if (rs == NONE) ms = me = NONE;  // exec.rs:656-660
        else ms = rs;
      }
    }
    ((uint64_t *)out)[2 * h] = ms;
    ((uint64_t *)out)[2 * h + 1] = me;
  }
}

template <int MODE>
hipError_t launch_big_m(const BatchDev &b, const BigDfaDev &f, const BigDfaDev &r, void *out, hipStream_t st,
                        int cus) {
  const uint64_t blocks = (b.count + 1023) / 1024;
  const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)cus * 2));
  if (b.offs)
    hipLaunchKernelGGL((big_dfa_kernel<MODE, false>), dim3(grid), dim3(1024), 0, st, b, f, r, out);
  else
    hipLaunchKernelGGL((big_dfa_kernel<MODE, true>), dim3(grid), dim3(1024), 0, st, b, f, r, out);
  return hipGetLastError();
}

// The on-demand DFA (LazyDfaDev): one lane per haystack as big_dfa_kernel;
// a lane that meets a row not built yet records where it stopped and parks
// (the host builds the rows the parked lanes need and runs another round
// from there, as the reference's lazy DFA builds a state when a search
// first steps into it, dfa.rs:910-1048).
constexpr uint32_t kLazyMatchBit = 0x80000000u, kLazyUnknownEntry = 0x7FFFFFFFu;
template <int MODE, bool STRIDED>
__global__ __launch_bounds__(1024) void lazy_dfa_kernel(BatchDev bt, LazyDfaDev f, RevDfaDev r, const LazyPark *in,
                                                        uint64_t nin, LazyPark *park, unsigned long long *npark,
                                                        void *out) {
  __shared__ __attribute__((aligned(16))) uint32_t hot_rows[kBigLdsBytes / 4];
  __shared__ uint8_t colmap[256];
  const uint32_t nhot = f.hot * f.ncol;
  for (uint32_t i = threadIdx.x; i < nhot; i += blockDim.x) hot_rows[i] = f.trans[i];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) colmap[i] = f.colmap[i];
  __syncthreads();
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x, nl = in ? nin : bt.count;
  for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nl; l += nthreads) {
    uint64_t h = l;
    if (in) h = in[l].h;
    const uint8_t *base;
    uint64_t len;
    if (STRIDED) {
      base = bt.hay + h * bt.stride;
      len = bt.length;
    } else {
      const uint64_t o0 = bt.offs[h], o1 = bt.offs[h + 1];
      base = bt.hay + o0;
      len = o1 - o0;
    }
    const uint64_t at = bt.start;
    uint64_t last = NONE, p = at;
    bool done = at > len, parked = false;
    uint32_t s = 0;
    if (in) {
      p = in[l].p;
      last = in[l].last;
      s = in[l].s;
    } else if (!done) {
      s = f.start[fwd_flag_index(base, len, at)];
      done = s == 0;  // dead start state (dfa.rs:484)
    }
    while (!done && p < len) {
      const uintptr_t a = (uintptr_t)(base + p);
      const uint4 v = *(const uint4 *)(a & ~(uintptr_t)15);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      const uint32_t j0 = (uint32_t)(a & 15);
      const uint32_t n = (uint32_t)min<uint64_t>(16 - j0, len - p);
      uint32_t j = j0;
      for (; j < j0 + n; ++j) {
        const uint32_t c = colmap[(w[j >> 2] >> (8 * (j & 3))) & 0xFF];
        const uint32_t e = s < f.hot ? hot_rows[s * f.ncol + c] : f.trans[(size_t)s * f.ncol + c];
        if (e == kLazyUnknownEntry) {
          parked = true;
          break;
        }
        if (e == 0) {
          done = true;  // dead
          break;
        }
        s = e & ~kLazyMatchBit;
        if (e & kLazyMatchBit) {  // dfa.rs:658-668: Match(at - 1)
          last = p + (j - j0);
          if (MODE != MODE_FIND) {
            done = true;  // quit_after_match
            break;
          }
        }
      }
      p += j - j0;
      if (parked) break;
    }
    if (parked) {
      const unsigned long long k = atomicAdd(npark, 1ull);
      LazyPark x;
      x.h = h;
      x.p = p;
      x.last = last;
      x.s = s;
      x.pad = 0;
      park[k] = x;
      continue;
    }
    if (!done && f.eof[s]) last = len;  // dfa.rs:748-763
    if (MODE == MODE_ISMATCH) {
      ((uint8_t *)out)[h] = last != NONE ? 1 : 0;
      continue;
    }
    if (MODE == MODE_SHORTEST) {
      ((uint64_t *)out)[h] = last;
      continue;
    }
    uint64_t ms = NONE, me = NONE;
    if (last != NONE) {
      me = last;
      if (me == at) {
        ms = at;  // exec.rs:647
      } else {
        const uint64_t rs = rev_scan(r, nullptr, base, len, at, me);
        if (rs == NONE) ms = me = NONE;  // exec.rs:656-660
        else ms = rs;
      }
    }
    ((uint64_t *)out)[2 * h] = ms;
    ((uint64_t *)out)[2 * h + 1] = me;
  }
}

template <int MODE>
hipError_t launch_lazy_m(const BatchDev &b, const LazyDfaDev &f, const RevDfaDev &r, const LazyPark *in,
                         uint64_t nin, LazyPark *park, unsigned long long *npark, void *out, hipStream_t st,
                         int cus) {
  const uint64_t lanes = in ? nin : b.count;
  const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((lanes + 1023) / 1024, (uint64_t)cus * 2));
  if (b.offs)
    hipLaunchKernelGGL((lazy_dfa_kernel<MODE, false>), dim3(grid), dim3(1024), 0, st, b, f, r, in, nin, park, npark,
                       out);
  else
    hipLaunchKernelGGL((lazy_dfa_kernel<MODE, true>), dim3(grid), dim3(1024), 0, st, b, f, r, in, nin, park, npark,
                       out);
  return hipGetLastError();
}

// find_iter on the on-demand DFA (re_trait.rs:197-221 over find_dfa_forward,
// exec.rs:632-662): one lane per haystack runs the whole iteration, every
// search the walk of lazy_dfa_kernel<MODE_FIND> from the iteration's position
// ip.  A search without a match ends the iteration: ip past the end, a dead
// start state, no match end, or a reverse NoMatch (exec.rs:656-660).  The
// step rule is iter_scan.hip iter_next's: an empty match moves ip to e + 1
// and is skipped when it ends where the last match did, any other match
// moves ip to its end.  Every pass of the loop leaves it, consumes a byte or
// ends a search, and a search that ends leaves the loop or raises ip.
//
// WRITE = false counts: a lane that meets a row not built yet parks with the
// iteration's state (ip, lm, count) and the search's (p, s, last), and the
// next round resumes it inside that search; a lane that finishes writes
// counts[h].  WRITE = true runs once after the counts are scanned to off:
// match k of haystack h goes to record off[h] + k when that is below cap.
// The walk is the count form's, so every row it reads is built; should it
// read an unknown entry all the same, it sets *flag and the lane stops.
template <bool WRITE, bool STRIDED>
__global__ __launch_bounds__(1024) void lazy_iter_kernel(BatchDev bt, LazyDfaDev f, RevDfaDev r,
                                                         const LazyIterPark *in, uint64_t nin, LazyIterPark *park,
                                                         unsigned long long *npark, uint32_t *counts,
                                                         const uint64_t *off, uint64_t *matches, uint64_t cap,
                                                         uint32_t *flag) {
  __shared__ __attribute__((aligned(16))) uint32_t hot_rows[kBigLdsBytes / 4];
  __shared__ uint8_t colmap[256];
  const uint32_t nhot = f.hot * f.ncol;
  for (uint32_t i = threadIdx.x; i < nhot; i += blockDim.x) hot_rows[i] = f.trans[i];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) colmap[i] = f.colmap[i];
  __syncthreads();
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x, nl = in ? nin : bt.count;
  for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nl; l += nthreads) {
    uint64_t h = l;
    if (in) h = in[l].h;
    const uint8_t *base;
    uint64_t len;
    if (STRIDED) {
      base = bt.hay + h * bt.stride;
      len = bt.length;
    } else {
      const uint64_t o0 = bt.offs[h], o1 = bt.offs[h + 1];
      base = bt.hay + o0;
      len = o1 - o0;
    }
    uint64_t ip = bt.start, lm = NONE, cnt = 0;  // the iteration
    uint64_t p = 0, last = NONE;                 // the search
    uint32_t s = 0;
    bool searching = false, parked = false;
    if (in) {
      ip = in[l].ip;
      lm = in[l].lm;
      cnt = in[l].count;
      p = in[l].p;
      last = in[l].last;
      s = in[l].s;
      searching = true;
    }
    // One loop for the whole iteration, a 16-byte block of a search per pass:
    // a lane whose search ends finds its start and begins the next search
    // inside the pass and walks on beside the wave's other lanes (a walk loop
    // inside a search loop made the whole wave wait for the slowest walk
    // before any lane could begin its next search: 1.9 times the time on
    // text where nearly every wave holds a match).
    while (true) {
      if (!searching) {
        if (ip > len) break;
        s = f.start[fwd_flag_index(base, len, ip)] & ~kLazyMatchBit;
        if (s == 0) break;  // dead start state (dfa.rs:484)
        p = ip;
        last = NONE;
        searching = true;
      }
      bool done = false;
      if (p < len) {
        const uintptr_t a = (uintptr_t)(base + p);
        const uint4 v = *(const uint4 *)(a & ~(uintptr_t)15);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const uint32_t j0 = (uint32_t)(a & 15);
        const uint32_t n = (uint32_t)min<uint64_t>(16 - j0, len - p);
        uint32_t j = j0;
        for (; j < j0 + n; ++j) {
          const uint32_t c = colmap[(w[j >> 2] >> (8 * (j & 3))) & 0xFF];
          const uint32_t e = s < f.hot ? hot_rows[s * f.ncol + c] : f.trans[(size_t)s * f.ncol + c];
          if (e == kLazyUnknownEntry) {
            parked = true;
            break;
          }
          if (e == 0) {
            done = true;  // dead
            break;
          }
          s = e & ~kLazyMatchBit;
          if (e & kLazyMatchBit) last = p + (j - j0);  // dfa.rs:658-668: Match(at - 1)
        }
        p += j - j0;
        if (parked) break;
        if (!done && p < len) continue;  // the next block
      }
      // the search is over: the automaton died, or the text ended
      searching = false;
      if (!done && f.eof[s]) last = len;  // dfa.rs:748-763
      if (last == NONE) break;
      uint64_t ms = ip;  // exec.rs:647
      if (last != ip) {
        ms = rev_scan(r, nullptr, base, len, ip, last);
        if (ms == NONE || ms == QUITMARK) break;  // exec.rs:656-660 (no quit state here)
      }
      if (ms == last) {
        ip = last + 1;
        if (lm == last) continue;
      } else {
        ip = last;
      }
      lm = last;
      if (WRITE) {
        const uint64_t k = off[h] + cnt;
        if (k < cap) {
          matches[2 * k] = ms;
          matches[2 * k + 1] = last;
        }
      }
      ++cnt;
    }
    if (parked) {
      if (WRITE) {
        *flag = 1;
        continue;
      }
      const unsigned long long k = atomicAdd(npark, 1ull);
      LazyIterPark x;
      x.h = h;
      x.ip = ip;
      x.lm = lm;
      x.p = p;
      x.last = last;
      x.count = cnt;
      x.s = s;
      x.pad = 0;
      park[k] = x;
      continue;
    }
    if (!WRITE) counts[h] = (uint32_t)cnt;
  }
}

// RegexSet matches on a set's on-demand DFA (many_matches_at, exec.rs:
// 998-1038 over dfa.rs:525-570): the walk of lazy_dfa_kernel, ORing up the
// patterns each step reports as dfa_set_kernel does (now[] of the state
// entered, a global u64 read taken only on entries with the match bit and
// not on the chain from one state to the next), until the text ends (the
// EOF step, dfa.rs:1004-1015: eof_mask[] of the last state), the automaton
// dies or every pattern of the set is in the mask.  A parked lane carries
// its mask in LazyPark::last.
template <bool STRIDED>
__global__ __launch_bounds__(1024) void lazy_set_kernel(BatchDev bt, LazyDfaDev f, uint64_t all, const LazyPark *in,
                                                        uint64_t nin, LazyPark *park, unsigned long long *npark,
                                                        uint64_t *out) {
  __shared__ __attribute__((aligned(16))) uint32_t hot_rows[kBigLdsBytes / 4];
  __shared__ uint8_t colmap[256];
  const uint32_t nhot = f.hot * f.ncol;
  for (uint32_t i = threadIdx.x; i < nhot; i += blockDim.x) hot_rows[i] = f.trans[i];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) colmap[i] = f.colmap[i];
  __syncthreads();
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x, nl = in ? nin : bt.count;
  for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nl; l += nthreads) {
    uint64_t h = l;
    if (in) h = in[l].h;
    const uint8_t *base;
    uint64_t len;
    if (STRIDED) {
      base = bt.hay + h * bt.stride;
      len = bt.length;
    } else {
      const uint64_t o0 = bt.offs[h], o1 = bt.offs[h + 1];
      base = bt.hay + o0;
      len = o1 - o0;
    }
    uint64_t mask = 0, p = bt.start;
    bool done = bt.start > len, parked = false;  // done: no EOF step (dead, or nothing left to find)
    uint32_t s = 0;
    if (in) {
      p = in[l].p;
      mask = in[l].last;
      s = in[l].s;
    } else if (!done) {
      const uint32_t e = f.start[fwd_flag_index(base, len, bt.start)];
      s = e & ~kLazyMatchBit;
      done = s == 0;  // dead start state (dfa.rs:484)
    }
    while (!done && p < len) {
      const uintptr_t a = (uintptr_t)(base + p);
      const uint4 v = *(const uint4 *)(a & ~(uintptr_t)15);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      const uint32_t j0 = (uint32_t)(a & 15);
      const uint32_t n = (uint32_t)min<uint64_t>(16 - j0, len - p);
      uint32_t j = j0;
      for (; j < j0 + n; ++j) {
        const uint32_t c = colmap[(w[j >> 2] >> (8 * (j & 3))) & 0xFF];
        const uint32_t e = s < f.hot ? hot_rows[s * f.ncol + c] : f.trans[(size_t)s * f.ncol + c];
        if (e == kLazyUnknownEntry) {
          parked = true;
          break;
        }
        if (e == 0) {
          done = true;  // dead
          break;
        }
        s = e & ~kLazyMatchBit;
        if (e & kLazyMatchBit) {
          mask |= f.now[s];
          if ((mask & all) == all) {
            done = true;
            break;
          }
        }
      }
      p += j - j0;
      if (parked) break;
    }
    if (parked) {
      const unsigned long long k = atomicAdd(npark, 1ull);
      LazyPark x;
      x.h = h;
      x.p = p;
      x.last = mask;
      x.s = s;
      x.pad = 0;
      park[k] = x;
      continue;
    }
    out[h] = done ? mask : mask | f.eof_mask[s];
  }
}

// Few long fixed-stride haystacks on the on-demand DFA: the cut-bounded
// search of long_scan.hip's long_unit, one lane per unit, with the walk,
// staging and match bookkeeping of lazy_dfa_kernel.  Unit [c0, c1) takes the
// start state at c0, walks through c1 - 1 (phase kLazyLongBefore), steps into
// strip[s] there (kLazyLongAtCut: the threads started in the unit alone go
// on) and walks until the automaton dies or the text ends (kLazyLongAfter);
// the unit that owns the end has no cut and is in the last phase from its
// start.  A lane parks on a row not built yet, or at the cut on a link not
// computed, and a later round resumes it in the phase it was in.
//
// Results as long_scan_m gathers them: is_match stores a byte, shortest_match
// takes the minimum end (best = the output for both), find keeps the unit's
// match end in ures[u] and the smallest matching unit in best[h]; the match's
// start is found once, for the winner (lazy_long_finish_kernel).  Once per
// 512 bytes of text a lane reads what its haystack has published and leaves
// when it cannot change it (a load outside the per-byte chain).
template <int MODE>
__device__ __forceinline__ void lazy_long_publish(unsigned long long *best, uint64_t *ures, uint64_t h, uint64_t u,
                                                  uint64_t last) {
  if (last == NONE) return;
  if (MODE == MODE_ISMATCH) {
    ((uint8_t *)best)[h] = 1;
  } else if (MODE == MODE_SHORTEST) {
    atomicMin(&best[h], (unsigned long long)last);
  } else {
    ures[u] = last;
    atomicMin(&best[h], (unsigned long long)u);
  }
}

template <int MODE>
__global__ __launch_bounds__(1024) void lazy_long_kernel(BatchDev bt, Geo g, uint64_t nunits, LazyDfaDev f,
                                                         const LazyLongPark *in, uint64_t nin, LazyLongPark *park,
                                                         unsigned long long *npark, uint64_t *ures,
                                                         unsigned long long *best) {
  __shared__ __attribute__((aligned(16))) uint32_t hot_rows[kBigLdsBytes / 4];
  __shared__ uint8_t colmap[256];
  const uint32_t nhot = f.hot * f.ncol;
  for (uint32_t i = threadIdx.x; i < nhot; i += blockDim.x) hot_rows[i] = f.trans[i];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) colmap[i] = f.colmap[i];
  __syncthreads();
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x, nl = in ? nin : nunits;
  for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nl; l += nthreads) {
    const uint64_t u = in ? in[l].u : l;
    uint64_t h, len, c0, c1;
    const uint8_t *base;
    unit_bounds<false>(bt, g, u, &h, &base, &len, &c0, &c1);
    const bool cut = c1 > c0 && c1 - 1 <= len;  // as long_unit
    uint64_t last = NONE, p = c0;
    uint32_t s = 0, phase = cut ? kLazyLongBefore : kLazyLongAfter;
    bool done = c0 > len, parked = false;
    uintptr_t nblk = 0;  // the block `nxt` holds (0: none)
    uint4 nxt = make_uint4(0, 0, 0, 0);
    if (in) {
      p = in[l].p;
      last = in[l].last;
      s = in[l].s;
      phase = in[l].phase;
    } else if (!done) {
      s = f.start[fwd_flag_index(base, len, c0)] & ~kLazyMatchBit;
      done = s == 0;  // dead start state (dfa.rs:484)
    }
    while (!done) {
      if (phase == kLazyLongAtCut) {
        const uint32_t e = f.strip ? f.strip[s] : kLazyUnknownEntry;
        if (e == kLazyUnknownEntry) {
          parked = true;
          break;
        }
        if (e == 0) {
          done = true;  // no thread started in the unit is alive
          lazy_long_publish<MODE>(best, ures, h, u, last);
          break;
        }
        s = e;
        phase = kLazyLongAfter;
      }
      const uint64_t lim = phase == kLazyLongBefore ? c1 - 1 : len;
      while (!done && !parked && p < lim) {
        const uintptr_t a = (uintptr_t)(base + p), blk = a & ~(uintptr_t)15;
        if ((a & 0x1F0) == 0) {  // what the haystack has published so far
          bool leave;
          if (MODE == MODE_ISMATCH) {
            leave = __hip_atomic_load((const uint8_t *)best + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
          } else {
            const unsigned long long v = __hip_atomic_load(&best[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // shortest_match: an end at or before c0 (this unit's are later); find: a smaller unit
            leave = MODE == MODE_SHORTEST ? v <= c0 : v < u;
          }
          if (leave) {
            last = NONE;
            done = true;
            break;
          }
        }
        // this block (loaded a pass ago when the walk came here in order),
        // and the next one's load in flight while this one's bytes are stepped
        const uint4 v = blk == nblk ? nxt : *(const uint4 *)blk;
        if (blk + 16 < (uintptr_t)(base + len)) {
          nblk = blk + 16;
          nxt = *(const uint4 *)nblk;
        }
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const uint32_t j0 = (uint32_t)(a & 15);
        const uint32_t n = (uint32_t)min<uint64_t>(16 - j0, lim - p);
        uint32_t j = j0;
        for (; j < j0 + n; ++j) {
          const uint32_t c = colmap[(w[j >> 2] >> (8 * (j & 3))) & 0xFF];
          const uint32_t e = s < f.hot ? hot_rows[s * f.ncol + c] : f.trans[(size_t)s * f.ncol + c];
          if (e == kLazyUnknownEntry) {
            parked = true;
            break;
          }
          if (e == 0) {
            done = true;  // dead
            break;
          }
          s = e & ~kLazyMatchBit;
          if (e & kLazyMatchBit) {  // dfa.rs:658-668: Match(at - 1)
            last = p + (j - j0);
            if (MODE != MODE_FIND) {
              done = true;  // quit_after_match
              break;
            }
          }
        }
        p += j - j0;
        // A finished unit publishes here, inside the walk: after the loop the
        // wave's lanes meet again only when its slowest one is through, and
        // the units that could leave on this result would walk on until then.
        if (done) lazy_long_publish<MODE>(best, ures, h, u, last);
      }
      if (done || parked || phase == kLazyLongAfter) break;
      phase = kLazyLongAtCut;
    }
    if (parked) {
      const unsigned long long k = atomicAdd(npark, 1ull);
      LazyLongPark x;
      x.u = u;
      x.p = p;
      x.last = last;
      x.s = s;
      x.phase = phase;
      park[k] = x;
      continue;
    }
    if (done) continue;  // (published where it finished)
    if (f.eof[s]) last = len;  // dfa.rs:748-763
    lazy_long_publish<MODE>(best, ures, h, u, last);
  }
}

// RegexSet matches over few long fixed-stride haystacks on a set's on-demand
// DFA: the units, the strip at c1 - 1 and the OR into the haystack's word of
// set_long_kernel (set_long.hip), with the walk, staging and phases of
// lazy_long_kernel and the set bookkeeping of lazy_set_kernel (now[] read on
// entries with the match bit, eof_mask[] where a unit reaches the end of the
// text alive; the mask travels in LazyLongPark::last).  out[h] is zeroed by
// the caller before the first round and only ever ORed into.
//
// A unit publishes where it finishes, inside the walk (lazy_long_kernel's
// note), and once per 512 bytes of text it ORs in the bits the word lacks and
// reads the word back: it leaves when every pattern of the set is there, or,
// past its cut, when everything its state can still report is (reach[s], a
// superset: a lingering `.*` thread need not drag the unit to the end of the
// haystack).  512 bytes as lazy_long_kernel, not set_long_kernel's 4096: a
// byte here is a dependent table read, not a quarter of a packed LDS lookup,
// so the poll (two loads and at most one atomic, none in the per-byte chain)
// is as small a share of the walk, and the other lanes of the wave wait for a
// unit that could have left at most that long.  The twin a unit steps into
// may be a state without threads (its row is all dead): any id but 0 walks on.
__global__ __launch_bounds__(1024) void lazy_set_long_kernel(BatchDev bt, Geo g, uint64_t nunits, LazyDfaDev f,
                                                             uint64_t all, const LazyLongPark *in, uint64_t nin,
                                                             LazyLongPark *park, unsigned long long *npark,
                                                             unsigned long long *out) {
  __shared__ __attribute__((aligned(16))) uint32_t hot_rows[kBigLdsBytes / 4];
  __shared__ uint8_t colmap[256];
  const uint32_t nhot = f.hot * f.ncol;
  for (uint32_t i = threadIdx.x; i < nhot; i += blockDim.x) hot_rows[i] = f.trans[i];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) colmap[i] = f.colmap[i];
  __syncthreads();
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x, nl = in ? nin : nunits;
  for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nl; l += nthreads) {
    const uint64_t u = in ? in[l].u : l;
    uint64_t h, len, c0, c1;
    const uint8_t *base;
    unit_bounds<false>(bt, g, u, &h, &base, &len, &c0, &c1);
    const bool cut = c1 > c0 && c1 - 1 <= len;  // as set_long_kernel
    uint64_t mask = 0, p = c0;
    uint32_t s = 0, phase = cut ? kLazyLongBefore : kLazyLongAfter;
    bool done = c0 > len, parked = false;  // done: no EOF step (a search from past the end reports nothing)
    uintptr_t nblk = 0;  // the block `nxt` holds (0: none)
    uint4 nxt = make_uint4(0, 0, 0, 0);
    if (in) {
      p = in[l].p;
      mask = in[l].last;
      s = in[l].s;
      phase = in[l].phase;
    } else if (!done) {
      s = f.start[fwd_flag_index(base, len, c0)] & ~kLazyMatchBit;
      done = s == 0;  // dead start state (dfa.rs:484)
    }
    while (!done) {
      if (phase == kLazyLongAtCut) {
        const uint32_t e = f.strip ? f.strip[s] : kLazyUnknownEntry;
        if (e == kLazyUnknownEntry) {
          parked = true;
          break;
        }
        if (e == 0) {
          done = true;  // no thread started in the unit is alive
          if (mask) atomicOr(&out[h], (unsigned long long)mask);
          break;
        }
        s = e;
        phase = kLazyLongAfter;
      }
      const uint64_t lim = phase == kLazyLongBefore ? c1 - 1 : len;
      while (!done && !parked && p < lim) {
        const uintptr_t a = (uintptr_t)(base + p), blk = a & ~(uintptr_t)15;
        if ((a & 0x1F0) == 0) {  // the haystack's word: add what it lacks, leave when nothing new can come
          uint64_t seen = __hip_atomic_load(&out[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          const uint64_t lack = mask & ~seen;
          if (lack) seen = atomicOr(&out[h], (unsigned long long)lack) | lack;
          if ((all & ~seen) == 0 || (phase == kLazyLongAfter && (f.reach[s] & ~seen) == 0)) {
            done = true;  // (what the unit had is in the word)
            break;
          }
        }
        const uint4 v = blk == nblk ? nxt : *(const uint4 *)blk;
        if (blk + 16 < (uintptr_t)(base + len)) {
          nblk = blk + 16;
          nxt = *(const uint4 *)nblk;
        }
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const uint32_t j0 = (uint32_t)(a & 15);
        const uint32_t n = (uint32_t)min<uint64_t>(16 - j0, lim - p);
        uint32_t j = j0;
        for (; j < j0 + n; ++j) {
          const uint32_t c = colmap[(w[j >> 2] >> (8 * (j & 3))) & 0xFF];
          const uint32_t e = s < f.hot ? hot_rows[s * f.ncol + c] : f.trans[(size_t)s * f.ncol + c];
          if (e == kLazyUnknownEntry) {
            parked = true;
            break;
          }
          if (e == 0) {
            done = true;  // dead
            break;
          }
          s = e & ~kLazyMatchBit;
          if (e & kLazyMatchBit) mask |= f.now[s];
        }
        p += j - j0;
        if (done && mask) atomicOr(&out[h], (unsigned long long)mask);
      }
      if (done || parked || phase == kLazyLongAfter) break;
      phase = kLazyLongAtCut;
    }
    if (parked) {
      const unsigned long long k = atomicAdd(npark, 1ull);
      LazyLongPark x;
      x.u = u;
      x.p = p;
      x.last = mask;
      x.s = s;
      x.phase = phase;
      park[k] = x;
      continue;
    }
    if (done) continue;  // (published where it finished)
    mask |= f.eof_mask[s];  // dfa.rs:1004-1015
    if (mask) atomicOr(&out[h], (unsigned long long)mask);
  }
}

// find: the winner's match (find_dfa_forward, exec.rs:632-662): its end from
// the smallest unit that matched, its start from the reverse DFA over
// text[start..end]; an empty match at `start` starts there (exec.rs:647), a
// reverse NoMatch makes the search's answer "no match" (exec.rs:656-660).
__global__ __launch_bounds__(256) void lazy_long_finish_kernel(BatchDev bt, RevDfaDev r, const uint64_t *ures,
                                                               const unsigned long long *best, uint64_t *out) {
  for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < bt.count; h += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long v = best[h];
    uint64_t ms = NONE, me = NONE;
    if (v != ~0ull) {
      me = ures[v];
      if (me == bt.start) {
        ms = me;
      } else {
        ms = rev_scan(r, nullptr, bt.hay + h * bt.stride, bt.length, bt.start, me);
        if (ms == NONE) me = NONE;
      }
    }
    out[2 * h] = ms;
    out[2 * h + 1] = me;
  }
}

// find_iter over few long fixed-stride haystacks on the on-demand DFA: the
// iteration of lazy_iter_kernel, one lane per unit of lazy_long_kernel's
// geometry.  A unit's iteration runs from an entry state (ip, lm) while ip is
// before its cut c1 and owns the matches that start before c1: each search is
// lazy_long_kernel's bounded one from ip (through c1 - 1, into strip[s] there,
// on until the automaton dies or the text ends, then the EOF step; the unit
// that owns the end has no cut), then lazy_iter_kernel's delayed match flag,
// rev_scan for the start and iter_next's step rule.  The unit ends when ip
// reaches c1 (exit (ip, lm), clean when ip == c1 and no match ended there),
// when a search finds nothing (exit: the state that search began in, clean:
// no match starts between there and c1, so the next unit's iteration is a
// fresh one) or on a reverse NoMatch (the stop exit: the haystack's iteration
// is over).  Which entries a round's fresh lanes take: kLilFresh .. kLilFinal
// (dfa_scan.hpp); how the records are combined: lazy_iter_long_device.hpp.
//
// One loop as lazy_iter_kernel (a 16-byte block, the step into the link, or
// the end of a search and the begin of the next per pass), staging and the
// next block's load in flight as lazy_long_kernel.  A lane parks on a row not
// built, or at the cut on a link not computed, with the iteration's state and
// the search's, and the next round resumes it inside that search.  WRITE as
// lazy_iter_kernel's: it runs once over the final entries, stops after the
// matches the count form found, and sets *flag where it would have parked.
template <bool WRITE>
__global__ __launch_bounds__(1024) void lazy_iter_long_kernel(
    BatchDev bt, Geo g, uint64_t nunits, LazyDfaDev f, RevDfaDev r, uint32_t from, const LilRec *ent,
    const LilTodo *todo, uint64_t ntodo, const LazyIterLongPark *in, uint64_t nin, LazyIterLongPark *park,
    unsigned long long *npark, LilRec *out, unsigned long long *stats, const uint64_t *off, uint64_t *matches,
    uint64_t cap, uint32_t *flag) {
  __shared__ __attribute__((aligned(16))) uint32_t hot_rows[kBigLdsBytes / 4];
  __shared__ uint8_t colmap[256];
  const uint32_t nhot = f.hot * f.ncol;
  for (uint32_t i = threadIdx.x; i < nhot; i += blockDim.x) hot_rows[i] = f.trans[i];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) colmap[i] = f.colmap[i];
  __syncthreads();
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t nl = in ? nin : from == kLilList ? ntodo : nunits;
  for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nl; l += nthreads) {
    const uint64_t u = in ? in[l].u : from == kLilList ? todo[l].u : l;
    if (u >= nunits) continue;
    uint64_t h, len, c0, c1;  // c1 == NONE: the unit that owns the end
    const uint8_t *base;
    unit_bounds<false>(bt, g, u, &h, &base, &len, &c0, &c1);
    uint64_t ip = c0, lm = NONE, cnt = 0, want = NONE;  // the iteration
    uint64_t p = 0, last = NONE;                        // the search
    uint32_t s = 0, phase = kLazyLongAfter;
    bool searching = false, parked = false;
    if (in) {
      ip = in[l].ip;
      lm = in[l].lm;
      cnt = in[l].count;
      p = in[l].p;
      last = in[l].last;
      s = in[l].s;
      phase = in[l].phase;
      searching = true;
    } else {
      if (from == kLilAfter) {
        if (u % g.nk == 0) {
          out[u].flags = 0;
          continue;
        }
        const LilRec pr = ent[u - 1];
        if (pr.flags & kLilClean) {
          out[u].flags = 0;
          continue;
        }
        atomicAdd(&stats[1], 1ull);
        if (lil_steps_over(pr.xp, c1)) {
          out[u] = lil_skip(pr.xp, pr.xlm, c1);
          continue;
        }
        ip = pr.xp;
        lm = pr.xlm;
      } else if (from == kLilList) {
        ip = todo[l].p;
        lm = todo[l].lm;
      } else if (from == kLilFinal) {
        const LilRec fr = ent[u];
        if (fr.count == 0) continue;
        ip = fr.ep;
        lm = fr.elm;
        want = fr.count;
      }
      if (!WRITE) {
        out[u].ep = ip;
        out[u].elm = lm;
      }
    }
    uint64_t xp = ip, xlm = lm;  // the exit, as long as the search under way finds nothing
    bool xclean = true;
    uintptr_t nblk = 0;  // the block `nxt` holds (0: none)
    uint4 nxt = make_uint4(0, 0, 0, 0);
    while (true) {
      if (!searching) {
        if (WRITE && cnt >= want) break;
        xp = ip;
        xlm = lm;
        if (ip >= c1) {
          xclean = ip == c1 && lm != c1;
          break;
        }
        xclean = true;
        if (ip > len) break;
        s = f.start[fwd_flag_index(base, len, ip)] & ~kLazyMatchBit;
        if (s == 0) break;  // dead start state (dfa.rs:484)
        p = ip;
        last = NONE;
        phase = c1 == NONE ? kLazyLongAfter : kLazyLongBefore;
        searching = true;
      }
      bool done = false;
      if (phase == kLazyLongAtCut) {
        const uint32_t e = f.strip ? f.strip[s] : kLazyUnknownEntry;
        if (e == kLazyUnknownEntry) {
          parked = true;
          break;
        }
        if (e == 0) {
          done = true;  // no thread started before the cut is alive
        } else {
          s = e;
          phase = kLazyLongAfter;
        }
      }
      if (!done) {
        const uint64_t lim = phase == kLazyLongBefore ? c1 - 1 : len;
        if (p < lim) {
          const uintptr_t a = (uintptr_t)(base + p), blk = a & ~(uintptr_t)15;
          const uint4 v = blk == nblk ? nxt : *(const uint4 *)blk;
          if (blk + 16 < (uintptr_t)(base + len)) {
            nblk = blk + 16;
            nxt = *(const uint4 *)nblk;
          }
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
          const uint32_t j0 = (uint32_t)(a & 15);
          const uint32_t n = (uint32_t)min<uint64_t>(16 - j0, lim - p);
          uint32_t j = j0;
          for (; j < j0 + n; ++j) {
            const uint32_t c = colmap[(w[j >> 2] >> (8 * (j & 3))) & 0xFF];
            const uint32_t e = s < f.hot ? hot_rows[s * f.ncol + c] : f.trans[(size_t)s * f.ncol + c];
            if (e == kLazyUnknownEntry) {
              parked = true;
              break;
            }
            if (e == 0) {
              done = true;  // dead
              break;
            }
            s = e & ~kLazyMatchBit;
            if (e & kLazyMatchBit) last = p + (j - j0);  // dfa.rs:658-668: Match(at - 1)
          }
          p += j - j0;
          if (parked) break;
          if (!done && p < lim) continue;  // the next block
        }
        if (!done && phase == kLazyLongBefore) {
          phase = kLazyLongAtCut;
          continue;
        }
      }
      // the search is over: the automaton died, or the text ended
      searching = false;
      if (!done && f.eof[s]) last = len;  // dfa.rs:748-763
      if (last == NONE) break;
      uint64_t ms = ip;  // exec.rs:647
      if (last != ip) {
        ms = rev_scan(r, nullptr, base, len, ip, last);
        if (ms == NONE || ms == QUITMARK) {  // exec.rs:656-660 (no quit state here): the stop exit
          xp = xlm = NONE;
          xclean = false;
          break;
        }
      }
      if (ms == last) {
        ip = last + 1;
        if (lm == last) continue;
      } else {
        ip = last;
      }
      lm = last;
      if (WRITE) {
        const uint64_t k = off[u] + cnt;
        if (k < cap) {
          matches[2 * k] = ms;
          matches[2 * k + 1] = last;
        }
      }
      ++cnt;
    }
    if (parked) {
      if (WRITE) {
        *flag = 1;
        continue;
      }
      const unsigned long long k = atomicAdd(npark, 1ull);
      LazyIterLongPark x;
      x.u = u;
      x.ip = ip;
      x.lm = lm;
      x.count = cnt;
      x.p = p;
      x.last = last;
      x.s = s;
      x.phase = phase;
      park[k] = x;
      continue;
    }
    if (!WRITE) {
      out[u].xp = xp;
      out[u].xlm = xlm;
      out[u].count = (uint32_t)cnt;
      out[u].flags = kLilHas | (xclean ? kLilClean : 0) | (from == kLilList ? (uint32_t)kLilRun << kLilSrcShift : 0);
    }
  }
}

// Pass C (lazy_iter_long_device.hpp): the parallel pass, one lane per unit ...
__global__ __launch_bounds__(256) void lazy_iter_long_parallel_kernel(uint64_t nunits, uint64_t nh, const LilRec *spec,
                                                                      const LilRec *fix, LilRec *fin,
                                                                      uint8_t *changed, LilWalk *walk) {
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x, t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (uint64_t u = t0; u < nunits; u += nthreads) {
    LilRec f;
    changed[u] = lil_parallel(spec[u], fix[u], &f) ? 1 : 0;
    fin[u] = f;
  }
  for (uint64_t h = t0; h < nh; h += nthreads) {
    LilWalk w;
    w.k = w.xp = w.xlm = 0;
    w.active = w.xclean = 0;
    walk[h] = w;
  }
}

// ... and the walkers, one lane per haystack: a haystack has few changed
// units (a match that crosses a cut and leaves the next unit otherwise than
// its own speculation did), and a walk between them is a chain of record
// loads, no DFA.
__global__ __launch_bounds__(64) void lazy_iter_long_walk_kernel(uint64_t nh, uint64_t nk, uint64_t start,
                                                                 uint64_t chunk, const LilRec *spec, const LilRec *fix,
                                                                 LilRec *fin, const uint8_t *changed, LilWalk *walk,
                                                                 LilTodo *todo, unsigned long long *stats) {
  for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < nh; h += (uint64_t)gridDim.x * blockDim.x) {
    LilWalk w = walk[h];
    if (w.k >= nk) continue;
    const uint64_t u0 = h * nk;
    LilTodo t;
    if (lil_walk(&w, nk, start, chunk, spec + u0, fix + u0, fin + u0, changed + u0, &t)) {
      t.u += u0;
      todo[atomicAdd(&stats[0], 1ull)] = t;
    }
    walk[h] = w;
  }
}

__global__ __launch_bounds__(256) void lazy_iter_long_counts_kernel(uint64_t nunits, const LilRec *fin,
                                                                    uint32_t *ucounts) {
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u <= nunits; u += (uint64_t)gridDim.x * blockDim.x)
    ucounts[u] = u < nunits ? fin[u].count : 0;
}

template <int MODE>
hipError_t launch_lazy_long_m(const BatchDev &b, const Geo &g, uint64_t nunits, const LazyDfaDev &f,
                              const LazyLongPark *in, uint64_t nin, LazyLongPark *park, unsigned long long *npark,
                              uint64_t *ures, unsigned long long *best, hipStream_t st, int cus) {
  const uint64_t lanes = in ? nin : nunits;
  const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((lanes + 1023) / 1024, (uint64_t)cus * 2));
  hipLaunchKernelGGL((lazy_long_kernel<MODE>), dim3(grid), dim3(1024), 0, st, b, g, nunits, f, in, nin, park, npark,
                     ures, best);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_lazy_long(int mode, const BatchDev &b, const LazyDfaDev &f, uint64_t chunk, const LazyLongPark *in,
                            uint64_t nin, LazyLongPark *park, unsigned long long *npark, uint64_t *ures,
                            unsigned long long *best, hipStream_t st, int cus) {
  if (b.offs || chunk == 0) return hipErrorInvalidValue;
  if (b.count == 0 || (in && nin == 0)) return hipSuccess;
  note_fwd_path(RURE_AMD_PATH_LAZY_DFA);
  Geo g;  // long_scan_m's
  g.chunk = chunk;
  g.end = ~0ull;
  g.slots = 0;
  const uint64_t nunits = lazy_long_units(b, chunk);
  g.nk = nunits / b.count;
  switch (mode) {
    case MODE_FIND: return launch_lazy_long_m<MODE_FIND>(b, g, nunits, f, in, nin, park, npark, ures, best, st, cus);
    case MODE_ISMATCH:
      return launch_lazy_long_m<MODE_ISMATCH>(b, g, nunits, f, in, nin, park, npark, ures, best, st, cus);
    default: return launch_lazy_long_m<MODE_SHORTEST>(b, g, nunits, f, in, nin, park, npark, ures, best, st, cus);
  }
}

static Geo lazy_long_geo(const BatchDev &b, uint64_t chunk, uint64_t *nunits) {
  Geo g;  // long_scan_m's
  g.chunk = chunk;
  g.end = ~0ull;
  g.slots = 0;
  *nunits = lazy_long_units(b, chunk);
  g.nk = *nunits / b.count;
  return g;
}

hipError_t launch_lazy_iter_long_count(const BatchDev &b, const LazyDfaDev &f, const RevDfaDev &r, uint64_t chunk,
                                       int from, const LilRec *ent, const LilTodo *todo, uint64_t ntodo,
                                       const LazyIterLongPark *in, uint64_t nin, LazyIterLongPark *park,
                                       unsigned long long *npark, LilRec *out, unsigned long long *stats,
                                       hipStream_t st, int cus) {
  if (b.offs || chunk == 0 || from < kLilFresh || from > kLilList) return hipErrorInvalidValue;
  if (b.count == 0 || (in && nin == 0) || (!in && from == kLilList && ntodo == 0)) return hipSuccess;
  note_fwd_path(RURE_AMD_PATH_LAZY_DFA);
  uint64_t nunits;
  const Geo g = lazy_long_geo(b, chunk, &nunits);
  const uint64_t lanes = in ? nin : from == kLilList ? ntodo : nunits;
  const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((lanes + 1023) / 1024, (uint64_t)cus * 2));
  hipLaunchKernelGGL((lazy_iter_long_kernel<false>), dim3(grid), dim3(1024), 0, st, b, g, nunits, f, r, (uint32_t)from,
                     ent, todo, ntodo, in, nin, park, npark, out, stats, (const uint64_t *)nullptr,
                     (uint64_t *)nullptr, (uint64_t)0, (uint32_t *)nullptr);
  return hipGetLastError();
}

hipError_t launch_lazy_iter_long_write(const BatchDev &b, const LazyDfaDev &f, const RevDfaDev &r, uint64_t chunk,
                                       const LilRec *fin, const uint64_t *off, uint64_t *matches, uint64_t cap,
                                       uint32_t *flag, hipStream_t st, int cus) {
  if (b.offs || chunk == 0) return hipErrorInvalidValue;
  if (b.count == 0) return hipSuccess;
  uint64_t nunits;
  const Geo g = lazy_long_geo(b, chunk, &nunits);
  const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((nunits + 1023) / 1024, (uint64_t)cus * 2));
  hipLaunchKernelGGL((lazy_iter_long_kernel<true>), dim3(grid), dim3(1024), 0, st, b, g, nunits, f, r,
                     (uint32_t)kLilFinal, fin, (const LilTodo *)nullptr, (uint64_t)0,
                     (const LazyIterLongPark *)nullptr, (uint64_t)0, (LazyIterLongPark *)nullptr,
                     (unsigned long long *)nullptr, (LilRec *)nullptr, (unsigned long long *)nullptr, off, matches, cap,
                     flag);
  return hipGetLastError();
}

hipError_t launch_lazy_iter_long_resolve(const BatchDev &b, uint64_t chunk, bool first, const LilRec *spec,
                                         const LilRec *fix, LilRec *fin, uint8_t *changed, LilWalk *walk,
                                         LilTodo *todo, unsigned long long *stats, hipStream_t st, int cus) {
  if (b.offs || chunk == 0) return hipErrorInvalidValue;
  if (b.count == 0) return hipSuccess;
  uint64_t nunits;
  const Geo g = lazy_long_geo(b, chunk, &nunits);
  if (first) {
    hipLaunchKernelGGL(lazy_iter_long_parallel_kernel, dim3(grid_cap(nunits, 256, cus, 8)), dim3(256), 0, st, nunits,
                       b.count, spec, fix, fin, changed, walk);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(lazy_iter_long_walk_kernel, dim3(grid_cap(b.count, 64, cus, 128)), dim3(64), 0, st, b.count,
                     g.nk, b.start, chunk, spec, fix, fin, (const uint8_t *)changed, walk, todo, stats);
  return hipGetLastError();
}

hipError_t launch_lazy_iter_long_counts(const BatchDev &b, uint64_t chunk, const LilRec *fin, uint32_t *ucounts,
                                        hipStream_t st, int cus) {
  if (b.offs || chunk == 0) return hipErrorInvalidValue;
  const uint64_t nunits = lazy_long_units(b, chunk);
  hipLaunchKernelGGL(lazy_iter_long_counts_kernel, dim3(grid_cap(nunits + 1, 256, cus, 8)), dim3(256), 0, st, nunits,
                     fin, ucounts);
  return hipGetLastError();
}

hipError_t launch_lazy_long_finish(const BatchDev &b, const RevDfaDev &r, const uint64_t *ures,
                                   const unsigned long long *best, uint64_t *out, hipStream_t st, int cus) {
  if (b.count == 0) return hipSuccess;
  hipLaunchKernelGGL(lazy_long_finish_kernel, dim3(grid_cap(b.count, 256, cus, 4)), dim3(256), 0, st, b, r, ures, best,
                     out);
  return hipGetLastError();
}

hipError_t launch_lazy_set_long(const BatchDev &b, const LazyDfaDev &f, uint64_t all, uint64_t chunk,
                                const LazyLongPark *in, uint64_t nin, LazyLongPark *park, unsigned long long *npark,
                                uint64_t *out, hipStream_t st, int cus) {
  if (b.offs || chunk == 0 || !f.now || !f.eof_mask || !f.reach) return hipErrorInvalidValue;
  if (b.count == 0 || (in && nin == 0)) return hipSuccess;
  note_fwd_path(RURE_AMD_PATH_LAZY_DFA);
  Geo g;  // launch_set_long's
  g.chunk = chunk;
  g.end = ~0ull;
  g.slots = 0;
  const uint64_t nunits = lazy_long_units(b, chunk);
  g.nk = nunits / b.count;
  const uint64_t lanes = in ? nin : nunits;
  const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((lanes + 1023) / 1024, (uint64_t)cus * 2));
  hipLaunchKernelGGL(lazy_set_long_kernel, dim3(grid), dim3(1024), 0, st, b, g, nunits, f, all, in, nin, park, npark,
                     (unsigned long long *)out);
  return hipGetLastError();
}

hipError_t launch_lazy_set(const BatchDev &b, const LazyDfaDev &f, uint64_t all, const LazyPark *in, uint64_t nin,
                           LazyPark *park, unsigned long long *npark, uint64_t *out, hipStream_t st, int cus) {
  if (b.count == 0 || (in && nin == 0)) return hipSuccess;
  note_fwd_path(RURE_AMD_PATH_LAZY_DFA);
  const uint64_t lanes = in ? nin : b.count;
  const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((lanes + 1023) / 1024, (uint64_t)cus * 2));
  if (b.offs)
    hipLaunchKernelGGL((lazy_set_kernel<false>), dim3(grid), dim3(1024), 0, st, b, f, all, in, nin, park, npark, out);
  else
    hipLaunchKernelGGL((lazy_set_kernel<true>), dim3(grid), dim3(1024), 0, st, b, f, all, in, nin, park, npark, out);
  return hipGetLastError();
}

hipError_t launch_lazy_dfa(int mode, const BatchDev &b, const LazyDfaDev &f, const RevDfaDev &r, const LazyPark *in,
                           uint64_t nin, LazyPark *park, unsigned long long *npark, void *out, hipStream_t st,
                           int cus) {
  if (b.count == 0 || (in && nin == 0)) return hipSuccess;
  note_fwd_path(RURE_AMD_PATH_LAZY_DFA);
  switch (mode) {
    case MODE_FIND: return launch_lazy_m<MODE_FIND>(b, f, r, in, nin, park, npark, out, st, cus);
    case MODE_ISMATCH: return launch_lazy_m<MODE_ISMATCH>(b, f, r, in, nin, park, npark, out, st, cus);
    default: return launch_lazy_m<MODE_SHORTEST>(b, f, r, in, nin, park, npark, out, st, cus);
  }
}

hipError_t launch_lazy_iter_count(const BatchDev &b, const LazyDfaDev &f, const RevDfaDev &r, const LazyIterPark *in,
                                  uint64_t nin, LazyIterPark *park, unsigned long long *npark, uint32_t *counts,
                                  hipStream_t st, int cus) {
  if (b.count == 0 || (in && nin == 0)) return hipSuccess;
  note_fwd_path(RURE_AMD_PATH_LAZY_DFA);
  const uint64_t lanes = in ? nin : b.count;
  const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((lanes + 1023) / 1024, (uint64_t)cus * 2));
  if (b.offs)
    hipLaunchKernelGGL((lazy_iter_kernel<false, false>), dim3(grid), dim3(1024), 0, st, b, f, r, in, nin, park, npark,
                       counts, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, (uint32_t *)nullptr);
  else
    hipLaunchKernelGGL((lazy_iter_kernel<false, true>), dim3(grid), dim3(1024), 0, st, b, f, r, in, nin, park, npark,
                       counts, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, (uint32_t *)nullptr);
  return hipGetLastError();
}

hipError_t launch_lazy_iter_write(const BatchDev &b, const LazyDfaDev &f, const RevDfaDev &r, const uint64_t *off,
                                  uint64_t *matches, uint64_t cap, uint32_t *flag, hipStream_t st, int cus) {
  if (b.count == 0) return hipSuccess;
  const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((b.count + 1023) / 1024, (uint64_t)cus * 2));
  if (b.offs)
    hipLaunchKernelGGL((lazy_iter_kernel<true, false>), dim3(grid), dim3(1024), 0, st, b, f, r,
                       (const LazyIterPark *)nullptr, (uint64_t)0, (LazyIterPark *)nullptr,
                       (unsigned long long *)nullptr, (uint32_t *)nullptr, off, matches, cap, flag);
  else
    hipLaunchKernelGGL((lazy_iter_kernel<true, true>), dim3(grid), dim3(1024), 0, st, b, f, r,
                       (const LazyIterPark *)nullptr, (uint64_t)0, (LazyIterPark *)nullptr,
                       (unsigned long long *)nullptr, (uint32_t *)nullptr, off, matches, cap, flag);
  return hipGetLastError();
}

uint32_t lazy_dfa_hot_rows(uint32_t ncol) { return kBigLdsBytes / 4 / std::max<uint32_t>(ncol, 1); }

uint32_t big_dfa_hot_rows(uint32_t ncol, uint32_t nstates) {
  return std::min<uint32_t>(nstates, kBigLdsBytes / 4 / std::max<uint32_t>(ncol, 1));
}

hipError_t launch_big_dfa(int mode, const BatchDev &b, const BigDfaDev &f, const BigDfaDev &r, void *out,
                          hipStream_t st, int cus) {
  if (b.count == 0) return hipSuccess;
  note_fwd_path(RURE_AMD_PATH_BIG_DFA);
  switch (mode) {
    case MODE_FIND: return launch_big_m<MODE_FIND>(b, f, r, out, st, cus);
    case MODE_ISMATCH: return launch_big_m<MODE_ISMATCH>(b, f, r, out, st, cus);
    default: return launch_big_m<MODE_SHORTEST>(b, f, r, out, st, cus);
  }
}

}  // namespace rure_amd
