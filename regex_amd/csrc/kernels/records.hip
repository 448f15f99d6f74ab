// Device grep for gfx950: the matching records of one delimited text.
//
// rure_amd_match_records: the text is cut into units (records_device.hpp), a
// unit's lane answers the records that start in it with the is_match walk of
// the lane kernels (dfa_device.hpp fwd_run, from each record's first byte over
// its own length, so that look-around sees the record's edges), and keeps the
// answers as bits indexed by record start.  A search never crosses a
// delimiter: a cut at a record start needs no speculation and no repair, and
// everything runs on grids fixed by the text's length.  Records the DFA quit
// on (a Unicode word boundary next to a non-ASCII byte) go to a second bitmap
// that the Pike VM sweeps, a wave per record, only when a device word says
// there are any.  The per-unit counts' exclusive sums then give every unit
// its place in the outputs, and the write pass walks the delimiters again.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "iter_device.hpp"
#include "nfa_device.hpp"

namespace rure_amd {

namespace {

using namespace pike;
using pike::NONE;  // (dfa_device.hpp has the same two constants)
using pike::QUITMARK;

__device__ __forceinline__ void set_bit(uint32_t *bits, uint64_t p) { atomicOr(&bits[p >> 5], 1u << (p & 31)); }

// DFA = false: a regex without an eager DFA, every record is left to the Pike VM.
template <bool DFA>
__global__ __launch_bounds__(256) void records_scan_kernel(const uint8_t *text, uint64_t length, uint32_t rep,
                                                           uint64_t chunk, uint64_t nunits, FwdDfaDev f,
                                                           RecordsScratch s) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  if (DFA) {
    for (uint32_t i = threadIdx.x * 16; i < f.lds_bytes; i += blockDim.x * 16)
      *(uint4 *)(lds + i) = *(const uint4 *)(f.lds_image + i);
    __syncthreads();
  }
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < nunits; u += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t owned = 0, selected = 0;
    bool any_quit = false;
    for (RecWalk w(text, length, chunk, u, rep); w.more(); w.next()) {
      ++owned;
      bool quit = !DFA, hit = false;
      if (DFA) {
        const uint8_t *base = text + w.s;
        const uint64_t len = w.e - w.s;
        LaneState L;
        lane_start(L, f, base, len, 0);
        fwd_run<MODE_ISMATCH>(L, f, lds, base, len, 0);
        quit = L.quit;
        hit = !quit && L.last != NONE;
      }
      if (hit) {
        set_bit(s.sel_bits, w.s);
        ++selected;
      }
      if (quit) {
        set_bit(s.quit_bits, w.s);
        any_quit = true;
      }
    }
    s.owned[u] = owned;
    s.selected[u] = selected;
    if (any_quit) atomicOr(s.quit_word, 1u);
  }
}

// A wave per 64 words of the quit bitmap; the set bits' records one after the
// other on the wave (nfa_scan.hip pike_kernel's lists).
__global__ __launch_bounds__(64) void records_pike_kernel(const uint8_t *text, uint64_t length, uint32_t rep,
                                                          uint64_t chunk, NfaDev nf, RecordsScratch s,
                                                          unsigned long long *served, uint8_t *scratch) {
  // the scan flagged no quit: nothing to answer
  if (__atomic_load_n(s.quit_word, __ATOMIC_RELAXED) == 0) return;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint8_t *mem = scratch ? scratch + (size_t)blockIdx.x * nfa_wave_bytes(nf.nleaves) : lds;
  Lists W;
  const uint32_t N = nf.nleaves;
  W.st[0] = (uint64_t *)mem;
  W.st[1] = W.st[0] + N;
  W.stamp = (uint32_t *)(W.st[1] + N);
  W.leaf[0] = W.stamp + N;
  W.leaf[1] = W.leaf[0] + N;
  const uint32_t lane = lane_id();
  for (uint32_t i = lane; i < N; i += 64) W.stamp[i] = 0xFFFFFFFFu;
  wave_sync();
  TagGen tg;
  const uint64_t words = (length + 31) / 32;
  unsigned long long nserved = 0;
  for (uint64_t g = blockIdx.x; g * 64 < words; g += gridDim.x) {
    const uint64_t wi = g * 64 + lane;
    const uint32_t qw = wi < words ? s.quit_bits[wi] : 0u;
    uint64_t todo = __ballot(qw != 0);
    while (todo) {
      const uint32_t t = (uint32_t)__builtin_ctzll(todo);
      todo &= todo - 1;
      uint32_t bits = __shfl(qw, t);
      while (bits) {
        const uint32_t b = (uint32_t)__builtin_ctz(bits);
        bits &= bits - 1;
        const uint64_t rs = (g * 64 + t) * 32 + b;
        const uint64_t re = rec_find_delim(text, length, rs, rep);
        uint64_t r0 = 0, r1 = NONE;
        pike_one<MODE_ISMATCH>(nf, W, tg, text + rs, re - rs, 0, &r0, &r1);
        ++nserved;
        if (r0 && lane == 0) {
          set_bit(s.sel_bits, rs);
          atomicAdd(&s.selected[rs / chunk], 1u);
        }
      }
    }
  }
  if (served && nserved && lane == 0) atomicAdd(served, nserved);
}

__global__ __launch_bounds__(256) void records_write_kernel(const uint8_t *text, uint64_t length, uint32_t rep,
                                                            uint64_t chunk, uint64_t nunits, uint32_t invert,
                                                            RecordsScratch s, uint64_t *nrecords, uint64_t *total,
                                                            uint64_t *records, uint64_t *numbers, uint64_t cap) {
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < nunits; u += (uint64_t)gridDim.x * blockDim.x) {
    if (u == 0) {
      const uint64_t nr = s.owned_off[nunits], ns = s.selected_off[nunits];
      *nrecords = nr;
      *total = invert ? nr - ns : ns;
    }
    uint64_t number = s.owned_off[u];
    uint64_t j = invert ? number - s.selected_off[u] : s.selected_off[u];
    uint32_t left = invert ? s.owned[u] - s.selected[u] : s.selected[u];
    if (left == 0 || j >= cap) continue;  // nothing of this unit is written: no second walk
    for (RecWalk w(text, length, chunk, u, rep); w.more() && left; w.next(), ++number) {
      const uint32_t bit = (s.sel_bits[w.s >> 5] >> (w.s & 31)) & 1u;
      if (bit == invert) continue;
      if (j < cap) {
        records[2 * j] = w.s;
        records[2 * j + 1] = w.e;
        if (numbers) numbers[j] = number;
      }
      ++j;
      --left;
    }
  }
}

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

size_t records_scratch_bytes(uint64_t length, uint64_t units, size_t *zeroed) {
  const size_t bits = al256(((length + 31) / 32) * 4);
  const size_t z = 2 * bits + 256;  // the two bitmaps and the quit word
  if (zeroed) *zeroed = z;
  return z + 2 * al256((units + 1) * 4) + 2 * al256((units + 1) * 8);
}

RecordsScratch records_scratch_at(void *block, uint64_t length, uint64_t units) {
  const size_t bits = al256(((length + 31) / 32) * 4);
  uint8_t *p = (uint8_t *)block;
  RecordsScratch s;
  s.sel_bits = (uint32_t *)p;
  s.quit_bits = (uint32_t *)(p + bits);
  s.quit_word = (uint32_t *)(p + 2 * bits);
  p += 2 * bits + 256;
  s.owned = (uint32_t *)p;
  p += al256((units + 1) * 4);
  s.selected = (uint32_t *)p;
  p += al256((units + 1) * 4);
  s.owned_off = (uint64_t *)p;
  p += al256((units + 1) * 8);
  s.selected_off = (uint64_t *)p;
  return s;
}

hipError_t launch_records_scan(const uint8_t *text, uint64_t length, uint8_t delim, uint64_t chunk,
                               const FwdDfaDev *f, const RecordsScratch &s, hipStream_t st, int cus) {
  if (!text || !length || !chunk) return hipErrorInvalidValue;
  const uint64_t nunits = rec_units(length, chunk);
  const uint32_t rep = delim * 0x01010101u;
  if (!f) {
    hipLaunchKernelGGL(records_scan_kernel<false>, dim3(grid_cap(nunits, 256, cus, 8)), dim3(256), 0, st, text, length,
                       rep, chunk, nunits, FwdDfaDev{}, s);
    return hipGetLastError();
  }
  const size_t lds = f->lds_bytes;
  const int per_cu = std::max<int>(1, std::min<int>(8, (int)((160u * 1024u) / std::max<size_t>(lds, 1))));
  const hipError_t e = allow_lds(records_scan_kernel<true>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(records_scan_kernel<true>, dim3(grid_cap(nunits, 256, cus, per_cu)), dim3(256), lds, st, text,
                     length, rep, chunk, nunits, *f, s);
  return hipGetLastError();
}

int records_pike_grid(uint64_t length, const NfaDev &n, int cus) {
  const uint64_t slices = ((length + 31) / 32 + 63) / 64;
  const size_t wb = nfa_wave_bytes(n.nleaves);
  const uint64_t per_cu = wb <= kNfaLdsMax ? std::max<uint64_t>(1, std::min<uint64_t>(32, (160u * 1024u) / wb)) : 4;
  return (int)std::max<uint64_t>(1, std::min<uint64_t>(slices, (uint64_t)cus * per_cu));
}

hipError_t launch_records_pike(const uint8_t *text, uint64_t length, uint8_t delim, uint64_t chunk, const NfaDev &n,
                               const RecordsScratch &s, unsigned long long *served, void *scratch, hipStream_t st,
                               int grid) {
  if (!text || !length || !chunk || grid < 1) return hipErrorInvalidValue;
  const size_t lds = scratch ? 0 : nfa_wave_bytes(n.nleaves);
  const hipError_t e = allow_lds(records_pike_kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(records_pike_kernel, dim3(grid), dim3(64), lds, st, text, length, delim * 0x01010101u, chunk, n,
                     s, served, (uint8_t *)scratch);
  return hipGetLastError();
}

hipError_t launch_records_write(const uint8_t *text, uint64_t length, uint8_t delim, uint64_t chunk, bool invert,
                                const RecordsScratch &s, uint64_t *nrecords, uint64_t *total, uint64_t *records,
                                uint64_t *numbers, uint64_t cap, hipStream_t st, int cus) {
  if (!text || !length || !chunk || !nrecords || !total || (!records && cap)) return hipErrorInvalidValue;
  const uint64_t nunits = rec_units(length, chunk);
  hipLaunchKernelGGL(records_write_kernel, dim3(grid_cap(nunits, 256, cus, 8)), dim3(256), 0, st, text, length,
                     delim * 0x01010101u, chunk, nunits, invert ? 1u : 0u, s, nrecords, total, records, numbers, cap);
  return hipGetLastError();
}

}  // namespace rure_amd
