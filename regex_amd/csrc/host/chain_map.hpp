// The byte map of a chain of one-byte-class replace_all steps, composed on
// the host: pure functions (no HIP, no library state), used by
// rure_amd_replace_all_chain and exported for the tests by
// rure_amd_chain_map_export.
//
// Step i maps each byte of its class to its replacement and every other byte
// to itself, so the chain maps each byte x to a string F(x) = h_n(...h_1(x)).
// The device runs the chain as that one map (launch_replace_hmap) when it is
// "mappable": every image is at most kChainImageMax bytes, the images fit
// the pool, and fewer than 256 byte values change (a changed byte's index is
// a u8 and 0xFF says "unchanged": with all 256 changed, byte 0xFF's index
// would be the sentinel).  Any other chain runs step by step.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

namespace rure_amd {

constexpr uint32_t kChainImageMax = 64;  // an image's length is 7 bits of the write kernel's table
constexpr uint8_t kChainSame = 0xFF;     // aidx of a byte the chain leaves alone

struct ChainMap {
  bool mappable = false;
  uint32_t nact = 0;      // byte values F changes (0 when an image is too long)
  uint32_t pool_len = 0;  // sum of |F(x)| (0 when an image is too long)
  // What launch_replace_hmap reads, built only when mappable: |F(x)| (256
  // u8), the offset of F(x) in the pool (256 u16), the index of x among the
  // changed bytes in byte order or kChainSame (256 u8), the pool (pool_max
  // bytes, pool_len used), then per step i |F_i(x)| - 1 (256 u32 each).
  std::vector<uint8_t> blob;
};

// cls[i]: the 256-entry class of step i (non-zero: in the class); reps[i],
// rep_lens[i]: its replacement (1..kChainImageMax bytes).
inline ChainMap compose_chain_map(const uint8_t *const *cls, const uint8_t *const *reps, const size_t *rep_lens,
                                  size_t n, uint32_t pool_max) {
  ChainMap m;
  std::vector<std::string> img(256);
  std::vector<uint32_t> dl(n * 256, 0);
  for (int x = 0; x < 256; ++x) {
    std::string cur(1, (char)x);
    for (size_t i = 0; i < n; ++i) {
      std::string nx;
      for (unsigned char c : cur) {
        if (cls[i][c]) nx.append((const char *)reps[i], rep_lens[i]);
        else nx.push_back((char)c);
      }
      cur.swap(nx);
      if (cur.size() > kChainImageMax) return m;  // (images may grow 64-fold per step: stop here)
      dl[i * 256 + x] = (uint32_t)cur.size() - 1;
    }
    img[x] = cur;
  }
  for (int x = 0; x < 256; ++x) {
    m.pool_len += (uint32_t)img[x].size();
    m.nact += img[x].size() == 1 && (uint8_t)img[x][0] == x ? 0 : 1;
  }
  if (m.pool_len > pool_max || m.nact > 255) return m;
  m.mappable = true;
  m.blob.assign(1024 + (size_t)pool_max + n * 256 * 4, 0);
  uint8_t *flen = m.blob.data(), *aidx = m.blob.data() + 768, *pool = m.blob.data() + 1024;
  uint16_t *soff = (uint16_t *)(m.blob.data() + 256);
  size_t at = 0;
  uint32_t a = 0;
  for (int x = 0; x < 256; ++x) {
    const bool same = img[x].size() == 1 && (uint8_t)img[x][0] == x;
    flen[x] = (uint8_t)img[x].size();
    soff[x] = (uint16_t)at;
    aidx[x] = same ? kChainSame : (uint8_t)a++;
    memcpy(pool + at, img[x].data(), img[x].size());
    at += img[x].size();
  }
  if (n) memcpy(pool + pool_max, dl.data(), dl.size() * 4);
  return m;
}

}  // namespace rure_amd
