// Device-side descriptors shared by the HIP kernels and the host runtime.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/rure_amd.h"
#include "../host/chunk_plan.hpp"
#include "../host/knobs.hpp"
#include "lazy_iter_long_device.hpp"
#include "records_device.hpp"
#include "tile_skip_device.hpp"

namespace rure_amd {

// Row pitch of the LDS hot tables (bytes).  256 columns + 48 bytes: row s
// starts 12 banks after row s-1, so lanes in the few dominant states reading
// random printable bytes (24 dwords of a row) collide least; a bank-conflict
// model over the C2 haystacks gives 4.15 LDS cycles per lookup
// wave-instruction at 304 vs 4.67 at 260 and 4.86 at 256 (2 = conflict free).
constexpr uint32_t kRow = 304;
// Column of the forward hot rows (in the padding) holding the row's own
// number: the identity step for bytes outside a masked block.
constexpr uint32_t kIdCol = 256;

enum { MODE_FIND = 0, MODE_ISMATCH = 1, MODE_SHORTEST = 2 };

// The LDS hand-over inside one wave: what its lanes stored before it is what
// its lanes load after it (the lanes run in lockstep, so no s_barrier; the
// fences keep the compiler and the LDS queue from reordering across it).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct BatchDev {
  const uint8_t *hay;
  const uint64_t *offs;   // n+1 offsets or nullptr (fixed stride)
  uint64_t stride, length, count, start;
  // set (atomic OR) by the DFA kernels when a haystack's DFA quit; the Pike VM
  // fallback pass then runs, else it returns at once (nullptr: always runs)
  uint32_t *quit_flag = nullptr;
  // a deferred fallback's gate (nullptr: always runs): the find_iter kernels
  // return at once unless (*gate != 0) == gate_set, so the ASCII shadow's
  // passes after its quit check and the full automaton's re-run are both
  // enqueued and one of them works (dispatch.cpp run_find_iter)
  const uint32_t *gate = nullptr;
  uint32_t gate_set = 0;
  // set masks (the Pike VM's MODE_SET): words between consecutive haystacks'
  // masks (a set of more than 64 patterns: group g writes word g)
  uint32_t out_stride = 1;
  // offset batches of find / is_match / shortest_match with the deferred long
  // scan (long_scan.hip launch_long_ragged; nullptr: none): a lane whose
  // haystack has defer_len bytes or more (the threshold on its span plus
  // `start`) appends it to the list behind `defer` (kDefer* words; a full
  // list leaves the haystack to the lane), writes "no match" and moves on
  unsigned long long *defer = nullptr;
  uint64_t defer_len = 0;
};

// The deferred long scan's device block (u64 words): the header, then the
// list of deferred haystacks (kDeferCap entries).  kDeferTried counts the
// lanes that asked (it may pass the capacity); the geometry kernel writes
// kDeferCount .. kDeferUnits (and the same figures into the host's record
// for rure_amd_last_long_units).
enum { kDeferTried = 0, kDeferTotal = 1, kDeferCount = 2, kDeferChunk = 3, kDeferUnits = 4, kDeferCap = 5, kDeferList = 8 };

// Forward DFA on the device.  State ids: [0, hot) are in the LDS fast table
// (u8, 256 columns, row `hot` = absorbing sentinel); [0, n_normal) carry no
// match flag; [n_normal, n_match_end) carry the match flag; `dead`, `quit`.
struct FwdDfaDev {
  const uint8_t *lds_image;   // (hot + 1) * 256 bytes, padded to 16
  uint32_t lds_bytes;
  uint32_t hot;
  // Multi-byte fast table for the coalesced-tile kernel (stride 2 or 4 bytes
  // per LDS lookup over local byte classes of the ASCII-hot sub-DFA);
  // stride == 1 means "use lds_image".  Image: 4 x 256 u8 class tables
  // (class * K^(stride-1-p) for byte position p) then (hot_s + 1) * P u16
  // entries holding next_state * P; sentinel = hot_s * P.
  const uint8_t *lds_image_s;
  uint32_t lds_bytes_s;
  uint32_t stride, hot_s, P, sent;
  uint32_t cus;               // compute units of the device (launch heuristics)
  const uint16_t *full;       // nstates * 256
  const uint8_t *eof;         // nstates: EOF step yields a match flag
  const uint16_t *start;      // 128 start states by flag index
  const uint16_t *strip;      // find_iter DFA only: state minus the `.*?` prefix (or null)
  uint32_t n_normal, n_match_end, dead, quit;
  uint32_t all;               // lds_image rows are exact for every state (hot = nstates <= 255)
  uint32_t ustart1;           // 1 + the start state when it does not depend on the flags, else 0
  uint32_t nonempty;          // the regex never matches the empty string (the iteration's
                              // last-match state then never matters)
  // find_iter DFA only: the regex as a finite string set (host/literals.hpp),
  // lit_n = 0 if it is not one.  Image (kLit* offsets): 64 Kibit bitmap over
  // a hash of the first lit_k bytes, then keys (u32, first lit_k bytes), lens
  // (u8) and bytes (32 per literal), in leftmost-first priority order.
  const uint8_t *lit_image;
  uint32_t lit_bytes, lit_n, lit_k, lit_minlen, lit_maxlen;
  uint32_t lit_k8;            // every literal has >= 8 bytes: a second bitmap filters on bytes 4..7
  // find_iter DFA only: the string set as a bit-parallel Shift-And automaton
  // (sa_len = 0: none).  Every string has sa_len bytes; the set is a union of
  // class sequences (strings that differ in one position merged), sequence x
  // owning bits [x * sa_len, (x + 1) * sa_len).  sa_image: 256 u64 masks,
  // bit i of mask[b] = byte b is in the class of bit position i.
  const uint64_t *sa_image;
  uint64_t sa_init, sa_final;   // first / last bit of every sequence
  uint32_t sa_len, sa_bits;
  // find_iter DFA only: the first-byte start rule (fb_n = 0: off).  Every
  // match starts with one of fb_n <= 4 bytes (fb_rep[i] = byte * 0x01010101),
  // and an anchored run from such a byte never dies before it has matched
  // (host: first_byte_rule).  Then the leftmost match of a search from p
  // that ends in the dead state before the end of the text starts at the
  // first of those bytes at or after p, so the start needs no reverse scan.
  uint32_t fb_n;
  uint32_t fb_rep[4];
  // find_iter DFA only: the lexer table (lex_bytes = 0: none; host build_lex).
  // When the first-byte start rule holds and every match-flag state is
  // terminal (all transitions dead), the iteration itself is a DFA: entering
  // a match state at byte x ends the search there and the next one starts at
  // x, so that transition goes to a twin of the start state's successor on
  // the same byte.  u8 rows of kRow bytes; states numbered [others, S0 =
  // lex_s0, twin(S0), other twins] with the codes 0, 1, 2, 3 = the byte's
  // flags: 1 = the state after it is the start state (Z), 2 = Z and a
  // match ended at it (EMIT), 3 = EMIT only.
  const uint8_t *lex_image;
  uint32_t lex_bytes, lex_s0;
  // The same lexer four bytes per step (host build_lex4; lex4_image null:
  // none): at most kLex4Rows rows and 3 byte classes over ASCII, class 3 =
  // "no byte" (a partial word's tail).  kLex4Bytes of LDS: next row at
  // [row * 256 + c] (c = the four bytes' classes, 2 bits each), the four
  // bytes' flags (2 bits each, codes as above) at kLex4Flags + the same
  // index, and four byte -> class << 2j tables at kLex4Cls + 256 j.
  const uint8_t *lex4_image;
  uint32_t lex4_s0;
  // The start-state prefix skip (dfa.rs:700-711, 1504-1506 prefix_at): when
  // the regex has prefix literals (literal_sets.hpp, dfa.prefixes) whose
  // first bytes are at most 4 (pfx_rep[i] = byte * 0x01010101), every match
  // starts with one of them, so a scan in the start state (ustart1 - 1: the
  // start does not depend on look-behind) jumps over the 128-byte bursts
  // that hold none of those bytes (fwd_range); pfx_n = 0: off.
  uint32_t pfx_n;
  uint32_t pfx_rep[4];
  // The same skip on the prefixes' rarest bytes (literals.rs:390-510
  // FreqyPacked picks the rarest byte by a frequency table; here the table
  // is host/byte_freq.h, and on 128-byte bursts a pair is needed, a single
  // common-word letter being in nearly every burst): every prefix has byte
  // class 1 at offset i1 and class 2 at i1 + rare_d (d <= 3; d = 0: one
  // byte), each one byte or an ASCII letter's two cases (x | rare_or ==
  // rare_rep).  A burst [a, a + 128) is skipped when no q in [a, a + 144)
  // has class 1 at q and class 2 at q + d (i1 + d <= 15, so every start in
  // the burst is covered; positions past it only add candidates).  Used
  // where the prefixes have several first bytes ((?i)holmes); rare_on = 0:
  // the first-byte skip above.
  uint32_t rare_on, rare_d;
  uint32_t rare_rep[2], rare_or[2];
  // find_iter DFA only: the regex has look-around assertions (the chunked
  // iteration then repairs units whose first reverse scan reached their
  // start, and a reverse NoMatch ends the iteration; iter_scan.hip), and its
  // DFA can quit (1; 2: a Unicode word boundary's quit, whose units the wave
  // serves, iter_scan.hip).  The literal, Shift-And, lexer and first-byte
  // engines are off.
  uint32_t looks, can_quit;
  // find_iter DFA only: the regex is one byte class repeated (C+, host
  // run_class): run_cls[b] bit 0 = b is in C, bit 1 = b quits (the ASCII
  // shadow: bytes >= 0x80), bit 2 = decode (a Unicode class C+, host
  // unicode_run_set: bytes >= 0x80 are read as UTF-8 against run_cp, its
  // code point bitmap); null: not such a regex (run_iter.hip)
  const uint8_t *run_cls;
  const uint32_t *run_cp;
  uint32_t run_quit;  // some byte quits (bit 1): the run engine's flag is read back
  // forward DFA of find / is_match / shortest_match only: the tile kernel's
  // skip rule (tile_skip_device.hpp; skip.on = 0: the regex is not eligible)
  TileSkipDev skip;
};
constexpr uint32_t kLexMaxRows = 24;  // lexer table rows (iter_spec_lex_tile_kernel's static LDS)
constexpr uint32_t kLexUnit = kRow / 4;  // lexer entry -> row address multiplier
constexpr uint32_t kLexBytes = (kLexMaxRows * kRow + 3 * kLexUnit + 15) & ~15u;  // largest lexer image
constexpr uint32_t kLex4Rows = 8, kLex4Flags = kLex4Rows * 256, kLex4Cls = 2 * kLex4Flags;
constexpr uint32_t kLex4Bytes = kLex4Cls + 4 * 256;

// Literal engine image layout (at most kLitMax literals of kLitLen bytes).
constexpr uint32_t kLitMax = 64, kLitLen = 32;
constexpr uint32_t kLitKeys = 8192, kLitLens = kLitKeys + 4 * kLitMax, kLitBytes = kLitLens + kLitMax;
constexpr uint32_t kLitBitmap2 = kLitBytes + kLitMax * kLitLen;  // second bitmap: bytes 4..7 (lit_k8)
constexpr uint32_t kLitImage = kLitBitmap2 + 8192;
__host__ __device__ inline uint32_t lit_hash(uint32_t key) { return (key * 0x9E3779B1u) >> 16; }

// The reference's engine choice where it differs from the forward DFA
// (host/literal_sets.hpp): MatchType::Literal over the reference's literal
// sets (exec.rs:601-625) and DfaSuffix (exec.rs:725-794).  Literal lists:
// `n` literals, literal i = bytes[off[i] .. off[i + 1]), in the searcher's
// iteration order; matcher 0 = Empty (literals.rs:92-96: every search finds
// the empty string at its start).
struct LitListDev {
  const uint8_t *bytes;
  const uint32_t *off;
  uint32_t n;
  int32_t matcher;
};
// mt: host/literal_sets.hpp MatchTypeCode (0-2 the Literal types, 5 DfaSuffix)
enum { MT_LIT_UNANCHORED = 0, MT_LIT_ANCHORED_START = 1, MT_LIT_ANCHORED_END = 2 };
struct MatchDev {
  int32_t mt;             // MT_* code
  LitListDev pre, suf;    // nfa.prefixes, suffixes
  const uint8_t *lcs;     // suffixes.lcs() (DfaSuffix)
  uint32_t lcs_len;
};

// The forward DFA as the reference's lazy DFA walks it, for the one question
// where the walk and not the language decides: whether a search quits.  A
// regex with prefix literals jumps, whenever a step lands on the search's own
// start state, to the next prefix occurrence (dfa.rs:700-711, 1032-1037), so
// it never reads (never quits on, with a Unicode \b) the bytes in between.
// "The start state" is a state identity (dfa.rs:1196-1244: the flags and the
// instruction list), which minimisation loses: f holds the raw, unminimised
// automaton (full / eof / start and the id bounds only; hot = all = ustart1 =
// 0), whose start[flag index] is that state.  pre: dfa.prefixes (exec.rs:
// 308-311).  Built only for a regex that needs it (DevTables::skip_on).
struct SkipDfaDev {
  FwdDfaDev f;
  LitListDev pre;
};

struct RevDfaDev {
  const uint8_t *lds_image;   // hot table (same layout as FwdDfaDev::lds_image)
  uint32_t lds_bytes;
  uint32_t hot;
  const uint16_t *full;
  const uint8_t *eof;
  const uint16_t *start;
  uint32_t n_normal, n_match_end, dead, quit;
  uint32_t all;               // as FwdDfaDev::all
  uint32_t ustart1;           // as FwdDfaDev::ustart1
};

// Set DFA: the answer is the union of now_mask[s] over the states entered
// ([n_normal, n_match_end) have now_mask != 0) and eof_mask[final state].
struct SetDfaDev {
  const uint8_t *lds_image;
  uint32_t lds_bytes;
  uint32_t hot;
  const uint16_t *full;
  const uint64_t *eof_mask;
  const uint64_t *now_mask;
  uint64_t all;               // every pattern (early exit)
  const uint16_t *start;
  uint32_t n_normal, n_match_end, dead, quit;
};

// The set DFA built with stripped states, for the chunked scan of long
// haystacks (set_long.hip): strip[s] = s without the `.*?` prefix threads (no
// match starts from there on), reach[s] = the patterns any walk from s can
// still report (now_mask and eof_mask over every state reachable from s).
struct SetLongDev {
  SetDfaDev d;
  const uint16_t *strip;
  const uint64_t *reach;
};

// Set DFA in "core" form for large sets (host: build_set_cores): states that
// differ only in the matches their entry reports share a core; a transition
// (core, byte class) carries the next core and an output code.  Entries of
// the LDS table (hot cores [0, hot), sentinel row `hot`): bits 15..6 = next
// core (`hot` = leaves the LDS set), bits 5..0 = output code (0 none, 1..62 =
// pattern code-1 matched, 63 = consult gout).  Global tables cover all cores.
struct SetCoreDev {
  const uint8_t *lds_image;   // 256-byte class map, then (hot + 1) x K u16 entries
  uint32_t lds_bytes;
  uint32_t hot, K;
  const uint16_t *gcore;      // ncores x K next core
  const uint64_t *gout;       // ncores x K matches reported by the transition
  const uint64_t *eof;        // ncores: matches at the end of the text
  const uint16_t *start;      // 128 start cores
  uint64_t all;
  uint32_t dead, quit;        // quit = 0xFFFFFFFF if none
  uint32_t mt_off;            // byte offset in the LDS image of the 64 u64 code masks
  const uint16_t *mid;        // profile only: ncores x K mask id + 1 of gout (0: none)
};
hipError_t launch_set_cores(const BatchDev &b, const SetCoreDev &f, uint64_t *out, hipStream_t st, int cus);

hipError_t launch_core_profile(const BatchDev &b, const SetCoreDev &f, uint64_t count, unsigned int *visits,
                               unsigned int *mask_counts, hipStream_t st, int cus);

// Pike VM closure tables (host/nfa_build.hpp) on the device.
struct NfaDev {
  const uint32_t *leaves;     // 3 words per leaf: kind | lo << 8 | hi << 16, closure, slot
  const uint32_t *cl_off;     // closure CSR offsets
  const uint2 *entries;       // (leaf, cond | (1 + prev same-leaf entry) << 8)
  const uint32_t *perlw;      // Unicode word-character ranges (pairs), regex-syntax PERLW
  uint32_t perlw_n;
  uint32_t nleaves, root, nmatch;
  uint32_t anchored, single, looks, unicode_wb;
  uint32_t ncl_off, nentries;  // cl_off's and entries' lengths (the wave kernels stage them in LDS)
  const uint32_t *cl_info;     // per closure: its Bytes leaves' bytes (8 words), needed looks | Match << 8
  const uint32_t *cl_big;      // per closure: its bucket set (closures of > 64 entries), else ~0
  const uint32_t *cl_boff;     // per bucket set: 258 offsets into cl_sub (bytes 0-255, the text end)
  const uint2 *cl_sub;         // the buckets' entries (as `entries`, same-leaf links within the bucket)
  const uint32_t *save_off;   // per entry: CSR offsets into save_slot (Saves on its path)
  const uint16_t *save_slot;
};

// Per-wave working set of the Pike VM: stamp + two thread lists.
__host__ __device__ inline size_t nfa_wave_bytes(uint32_t nleaves) { return ((size_t)nleaves * 28 + 64 + 255) & ~(size_t)255; }
constexpr size_t kNfaLdsMax = 160 * 1024;   // a gfx950 workgroup may take the whole LDS

// mode: MODE_FIND / MODE_ISMATCH / MODE_SHORTEST, or MODE_SET.  fallback:
// only haystacks whose DFA result is the quit marker are (re)computed.
enum { MODE_SET = 3 };
hipError_t launch_pike(int mode, bool fallback, const BatchDev &b, const NfaDev &n, void *out, void *scratch,
                       hipStream_t st, int grid);

// Captures (exec.rs:524-596 read_captures_at; Pike VM with capture slots,
// pikevm.rs:237-352).  found: per haystack the forward/reverse DFA's
// (start, end), NONE or the quit marker; null when every haystack is searched
// whole from `start` (anchored-start programs).  slots: count x nslots u64,
// NONE = unset.  Per-wave working set: caps_wave_bytes (LDS when it fits).
// sk (or null) / r: where `found` holds the quit marker, the search is
// repeated with the reference's start-state prefix skip (SkipDfaDev), which
// may not quit: then its bounds cut the window as any DFA match's do.
__host__ __device__ inline size_t caps_wave_bytes(uint32_t nleaves, uint32_t nslots) {
  return ((size_t)nleaves * (16 * (size_t)nslots + 12) + 64 + 255) & ~(size_t)255;
}
hipError_t launch_captures(const BatchDev &b, const NfaDev &n, const uint64_t *found, uint64_t *slots,
                           uint32_t nslots, void *scratch, const SkipDfaDev *sk, const RevDfaDev &r, hipStream_t st,
                           int grid);

// captures_iter over the batched find_iter's match list (nfa_scan.hip
// caps_iter_kernel): moff (count + 1) / m (nm records) as below; row g of
// `rows` (nslots u64, NONE = unset) = the groups of match g, for the matches
// whose index within their haystack is below `limit`; diverged[h] (bytes,
// zeroed by the caller) set where a row's group 0 is not its match.  fq / r:
// the forward DFA when it can quit (else nullptr) and the reverse DFA, with
// which a failing row repeats the reference's search (a quit there takes the
// captures from the whole text); sk (or null): that search with the
// reference's start-state prefix skip, in fq's place.  scratch and grid as
// launch_captures.
hipError_t launch_captures_iter(const BatchDev &b, const NfaDev &n, const uint64_t *moff, const uint64_t *m,
                                uint64_t nm, uint64_t limit, uint64_t *rows, uint32_t nslots, uint8_t *diverged,
                                void *scratch, const FwdDfaDev *fq, const SkipDfaDev *sk, const RevDfaDev &r,
                                hipStream_t st, int grid);

// replacen with a `$` template over find_iter output and captures_iter rows
// (expand_scan.hip).  The compiled template (device): npieces records of 3
// u32 (0, offset into lits, length) | (1, group, 0); lit_total = the sum of
// the literal lengths.  seg / S: nm + 1 entries, olen: count + 1 (scratch);
// units / uoff: count + 1 entries, used for offset batches only.
struct ExpandTpl {
  const uint32_t *pieces;
  uint32_t npieces;
  const uint8_t *lits;
  uint64_t lit_total;
};
hipError_t launch_expand_plan(const BatchDev &b, const uint64_t *counts, const uint64_t *moff, const uint64_t *m,
                              uint64_t nm, uint64_t limit, const uint64_t *rows, uint32_t ns, const ExpandTpl &tp,
                              uint64_t *seg, uint64_t *S, uint64_t *olen, uint64_t *out_offsets, hipStream_t st);
hipError_t launch_expand_write(const BatchDev &b, const uint64_t *counts, const uint64_t *moff, const uint64_t *m,
                               uint64_t nm, uint64_t limit, const uint64_t *rows, uint32_t ns, const ExpandTpl &tp,
                               const uint64_t *S, const uint64_t *out_offsets, uint64_t *units, uint64_t *uoff,
                               uint8_t *out, uint64_t cap, hipStream_t st, int cus);

// replacen / split over find_iter output (replace_scan.hip).  counts / moff:
// matches per haystack and their exclusive sums; m: the records.
hipError_t exclusive_scan_u64(const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t st);
// shift: nm + 1 entries; one haystack with every match replaced holds the
// replacement starts there instead (the plan's output, the copy's input).
hipError_t launch_replace_plan(const BatchDev &b, const uint64_t *counts, const uint64_t *moff, const uint64_t *m,
                               uint64_t limit, uint64_t rep_len, int64_t *shift, uint64_t *out_len, hipStream_t st,
                               int cus,
                               uint64_t nm);
hipError_t launch_replace_copy(const BatchDev &b, const uint64_t *ooff, const uint64_t *counts, const uint64_t *moff,
                               const uint64_t *m, const int64_t *shift, uint64_t limit, const uint8_t *rep,
                               uint64_t rep_len, uint8_t *out, uint64_t cap, uint64_t total_hint, hipStream_t st,
                               int cus,
                               uint64_t nm);
// replace_all of a regex whose matches are single bytes of one class over
// one 16-byte aligned haystack (replace_scan.hip); hipErrorNotSupported if
// the replacement is empty or longer than 64 bytes.
// sw1 / sw2: a class of at most two bytes (byte * 0x01010101; sw2 = sw1 for
// one byte), else 0 (the cls table).
hipError_t launch_replace_class(const uint8_t *hay, uint64_t n, const uint8_t *cls, const uint8_t *rep,
                                uint32_t rep_len, uint8_t *out, uint64_t cap, uint64_t *ooff, uint64_t *total,
                                hipStream_t st, int cus, uint32_t sw1, uint32_t sw2);
// A chain of one-byte-class replace_all calls (replace_scan.hip): step i
// reads step i - 1's output, buffers alternate out0 / out1, lengths (device,
// steps + 1) = the input length, then each step's output length; sw[i] = step
// i's class as up to two SWAR bytes ({0, 0}: wider, counted from cls[i]).
// The same chain as one byte -> string map composed on the host (blob:
// |F(x)| 256 u8, offsets 256 u16, changed-byte indices 256 u8 (0xFF: F(x) =
// x; nact changed), the strings (<= 4096 bytes), per step |F_i(x)| - 1 as
// 256 u32); the final text to out.
constexpr uint32_t kHMapPoolMax = 4096;
hipError_t launch_replace_hmap(const uint8_t *in, uint64_t n, int steps, const uint8_t *blob, uint32_t pool_len,
                               uint32_t nact, uint8_t *out, uint64_t cap, uint64_t *lengths, hipStream_t st,
                               int cus);
// nrep[i] = the bytes of step i's replacement in step i + 1's class.
hipError_t launch_replace_class_chain(const uint8_t *hay, uint64_t n0, int steps, const uint8_t *const *cls,
                                      const uint8_t *const *rep, const uint32_t *rep_len, const uint32_t (*sw)[2],
                                      const uint32_t *nrep, uint8_t *out0, uint8_t *out1, uint64_t cap,
                                      uint64_t *lengths, hipStream_t st, int cus);
hipError_t launch_split(const BatchDev &b, const uint64_t *counts, const uint64_t *moff, const uint64_t *m,
                        uint64_t lim, uint64_t *fields, uint64_t *foff, uint64_t *pieces, uint64_t cap,
                        uint64_t nmatches, hipStream_t st, int cus);

// Batched find_iter (iter_scan.hip).  counts: per haystack; matches:
// (start, end) pairs, the first `cap` written; total: number of matches.
struct IterOut {
  uint64_t *counts;
  uint64_t *matches;
  uint64_t cap;
  uint64_t *total;
};
// A span of one haystack (sharded / streamed find_iter): the iteration owns
// the matches starting before `hi`; entry (device, 3 u64: next, last match,
// fresh) = the state the previous span left (fresh: start at b.start); exit
// (device, 3 u64) receives the state at hi (fresh = equivalent to a fresh
// iteration starting at hi).
struct IterSpan {
  uint64_t hi;
  const uint64_t *entry;
  uint64_t *exit;
  uint64_t tail;  // the text length when the span runs to the end (hi = ~0), else ~0
};
// find_iter of a C+ regex (FwdDfaDev::run_cls, run_iter.hip): fixed-stride
// batches whose searched bytes are 16-byte aligned (hipErrorNotSupported
// otherwise); *quit = a byte of the quit class was read (can_quit: the
// flag is read back) and the results are not the answer.
// cp: a Unicode class's code point bitmap (class bit 2 on bytes >= 0x80),
// else null.
hipError_t launch_find_iter_runs(const BatchDev &b, const uint8_t *cls, const uint32_t *cp, const IterOut &o,
                                 hipStream_t st, int cus, bool can_quit, bool *quit);
// find_iter with one wavefront per haystack (iter_scan.hip): per search the
// DFA on one lane (f; null: no DFA) and the Pike VM on the wave where it quits
// or is absent; mt: the reference's Literal / DfaSuffix searches instead.
hipError_t launch_find_iter_wave(const BatchDev &b, const FwdDfaDev *f, const RevDfaDev &r, const NfaDev &nf,
                                 const IterOut &o, hipStream_t st, int cus, const IterSpan *span = nullptr,
                                 const MatchDev *mt = nullptr);
// What the chunked find_iter does when a search's DFA quits (f.can_quit).
struct IterQuit {
  enum Kind {
    // Nothing: for a DFA that cannot quit (hipErrorInvalidValue if it can).
    None,
    // *flag is set when a search quit, the outputs then being void: the
    // caller runs the wave path.  Reads the flag back, so the call
    // synchronises the stream.  A DFA that cannot quit leaves *flag alone.
    ReadBack,
    // word (device, zeroed): a quit ORs 1 into it and the passes after the
    // speculative one run gated on it staying 0 -- nothing is read back, and
    // the caller enqueues its fallback gated on the word being set.  Needs a
    // DFA that can quit, an ungated batch and no span.
    DeviceWord,
    // The units whose searches quit are served by the Pike VM (nfa) on a wave
    // inside the iteration; nothing is read back.  No span.
    WaveServed,
  } kind = None;
  union {  // the selected kind's
    bool *flag = nullptr;
    uint32_t *word;
    const NfaDev *nfa;
  };
  static IterQuit none() { return IterQuit(); }
  static IterQuit read_back(bool *flag) { IterQuit q; q.kind = ReadBack; q.flag = flag; return q; }
  static IterQuit device_word(uint32_t *word) { IterQuit q; q.kind = DeviceWord; q.word = word; return q; }
  static IterQuit wave_served(const NfaDev *nfa) { IterQuit q; q.kind = WaveServed; q.nfa = nfa; return q; }
};
// Ragged unit geometry of an offset batch (iter_device.hpp Geo::uoff):
// haystack h, searched over span_h = max(0, len_h - start) bytes, has
// max(1, ceil(span_h / chunk)) units.
struct IterRagged {
  const uint64_t *uoff;  // device, count + 1: exclusive sums of the units per haystack
  uint64_t nunits;       // uoff[count], read back by the caller
  uint64_t total;        // the sum of the spans (sizes the slots per unit)
};
// stats (device, 2 u64) = the longest span of an offset batch and the spans' sum.
hipError_t launch_iter_span_stats(const BatchDev &b, uint64_t *stats, hipStream_t st, int cus);
// nk (device scratch, count + 1) = the units per haystack, uoff = their exclusive sums.
hipError_t launch_iter_ragged_units(const BatchDev &b, uint64_t chunk, uint64_t *nk, uint64_t *uoff, hipStream_t st);
// The chunked speculative find_iter (iter_scan.hip): units of `chunk` bytes;
// rag: an offset batch in its ragged geometry (built with the same chunk; no
// span), else one unit per haystack of an offset batch.
hipError_t launch_find_iter_chunked(const BatchDev &b, const FwdDfaDev &f, const RevDfaDev &r, uint64_t chunk,
                                    const IterOut &o, hipStream_t st, int cus, const IterQuit &quit,
                                    const IterSpan *span = nullptr, const IterRagged *rag = nullptr);
// The k-mer probe engine of launch_find_iter_multi: the regexes' strings all
// have one length len <= 8 over an alphabet of at most 4 bytes whose codes
// (b >> shift) & 3 are distinct.  bitmap: 2048 u32, bit c set iff the L-mer
// with code c (2 bits per byte, first byte lowest) is a string of some regex;
// mask: 4^len u16, regex q's bit set iff its strings hold it; lut / present:
// the byte of each code (verification of probe hits on the text).
struct KmerDev {
  const uint32_t *bitmap;
  const uint16_t *mask;
  const uint16_t *hmask;  // 1024: mask[c] at (c * hmul) >> 22, injective on the string codes
  uint32_t hmul;
  uint32_t hglobal;       // 1: no injective hash was found; hits read mask[code] from global memory
  uint32_t vlut;  // byte k: the alphabet byte of code k (absent code: a byte of another code)
  uint32_t shift, lut, present, cmask;
  uint64_t len;
};
// Several Shift-And regexes over one span in one speculative pass, then each
// regex's own passes; hipErrorNotSupported (nothing launched) if they do not
// qualify (iter_scan.hip).  km (may be null): the k-mer probe engine for the
// pass instead of the Shift-And words.
hipError_t launch_find_iter_multi(const BatchDev &b, int nre, const FwdDfaDev *const *f, const RevDfaDev *const *r,
                                  uint64_t chunk, const IterOut *o, hipStream_t st, int cus, const IterSpan *spn,
                                  const KmerDev *km = nullptr);

// One search per haystack over few long fixed-stride haystacks, chunked
// (long_scan.hip); f must be the find_iter DFA (with strip).
hipError_t launch_long_scan(int mode, const BatchDev &b, const FwdDfaDev &f, const RevDfaDev &r, uint64_t chunk,
                            void *out, hipStream_t st, int cus);

// The same search over the long haystacks of an offset batch that the lane
// kernels deferred (long_scan.hip): b.defer = the header that
// launch_long_defer_init set (a list of `cap` haystacks) and the list the
// lane kernel filled, in a block of long_ragged_bytes(mode, cap, lanes).  The
// chunk is made on the device: max(floor, deferred bytes / lanes), rounded
// with odd_lines if `round`; the units and the scan follow in fixed grids
// (find's winner per haystack is written by its last unit to finish).  rec
// (device-visible host memory, or null) receives the haystacks, the chunk and
// the units.  Enqueues only.
size_t long_ragged_bytes(int mode, uint64_t cap, uint64_t lanes);
hipError_t launch_long_defer_init(unsigned long long *defer, uint64_t cap, hipStream_t st);
hipError_t launch_long_ragged(int mode, const BatchDev &b, uint64_t cap, const FwdDfaDev &f, const RevDfaDev &r,
                              uint64_t floor, bool round, uint64_t lanes, uint64_t *rec, void *out, hipStream_t st,
                              int cus);
// The haystacks, chunk and units of the last launch_long_ragged of this
// process (rure_amd_last_long_units; dispatch.cpp): waits for the event the
// call recorded behind its kernels.
uint64_t last_long_units(uint64_t *haystacks, uint64_t *chunk);
// A find / is_match / shortest_match call over an offset batch that took
// another path: that diagnostic reads 0.
void note_long_none();

hipError_t launch_dfa_fwd(int mode, const BatchDev &b, const FwdDfaDev &f, const RevDfaDev &r, void *out,
                          hipStream_t st, int grid);
// find / is_match / shortest_match of a batch under the reference's Literal
// or DfaSuffix match type (match_types.hip): one lane per haystack, global
// DFA tables for DfaSuffix's reverse / forward scans; same output layout and
// quit markers as launch_dfa_fwd (the Pike VM pass resolves quits).
hipError_t launch_lane_search(int mode, const BatchDev &b, const MatchDev &m, const FwdDfaDev &f,
                              const RevDfaDev &r, void *out, hipStream_t st, int cus);
// DfaSuffix over few long fixed-stride haystacks (match_types.hip): answers
// into out where the reverse suffix scans decide; status[h] = 3 where the
// reference falls back to the forward DFA (the caller runs it).  Needs a
// longest common suffix that cannot overlap itself.
// find_iter of a DfaSuffix regex over few long fixed-stride haystacks
// (match_types.hip): every suffix occurrence's slice scanned once, each
// search's match and successor per occurrence, the iteration's searches
// marked by pointer doubling.  hipErrorNotSupported: nothing written (a
// reverse scan quit), the caller runs the wave path.
hipError_t launch_suffix_iter(const BatchDev &b, const MatchDev &m, const FwdDfaDev &f, const RevDfaDev &r,
                              uint64_t chunk, const IterOut &o, hipStream_t st, int cus);
hipError_t launch_suffix_long(int mode, const BatchDev &b, const MatchDev &m, const FwdDfaDev &f,
                              const RevDfaDev &r, uint64_t chunk, void *out, uint8_t *status, hipStream_t st,
                              int cus);
// MatchType::Literal (exec.rs:601-625, 1148-1166) for MODE_FIND / MODE_ISMATCH
// batches of a regex that is a finite string set: f = the find_iter DFA
// (lit_n > 0); same output layout as launch_dfa_fwd.
hipError_t launch_lit_find(int mode, const BatchDev &b, const FwdDfaDev &f, void *out, hipStream_t st);
// Which engine answered the last batched launch of this process
// (rure_amd_last_fwd_path; dispatch.cpp): the launchers and the dispatch note
// it, tests and the bench assert it.
int last_fwd_path();
void note_fwd_path(rure_amd_path path);
// The units and haystacks of the last launch_find_iter_chunked of this
// process (rure_amd_last_iter_units; 0, 0 before the first).
uint64_t last_iter_units(uint64_t *haystacks);
void note_iter_units(uint64_t units, uint64_t haystacks);
// The units, haystacks and unit size of the last chunked RegexSet launch
// (rure_amd_last_set_units; all 0 after a set call that did not chunk).
uint64_t last_set_units(uint64_t *haystacks, uint64_t *chunk);
void note_set_units(uint64_t units, uint64_t haystacks, uint64_t chunk);
// The units, haystacks, unit size, rounds and whether the Pike VM answered
// instead, of the last chunked on-demand DFA call (rure_amd_last_lazy_long;
// all 0 after a regex search that did not take that path).
uint64_t last_lazy_long(uint64_t *haystacks, uint64_t *chunk, uint32_t *rounds, uint32_t *fell_back);
// The last chunked find_iter on the on-demand DFA (rure_amd_last_lazy_iter_long;
// all 0 after a find_iter that took another path): v = units, haystacks, unit
// size, rounds summed over the passes, repaired units, resume passes, fell back.
void last_lazy_iter_long(uint64_t v[7]);
// Kernel timer (rure_amd_kernel_timer): HIP event pairs around bracketed launches.
void ktimer_begin(hipStream_t st);
void ktimer_end(hipStream_t st);
int ktimer_set(int on);
double ktimer_read(uint64_t *launches);
// Multi-GPU gather (gather_scan.hip): records (3 u64: base + haystack, start,
// end) of the haystacks whose find result holds a match, first `cap`; *count.
hipError_t launch_compact_matches(const uint64_t *found, uint64_t n, uint64_t base, uint64_t *rec, uint64_t cap,
                                  uint64_t *count, hipStream_t st);
// find_iter from the batched find result when a haystack holds at most that
// match (gather_scan.hip): counts, records, total as IterOut's.
hipError_t launch_find_to_iter(const uint64_t *found, uint64_t n, uint64_t *counts, uint64_t *matches, uint64_t cap,
                               uint64_t *total, hipStream_t st);
// dst[i * words + w] = src (u8 0/1 or u64 mask) of haystack i (gather_scan.hip).
hipError_t launch_mask_column(const uint8_t *s8, const uint64_t *s64, uint64_t n, uint64_t *dst, uint64_t words,
                              uint64_t w, hipStream_t st);
// MatchType::DfaAnchoredReverse (exec.rs:671-688, 395-406, 442-453): the
// reverse DFA over text[start..] from its end; same output layout and quit
// markers as launch_dfa_fwd.
hipError_t launch_dfa_anchored_rev(int mode, const BatchDev &b, const RevDfaDev &r, void *out, hipStream_t st,
                                   int grid);
hipError_t launch_dfa_set(const BatchDev &b, const SetDfaDev &f, uint64_t *out, hipStream_t st, int grid);
// RegexSet masks over few long fixed-stride haystacks, chunked (set_long.hip):
// out[h] is zeroed on the stream and the units OR their patterns into it.
// *units = the units the batch was cut into.
hipError_t launch_set_long(const BatchDev &b, const SetLongDev &f, uint64_t chunk, uint64_t *out, hipStream_t st,
                           int cus, uint64_t *units);

// The matching records of one delimited text (records.hip; the ownership rule:
// records_device.hpp).  The text is cut into units of `chunk` bytes; every
// launch runs on a grid fixed by `length`, nothing is read back.
struct RecordsScratch {
  uint32_t *sel_bits;    // bit p: the record starting at p is selected (before INVERT); (length + 31) / 32 words
  uint32_t *quit_bits;   // bit p: the DFA quit on the record starting at p (left to the Pike VM)
  uint32_t *quit_word;   // raised when any record quit
  uint32_t *owned;       // per unit (+ 1 entry): the records it owns
  uint32_t *selected;    // per unit (+ 1 entry): those with their bit in sel_bits
  uint64_t *owned_off;   // their exclusive sums (units + 1 entries)
  uint64_t *selected_off;
};
// The layout of one scratch block holding it all: its size, and the bytes
// from its start that must be zero before the scan (the bitmaps and the word).
size_t records_scratch_bytes(uint64_t length, uint64_t units, size_t *zeroed);
RecordsScratch records_scratch_at(void *block, uint64_t length, uint64_t units);
// The scan: one lane per unit walks its records through f (is_match from each
// record's start; f null: no eager DFA, every record is marked as quit).
hipError_t launch_records_scan(const uint8_t *text, uint64_t length, uint8_t delim, uint64_t chunk,
                               const FwdDfaDev *f, const RecordsScratch &s, hipStream_t st, int cus);
// The Pike VM over the records whose bit is in quit_bits (returns at once
// while quit_word is 0): sets sel_bits, adds to `selected` and to *served
// (may be null).  scratch: the waves' lists when they do not fit the LDS
// (grid * nfa_wave_bytes), else null.
int records_pike_grid(uint64_t length, const NfaDev &n, int cus);
hipError_t launch_records_pike(const uint8_t *text, uint64_t length, uint8_t delim, uint64_t chunk, const NfaDev &n,
                               const RecordsScratch &s, unsigned long long *served, void *scratch, hipStream_t st,
                               int grid);
// After scan_counts over owned and selected: *nrecords, *total, and the
// selected (invert: the others) records' (start, end) and numbers (may be
// null) below cap, in text order.
hipError_t launch_records_write(const uint8_t *text, uint64_t length, uint8_t delim, uint64_t chunk, bool invert,
                                const RecordsScratch &s, uint64_t *nrecords, uint64_t *total, uint64_t *records,
                                uint64_t *numbers, uint64_t cap, hipStream_t st, int cus);
// The units and unit size of the last record scan (rure_amd_last_records).
uint64_t last_records(uint64_t *chunk);
void note_records(uint64_t units, uint64_t chunk);

// An automaton past the u16 tables (more than 65535 states, host
// kBigDfaRawStates budget): u32 next states in column form, trans[s * ncol +
// colmap[b]], same state numbering as FwdDfaDev / RevDfaDev (no quit state:
// programs with a Unicode word boundary keep the Pike VM).  The first `hot`
// rows are staged in LDS (states in BFS order from the start states).
struct BigDfaDev {
  const uint32_t *trans;
  const uint8_t *colmap;      // 256 bytes
  const uint8_t *eof;         // nstates
  const uint32_t *start;      // 128 start states by flag index
  uint32_t ncol, nstates, hot, n_normal, n_match_end, dead, ustart1;
};
// find / is_match / shortest_match over a batch, one lane per haystack:
// find_dfa_forward (exec.rs:632-662) with the big forward and reverse DFAs.
hipError_t launch_big_dfa(int mode, const BatchDev &b, const BigDfaDev &f, const BigDfaDev &r, void *out,
                          hipStream_t st, int cus);
// Rows of a big forward DFA the kernel holds in LDS.
uint32_t big_dfa_hot_rows(uint32_t ncol, uint32_t nstates);

// A forward DFA built on demand (host LazyDfa): entries are next-state ids,
// | 0x80000000 when that state carries the match flag, 0x7FFFFFFF for a row
// not built yet; id 0 is the dead state.  The first `hot` rows sit in LDS.
// A set's automaton: the bit marks a state whose entry reports matches, now /
// eof_mask are the patterns reported on entering a state / at the end of the
// text from it (null for a regex).
struct LazyDfaDev {
  const uint32_t *trans;
  const uint8_t *colmap;      // 256 bytes
  const uint8_t *eof;         // per state
  const uint32_t *start;      // 128 start entries by flag index
  uint32_t ncol, hot;
  const uint64_t *now;        // per state (sets)
  const uint64_t *eof_mask;   // per state (sets)
  // per state: the twin without the `.*?` prefix threads that a chunked scan
  // steps into at a unit's cut (an id without the match bit, 0 = dead,
  // 0x7FFFFFFF = not computed yet); null until a chunked call made a link
  const uint32_t *strip;
  // per state (sets): the patterns a walk from the state can still report, or
  // more (0 for dead); the chunked set scan leaves a unit past its cut on it
  const uint64_t *reach;
};
// A lane stopped at a row not built yet: haystack, position of the byte it
// needs, the last match end so far (~0: none; a set: the mask collected so
// far), the state.
struct LazyPark {
  uint64_t h, p, last;
  uint32_t s, pad;
};
// One round of a batched forward scan on a LazyDfaDev (find: the reverse
// DFA r gives the start, exec.rs:632-662): lanes are the haystacks (in =
// nullptr) or the parked lanes of the previous round; lanes that need a
// missing row are appended to park (*npark).
hipError_t launch_lazy_dfa(int mode, const BatchDev &b, const LazyDfaDev &f, const RevDfaDev &r, const LazyPark *in,
                           uint64_t nin, LazyPark *park, unsigned long long *npark, void *out, hipStream_t st,
                           int cus);
// One round of RegexSet matches (many_matches_at, exec.rs:998-1038) on a
// set's LazyDfaDev: out[h] = the mask of the patterns matching haystack h,
// written by the round in which its lane finishes; `all` = every pattern of
// the set (a lane stops once it has them all).  Lanes and parking as above.
hipError_t launch_lazy_set(const BatchDev &b, const LazyDfaDev &f, uint64_t all, const LazyPark *in, uint64_t nin,
                           LazyPark *park, unsigned long long *npark, uint64_t *out, hipStream_t st, int cus);
uint32_t lazy_dfa_hot_rows(uint32_t ncol);
// A unit of the chunked scan on a LazyDfaDev (lazy_long_kernel) stopped: the
// unit, the position of the byte it needs, its last match end so far (~0:
// none), the state, and where in the unit's walk it stood.
enum { kLazyLongBefore = 0, kLazyLongAtCut = 1, kLazyLongAfter = 2 };
struct LazyLongPark {
  uint64_t u, p, last;
  uint32_t s, phase;
};
// find / is_match / shortest_match over few long fixed-stride haystacks on a
// regex's LazyDfaDev, cut into units of `chunk` bytes as launch_long_scan
// cuts them: unit [c0, c1) walks from c0, steps into strip[state] at c1 - 1
// and walks on until the automaton dies.  One round: lanes are the units (in
// = nullptr) or the units parked by the previous round; a unit that needs a
// missing row, or a link not computed (phase kLazyLongAtCut), is appended to
// park (*npark).  is_match stores 1 into out[h] and shortest_match takes the
// minimum into out[h], both initialised by the caller; find keeps the unit's
// match end in ures[u] and the smallest matching unit in best[h] (initialised
// to ~0), which launch_lazy_long_finish turns into out after the last round
// (the reverse DFA r gives the winner's start).
hipError_t launch_lazy_long(int mode, const BatchDev &b, const LazyDfaDev &f, uint64_t chunk, const LazyLongPark *in,
                            uint64_t nin, LazyLongPark *park, unsigned long long *npark, uint64_t *ures,
                            unsigned long long *best, hipStream_t st, int cus);
hipError_t launch_lazy_long_finish(const BatchDev &b, const RevDfaDev &r, const uint64_t *ures,
                                   const unsigned long long *best, uint64_t *out, hipStream_t st, int cus);
// RegexSet matches (many_matches_at) over few long fixed-stride haystacks on
// a set's LazyDfaDev, cut into units as launch_set_long cuts them; rounds,
// lanes and parking as launch_lazy_long (the mask a parked unit has collected
// travels in LazyLongPark::last).  out[h], zeroed by the caller before the
// first round, is only ever ORed into; `all` = every pattern of the set.
hipError_t launch_lazy_set_long(const BatchDev &b, const LazyDfaDev &f, uint64_t all, uint64_t chunk,
                                const LazyLongPark *in, uint64_t nin, LazyLongPark *park, unsigned long long *npark,
                                uint64_t *out, hipStream_t st, int cus);
// The units per haystack and in all for that geometry.
inline uint64_t lazy_long_units(const BatchDev &b, uint64_t chunk) {
  const uint64_t span = b.length > b.start ? b.length - b.start : 0;
  return b.count * (span <= chunk ? 1 : (span + chunk - 1) / chunk);
}
// A find_iter lane stopped at a row not built yet: the haystack, the
// iteration's state (ip: the start of the search under way, lm: the end of
// the last match or ~0, count: the matches so far) and that search's (p: the
// position of the byte it needs, last: its last match end so far or ~0, s:
// the state).
struct LazyIterPark {
  uint64_t h, ip, lm, p, last, count;
  uint32_t s, pad;
};
// The batched find_iter (re_trait.rs:197-221) on a regex's LazyDfaDev, one
// lane per haystack.  The count form runs in rounds as launch_lazy_dfa:
// counts[h] (u32) is written by the round in which haystack h's lane
// finishes.  The write form runs once when no lane is parked any more, over
// off = the exclusive sums of counts: match k of haystack h goes to record
// off[h] + k when that is below cap.  *flag (device, zeroed) is set should
// the write form meet a row not built: its records are then not the answer.
hipError_t launch_lazy_iter_count(const BatchDev &b, const LazyDfaDev &f, const RevDfaDev &r, const LazyIterPark *in,
                                  uint64_t nin, LazyIterPark *park, unsigned long long *npark, uint32_t *counts,
                                  hipStream_t st, int cus);
hipError_t launch_lazy_iter_write(const BatchDev &b, const LazyDfaDev &f, const RevDfaDev &r, const uint64_t *off,
                                  uint64_t *matches, uint64_t cap, uint32_t *flag, hipStream_t st, int cus);
// The tail of the one-lane-per-haystack find_iter engines (iter_scan.hip):
// off[0..n] = the exclusive sums of counts[0..n) (u32; off[n] = their
// total), and from them o.counts per haystack and o.total.
hipError_t scan_counts(const uint32_t *counts, uint64_t *off, uint64_t n, hipStream_t st);
// (nk: off holds nk entries per haystack, the units of a chunked engine)
hipError_t launch_iter_counts(const BatchDev &b, const uint64_t *off, const IterOut &o, hipStream_t st, int cus,
                              uint64_t nk = 1);

// find_iter over few long fixed-stride haystacks on a regex's LazyDfaDev, cut
// into units as launch_lazy_long cuts them (lazy_iter_long_kernel; the records
// and the resolve rule: lazy_iter_long_device.hpp).  A unit's iteration runs
// from an entry state and owns the matches that start before its cut: every
// search is bounded by the cut as lazy_long_kernel bounds it.  A lane stopped
// at a row not built yet, or at the cut on a link not computed (phase
// kLazyLongAtCut): the unit, the iteration's state (ip: the start of the
// search under way, lm: the end of the last match or ~0, count: the matches
// so far) and that search's (p: the position of the byte it needs, last: its
// last match end so far or ~0, s: the state, phase: where in the bounded
// search it stood).
struct LazyIterLongPark {
  uint64_t u, ip, lm, count, p, last;
  uint32_t s, phase;
};
// Where a round's fresh lanes take their entries from, and what they are:
enum {
  kLilFresh = 0,  // every unit, from (c0, none)
  kLilAfter = 1,  // every unit but a haystack's first whose predecessor's record in `ent` has no clean
                  // exit, from that exit; a unit that exit steps over gets its record without a walk,
                  // every other unit none (flags 0).  stats[1] += the records made.
  kLilList = 2,   // the units of `todo` (ntodo of them), from the states listed; their records are
                  // marked kLilRun
  kLilFinal = 3,  // (write form) every unit whose record in `ent` has matches, from that record's entry
};
// One round of the count form: lanes are the fresh ones `from` names (in =
// nullptr) or the lanes parked by the previous round; a finished lane writes
// the unit's record (entry, matches owned, exit, clean) into out[u].
hipError_t launch_lazy_iter_long_count(const BatchDev &b, const LazyDfaDev &f, const RevDfaDev &r, uint64_t chunk,
                                       int from, const LilRec *ent, const LilTodo *todo, uint64_t ntodo,
                                       const LazyIterLongPark *in, uint64_t nin, LazyIterLongPark *park,
                                       unsigned long long *npark, LilRec *out, unsigned long long *stats,
                                       hipStream_t st, int cus);
// The write form, once: match k of unit u goes to record off[u] + k when that
// is below cap.  *flag (device, zeroed) is set should it meet a row or link
// not built.
hipError_t launch_lazy_iter_long_write(const BatchDev &b, const LazyDfaDev &f, const RevDfaDev &r, uint64_t chunk,
                                       const LilRec *fin, const uint64_t *off, uint64_t *matches, uint64_t cap,
                                       uint32_t *flag, hipStream_t st, int cus);
// Pass C on the device.  first: the parallel pass (fin, changed[u], walk
// zeroed) before the walkers; else the walkers resume.  A walker that needs a
// unit run appends it to todo (stats[0] = their number, zeroed by the
// caller).  ucounts[u] = fin[u].count for every unit, ucounts[nunits] = 0.
hipError_t launch_lazy_iter_long_resolve(const BatchDev &b, uint64_t chunk, bool first, const LilRec *spec,
                                         const LilRec *fix, LilRec *fin, uint8_t *changed, LilWalk *walk,
                                         LilTodo *todo, unsigned long long *stats, hipStream_t st, int cus);
hipError_t launch_lazy_iter_long_counts(const BatchDev &b, uint64_t chunk, const LilRec *fin, uint32_t *ucounts,
                                        hipStream_t st, int cus);

// Scratch device memory for the scans, cached by the library (scratch.cpp):
// a freed block is kept with an event recorded on the freeing stream and
// reused, after a wait on that event, by the next allocation of at most twice
// its size on any stream of the device — freeing to the driver (hipFree,
// hipFreeAsync) waits for queued work: 1-2 ms host stalls, one per freed
// scratch, made the C3 variant phase spend more host time freeing than the
// GPU spent scanning.  The cache is bounded and released on request
// (rure_amd_release_scratch).  Same signatures as hipMallocAsync /
// hipFreeAsync (the memory is usable on any stream once the call returns).
hipError_t scratch_malloc(void **p, size_t bytes, hipStream_t st);
hipError_t scratch_free(void *p, hipStream_t st);

// One scratch block, freed (stream-ordered) when its owner's scope ends,
// whichever return is taken; reset() frees it sooner.  The status of
// scratch_free is dropped: it fails only for a pointer that is not a scratch
// block, which a Scratch never holds.
template <class T = void>
class Scratch {
 public:
  Scratch() = default;
  Scratch(Scratch &&o) noexcept : p_(o.p_), st_(o.st_) { o.p_ = nullptr; }
  Scratch &operator=(Scratch &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, st_ = o.st_;
      o.p_ = nullptr;
    }
    return *this;
  }
  Scratch(const Scratch &) = delete;
  Scratch &operator=(const Scratch &) = delete;
  ~Scratch() { reset(); }
  // `bytes` of scratch for work on `st` (a block held before is freed first)
  hipError_t alloc(size_t bytes, hipStream_t st) {
    reset();
    st_ = st;
    return scratch_malloc((void **)&p_, bytes, st);
  }
  void reset() {
    if (p_) (void)scratch_free(p_, st_);
    p_ = nullptr;
  }
  T *get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  T *p_ = nullptr;
  hipStream_t st_ = nullptr;
};

}  // namespace rure_amd
