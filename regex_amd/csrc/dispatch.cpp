// The reference's engine dispatch over batches (src/exec.rs:382-420, 473-514,
// 998-1038, re_trait.rs:197-221): which kernel answers which search, the DFA
// -> quit -> Pike VM fallback, sets in 64-pattern groups, the find_iter
// passes and the k-mer table cache.
#include "runtime.hpp"

namespace rure_amd {

// rure_amd_last_fwd_path: one value for the whole process, touched only here.
static std::atomic<int> g_last_fwd_path{RURE_AMD_PATH_NONE};
int last_fwd_path() { return g_last_fwd_path.load(); }
void note_fwd_path(rure_amd_path path) { g_last_fwd_path.store(path); }

// rure_amd_last_iter_units: likewise (the pair under one lock).
static std::mutex g_iter_units_mu;
static uint64_t g_iter_units[2] = {0, 0};
uint64_t last_iter_units(uint64_t *haystacks) {
  std::lock_guard<std::mutex> g(g_iter_units_mu);
  if (haystacks) *haystacks = g_iter_units[1];
  return g_iter_units[0];
}
void note_iter_units(uint64_t units, uint64_t haystacks) {
  std::lock_guard<std::mutex> g(g_iter_units_mu);
  g_iter_units[0] = units;
  g_iter_units[1] = haystacks;
}

// rure_amd_last_set_units: likewise (the host knows the geometry).
static std::mutex g_set_units_mu;
static uint64_t g_set_units[3] = {0, 0, 0};
uint64_t last_set_units(uint64_t *haystacks, uint64_t *chunk) {
  std::lock_guard<std::mutex> g(g_set_units_mu);
  if (haystacks) *haystacks = g_set_units[1];
  if (chunk) *chunk = g_set_units[2];
  return g_set_units[0];
}
void note_set_units(uint64_t units, uint64_t haystacks, uint64_t chunk) {
  std::lock_guard<std::mutex> g(g_set_units_mu);
  g_set_units[0] = units;
  g_set_units[1] = haystacks;
  g_set_units[2] = chunk;
}

// rure_amd_last_records: likewise (units, chunk).
static std::mutex g_records_mu;
static uint64_t g_records[2] = {0, 0};
uint64_t last_records(uint64_t *chunk) {
  std::lock_guard<std::mutex> g(g_records_mu);
  if (chunk) *chunk = g_records[1];
  return g_records[0];
}
void note_records(uint64_t units, uint64_t chunk) {
  std::lock_guard<std::mutex> g(g_records_mu);
  g_records[0] = units;
  g_records[1] = chunk;
}

// rure_amd_last_lazy_long: likewise (units, haystacks, chunk, rounds, fell back).
static std::mutex g_lazy_long_mu;
static uint64_t g_lazy_long[5] = {0, 0, 0, 0, 0};
uint64_t last_lazy_long(uint64_t *haystacks, uint64_t *chunk, uint32_t *rounds, uint32_t *fell_back) {
  std::lock_guard<std::mutex> g(g_lazy_long_mu);
  if (haystacks) *haystacks = g_lazy_long[1];
  if (chunk) *chunk = g_lazy_long[2];
  if (rounds) *rounds = (uint32_t)g_lazy_long[3];
  if (fell_back) *fell_back = (uint32_t)g_lazy_long[4];
  return g_lazy_long[0];
}
static std::atomic<bool> g_lazy_long_any{false};  // the record is not all 0
static void note_lazy_long(uint64_t units, uint64_t haystacks, uint64_t chunk, uint32_t rounds, bool fell_back) {
  if (!units && !g_lazy_long_any.load(std::memory_order_relaxed)) return;  // (nothing to clear: no lock per search)
  std::lock_guard<std::mutex> g(g_lazy_long_mu);
  g_lazy_long_any.store(units != 0, std::memory_order_relaxed);
  const uint64_t v[5] = {units, haystacks, chunk, rounds, fell_back ? 1u : 0u};
  memcpy(g_lazy_long, v, sizeof(v));
}

// rure_amd_last_lazy_iter_long: likewise (units, haystacks, chunk, rounds,
// repaired units, resume passes, fell back).
static std::mutex g_lazy_iter_long_mu;
static uint64_t g_lazy_iter_long[7] = {0, 0, 0, 0, 0, 0, 0};
static std::atomic<bool> g_lazy_iter_long_any{false};  // the record is not all 0
void last_lazy_iter_long(uint64_t v[7]) {
  std::lock_guard<std::mutex> g(g_lazy_iter_long_mu);
  memcpy(v, g_lazy_iter_long, sizeof(g_lazy_iter_long));
}
static void note_lazy_iter_long(const uint64_t v[7]) {
  if (!v[0] && !g_lazy_iter_long_any.load(std::memory_order_relaxed)) return;  // (nothing to clear)
  std::lock_guard<std::mutex> g(g_lazy_iter_long_mu);
  g_lazy_iter_long_any.store(v[0] != 0, std::memory_order_relaxed);
  memcpy(g_lazy_iter_long, v, sizeof(g_lazy_iter_long));
}

// rure_amd_last_long_units: the deferred long scan's figures (haystacks,
// chunk, units) are made on the device, so its geometry kernel writes them
// into one pinned record of the process and each call records an event behind
// its kernels; the diagnostic waits for the event of the last call.
namespace {
struct LongRecord {
  std::mutex mu;
  uint64_t *host = nullptr;  // pinned, 3 words (allocated with the first call)
  std::map<int, hipEvent_t> ev;  // per device
  hipEvent_t last = nullptr;
  bool none = true;  // the last such call deferred nothing (it took another path)
};
LongRecord &long_record() {
  static LongRecord *r = new LongRecord();  // never destroyed: the runtime may be gone at exit
  return *r;
}
}  // namespace

// The record as the current device addresses it (allocated with the first call).
hipError_t long_record_device(uint64_t **rec) {
  LongRecord &r = long_record();
  std::lock_guard<std::mutex> g(r.mu);
  hipError_t e;
  if (!r.host) {
    if ((e = hipHostMalloc((void **)&r.host, 3 * sizeof(uint64_t), hipHostMallocPortable | hipHostMallocMapped)) !=
        hipSuccess)
      return e;
    r.host[0] = r.host[1] = r.host[2] = 0;
  }
  return hipHostGetDevicePointer((void **)rec, r.host, 0);
}

hipError_t note_long_units(hipStream_t st) {
  LongRecord &r = long_record();
  std::lock_guard<std::mutex> g(r.mu);
  hipError_t e;
  int d = 0;
  if ((e = hipGetDevice(&d)) != hipSuccess) return e;
  hipEvent_t &ev = r.ev[d];
  if (!ev && (e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return e;
  r.last = ev;
  r.none = false;
  return hipEventRecord(ev, st);
}

void note_long_none() {
  LongRecord &r = long_record();
  std::lock_guard<std::mutex> g(r.mu);
  r.none = true;
}

uint64_t last_long_units(uint64_t *haystacks, uint64_t *chunk) {
  LongRecord &r = long_record();
  std::lock_guard<std::mutex> g(r.mu);
  if (r.none || !r.host) {
    if (haystacks) *haystacks = 0;
    if (chunk) *chunk = 0;
    return 0;
  }
  (void)hipEventSynchronize(r.last);
  if (haystacks) *haystacks = r.host[0];
  if (chunk) *chunk = r.host[1];
  return r.host[2];
}

}  // namespace rure_amd

namespace rt {

int device_cus(int dev) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
  return prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
}

int grid_for(size_t count, uint32_t lds_bytes, int cus) {
  size_t blocks = (count + 255) / 256;
  uint32_t per_cu = 8;
  if (lds_bytes > 0) per_cu = std::max<uint32_t>(1, std::min<uint32_t>(8, (160u * 1024u) / lds_bytes));
  size_t cap = (size_t)cus * per_cu;
  if (blocks > cap) blocks = cap;
  if (blocks == 0) blocks = 1;
  return (int)blocks;
}


static int pike_grid(size_t count, bool fallback, const NfaDev &n, int cus) {
  size_t units = fallback ? (count + 63) / 64 : count;
  size_t wb = nfa_wave_bytes(n.nleaves);
  size_t per_cu = wb <= kNfaLdsMax ? std::max<size_t>(1, std::min<size_t>(32, (160u * 1024u) / wb)) : 4;
  size_t g = std::min(units, (size_t)cus * per_cu);
  return (int)std::max<size_t>(g, 1);
}

// Pike VM pass: all haystacks (no DFA) or only those the DFA quit on.
static hipError_t run_pike(int mode, bool fallback, const BatchDev &b, const DevTables &t, void *out, hipStream_t st) {
  if (!fallback) note_fwd_path(RURE_AMD_PATH_PIKE_ONLY);
  int grid = pike_grid(b.count, fallback, t.n, t.cus);
  size_t wb = nfa_wave_bytes(t.n.nleaves);
  if (wb <= kNfaLdsMax) return launch_pike(mode, fallback, b, t.n, out, nullptr, st, grid);
  Scratch<> scratch;
  const hipError_t e = scratch.alloc(wb * (size_t)grid, st);
  if (e != hipSuccess) return e;
  return launch_pike(mode, fallback, b, t.n, out, scratch.get(), st, grid);
}


// The engine dispatch of exec.rs:473-514 / 382-420 for a batch: DFA, and the
// Pike VM where the DFA quits (or instead of it when it does not fit).
// The unit sizes of its chunked paths are host/chunk_plan.hpp's rule.

// The lanes in flight: kLanesPerCu per CU, or what a tuning knob
// (RURE_AMD_LONG_LANES, RURE_AMD_ITER_LANES; per CU) says.
uint64_t lanes_in_flight(int cus, Knob k) {
  uint64_t per_cu = kLanesPerCu;
  if (knob(k) > 0) per_cu = std::max<uint64_t>(64, knob(k));
  return (uint64_t)cus * per_cu;
}

// Few long haystacks: one lane per haystack would leave the chip idle, so the
// search is split into chunks (launch_long_scan).  Needs a DFA that cannot
// quit (the Pike VM fallback is per haystack).
static bool long_batch(int mode, const BatchDev &b, const DevTables &t, uint64_t *chunk) {
  if (b.offs || !t.has_dfa || t.quit_possible || b.count == 0) return false;
  const uint64_t span = b.length > b.start ? b.length - b.start : 0;
  if (span < kLongSpan || b.count >= (uint64_t)t.cus * 128) {
    // Small batches of medium haystacks (C1: 1024 x 1 KiB): one lane per
    // haystack runs count / 256 workgroups on a 256-CU chip, each lane a
    // dependent chain over its whole haystack; units of >= 128 B spread the
    // searches over about one wave per CU.  End-anchored regexes keep the
    // reverse scan (it reads O(match) bytes); single calls and batches of
    // fewer than 64 haystacks keep one lane each.  RURE_AMD_SPLIT=0 turns it off.
    // Only is_match: a unit stops at its first match there, while a find /
    // shortest_match unit scans on until the DFA dies, so a pattern that never
    // dies ([^\n]* over text without newlines) would cost every unit the rest
    // of its haystack (about units / 2 times the unsplit work).
    if (knob(Knob::Split) == 0 || mode != MODE_ISMATCH || t.anchored_rev || span < 512 || b.count < 64 ||
        b.count > (uint64_t)t.cus * 16)
      return false;
    const uint64_t c = split_unit_bytes(span, b.count, (uint64_t)t.cus);
    if (!c) return false;
    *chunk = c;
    return true;
  }
  *chunk = unit_bytes(span, b.count, lanes_in_flight(t.cus, Knob::LongLanes), kLongFloor);
  return true;
}

// The DFA step of find / is_match / shortest_match (the quit marker where the
// DFA quit): the forward DFA (+ reverse for find), or for DfaAnchoredReverse
// regexes the reverse DFA from the end of each haystack.  Long haystacks
// searched from their start take the chunked forward scan for either (the
// two answer alike at start 0: only the look-behind at `start` differs).
static hipError_t run_dfa_step(int mode, const BatchDev &b, const DevTables &t, void *out, hipStream_t st,
                               int dfa_grid, const FwdDfaDev *iter) {
  uint64_t chunk = 0;
  const bool long_fwd = iter && long_batch(mode, b, t, &chunk);
  if (t.anchored_rev && !(long_fwd && b.start == 0)) return launch_dfa_anchored_rev(mode, b, t.r, out, st, dfa_grid);
  if (long_fwd) return launch_long_scan(mode, b, *iter, t.r, chunk, out, st, t.cus);
  return launch_dfa_fwd(mode, b, t.f, t.r, out, st, dfa_grid);
}

// The Literal / DfaSuffix match types (DevTables::mt_lane): literal searches
// need no DFA; DfaSuffix steps the DFA tables (without them the reference's
// DFA would have quit too: the Pike VM answers).
bool lane_search_ok(const DevTables &t) { return t.mt_lane && (t.m.mt != MT_DFA_SUFFIX || t.has_dfa); }

// DfaSuffix over few long fixed-stride haystacks: the reverse suffix scans
// cut into units (launch_suffix_long) instead of one lane per haystack; the
// haystacks where the reference falls back to the forward DFA (None) then
// take the chunked forward scan.  RURE_AMD_SUFFIX_LONG=0 keeps the lanes.
// The unit of the two chunked DfaSuffix paths (the scan below and the
// iteration of run_find_iter): the long scan's rule, one line's floor where a
// test forces the path at any length.  Kept from before: a fixed kLanesPerCu,
// the lanes knobs do not reach these paths.
static uint64_t suffix_unit_bytes(uint64_t span, uint64_t count, int cus, bool forced) {
  return unit_bytes(span, count, (uint64_t)cus * kLanesPerCu, forced ? kLineFloor : kLongFloor);
}

static bool suffix_long_ok(const BatchDev &b, const DevTables &t, uint64_t *chunk) {
  if (t.m.mt != MT_DFA_SUFFIX || !t.lcs_free || !t.has_dfa || t.quit_possible || b.offs || b.count == 0 || !t.owner)
    return false;
  if (knob(Knob::SuffixLong) == 0) return false;
  const uint64_t span = b.length > b.start ? b.length - b.start : 0;
  const bool forced = knob(Knob::SuffixLong) == 2;
  if (b.count >= (uint64_t)t.cus * 16 || (span < kLongSpan && !forced)) return false;
  *chunk = suffix_unit_bytes(span, b.count, t.cus, forced);
  return true;
}

static hipError_t run_suffix_long(int mode, const BatchDev &b, const DevTables &t, uint64_t chunk, void *out,
                                  hipStream_t st) {
  Scratch<uint8_t> status;
  hipError_t e = status.alloc(b.count, st);
  if (e == hipSuccess) e = launch_suffix_long(mode, b, t.m, t.f, t.r, chunk, out, status.get(), st, t.cus);
  std::vector<uint8_t> hs(b.count);
  if (e == hipSuccess) e = hipMemcpyAsync(hs.data(), status.get(), b.count, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  status.reset();  // before the forward scan's scratch
  if (e != hipSuccess) return e;
  size_t nf = 0;
  for (uint8_t x : hs) nf += x == 3;
  if (!nf) return hipSuccess;
  // exec.rs:764-769 / 700-709: None -> the forward DFA from the search start
  std::string err;
  const FwdDfaDev *iter = iter_device(t.owner, t, &err);
  if (!iter) return hipErrorInvalidValue;
  uint64_t fchunk = 0;
  if (!long_batch(mode, b, t, &fchunk)) fchunk = chunk;
  const size_t rec = mode == MODE_FIND ? 16 : mode == MODE_SHORTEST ? 8 : 1;
  if (nf == b.count) return launch_long_scan(mode, b, *iter, t.r, fchunk, out, st, t.cus);
  Scratch<uint8_t> tmp;
  e = tmp.alloc(b.count * rec, st);
  if (e == hipSuccess) e = launch_long_scan(mode, b, *iter, t.r, fchunk, tmp.get(), st, t.cus);
  for (size_t h = 0; e == hipSuccess && h < b.count; ++h)
    if (hs[h] == 3) e = hipMemcpyAsync((uint8_t *)out + h * rec, tmp.get() + h * rec, rec, hipMemcpyDeviceToDevice, st);
  return e;
}

// A DFA step that can quit, then the Pike VM over the haystacks it quit on:
// the DFA kernels flag a quit in b.quit_flag (`step` gets the batch with the
// flag), and the Pike VM fallback returns at once without one.
template <class Step>
static hipError_t with_quit_fallback(int mode, const BatchDev &b, const DevTables &t, void *out, hipStream_t st,
                                     Step step) {
  Scratch<uint32_t> flag;
  hipError_t e = flag.alloc(4, st);
  BatchDev bq = b;
  bq.quit_flag = flag.get();
  if (e == hipSuccess) e = hipMemsetAsync(bq.quit_flag, 0, 4, st);
  if (e == hipSuccess) e = step(bq);
  if (e == hipSuccess) e = run_pike(mode, true, bq, t, out, st);
  return e;
}

static hipError_t run_lane_search(int mode, const BatchDev &b, const DevTables &t, void *out, hipStream_t st) {
  uint64_t chunk = 0;
  if (suffix_long_ok(b, t, &chunk)) return run_suffix_long(mode, b, t, chunk, out, st);
  const auto step = [&](const BatchDev &bq) { return launch_lane_search(mode, bq, t.m, t.f, t.r, out, st, t.cus); };
  if (!t.quit_possible || t.m.mt != MT_DFA_SUFFIX) return step(b);
  return with_quit_fallback(mode, b, t, out, st, step);
}

// The big-DFA kernel runs one lane per haystack: for batches that fill the
// device (a handful of long haystacks stay on the Pike VM, which spreads one
// haystack over a wave).  RURE_AMD_BIG=2 forces it (tests), =0 keeps the
// Pike VM (A/B; read per call).
static bool big_batch(const BatchDev &b, const DevTables &t) {
  if (knob(Knob::Big) == 2) return true;
  if (knob(Knob::Big) == 0) return false;
  return b.count >= (uint64_t)t.cus * 64;
}

// The rounds of a batched scan on an on-demand DFA (a regex's: run_lazy,
// run_lazy_long, run_lazy_iter and run_lazy_iter_long; a set's: run_lazy_set and
// run_lazy_set_long): `launch` runs one round of the
// kernel; between rounds the host builds the rows the parked lanes need (and, ahead of them,
// more rows in discovery order) and uploads the grown table, which stays in
// t.lazy_buf for the next call.  Synchronous, as the reference's
// construction happens inside its search.  The reference gives up on its
// lazy DFA when the cache thrashes (dfa.rs:1282-1293) and runs the Pike VM;
// here a spent memory budget or kLazyRounds rounds do the same for the batch:
// *ok is then false and the caller runs the Pike VM over the whole batch
// (the rounds' scratch is freed by then).  *rounds = the rounds launched.
// Park is the kernel's record of a parked lane (LazyPark, LazyIterPark,
// LazyLongPark, LazyIterLongPark): the rounds read its state `s` and hand the records back to
// the next launch.  A chunked scan's lane may also park at its unit's cut for
// the link of `s` (wants_link): the host makes it (LazyDfa::strip_of) and
// builds the twin's row ahead, and the table carries the links from then on.
// The caller holds the lock of L's owner.
constexpr int kLazyRounds = 256;
static bool wants_link(const LazyPark &) { return false; }
static bool wants_link(const LazyIterPark &) { return false; }
static bool wants_link(const LazyLongPark &x) { return x.phase == kLazyLongAtCut; }
static bool wants_link(const LazyIterLongPark &x) { return x.phase == kLazyLongAtCut; }
template <class Park, class Launch>
static hipError_t lazy_rounds(LazyDfa &L, DevTables &t, uint64_t count, hipStream_t st, bool *ok_out, uint32_t *rounds,
                              Launch launch) {
  size_t ahead = 4096;  // rows built ahead per round (knob lazy_rows: tests)
  if (knob(Knob::LazyRows) > 0) ahead = (size_t)knob(Knob::LazyRows);
  bool ok = L.nbuilt() > 0 || L.expand(ahead);
  *ok_out = ok;
  *rounds = 0;
  hipError_t e = hipSuccess;
  Scratch<Park> pk[2];
  Scratch<unsigned long long> cnt;
  const size_t pbytes = std::max<uint64_t>(count, 1) * sizeof(Park);
  if ((e = pk[0].alloc(pbytes, st)) != hipSuccess) return e;
  if ((e = pk[1].alloc(pbytes, st)) != hipSuccess) return e;
  if ((e = cnt.alloc(16, st)) != hipSuccess) return e;
  const Park *in = nullptr;
  uint64_t nin = 0;
  std::vector<Park> host;
  for (int round = 0; ok && e == hipSuccess; ++round) {
    // the table: [colmap 256][start 512][now cap * 8][eof_mask cap * 8][reach cap * 8][eof cap]
    // [trans cap * ncol * 4][strip cap * 4]
    // (now, eof_mask and reach: a set's, 8-byte aligned; none for a regex.
    // strip: once a chunked call has made a link)
    const size_t ns = L.nstates(), nm = L.is_set ? ns : 0, nl = L.nlinks() ? ns : 0;
    const size_t need = 768 + nm * 24 + ns + ns * (size_t)L.ncol * 4 + nl * 4 + 16;
    if (need > t.lazy_cap) {
      if ((e = hipStreamSynchronize(st)) != hipSuccess) break;
      if (t.lazy_buf) (void)hipFree(t.lazy_buf);
      t.lazy_buf = nullptr;
      t.lazy_up_states = 0;
      t.lazy_cap = std::max(need * 3 / 2, (size_t)1 << 20);
      if ((e = hipMalloc(&t.lazy_buf, t.lazy_cap)) != hipSuccess) { t.lazy_cap = 0; break; }
    }
    uint8_t *base = (uint8_t *)t.lazy_buf;
    const size_t o_now = 768, o_mask = o_now + nm * 8, o_reach = o_mask + nm * 8, o_eof = o_reach + nm * 8;
    const size_t o_trans = (o_eof + ns + 15) & ~(size_t)15;
    const size_t o_strip = o_trans + ns * (size_t)L.ncol * 4;
    // Uploaded unless the device copy is this very table: states, rows and
    // links only ever grow, so their counts name its contents (a state's masks,
    // reach among them, are set when it is interned).  A call over text
    // whose rows exist copies nothing (1.4 M states are 186 MB).
    if (t.lazy_up_states != ns || t.lazy_up_built != L.nbuilt() || t.lazy_up_links != L.nlinks()) {
      t.lazy_up_states = 0;
      const auto up = [&](size_t off, const void *src, size_t bytes) {
        return bytes ? hipMemcpyAsync(base + off, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
      };
      if ((e = up(0, L.colmap, 256)) != hipSuccess || (e = up(256, L.start, 512)) != hipSuccess ||
          (e = up(o_now, L.now.data(), nm * 8)) != hipSuccess ||
          (e = up(o_mask, L.eof_mask.data(), nm * 8)) != hipSuccess ||
          (e = up(o_reach, L.reach.data(), nm * 8)) != hipSuccess || (e = up(o_eof, L.eof.data(), ns)) != hipSuccess ||
          (e = up(o_trans, L.trans.data(), L.trans.size() * 4)) != hipSuccess ||
          (e = up(o_strip, L.strip.data(), nl * 4)) != hipSuccess)
        break;
      t.lazy_up_states = ns;
      t.lazy_up_built = L.nbuilt();
      t.lazy_up_links = L.nlinks();
    }
    LazyDfaDev f{};
    f.colmap = base;
    f.start = (const uint32_t *)(base + 256);
    f.now = nm ? (const uint64_t *)(base + o_now) : nullptr;
    f.eof_mask = nm ? (const uint64_t *)(base + o_mask) : nullptr;
    f.reach = nm ? (const uint64_t *)(base + o_reach) : nullptr;
    f.eof = base + o_eof;
    f.trans = (const uint32_t *)(base + o_trans);
    f.strip = nl ? (const uint32_t *)(base + o_strip) : nullptr;
    f.ncol = L.ncol;
    f.hot = std::min<uint32_t>((uint32_t)ns, lazy_dfa_hot_rows(L.ncol));
    Park *po = pk[round & 1].get();
    if ((e = hipMemsetAsync(cnt.get(), 0, 8, st)) != hipSuccess) break;
    if ((e = launch(f, in, nin, po, cnt.get())) != hipSuccess) break;
    *rounds = (uint32_t)round + 1;
    unsigned long long n = 0;
    if ((e = hipMemcpyAsync(&n, cnt.get(), 8, hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) break;
    if (n == 0) break;
    if (round + 1 >= kLazyRounds) { ok = false; break; }
    host.resize(n);
    if ((e = hipMemcpyAsync(host.data(), po, n * sizeof(Park), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
      break;
    for (const Park &x : host) {
      if (!wants_link(x)) ok = L.build_row(x.s);
      else if (x.s < L.nstates() && (ok = L.strip_of(x.s))) ok = L.build_row(L.strip[x.s]);
      if (!ok) break;
    }
    // (a fixed number ahead: doubling the rows built ahead each round built
    // states in discovery order the text never visits, seconds of host work
    // for (?:a|b)*a(?:a|b){20})
    if (ok) ok = L.expand(ahead);
    in = po;
    nin = n;
  }
  if (e != hipSuccess) t.lazy_up_states = 0;  // (a copy may not have happened)
  *ok_out = ok;
  return e;
}

// find / is_match / shortest on the on-demand forward DFA (lazy_device):
// rounds of lazy_dfa_kernel.
static hipError_t run_lazy(int mode, const BatchDev &b, const DevTables &tc, void *out, hipStream_t st) {
  DevTables &t = const_cast<DevTables &>(tc);
  rure *re = t.owner;
  std::lock_guard<std::mutex> g(re->mu);
  bool ok = true;
  uint32_t rounds = 0;
  const hipError_t e = lazy_rounds<LazyPark>(*re->lazy, t, b.count, st, &ok, &rounds,
                                   [&](const LazyDfaDev &f, const LazyPark *in, uint64_t nin, LazyPark *po,
                                       unsigned long long *cnt) {
                                     return launch_lazy_dfa(mode, b, f, t.lr, in, nin, po, cnt, out, st, t.cus);
                                   });
  if (e != hipSuccess || ok) return e;
  return run_pike(mode, false, b, t, out, st);  // the whole batch again
}

// The on-demand DFA where the eager automata did not materialise (or
// RURE_AMD_LAZY=1: tests, any regex), for batches that fill the device.
static bool lazy_batch(const BatchDev &b, const DevTables &t) {
  if (knob(Knob::Lazy) == 0) return false;
  const bool force = knob(Knob::Lazy) == 1;
  if (!force && (t.has_dfa || !big_batch(b, t))) return false;
  return lazy_device(t);
}

// Few long fixed-stride haystacks (a log buffer, one document) of such a
// regex: one lane per haystack would walk each alone and the Pike VM gives
// one a wave, so the search is cut into units as long_batch cuts it for a
// regex with an eager DFA (its span and count thresholds, its chunk rule) and
// the units run on the on-demand DFA (run_lazy_long).  Not for batches that
// fill the device (big_batch: one lane per haystack), offset batches, nor a
// program anchored at the start (no `.*?` prefix, so no links: its lanes die
// where the text stops matching).  Knobs lazy_long: 0 never, 2 at any length
// and count (tests); lazy_chunk: the unit size in bytes.  locked: the caller
// holds the lock of t's owner (the single-haystack calls).
static bool lazy_long_batch(const BatchDev &b, const DevTables &t, bool locked, uint64_t *chunk) {
  const long long mode = knob(Knob::LazyLong);
  if (mode == 0 || knob(Knob::Lazy) == 0 || b.offs || b.count == 0 || !t.owner) return false;
  if (t.has_dfa && knob(Knob::Lazy) != 1) return false;
  const uint64_t span = b.length > b.start ? b.length - b.start : 0;
  if (mode != 2 && (big_batch(b, t) || span < kLongSpan || b.count >= (uint64_t)t.cus * 128)) return false;
  if (t.owner->fwd.dotstar_end == 0) return false;  // anchored at the start (before any automaton is made for it)
  if (!lazy_device(t, locked) || !t.owner->lazy->has_strip()) return false;
  *chunk = unit_bytes(span, b.count, lanes_in_flight(t.cus, Knob::LongLanes), kLongFloor);
  if (knob(Knob::LazyChunk) > 0) *chunk = std::max<uint64_t>(16, knob(Knob::LazyChunk));
  return true;
}

// Rounds of lazy_long_kernel over the units until none is parked, then (find)
// the finish step.  Synchronous, as run_lazy; a spent budget or kLazyRounds
// rounds send the whole batch to the Pike VM.
static hipError_t run_lazy_long(int mode, const BatchDev &b, const DevTables &tc, uint64_t chunk, void *out,
                                hipStream_t st, bool locked) {
  DevTables &t = const_cast<DevTables &>(tc);
  rure *re = t.owner;
  std::unique_lock<std::mutex> g(re->mu, std::defer_lock);
  if (!locked) g.lock();
  const uint64_t units = lazy_long_units(b, chunk);
  const auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  Scratch<uint8_t> buf;
  uint64_t *ures = nullptr;
  unsigned long long *best = (unsigned long long *)out;  // is_match / shortest_match: the output itself
  hipError_t e;
  if (mode == MODE_FIND) {
    if ((e = buf.alloc(al(units * 8) + al(b.count * 8), st)) != hipSuccess) return e;
    ures = (uint64_t *)buf.get();
    best = (unsigned long long *)(buf.get() + al(units * 8));
    e = hipMemsetAsync(best, 0xFF, b.count * 8, st);
  } else {
    e = hipMemsetAsync(out, mode == MODE_ISMATCH ? 0 : 0xFF, b.count * (mode == MODE_ISMATCH ? 1 : 8), st);
  }
  if (e != hipSuccess) return e;
  bool ok = true;
  uint32_t rounds = 0;
  e = lazy_rounds<LazyLongPark>(*re->lazy, t, units, st, &ok, &rounds,
                                [&](const LazyDfaDev &f, const LazyLongPark *in, uint64_t nin, LazyLongPark *po,
                                    unsigned long long *cnt) {
                                  return launch_lazy_long(mode, b, f, chunk, in, nin, po, cnt, ures, best, st, t.cus);
                                });
  if (e == hipSuccess && ok && mode == MODE_FIND)
    e = launch_lazy_long_finish(b, t.lr, ures, best, (uint64_t *)out, st, t.cus);
  buf.reset();
  note_lazy_long(units, b.count, chunk, rounds, e == hipSuccess && !ok);
  if (e != hipSuccess || ok) return e;
  return run_pike(mode, false, b, t, out, st);  // the whole batch again
}

// The batched find_iter on the on-demand forward DFA (lazy_batch's regexes):
// rounds of lazy_iter_kernel's count form until no lane is parked, the counts
// scanned to offsets, its write form once, then the counts and total as the
// wave path makes them.  *taken = false where the on-demand DFA gave the batch
// up (a spent budget, kLazyRounds, or the write form met a row not built):
// nothing of the outputs is the answer, no scratch is held, and the caller's
// other engines run the batch.
static hipError_t run_lazy_iter(rure *re, DevTables &t, const BatchDev &b, const IterOut &o, hipStream_t st,
                                bool *taken) {
  *taken = false;
  std::lock_guard<std::mutex> g(re->mu);
  const auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t sz_counts = al((b.count + 1) * 4), sz_off = al((b.count + 1) * 8);
  Scratch<uint8_t> buf;
  hipError_t e = buf.alloc(sz_counts + sz_off + 256, st);
  if (e != hipSuccess) return e;
  uint32_t *counts = (uint32_t *)buf.get(), *flag = (uint32_t *)(buf.get() + sz_counts + sz_off);
  uint64_t *off = (uint64_t *)(buf.get() + sz_counts);
  if ((e = hipMemsetAsync(counts + b.count, 0, 4, st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(flag, 0, 4, st)) != hipSuccess) return e;
  bool ok = true;
  LazyDfaDev table{};  // the last round's: every row the batch reads is in it
  e = lazy_rounds<LazyIterPark>(*re->lazy, t, b.count, st, &ok, &re->lazy_iter_rounds,
                                [&](const LazyDfaDev &f, const LazyIterPark *in, uint64_t nin, LazyIterPark *po,
                                    unsigned long long *cnt) {
                                  table = f;
                                  return launch_lazy_iter_count(b, f, t.lr, in, nin, po, cnt, counts, st, t.cus);
                                });
  re->lazy_iter_fell_back = e == hipSuccess && !ok;
  if (e != hipSuccess || !ok) return e;
  uint32_t unknown = 0;
  if ((e = scan_counts(counts, off, b.count, st)) != hipSuccess) return e;
  if ((e = launch_lazy_iter_write(b, table, t.lr, off, o.matches, o.cap, flag, st, t.cus)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(&unknown, flag, 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  if (unknown) {
    re->lazy_iter_fell_back = 1;
    return hipSuccess;
  }
  *taken = true;
  return launch_iter_counts(b, off, o, st, t.cus);
}

// find_iter over few long fixed-stride haystacks of such a regex: one lane
// per haystack (run_lazy_iter) would iterate each alone and the Pike VM gives
// one a wave, so the iteration is cut into units as lazy_long_batch cuts the
// search (its conditions, its chunk rule) and the units iterate on the
// on-demand DFA (run_lazy_iter_long).  Not for a regex with look-around: a
// unit's speculation is then not equivalent to the true iteration entering
// earlier (iter_scan.hip's U_UNSURE and strict equivalence), and those keep
// their path.  Knobs lazy_iter_long: 0 never, 2 at any length and count
// (tests); lazy_chunk: the unit size in bytes.
static bool lazy_iter_long_batch(const BatchDev &b, const DevTables &t, uint64_t *chunk) {
  const long long mode = knob(Knob::LazyIterLong);
  if (mode == 0 || knob(Knob::Lazy) == 0 || b.offs || b.count == 0 || !t.owner) return false;
  if (t.has_dfa && knob(Knob::Lazy) != 1) return false;
  if (t.owner->nt.looks_used != 0) return false;
  const uint64_t span = b.length > b.start ? b.length - b.start : 0;
  if (mode != 2 && (big_batch(b, t) || span < kLongSpan || b.count >= (uint64_t)t.cus * 128)) return false;
  if (t.owner->fwd.dotstar_end == 0) return false;  // anchored at the start: no links
  if (!lazy_device(t) || !t.owner->lazy->has_strip()) return false;
  *chunk = unit_bytes(span, b.count, lanes_in_flight(t.cus, Knob::LongLanes), kLongFloor);
  if (knob(Knob::LazyChunk) > 0) *chunk = std::max<uint64_t>(16, knob(Knob::LazyChunk));
  return true;
}

// The chunked find_iter on the on-demand DFA (lazy_iter_long_device.hpp has
// the records and the resolve rule).  Pass A: every unit iterates from
// (c0, none).  Pass B: every unit whose predecessor left otherwise than clean
// iterates from that exit.  Pass C: the resolve rule on the device; the units
// its walkers still need run are iterated in one more pass each time, and the
// walkers resume, until none is asked for.  Pass D: the unit counts scanned
// to offsets.  Pass E: the write form over the final entries, then the
// counts and the total.  Passes A, B and each resume pass are rounds of
// lazy_iter_long_kernel's count form (lazy_rounds); four synchronisations
// when no unit is asked for and every row is built.
//
// kLazyIterPasses: a resume pass is the walk of one unit per haystack, a lone
// wave's work: about 4 ms by the chunked find's figures, so 64
// of them are about what the Pike VM takes for 256 KiB, the shortest text this
// path takes by itself.  A text that needs more (a fixed-length match repeated
// through a long run never rejoins its speculation) is given up.
// *taken = false where the batch is given up (a spent budget, kLazyRounds in
// a pass, more than kLazyIterPasses resume passes, or the write form met a
// row not built): nothing of the outputs is the answer, no scratch is held,
// and the caller's other engines run the batch.
constexpr uint32_t kLazyIterPasses = 64;
static hipError_t run_lazy_iter_long(rure *re, DevTables &t, const BatchDev &b, uint64_t chunk, const IterOut &o,
                                     hipStream_t st, bool *taken) {
  *taken = false;
  std::lock_guard<std::mutex> g(re->mu);
  const uint64_t units = lazy_long_units(b, chunk);
  const auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t sz_rec = al(units * sizeof(LilRec)), sz_changed = al(units), sz_walk = al(b.count * sizeof(LilWalk)),
               sz_todo = al(b.count * sizeof(LilTodo)), sz_counts = al((units + 1) * 4), sz_off = al((units + 1) * 8);
  Scratch<uint8_t> buf;
  hipError_t e = buf.alloc(3 * sz_rec + sz_changed + sz_walk + sz_todo + sz_counts + sz_off + 256, st);
  if (e != hipSuccess) return e;
  uint8_t *at = buf.get();
  const auto take = [&](size_t bytes) {
    uint8_t *p = at;
    at += bytes;
    return p;
  };
  LilRec *spec = (LilRec *)take(sz_rec), *fix = (LilRec *)take(sz_rec), *fin = (LilRec *)take(sz_rec);
  uint8_t *changed = take(sz_changed);
  LilWalk *walk = (LilWalk *)take(sz_walk);
  LilTodo *todo = (LilTodo *)take(sz_todo);
  uint32_t *ucounts = (uint32_t *)take(sz_counts);
  uint64_t *off = (uint64_t *)take(sz_off);
  unsigned long long *stats = (unsigned long long *)take(64);  // units asked for, fix records
  uint32_t *flag = (uint32_t *)take(64);
  if ((e = hipMemsetAsync(stats, 0, 128, st)) != hipSuccess) return e;
  uint64_t rec[7] = {units, b.count, chunk, 0, 0, 0, 0};
  LazyDfaDev table{};  // the last round's: every row and link the batch reads is in it
  bool ok = true;
  const auto pass = [&](int from, const LilRec *ent, uint64_t ntodo, LilRec *out) {
    uint32_t rounds = 0;
    const hipError_t pe = lazy_rounds<LazyIterLongPark>(
        *re->lazy, t, from == kLilList ? ntodo : units, st, &ok, &rounds,
        [&](const LazyDfaDev &f, const LazyIterLongPark *in, uint64_t nin, LazyIterLongPark *po,
            unsigned long long *cnt) {
          table = f;
          return launch_lazy_iter_long_count(b, f, t.lr, chunk, from, ent, todo, ntodo, in, nin, po, cnt, out, stats,
                                             st, t.cus);
        });
    rec[3] += rounds;
    return pe;
  };
  const auto give_up = [&]() {
    rec[6] = 1;
    note_lazy_iter_long(rec);
    return hipSuccess;
  };
  if ((e = pass(kLilFresh, nullptr, 0, spec)) != hipSuccess) return e;
  if (!ok) return give_up();
  if ((e = pass(kLilAfter, spec, 0, fix)) != hipSuccess) return e;
  if (!ok) return give_up();
  unsigned long long host[2] = {0, 0};
  for (bool first = true;; first = false) {
    if ((e = launch_lazy_iter_long_resolve(b, chunk, first, spec, fix, fin, changed, walk, todo, stats, st, t.cus)) !=
            hipSuccess ||
        (e = hipMemcpyAsync(host, stats, 16, hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
      return e;
    if (first) rec[4] = host[1];
    const uint64_t ntodo = host[0];
    if (ntodo == 0) break;
    if (ntodo > b.count) return hipErrorUnknown;  // (a walker asks for one unit at a time)
    if (++rec[5] > kLazyIterPasses) return give_up();
    rec[4] += ntodo;
    if ((e = pass(kLilList, nullptr, ntodo, fin)) != hipSuccess) return e;
    if (!ok) return give_up();
    if ((e = hipMemsetAsync(stats, 0, 8, st)) != hipSuccess) return e;
  }
  uint32_t unknown = 0;
  if ((e = launch_lazy_iter_long_counts(b, chunk, fin, ucounts, st, t.cus)) != hipSuccess) return e;
  if ((e = scan_counts(ucounts, off, units, st)) != hipSuccess) return e;
  if ((e = launch_lazy_iter_long_write(b, table, t.lr, chunk, fin, off, o.matches, o.cap, flag, st, t.cus)) !=
      hipSuccess)
    return e;
  if ((e = hipMemcpyAsync(&unknown, flag, 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  if (unknown) return give_up();
  *taken = true;
  note_lazy_iter_long(rec);
  return launch_iter_counts(b, off, o, st, t.cus, units / b.count);
}

// Offset batches (documents of their own lengths) of find / is_match /
// shortest_match: one lane per haystack would walk a long document alone
// (64 MiB: seconds), and the host knows no length without reading the offsets
// back, which these calls never do (they only enqueue).  So the lane kernel
// defers: a haystack whose span reaches kLongSpan (long_batch's threshold) goes
// on a device list and gets "no match"; the chunk, the units and the chunked
// scan of the listed haystacks follow on the device (launch_long_ragged),
// empty launches when nothing was listed.  For a forward DFA that cannot
// quit and has the find_iter automaton's strip table (an anchored-start regex
// has none: its lanes die where the text stops matching).  Knobs long_ragged:
// 0 never, 2 every haystack longer than one chunk; long_chunk: the chunk
// floor (tests: cuts everywhere); long_list: the list's capacity.
static const FwdDfaDev *ragged_long_iter(rure *re, const BatchDev &b, const DevTables &t) {
  if (!b.offs || !b.count || !t.has_dfa || t.quit_possible || t.anchored_rev || lane_search_ok(t)) return nullptr;
  if (knob(Knob::LongRagged) == 0) return nullptr;
  std::string err;
  const FwdDfaDev *fi = iter_device(re, t, &err);
  return fi && !re->dfwd_iter.strip.empty() ? fi : nullptr;
}

static uint64_t device_mem_cached() {
  int d = 0;
  (void)hipGetDevice(&d);
  static std::mutex mu;
  static std::map<int, uint64_t> cache;
  std::lock_guard<std::mutex> g(mu);
  auto it = cache.find(d);
  if (it != cache.end()) return it->second;
  hipDeviceProp_t prop;
  const uint64_t bytes = hipGetDeviceProperties(&prop, d) == hipSuccess ? (uint64_t)prop.totalGlobalMem : 0;
  return cache[d] = bytes ? bytes : 1ull << 40;
}

// lit: the literal engine is the lane kernel (iter is its image too).  The
// scratch holds the list and the units' results for the most there can be:
// no buffer of the device holds more than memory / threshold haystacks of
// that length, and units <= listed + lanes (long_scan.hip).
static hipError_t run_ragged_long(int mode, const BatchDev &b, const DevTables &t, const FwdDfaDev &iter, bool lit,
                                  void *out, hipStream_t st, int dfa_grid) {
  const uint64_t lanes = lanes_in_flight(t.cus, Knob::LongLanes);  // long_batch's
  const bool any = knob(Knob::LongRagged) == 2;
  const long long kc = knob(Knob::LongChunk);
  const uint64_t floor = kc > 0 ? std::max<uint64_t>(16, kc) : kLongFloor;
  const uint64_t least = any ? floor + 1 : kLongSpan;  // the span that defers
  uint64_t cap = any ? b.count : std::min<uint64_t>(b.count, device_mem_cached() / least);
  if (knob(Knob::LongList) > 0) cap = std::min<uint64_t>(cap, knob(Knob::LongList));
  cap = std::max<uint64_t>(cap, 1);
  BatchDev bd = b;
  bd.defer_len = b.start > ~0ull - least ? ~0ull : b.start + least;
  uint64_t *rec = nullptr;
  hipError_t e = long_record_device(&rec);
  if (e != hipSuccess) return e;
  Scratch<unsigned long long> defer;
  if ((e = defer.alloc(long_ragged_bytes(mode, cap, lanes), st)) != hipSuccess) return e;
  bd.defer = defer.get();
  e = launch_long_defer_init(bd.defer, cap, st);
  if (e == hipSuccess)
    e = lit ? launch_lit_find(mode, bd, iter, out, st) : launch_dfa_fwd(mode, bd, t.f, t.r, out, st, dfa_grid);
  if (e == hipSuccess) e = launch_long_ragged(mode, bd, cap, iter, t.r, floor, kc <= 0, lanes, rec, out, st, t.cus);
  if (e == hipSuccess) e = note_long_units(st);
  return e;
}

static hipError_t run_lit_find(int mode, rure *re, const BatchDev &b, const DevTables &t, const FwdDfaDev &lit,
                               void *out, hipStream_t st) {
  if (ragged_long_iter(re, b, t)) return run_ragged_long(mode, b, t, lit, true, out, st, 0);
  if (b.offs) note_long_none();
  return launch_lit_find(mode, b, lit, out, st);
}

// locked: the caller holds the lock of t's owner (the single-haystack calls).
static hipError_t run_regex(int mode, const BatchDev &b, const DevTables &t, void *out, hipStream_t st, int dfa_grid,
                            const FwdDfaDev *iter = nullptr, bool locked = false) {
  uint64_t lchunk = 0;
  if (!lane_search_ok(t) && lazy_long_batch(b, t, locked, &lchunk)) return run_lazy_long(mode, b, t, lchunk, out, st, locked);
  note_lazy_long(0, 0, 0, 0, false);
  if (lane_search_ok(t)) return run_lane_search(mode, b, t, out, st);
  if (knob(Knob::Lazy) == 1 && lazy_batch(b, t))
    return run_lazy(mode, b, t, out, st);
  if (!t.has_dfa && big_batch(b, t) && big_device(t)) return launch_big_dfa(mode, b, t.bf, t.br, out, st, t.cus);
  if (!t.has_dfa && lazy_batch(b, t)) return run_lazy(mode, b, t, out, st);
  if (!t.has_dfa) return run_pike(mode, false, b, t, out, st);
  uint64_t chunk = 0;
  if (iter && long_batch(mode, b, t, &chunk) && !(t.anchored_rev && b.start != 0))
    return launch_long_scan(mode, b, *iter, t.r, chunk, out, st, t.cus);
  // an offset batch comes with the find_iter automaton only from ragged_long_iter
  if (iter && b.offs) return run_ragged_long(mode, b, t, *iter, false, out, st, dfa_grid);
  const auto step = [&](const BatchDev &bq) { return run_dfa_step(mode, bq, t, out, st, dfa_grid, nullptr); };
  return t.quit_possible ? with_quit_fallback(mode, b, t, out, st, step) : step(b);
}


// Few long fixed-stride haystacks of a RegexSet: one lane per haystack would
// walk a 1 GiB log alone, so the scan is cut into units (launch_set_long) of
// the long scan's size, long_batch's threshold and chunk rule.  Needs the
// strip-built set automaton (set_long_device: not a DFA that can quit, nor a
// set anchored at the start), which is built here on the first such call.
// Offset batches keep one lane per haystack.  Knobs set_long: 0 never, 2 at
// any length and count (tests); set_chunk: the unit size in bytes.
static const SetLongDev *set_long_batch(rure_set *rs, const BatchDev &b, DevTables *t, uint64_t *chunk) {
  const long long mode = knob(Knob::SetLong);
  if (mode == 0 || b.offs || b.count == 0 || !t->has_dfa || t->quit_possible) return nullptr;
  const uint64_t span = b.length > b.start ? b.length - b.start : 0;
  if (mode != 2 && (span < kLongSpan || b.count >= (uint64_t)t->cus * 128)) return nullptr;
  std::string err;
  const SetLongDev *sl = set_long_device(rs, t, &err);
  if (!sl) return nullptr;
  *chunk = unit_bytes(span, b.count, lanes_in_flight(t->cus, Knob::LongLanes), kLongFloor);
  if (knob(Knob::SetChunk) > 0) *chunk = std::max<uint64_t>(16, knob(Knob::SetChunk));
  return sl;
}

// A set's matches on its on-demand DFA (set_lazy): rounds of lazy_set_kernel.
static hipError_t run_lazy_set(rure_set *rs, const BatchDev &b, const DevTables &tc, uint64_t *out, hipStream_t st) {
  DevTables &t = const_cast<DevTables &>(tc);  // the set's own entry of rure_set::dev
  std::lock_guard<std::mutex> g(rs->mu);
  const size_t np = rs->exprs.size();
  const uint64_t all = np >= 64 ? ~0ull : (1ull << np) - 1;
  bool ok = true;
  const hipError_t e = lazy_rounds<LazyPark>(*rs->lazy, t, b.count, st, &ok, &rs->lazy_rounds,
                                   [&](const LazyDfaDev &f, const LazyPark *in, uint64_t nin, LazyPark *po,
                                       unsigned long long *cnt) {
                                     return launch_lazy_set(b, f, all, in, nin, po, cnt, out, st, t.cus);
                                   });
  rs->lazy_fell_back = e == hipSuccess && !ok;
  if (e != hipSuccess || ok) return e;
  return run_pike(MODE_SET, false, b, t, out, st);  // the whole batch again
}

// The on-demand DFA for a set past the eager budget, on batches that fill
// the device: the regex rule (lazy_batch).  Knob lazy: 0 never, 1 any set
// that can have it, also one with an eager DFA (tests); big: 2 any batch, 0
// keeps the Pike VM.  Not asked for the single-haystack host calls (run_set:
// locked), which keep the Pike VM below the chunked scan's span.
static bool lazy_set_batch(rure_set *rs, const BatchDev &b, const DevTables &t) {
  if (!rs || !rs->nfa_ok || knob(Knob::Lazy) == 0) return false;
  const bool force = knob(Knob::Lazy) == 1;
  if (!force && (t.has_dfa || !big_batch(b, t))) return false;
  return set_lazy(rs) != nullptr;
}

// Few long fixed-stride haystacks of a set without an eager DFA: the units of
// set_long_batch (its span and count thresholds, its chunk rule) on the
// set's on-demand DFA (run_lazy_set_long), as lazy_long_batch sends a regex's.
// Asked after set_long_batch: a set with an eager DFA keeps set_long_kernel.
// Not for batches that fill the device (big_batch: lazy_set_kernel, one lane
// per haystack), offset batches, sets set_lazy refuses, nor a program
// anchored at the start (no `.*?` prefix, so no links).  Knobs: the regex
// path's lazy_long (0 never, 2 at any length and count) and lazy_chunk (the
// unit size in bytes); lazy = 0 and set_long = 0 turn the path off, lazy = 1
// takes a set with an eager DFA too.  set_long = 2 and set_chunk do not force
// it.  locked: the caller holds rs->mu (the single-haystack calls).
static bool lazy_set_long_batch(rure_set *rs, const BatchDev &b, const DevTables &t, bool locked, uint64_t *chunk) {
  const long long mode = knob(Knob::LazyLong);
  if (!rs || !rs->nfa_ok || mode == 0 || knob(Knob::Lazy) == 0 || knob(Knob::SetLong) == 0) return false;
  if (b.offs || b.count == 0) return false;
  if (t.has_dfa && knob(Knob::Lazy) != 1) return false;
  const uint64_t span = b.length > b.start ? b.length - b.start : 0;
  if (mode != 2 && (big_batch(b, t) || span < kLongSpan || b.count >= (uint64_t)t.cus * 128)) return false;
  if (rs->fwd.dotstar_end == 0) return false;  // anchored at the start (before any automaton is made for it)
  LazyDfa *L = set_lazy(rs, locked);
  if (!L || !L->has_strip()) return false;
  *chunk = unit_bytes(span, b.count, lanes_in_flight(t.cus, Knob::LongLanes), kLongFloor);
  if (knob(Knob::LazyChunk) > 0) *chunk = std::max<uint64_t>(16, knob(Knob::LazyChunk));
  return true;
}

// Rounds of lazy_set_long_kernel over the units until none is parked: the
// haystacks' words are zeroed once, before the first round, and the units OR
// into them.  Synchronous, as run_lazy_set; a spent budget or kLazyRounds
// rounds send the whole batch to the Pike VM (which writes every word).
static hipError_t run_lazy_set_long(rure_set *rs, const BatchDev &b, const DevTables &tc, uint64_t chunk,
                                    uint64_t *out, hipStream_t st, bool locked) {
  DevTables &t = const_cast<DevTables &>(tc);  // the set's own entry of rure_set::dev
  std::unique_lock<std::mutex> g(rs->mu, std::defer_lock);
  if (!locked) g.lock();
  const size_t np = rs->exprs.size();
  const uint64_t all = np >= 64 ? ~0ull : (1ull << np) - 1;
  const uint64_t units = lazy_long_units(b, chunk);
  hipError_t e = hipMemsetAsync(out, 0, b.count * 8, st);
  if (e != hipSuccess) return e;
  bool ok = true;
  e = lazy_rounds<LazyLongPark>(*rs->lazy, t, units, st, &ok, &rs->lazy_rounds,
                                [&](const LazyDfaDev &f, const LazyLongPark *in, uint64_t nin, LazyLongPark *po,
                                    unsigned long long *cnt) {
                                  return launch_lazy_set_long(b, f, all, chunk, in, nin, po, cnt, out, st, t.cus);
                                });
  rs->lazy_fell_back = e == hipSuccess && !ok;
  note_set_units(units, b.count, chunk);
  if (e != hipSuccess || ok) return e;
  return run_pike(MODE_SET, false, b, t, out, st);  // the whole batch again
}

// exec.rs:998-1038 many_matches_at for a batch.  sl: the chunked scan's
// automaton where set_long_batch chose it (chunk its unit), else null.  rs:
// the set (the on-demand DFA is its host object); locked: the caller holds
// rs->mu (the single-haystack host calls, which take the chunked on-demand
// scan and otherwise keep the Pike VM).
static hipError_t run_set(rure_set *rs, const BatchDev &b, const DevTables &t, uint64_t *out, hipStream_t st,
                          int dfa_grid, const SetLongDev *sl, uint64_t chunk, bool locked = false) {
  if (sl) {
    uint64_t units = 0;
    const hipError_t e = launch_set_long(b, *sl, chunk, out, st, t.cus, &units);
    if (e == hipSuccess) {
      note_fwd_path(RURE_AMD_PATH_LONG_SCAN);
      note_set_units(units, b.count, chunk);
    }
    return e;
  }
  uint64_t lchunk = 0;
  if (lazy_set_long_batch(rs, b, t, locked, &lchunk)) return run_lazy_set_long(rs, b, t, lchunk, out, st, locked);
  note_set_units(0, 0, 0);
  if (!locked && lazy_set_batch(rs, b, t)) return run_lazy_set(rs, b, t, out, st);
  if (!t.has_dfa) return run_pike(MODE_SET, false, b, t, out, st);
  const auto step = [&](const BatchDev &bq) {
    return t.use_cores ? launch_set_cores(bq, t.c, out, st, t.cus) : launch_dfa_set(bq, t.s, out, st, dfa_grid);
  };
  return t.quit_possible ? with_quit_fallback(MODE_SET, b, t, out, st, step) : step(b);
}

// The captures Pike VM's grid over `units` waves of work (haystacks, or
// matches), and the scratch its waves need where their working set does not
// fit the LDS (*scratch stays empty where it does).
static hipError_t caps_grid(size_t units, const DevTables &t, uint32_t ns, hipStream_t st, int *grid,
                            Scratch<> *scratch) {
  const size_t wb = caps_wave_bytes(t.n.nleaves, ns);
  const bool in_lds = wb <= kNfaLdsMax;
  const size_t per_cu = in_lds ? std::max<size_t>(1, std::min<size_t>(32, (160u * 1024u) / wb)) : 4;
  size_t g = std::min<size_t>(units, (size_t)t.cus * per_cu);
  if (!in_lds) g = std::min<size_t>(g, (256u << 20) / wb);  // bound the scratch (wide programs: MiBs per wave)
  *grid = (int)std::max<size_t>(1, g);
  return in_lds ? hipSuccess : scratch->alloc(wb * (size_t)*grid, st);
}

// exec.rs:524-596 read_captures_at for a batch.  One group (two slots): the
// plain find.  Otherwise the DFA's (start, end) per haystack (the quit marker
// kept, not resolved), then the Pike VM with slots: from the match start over
// the text up to two characters past the match end, or over the whole
// haystack where the DFA quit and for anchored-start programs.  A regex whose
// DFA does not materialise takes its bounds from the on-demand DFA on batches
// that fill the device (lazy_batch; the reference's lazy DFA produces them)
// and on few long haystacks (lazy_long_batch: the captures Pike VM then runs
// over the match window of a long text, not over all of it), else from the
// Pike VM.  locked: the caller holds the lock of t's owner.
hipError_t run_captures(const BatchDev &b, const DevTables &t, uint64_t *slots, uint32_t ns, hipStream_t st,
                        int dfa_grid, bool locked) {
  if (ns <= 2) return run_regex(MODE_FIND, b, t, slots, st, dfa_grid, nullptr, locked);
  hipError_t e = hipSuccess;
  Scratch<uint64_t> found;
  if (!t.n.anchored) {
    if ((e = found.alloc(b.count * 16, st)) != hipSuccess) return e;
    uint64_t lchunk = 0;
    const bool chunked = !lane_search_ok(t) && lazy_long_batch(b, t, locked, &lchunk);
    if (!chunked) note_lazy_long(0, 0, 0, 0, false);
    e = lane_search_ok(t) ? launch_lane_search(MODE_FIND, b, t.m, t.f, t.r, found.get(), st, t.cus)
        : chunked         ? run_lazy_long(MODE_FIND, b, t, lchunk, found.get(), st, locked)
        : t.has_dfa       ? run_dfa_step(MODE_FIND, b, t, found.get(), st, dfa_grid, nullptr)
        : lazy_batch(b, t) ? run_lazy(MODE_FIND, b, t, found.get(), st)
                           : run_pike(MODE_FIND, false, b, t, found.get(), st);
  }
  int grid = 1;
  Scratch<> scratch;
  if (e == hipSuccess) e = caps_grid(b.count, t, ns, st, &grid, &scratch);
  if (e == hipSuccess)
    e = launch_captures(b, t.n, found.get(), slots, ns, scratch.get(),
                        found && t.skip_on && !lane_search_ok(t) ? &t.sk : nullptr, t.r, st, grid);
  return e;
}

// captures_iter for a batch (re_trait.rs:243-273 over read_captures_at): the
// captures Pike VM once per match of the batched find_iter's list, a wave
// per match; row placement and grid as run_captures, with the matches in the
// haystacks' place.
hipError_t run_captures_iter(const BatchDev &b, const DevTables &t, const IterBufs &ib, uint64_t limit, uint64_t *rows,
                             uint32_t ns, uint8_t *diverged, hipStream_t st) {
  if (ib.nm == 0) return hipSuccess;
  int grid = 1;
  Scratch<> scratch;
  hipError_t e = caps_grid(ib.nm, t, ns, st, &grid, &scratch);
  if (e == hipSuccess)
    e = launch_captures_iter(b, t.n, ib.moff.get(), ib.m.get(), ib.nm, limit, rows, ns, diverged, scratch.get(),
                             t.has_dfa && t.quit_possible && !lane_search_ok(t) ? &t.f : nullptr,
                             t.skip_on ? &t.sk : nullptr, t.r, st, grid);
  return e;
}

bool to_batch(const rure_amd_batch *b, BatchDev *o) {
  if (!b || (!b->haystack && b->count > 0)) return false;
  o->hay = b->haystack;
  o->offs = b->offsets;
  o->stride = b->stride;
  o->length = b->length;
  o->count = b->count;
  o->start = b->start;
  o->quit_flag = nullptr;
  return true;
}


// Runs one regex over one host haystack on the GPU (single-call entry points).
// mode: MODE_FIND / MODE_ISMATCH / MODE_SHORTEST.  Returns false if no match.
bool single_call(rure *re, int mode, const uint8_t *hay, size_t len, size_t start, uint64_t *r0, uint64_t *r1) {
  std::string err;
  DevTables *t = regex_device(re, &err);
  if (!t) die(err);
  uint64_t chunk;
  BatchDev probe{nullptr, nullptr, len, len, 1, start};
  const FwdDfaDev *iter = long_batch(mode, probe, *t, &chunk) ? iter_device(re, *t, &err) : nullptr;  // locks re->mu
  std::lock_guard<std::mutex> g(re->mu);
  int d = 0;
  if (!hip_ok(hipGetDevice(&d), &err)) die(err);
  if (!re->stage.ensure(d, len, &err)) die(err);
  hipStream_t st = re->stage.stream;
  if (len && !hip_ok(hipMemcpyAsync(re->stage.hay, hay, len, hipMemcpyHostToDevice, st), &err)) die(err);
  BatchDev b{re->stage.hay, nullptr, len, len, 1, start};
  if (!hip_ok(run_regex(mode, b, *t, re->stage.res, st, 1, iter, true), &err)) die(err);
  uint64_t out[2] = {~0ull, ~0ull};
  size_t nbytes = mode == MODE_FIND ? 16 : mode == MODE_SHORTEST ? 8 : 1;
  if (!hip_ok(hipMemcpyAsync(out, re->stage.res, nbytes, hipMemcpyDeviceToHost, st), &err)) die(err);
  if (!hip_ok(hipStreamSynchronize(st), &err)) die(err);
  if (mode == MODE_ISMATCH) {
    uint8_t v = (uint8_t)(out[0] & 0xFF);
    if (v > 1) die("internal error: unresolved DFA quit");
    return v == 1;
  }
  if (out[0] == kQuit || (mode == MODE_FIND && out[1] == kQuit)) die("internal error: unresolved DFA quit");
  if (out[0] == ~0ull) return false;
  *r0 = out[0];
  if (r1) *r1 = out[1];
  return true;
}

uint64_t set_single_call(rure_set *rs, const uint8_t *hay, size_t len, size_t start) {
  std::string err;
  DevTables *t = set_device(rs, &err);
  if (!t) die(err);
  uint64_t chunk = 0;
  BatchDev probe{nullptr, nullptr, 0, len, 1, start};
  const SetLongDev *sl = set_long_batch(rs, probe, t, &chunk);  // locks rs->mu
  std::lock_guard<std::mutex> g(rs->mu);
  int d = 0;
  if (!hip_ok(hipGetDevice(&d), &err)) die(err);
  if (!rs->stage.ensure(d, len, &err)) die(err);
  hipStream_t st = rs->stage.stream;
  if (len && !hip_ok(hipMemcpyAsync(rs->stage.hay, hay, len, hipMemcpyHostToDevice, st), &err)) die(err);
  BatchDev b{rs->stage.hay, nullptr, 0, len, 1, start};
  if (!hip_ok(run_set(rs, b, *t, rs->stage.res, st, 1, sl, chunk, true), &err)) die(err);
  uint64_t out = 0;
  if (!hip_ok(hipMemcpyAsync(&out, rs->stage.res, 8, hipMemcpyDeviceToHost, st), &err)) die(err);
  if (!hip_ok(hipStreamSynchronize(st), &err)) die(err);
  if (out == kQuit) die("internal error: unresolved DFA quit");
  return out;
}


// ------------------------------------------------------------------ batches
// MatchType::Literal (exec.rs:1148-1166 -> find_literals, exec.rs:601-625):
// a regex that is a finite string set can answer find / is_match from its
// literals instead of the DFA.  On the GPU that wins for a few literals
// (tools/lit_find_bench.py, find over 262144 x 2000 B of sherlock text,
// literal engine vs DFA: 1 word 0.19 vs 0.22 ms, 3 words 0.19 vs 0.32,
// 4 words 0.24 vs 0.30, 8 words 0.24 vs 0.29, 2 rare words 0.29 vs 0.29;
// 16 words 0.30 vs 0.25 and 64 words 0.76 vs 0.63 favour the DFA, whose
// lookups stay one LDS read per byte while candidate verification grows with
// the literal count), so by default it runs for at most kLitFindMax
// literals, on batches of many haystacks (few long ones keep the chunked DFA
// scan).  RURE_AMD_LIT=1 / 0 forces it on / off.
static constexpr size_t kLitFindMax = 8;
static const FwdDfaDev *literal_engine(int mode, rure *re, DevTables &t, const BatchDev &b) {
  uint64_t chunk;
  const long long env = knob(Knob::Lit);
  if (env >= 0 && env != 1) return nullptr;
  if (t.mt_lane) return nullptr;  // the reference's literal searcher differs from the regex's strings
  if (env < 0 && long_batch(mode, b, t, &chunk)) return nullptr;  // lit=1 forces the literal engine
  {
    // the literal set alone (cheap) before any find_iter DFA is built
    std::lock_guard<std::mutex> g(re->mu);
    if (!re->iter_built && !re->lits_done) re->lit_ok = extract_literals(re->nfa, kLitMax, kLitLen, &re->lits);
    re->lits_done = true;
    if (!re->lit_ok || (env < 0 && re->lits.lits.size() > kLitFindMax)) return nullptr;
  }
  std::string err;
  const FwdDfaDev *fi = iter_device(re, t, &err);
  return fi && fi->lit_n ? fi : nullptr;
}

// rure_amd_find_batch / _is_match_batch / _shortest_match_batch: `out` holds
// the mode's record per haystack.  The literal engine is asked for find and
// is_match only.
int search_batch(int mode, rure *re, const rure_amd_batch *batch, void *out, hipStream_t st) {
  BatchDev b;
  if (!re || !to_batch(batch, &b) || (!out && b.count)) return RURE_AMD_ERR_ARG;
  if (b.count == 0) return RURE_AMD_OK;
  note_lazy_long(0, 0, 0, 0, false);  // (run_lazy_long writes it)
  std::string err;
  DevTables *t = regex_device(re, &err);
  if (!t) return err.rfind("HIP", 0) == 0 ? RURE_AMD_ERR_HIP : RURE_AMD_ERR_DFA;
  if (const FwdDfaDev *lit = mode == MODE_SHORTEST ? nullptr : literal_engine(mode, re, *t, b))
    return run_lit_find(mode, re, b, *t, *lit, out, st) == hipSuccess ? RURE_AMD_OK : RURE_AMD_ERR_HIP;
  const int grid = grid_for(b.count, t->f.lds_bytes, t->cus);
  uint64_t chunk;
  const FwdDfaDev *iter = long_batch(mode, b, *t, &chunk) ? iter_device(re, *t, &err) : ragged_long_iter(re, b, *t);
  if (b.offs && !iter) note_long_none();
  return run_regex(mode, b, *t, out, st, grid, iter) == hipSuccess ? RURE_AMD_OK : RURE_AMD_ERR_HIP;
}


// rure_amd_match_records: the records of one delimited text that match
// (kernels/records.hip).  The unit size is the long scan's (long_batch's rule
// over the whole text; knob records_chunk overrides it), the forward DFA
// answers each record from its start, and the Pike VM, gated on the device,
// the records it quit on -- or all of them for a regex without an eager DFA
// (the on-demand DFA does not run records).  Everything is enqueued on grids
// fixed by the length: nothing is read back.  rure_amd_last_fwd_path is not
// touched: the call is its own path.
int run_match_records(rure *re, const uint8_t *text, size_t length, uint8_t delim, uint32_t flags, uint64_t *nrecords,
                      uint64_t *total, uint64_t *records, uint64_t *numbers, size_t capacity, uint64_t *pike_served,
                      hipStream_t st) {
  if (!re || (!text && length) || !nrecords || !total || (!records && capacity) ||
      (flags & ~(uint32_t)RURE_AMD_RECORDS_INVERT))
    return RURE_AMD_ERR_ARG;
  std::string err;
  DevTables *t = regex_device(re, &err);
  if (!t) return err.rfind("HIP", 0) == 0 ? RURE_AMD_ERR_HIP : RURE_AMD_ERR_DFA;
  if (!t->has_dfa && !re->nfa_ok) return RURE_AMD_ERR_DFA;
  const auto rc = [](hipError_t e) { return e == hipSuccess ? RURE_AMD_OK : RURE_AMD_ERR_HIP; };
  hipError_t e = pike_served ? hipMemsetAsync(pike_served, 0, 8, st) : hipSuccess;
  if (length == 0) {  // no record
    note_records(0, 0);
    if (e == hipSuccess) e = hipMemsetAsync(nrecords, 0, 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(total, 0, 8, st);
    return rc(e);
  }
  uint64_t chunk = unit_bytes(length, 1, lanes_in_flight(t->cus, Knob::LongLanes), kLongFloor);
  if (knob(Knob::RecordsChunk) > 0) chunk = std::max<uint64_t>(16, knob(Knob::RecordsChunk));
  const uint64_t units = rec_units(length, chunk);
  note_records(units, chunk);
  size_t zeroed = 0;
  Scratch<> block;
  if (e == hipSuccess) e = block.alloc(records_scratch_bytes(length, units, &zeroed), st);
  if (e != hipSuccess) return rc(e);
  const RecordsScratch s = records_scratch_at(block.get(), length, units);
  e = hipMemsetAsync(block.get(), 0, zeroed, st);
  if (e == hipSuccess) e = launch_records_scan(text, length, delim, chunk, t->has_dfa ? &t->f : nullptr, s, st, t->cus);
  Scratch<> lists;  // the Pike VM's waves, where their lists do not fit the LDS
  if (e == hipSuccess && (!t->has_dfa || t->quit_possible)) {
    const int grid = records_pike_grid(length, t->n, t->cus);
    const size_t wb = nfa_wave_bytes(t->n.nleaves);
    if (wb > kNfaLdsMax) e = lists.alloc(wb * (size_t)grid, st);
    if (e == hipSuccess)
      e = launch_records_pike(text, length, delim, chunk, t->n, s, (unsigned long long *)pike_served, lists.get(), st,
                              grid);
  }
  if (e == hipSuccess) e = scan_counts(s.owned, s.owned_off, units, st);
  if (e == hipSuccess) e = scan_counts(s.selected, s.selected_off, units, st);
  if (e == hipSuccess)
    e = launch_records_write(text, length, delim, chunk, (flags & RURE_AMD_RECORDS_INVERT) != 0, s, nrecords, total,
                             records, numbers, capacity, st, t->cus);
  return rc(e);
}


// One set of at most 64 patterns (>= 2) into one mask word per haystack.
int set_batch_word(rure_set *rs, const BatchDev &b, uint64_t *mask, hipStream_t stream) {
  std::string err;
  DevTables *t = set_device(rs, &err);
  if (!t) return err.rfind("HIP", 0) == 0 ? RURE_AMD_ERR_HIP : RURE_AMD_ERR_DFA;
  uint64_t chunk = 0;
  const SetLongDev *sl = set_long_batch(rs, b, t, &chunk);
  if (!sl && t->use_cores && !t->cores_adapted && !adapt_cores(rs, t, b, stream, &err)) return RURE_AMD_ERR_HIP;
  int grid = grid_for(b.count, t->s.lds_bytes, t->cus);
  if (run_set(rs, b, *t, mask, stream, grid, sl, chunk) != hipSuccess) return RURE_AMD_ERR_HIP;
  return RURE_AMD_OK;
}

// Group g (patterns [64 g, 64 g + len)) into word g of mask (words per haystack).
int set_batch_group(rure_set *g, const rure_amd_batch *batch, const BatchDev &b, uint64_t *mask, size_t words,
                    size_t w, hipStream_t st) {
  Scratch<> tmp;
  const bool single = g->single != nullptr;
  if (tmp.alloc(b.count * (single ? 1 : 8), st) != hipSuccess) return RURE_AMD_ERR_HIP;
  int rc = single ? rure_amd_is_match_batch(g->single, batch, (uint8_t *)tmp.get(), st)
                  : set_batch_word(g, b, (uint64_t *)tmp.get(), st);
  if (rc == RURE_AMD_OK &&
      launch_mask_column(single ? (const uint8_t *)tmp.get() : nullptr, single ? nullptr : (const uint64_t *)tmp.get(),
                         b.count, mask, words, w, st) != hipSuccess)
    rc = RURE_AMD_ERR_HIP;
  return rc;
}

// knob iter_chunk: the find_iter unit size in bytes (tests: many boundaries)
static uint64_t iter_chunk_knob(uint64_t chunk) {
  return knob(Knob::IterChunk) > 0 ? std::max<uint64_t>(16, knob(Knob::IterChunk)) : chunk;
}

// The unit geometry of an offset batch (documents of their own lengths) in
// the chunked find_iter.  One unit per haystack (rag->uoff stays null) unless
// a haystack is long: one 64 MiB document among short ones would be iterated
// by a single lane.  The longest and the total span are reduced on the
// device and read back (16 bytes, one synchronisation); from kLongSpan (the
// threshold of long_batch and the suffix iteration) the batch is cut into
// units of about total / lanes-in-flight bytes, a haystack shorter than that
// keeping its one unit (iter_device.hpp Geo::uoff), and the unit total is read
// back (a second synchronisation, this path only) so that the scratch is
// sized by the units there are.  Knob iter_ragged: 0 never, 2 at any length
// (tests, with iter_chunk: many boundaries).
static hipError_t ragged_plan(const BatchDev &b, int cus, hipStream_t st, uint64_t *chunk, IterRagged *rag,
                              Scratch<uint64_t> *hold) {
  rag->uoff = nullptr;
  const long long mode = knob(Knob::IterRagged);
  if (mode == 0) return hipSuccess;
  hipError_t e;
  uint64_t span[2] = {0, 0};  // longest, total
  Scratch<uint64_t> stats;
  if ((e = stats.alloc(16, st)) != hipSuccess) return e;
  if ((e = launch_iter_span_stats(b, stats.get(), st, cus)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(span, stats.get(), 16, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  stats.reset();  // before the units' scratch
  if (mode != 2 && span[0] < kLongSpan) return hipSuccess;
  // The fixed-stride rule's lanes in flight over the batch's bytes.  Kept from
  // before: this one site divides rounding down.
  const uint64_t c = iter_chunk_knob(
      unit_bytes(span[1], 1, lanes_in_flight(cus, Knob::IterLanes), kIterFloor, true, Share::RoundDown));
  const size_t n = b.count + 1;
  if ((e = hold->alloc(2 * n * 8, st)) != hipSuccess) return e;
  uint64_t *nk = hold->get(), *uoff = nk + n;
  if ((e = launch_iter_ragged_units(b, c, nk, uoff, st)) != hipSuccess) return e;
  uint64_t nunits = 0;
  if ((e = hipMemcpyAsync(&nunits, uoff + b.count, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  *chunk = c;
  *rag = IterRagged{uoff, nunits, span[1]};
  return hipSuccess;
}

// ------------------------------------------------- the batched find_iter
// run_find_iter's steps, in the order it tries them.

// DfaAnchoredReverse regexes match only at the end of the text, so the
// iteration (re_trait.rs:197-221) yields at most the first search's match
// (the next search starts at the end, where an empty match is the one just
// reported or skipped).  Searched from `start` > 0, that first search is
// the reverse DFA over text[start..] (its look-behind differs from the
// forward scan's); from 0 the chunked path answers the same.
static hipError_t find_iter_anchored_rev(const DevTables &t, const BatchDev &b, const IterOut &o, hipStream_t st) {
  Scratch<uint64_t> found;
  hipError_t e = found.alloc(b.count * 16, st);
  if (e != hipSuccess) return e;
  e = run_regex(MODE_FIND, b, t, found.get(), st, grid_for(b.count, t.r.lds_bytes, t.cus));
  if (e == hipSuccess) e = launch_find_to_iter(found.get(), b.count, o.counts, o.matches, o.cap, o.total, st);
  return e;
}

// DfaSuffix over few long haystacks: the iteration over suffix occurrences
// in parallel (launch_suffix_iter); RURE_AMD_SUFFIX_ITER=0 keeps the wave
// path, =2 takes it at any length with 128-byte units (tests).
// (a DFA that can quit: the path gives up on the first quit, the wave path
// then runs with its Pike VM fallback)
// hipErrorNotSupported: not this path's batch, or it gave up.
static hipError_t find_iter_suffix(const DevTables &t, const BatchDev &b, const IterOut &o, hipStream_t st) {
  if (t.m.mt != MT_DFA_SUFFIX || !t.lcs_free || b.offs || !b.count || b.count >= (uint64_t)t.cus * 16 ||
      b.length <= b.start)
    return hipErrorNotSupported;
  const uint64_t span = b.length - b.start;
  const bool forced = knob(Knob::SuffixIter) == 2;
  if (knob(Knob::SuffixIter) == 0 || (span < kLongSpan && !forced)) return hipErrorNotSupported;
  return launch_suffix_iter(b, t.m, t.f, t.r, suffix_unit_bytes(span, b.count, t.cus, forced), o, st, t.cus);
}

// What the engines of the chunked iteration are called with.
struct IterCall {
  rure *re;
  DevTables *t;
  const BatchDev &b;
  const IterOut &o;
  hipStream_t st;
  std::string *err;
  uint64_t chunk = ~0ull >> 2;
  IterRagged ragged{};
  Scratch<uint64_t> ragged_buf;
  const IterRagged *rag() const { return ragged.uoff ? &ragged : nullptr; }
};

// The geometry: the fixed-stride unit (the span over the haystack's share of
// the lanes in flight: 16 waves per CU, tools/iter_sweep.py), or for offset
// batches the ragged geometry when a haystack is long (ragged_plan).
static hipError_t find_iter_geometry(IterCall &c, const IterSpan *sp) {
  const BatchDev &b = c.b;
  const uint64_t lim = sp ? std::min<uint64_t>(b.length, sp->hi) : b.length;
  if (!b.offs && lim > b.start && b.count)
    c.chunk = iter_chunk_knob(
        unit_bytes(lim - b.start, b.count, lanes_in_flight(c.t->cus, Knob::IterLanes), kIterFloor));
  if (b.offs && !sp && b.count) return ragged_plan(b, c.t->cus, c.st, &c.chunk, &c.ragged, &c.ragged_buf);
  return hipSuccess;
}

// A regex that is one class repeated (C+: [a-z]+, (?-u)\w+, and Unicode
// classes \w+, \S+, \pL+ over UTF-8): its matches are the maximal runs
// (run_iter.hip), no DFA walk; the ASCII shadow's class (an ASCII-only
// class in Unicode mode) answers ASCII text and quits on any other
// byte.  Knob runs=0 keeps the DFA paths (A/B).
// True: the call is answered (*e its result, `path` noted); false: the
// engine does not take the batch, or it quit (*quit).
static bool find_iter_runs(const IterCall &c, const uint8_t *cls, const uint32_t *cp, bool can_quit,
                           rure_amd_path path, hipError_t *e, bool *quit) {
  *quit = false;
  *e = launch_find_iter_runs(c.b, cls, cp, c.o, c.st, c.t->cus, can_quit, quit);
  if (*e == hipErrorNotSupported || (*e == hipSuccess && *quit)) return false;
  if (*e == hipSuccess) note_fwd_path(path);
  return true;
}

// The ASCII shadow (all-rows LDS tables; a non-ASCII byte quits and the full
// automaton re-runs the batch, still chunked).  True: the call is answered
// (*e its result); false: there is no shadow, or it quit (*quit) and the
// full automaton answers.
static bool find_iter_shadow(const IterCall &c, const FwdDfaDev &fi, bool runs, hipError_t *e, bool *quit) {
  *quit = false;
  const FwdDfaDev *fa = iter_ascii_device(c.re, *c.t, c.err);
  if (!fa) return false;
  const DevTables &t = *c.t;
  bool q = false;
  if (runs && fa->run_cls && find_iter_runs(c, fa->run_cls, nullptr, true, RURE_AMD_PATH_ITER_RUNS_ASCII, e, &q))
    return true;
  // The full automaton cannot quit: both passes are enqueued, the
  // shadow's quit staying a device word -- its passes after the quit
  // check run while the word is 0, the full automaton's while it is set
  // (nothing read back, the call only enqueues).  Knob shadow_sync=1
  // reads the quit back.
  if (!fi.can_quit && knob(Knob::ShadowSync) != 1) {
    Scratch<uint32_t> qf;
    *e = qf.alloc(8, c.st);
    if (*e == hipSuccess) *e = hipMemsetAsync(qf.get(), 0, 4, c.st);
    if (*e == hipSuccess)
      *e = launch_find_iter_chunked(c.b, *fa, t.r, c.chunk, c.o, c.st, t.cus, IterQuit::device_word(qf.get()), nullptr,
                                    c.rag());
    if (*e == hipSuccess) {
      BatchDev bf = c.b;
      bf.gate = qf.get();
      bf.gate_set = 1;
      *e = launch_find_iter_chunked(bf, fi, t.r, c.chunk, c.o, c.st, t.cus, IterQuit::none(), nullptr, c.rag());
    }
    if (*e == hipSuccess) note_fwd_path(RURE_AMD_PATH_ITER_SHADOW_GATED);
    return true;
  }
  *e = launch_find_iter_chunked(c.b, *fa, t.r, c.chunk, c.o, c.st, t.cus, IterQuit::read_back(quit), nullptr, c.rag());
  if (*e == hipSuccess && *quit) return false;  // a quit: the full automaton answers
  if (*e == hipSuccess) note_fwd_path(RURE_AMD_PATH_ITER_SHADOW);
  return true;
}

// The full automaton.  *quit: its DFA quit and the quit was read back, the
// one-wave-per-haystack path answers.
static hipError_t find_iter_full(const IterCall &c, const FwdDfaDev &fi, const IterSpan *sp, bool looks,
                                 bool shadow_quit, bool *quit) {
  const DevTables &t = *c.t;
  // A DFA that can quit (Unicode \b over non-ASCII bytes): the units whose
  // searches quit are served by the wave's Pike VM inside the chunked
  // iteration (iter_scan.hip iter_wspec_kernel .. iter_wemit_kernel;
  // nothing read back).  Spans, and knob iter_wave=0, keep the read-back of
  // the quit and the one-wave-per-haystack fallback.
  if (fi.can_quit && !sp && c.re->nfa_ok && knob(Knob::IterWave) != 0) {
    const hipError_t e = launch_find_iter_chunked(c.b, fi, t.r, c.chunk, c.o, c.st, t.cus,
                                                  IterQuit::wave_served(&t.n), nullptr, c.rag());
    if (e == hipSuccess) note_fwd_path(RURE_AMD_PATH_ITER_WAVE_SERVED);
    return e;
  }
  const hipError_t e =
      launch_find_iter_chunked(c.b, fi, t.r, c.chunk, c.o, c.st, t.cus, IterQuit::read_back(quit), sp, c.rag());
  if (e == hipSuccess) {
    if (looks)
      note_fwd_path(*quit ? RURE_AMD_PATH_ITER_LOOKS_QUIT : RURE_AMD_PATH_ITER_LOOKS);
    else
      note_fwd_path(shadow_quit ? RURE_AMD_PATH_ITER_SHADOW_QUIT : RURE_AMD_PATH_ITER_CHUNKED);
  }
  return e;
}

// The batched find_iter (re_trait.rs:197-221) on one stream.
hipError_t run_find_iter(rure *re, DevTables *t, const BatchDev &b, const IterOut &o, hipStream_t st,
                         std::string *err, const IterSpan *sp) {
  const uint64_t none[7] = {0, 0, 0, 0, 0, 0, 0};
  note_lazy_iter_long(none);  // (run_lazy_iter_long records its call)
  if (!sp && t->anchored_rev && b.start > 0 && b.count) return find_iter_anchored_rev(*t, b, o, st);
  if (lane_search_ok(*t) && !sp) {
    const hipError_t e = find_iter_suffix(*t, b, o, st);
    if (e != hipErrorNotSupported) return e;
  }
  // The reference's Literal / DfaSuffix searches (DevTables::mt_lane): every
  // search of the iteration is one of those, on a wave per haystack (lane 0
  // searches, the wave runs the Pike VM where a DfaSuffix scan quits).
  // Except an offset batch of a DfaSuffix regex whose iteration is the
  // forward DFA's (rure::suffix_fwd; an lcs that cannot overlap itself, no
  // quit): it takes the chunked iteration below, where a long haystack is cut
  // into units (one wave would walk a 64 MiB document alone: 10 s) and a
  // short one is a lane's, not a wave's.
  const bool suffix_fwd = t->m.mt == MT_DFA_SUFFIX && t->lcs_free && !t->quit_possible && b.offs && !sp && b.count &&
                          build_iter_dfa(re) && re->suffix_fwd;
  if (lane_search_ok(*t) && re->nfa_ok && !suffix_fwd)
    return launch_find_iter_wave(b, t->has_dfa ? &t->f : nullptr, t->r, t->n, o, st, t->cus, sp, &t->m);
  // A regex whose forward DFA did not materialise, on a batch that fills the
  // device (lazy_batch; knob lazy=1: any regex that can have it, ahead of the
  // chunked engines): every search of the iteration on the on-demand DFA, as
  // the reference's lazy DFA serves them whatever the state count.  Whole
  // haystacks only.  Few long fixed-stride haystacks of such a regex
  // (lazy_iter_long_batch) are cut into units that iterate on it.  Where
  // either gives the batch up, the engines below answer.
  uint64_t lchunk = 0;
  if (!sp && b.count && !lane_search_ok(*t) && lazy_iter_long_batch(b, *t, &lchunk)) {
    bool taken = false;
    const hipError_t e = run_lazy_iter_long(re, *t, b, lchunk, o, st, &taken);
    if (e != hipSuccess || taken) return e;
  } else if (!sp && b.count && !lane_search_ok(*t) && lazy_batch(b, *t)) {
    bool taken = false;
    const hipError_t e = run_lazy_iter(re, *t, b, o, st, &taken);
    if (e != hipSuccess || taken) return e;
  }
  // Chunked speculative iteration (iter_scan.hip); otherwise one wave per
  // haystack.  With look-around (or a DFA that can quit) it needs the
  // stripped states (not an anchored regex) and a whole haystack (no span:
  // a span's "fresh" exit is not enough to enter the next); a quit sends the
  // batch to the wave path.  RURE_AMD_ITER_LOOKS=0 keeps those on the wave
  // path (A/B).
  const FwdDfaDev *fi = nullptr;
  const bool looks = re->nt.looks_used != 0 || t->quit_possible;
  if (t->has_dfa && re->nfa_ok && (!looks || (!sp && knob(Knob::IterLooks) != 0))) fi = iter_device(re, *t, err);
  if (fi && looks && re->dfwd_iter.strip.empty()) fi = nullptr;
  bool looks_quit = false;  // the chunked pass of a look-around regex quit
  if (fi) {
    IterCall c{re, t, b, o, st, err};
    hipError_t e = find_iter_geometry(c, sp);
    if (e != hipSuccess) return e;
    // the run engine, then the ASCII shadow: not for spans (the quit is read
    // back), and no shadow after the run engine quit (it quits on a byte >=
    // 0x80, where the shadow would quit too)
    const bool runs = !sp && knob(Knob::Runs) != 0;
    bool run_quit = false, shadow_quit = false, quit = false;
    if (runs && fi->run_cls &&
        find_iter_runs(c, fi->run_cls, fi->run_cp, fi->run_quit != 0, RURE_AMD_PATH_ITER_RUNS, &e, &run_quit))
      return e;
    if (!sp && !run_quit && find_iter_shadow(c, *fi, runs, &e, &shadow_quit)) return e;
    e = find_iter_full(c, *fi, sp, looks, shadow_quit, &quit);
    if (e != hipSuccess || !quit) return e;
    looks_quit = looks;
  }
  if (!re->nfa_ok) return hipErrorInvalidValue;
  const hipError_t e = launch_find_iter_wave(b, t->has_dfa ? &t->f : nullptr, t->r, t->n, o, st, t->cus, sp);
  // after a look-around regex's quit, ITER_LOOKS_QUIT stands for the pair
  if (e == hipSuccess && !looks_quit) note_fwd_path(RURE_AMD_PATH_ITER_WAVE);
  return e;
}


hipError_t iter_to_device(rure *re, DevTables *t, const BatchDev &b, hipStream_t st, IterBufs *ib, std::string *err) {
  hipError_t e;
  const size_t n = b.count;
  if ((e = ib->counts.alloc((n + 1) * 8, st)) != hipSuccess) return e;
  if ((e = ib->moff.alloc((n + 1) * 8, st)) != hipSuccess) return e;
  if ((e = ib->total.alloc(8, st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(ib->counts.get(), 0, (n + 1) * 8, st)) != hipSuccess) return e;
  const uint64_t bytes = b.offs ? 0 : (uint64_t)b.count * b.length;
  // first guess: the regex's density on its previous call plus an eighth,
  // else a match per 64 bytes (an overflow re-runs the search once with the
  // exact size: the regex-dna strip, a match per 61 bytes, paid that once)
  const int64_t per_mib = re->iter_per_mib.load(std::memory_order_relaxed);
  uint64_t cap = per_mib >= 0 ? (uint64_t)((double)bytes / (1 << 20) * (double)per_mib * 1.125) + 2 * n
                              : bytes / 64 + 2 * n;
  cap = std::max<uint64_t>(1024, cap);
  for (int pass = 0; pass < 2; ++pass) {
    if ((e = ib->m.alloc(cap * 16, st)) != hipSuccess) return e;
    IterOut o{ib->counts.get(), ib->m.get(), cap, ib->total.get()};
    if ((e = run_find_iter(re, t, b, o, st, err)) != hipSuccess) return e;
    uint64_t tot = 0;
    if ((e = hipMemcpyAsync(&tot, ib->total.get(), 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    ib->nm = tot;
    if (bytes >= (1u << 20)) re->iter_per_mib.store((int64_t)((double)tot / ((double)bytes / (1 << 20)) + 1),
                                                    std::memory_order_relaxed);
    if (tot <= cap) break;
    ib->m.reset();  // before the exact-size retry
    cap = tot;
  }
  return exclusive_scan_u64(ib->counts.get(), ib->moff.get(), n + 1, st);
}


// k-mer probe tables of a regex list (KmerDev), built once per list and
// device: every regex a finite set of strings of one length L <= 8 over an
// alphabet of at most 4 bytes with distinct codes (b >> shift) & 3.
struct KmerCacheEntry {
  std::vector<const rure *> res;
  int dev;
  void *blob;
  KmerDev km;
};
std::mutex g_kmer_mu;
std::vector<KmerCacheEntry> g_kmer;

static bool build_kmer(rure *const *res, size_t n, std::vector<uint32_t> *bitmap, std::vector<uint16_t> *mask,
                std::vector<uint16_t> *hmask, KmerDev *km) {
  if (n == 0 || n > 16) return false;
  size_t L = 0;
  bool seen[256] = {false};
  std::vector<uint8_t> alpha;
  for (size_t i = 0; i < n; ++i) {
    rure *re = res[i];
    if (!re->lit_ok || re->lits.lits.empty() || re->lits.minlen != re->lits.maxlen) return false;
    if (L == 0) L = re->lits.minlen;
    if (re->lits.minlen != L) return false;
    for (const std::string &l : re->lits.lits)
      for (unsigned char c : l)
        if (!seen[c]) {
          seen[c] = true;
          alpha.push_back(c);
        }
  }
  if (L == 0 || L > 8 || alpha.size() > 4) return false;
  int shift = -1;
  for (int sh = 0; sh <= 6 && shift < 0; ++sh) {
    uint32_t used = 0;
    bool ok = true;
    for (uint8_t c : alpha) {
      const uint32_t code = (c >> sh) & 3u;
      if (used & (1u << code)) ok = false;
      used |= 1u << code;
    }
    if (ok) shift = sh;
  }
  if (shift < 0) return false;
  km->shift = (uint32_t)shift;
  km->lut = 0;
  km->present = 0;
  for (uint8_t c : alpha) {
    const uint32_t code = (c >> shift) & 3u;
    km->lut |= (uint32_t)c << (8 * code);
    km->present |= 1u << code;
  }
  km->vlut = 0;
  for (uint32_t c = 0; c < 4; ++c) {
    const uint32_t v = (km->present >> c) & 1u ? (km->lut >> (8 * c)) & 0xFFu : ((c ^ 1u) << shift);
    km->vlut |= v << (8 * c);
  }
  km->len = L;
  km->cmask = (uint32_t)((1ull << (2 * L)) - 1);
  bitmap->assign(2048, 0);
  mask->assign((size_t)1 << (2 * L), 0);
  for (size_t i = 0; i < n; ++i)
    for (const std::string &l : res[i]->lits.lits) {
      uint32_t code = 0;
      for (size_t j = 0; j < L; ++j) code |= (((uint8_t)l[j] >> shift) & 3u) << (2 * j);
      (*bitmap)[code >> 5] |= 1u << (code & 31);
      (*mask)[code] |= (uint16_t)(1u << i);
    }
  // the masks' perfect hash for the tile kernel's LDS (kmer_hit_lds): an odd
  // multiplier whose top 10 product bits are distinct over the string codes.
  // Random multipliers find one with probability ~exp(-c^2 / 2048) per try
  // for c codes, so past 160 codes (< 4e-6 per try) none is searched for;
  // without one the hits read mask[code] from global memory (hglobal).
  std::vector<uint32_t> codes;
  for (uint32_t c = 0; c < (uint32_t)mask->size(); ++c)
    if ((*mask)[c]) codes.push_back(c);
  if (codes.size() > 512) return false;
  km->hmul = 0;
  km->hglobal = 1;
  hmask->assign(1024, 0);
  if (codes.size() > 160) return true;
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  std::vector<uint16_t> slot(1024);
  std::vector<uint8_t> used(1024);
  for (int t = 0; t < 100000; ++t) {
    rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
    const uint32_t K = (uint32_t)rng | 1u;
    std::fill(slot.begin(), slot.end(), 0);
    std::fill(used.begin(), used.end(), 0);
    bool ok = true;
    for (uint32_t c : codes) {
      const uint32_t h = (c * K) >> 22;
      if (used[h]) { ok = false; break; }
      used[h] = 1;
      slot[h] = (*mask)[c];
    }
    if (ok) {
      km->hmul = K;
      km->hglobal = 0;
      *hmask = slot;
      return true;
    }
  }
  return true;
}

// The cached device tables for this regex list, copied into *out while the
// cache lock is held (an entry's address does not outlive the lock: another
// thread's push_back or kmer_forget moves the vector).  False: not eligible.
bool kmer_device(rure *const *res, size_t n, KmerDev *out) {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) return false;
  std::lock_guard<std::mutex> g(g_kmer_mu);
  for (const KmerCacheEntry &e : g_kmer)
    if (e.dev == d && e.res.size() == n && std::equal(e.res.begin(), e.res.end(), res)) {
      if (e.blob) *out = e.km;
      return e.blob != nullptr;
    }
  KmerCacheEntry ent;
  ent.res.assign(res, res + n);
  ent.dev = d;
  ent.blob = nullptr;
  std::vector<uint32_t> bm;
  std::vector<uint16_t> mk;
  std::vector<uint16_t> hm;
  if (build_kmer(res, n, &bm, &mk, &hm, &ent.km)) {
    Blob b;
    const size_t ob = b.add(bm.data(), bm.size() * 4), om = b.add(mk.data(), mk.size() * 2);
    const size_t oh = b.add(hm.data(), hm.size() * 2);
    DevTables tmp;
    std::string err;
    if (upload_blob(b, &tmp, &err)) {
      ent.blob = tmp.blob;
      ent.km.bitmap = (const uint32_t *)((uint8_t *)tmp.blob + ob);
      ent.km.mask = (const uint16_t *)((uint8_t *)tmp.blob + om);
      ent.km.hmask = (const uint16_t *)((uint8_t *)tmp.blob + oh);
    }
  }
  g_kmer.push_back(ent);
  if (ent.blob) *out = ent.km;
  return ent.blob != nullptr;
}

// rure_free: drop the k-mer tables of lists holding this regex.
void kmer_forget(const rure *re) {
  std::lock_guard<std::mutex> g(g_kmer_mu);
  for (size_t i = 0; i < g_kmer.size();) {
    if (std::find(g_kmer[i].res.begin(), g_kmer[i].res.end(), re) != g_kmer[i].res.end()) {
      if (g_kmer[i].blob) {
        int cur = 0;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(g_kmer[i].dev);
        (void)hipFree(g_kmer[i].blob);
        (void)hipSetDevice(cur);
      }
      g_kmer.erase(g_kmer.begin() + i);
    } else {
      ++i;
    }
  }
}

}  // namespace rt
