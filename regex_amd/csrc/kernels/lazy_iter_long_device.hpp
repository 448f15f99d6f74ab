// The resolve rule of the chunked find_iter on the on-demand DFA (big_dfa.hip
// lazy_iter_long_kernel, dispatch.cpp run_lazy_iter_long), shared with the
// host: rure_amd_lazy_iter_resolve runs this very code over caller-supplied
// unit records (tests/test_lazy_iter_long_host.py).
//
// A haystack is cut into units [c0, c1); a unit's iteration owns the matches
// that start before c1.  An iteration state is (p, lm): the next search
// start and the end of the last match (kLilNone: none); p == kLilNone is the
// stop state (a reverse NoMatch ended the iteration).  A unit record says
// what the unit's iteration gives from one entry: the matches it owns, the
// state it leaves, and whether that exit is clean (the next unit's true
// iteration equals a fresh one at its c0).
//
// Every unit has run from (c0, none) (spec), and every unit whose
// predecessor's speculative exit is not clean has run, or been skipped, from
// that exit (fix).  A unit is changed when its fix record leaves it otherwise
// than its speculative one (lil_equiv); where no unit of a haystack is
// changed, every unit's final record is its fix record if it has one, else
// its speculative one (lil_parallel, per unit).  From each changed unit, in
// ascending order, a walker (lil_walk, per haystack) carries the true exit X
// forward: a unit entered clean takes its speculative record, one entered in
// the state a record of its has as entry takes that record, one that X steps
// over is skipped, and any other unit must run from X: the walker reports it
// and waits (the caller runs the unit, stores the result as the unit's final
// record with source kLilRun and calls lil_walk again).  A walk ends where X
// is equivalent to the exit the parallel passes assumed.  No DFA is walked
// here.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RURE_LIL_HD __host__ __device__ __forceinline__
#else
#define RURE_LIL_HD inline
#endif

namespace rure_amd {

constexpr uint64_t kLilNone = ~0ull;
// LilRec::flags: the record exists; its exit is clean; where a final record came from
constexpr uint32_t kLilHas = 1, kLilClean = 2, kLilSrcShift = 4;
enum { kLilSpec = 0, kLilFix = 1, kLilSkip = 2, kLilRun = 3 };

struct LilRec {
  uint64_t ep, elm;  // entry
  uint64_t xp, xlm;  // exit (xp == kLilNone: stop)
  uint32_t count, flags;
};

// What a haystack's walker keeps between calls.
struct LilWalk {
  uint64_t k;        // the next unit of the haystack to look at
  uint64_t xp, xlm;  // active: the true exit of unit k - 1
  uint32_t active, xclean;
};

// A unit the walker needs run from (p, lm).
struct LilTodo {
  uint64_t u, p, lm;
};

RURE_LIL_HD bool lil_clean(const LilRec &r) { return (r.flags & kLilClean) != 0; }

// Two exits lead the next unit alike: both clean, or the same state.
RURE_LIL_HD bool lil_equiv(bool ca, uint64_t ap, uint64_t alm, bool cb, uint64_t bp, uint64_t blm) {
  if (ca || cb) return ca && cb;
  return ap == bp && alm == blm;
}

// The record of a unit with cut c1 that the iteration state (p, lm) steps
// over (p >= c1, or the stop state): no match, the same state out.
RURE_LIL_HD bool lil_steps_over(uint64_t p, uint64_t c1) { return p == kLilNone || p >= c1; }
RURE_LIL_HD LilRec lil_skip(uint64_t p, uint64_t lm, uint64_t c1) {
  LilRec r;
  r.ep = r.xp = p;
  r.elm = r.xlm = lm;
  r.count = 0;
  r.flags = kLilHas | ((p != kLilNone && p == c1 && lm != c1) ? kLilClean : 0);
  return r;
}

// The parallel pass, per unit: its final record as long as no walker says
// otherwise; true when the unit is changed.
RURE_LIL_HD bool lil_parallel(const LilRec &spec, const LilRec &fix, LilRec *fin) {
  const bool has = (fix.flags & kLilHas) != 0;
  *fin = has ? fix : spec;
  fin->flags = (fin->flags & (kLilHas | kLilClean)) | ((has ? kLilFix : kLilSpec) << kLilSrcShift);
  return has && !lil_equiv(lil_clean(fix), fix.xp, fix.xlm, lil_clean(spec), spec.xp, spec.xlm);
}

// The first changed unit at or after k (nk: none).
RURE_LIL_HD uint64_t lil_next_changed(const uint8_t *changed, uint64_t k, uint64_t nk) {
  while (k < nk) {
    if ((((uintptr_t)(changed + k)) & 7) == 0 && k + 8 <= nk && *(const uint64_t *)(changed + k) == 0) {
      k += 8;
      continue;
    }
    if (changed[k]) return k;
    ++k;
  }
  return nk;
}

// The walker of one haystack: its nk units' records (spec, fix, fin) and
// changed flags, chunk bytes per unit from `start` (the last unit has no
// cut).  w is zero before the first call.  Returns true when unit todo->u
// (an index into the haystack's units) must run from (todo->p, todo->lm): the
// caller stores that run as fin[todo->u], source kLilRun, and calls again.
// Returns false when the haystack is resolved.
RURE_LIL_HD bool lil_walk(LilWalk *w, uint64_t nk, uint64_t start, uint64_t chunk, const LilRec *spec,
                          const LilRec *fix, LilRec *fin, const uint8_t *changed, LilTodo *todo) {
  uint64_t k = w->k;
  while (k < nk) {
    if (w->active) {
      const LilRec &ps = spec[k - 1];  // what the parallel passes took unit k - 1 to leave
      if (lil_equiv(w->xclean != 0, w->xp, w->xlm, lil_clean(ps), ps.xp, ps.xlm)) {
        w->active = 0;
        continue;
      }
      const uint64_t c1 = k + 1 == nk ? kLilNone : start + (k + 1) * chunk;
      LilRec f;
      if (w->xclean) {
        f = spec[k];
        f.flags = (f.flags & (kLilHas | kLilClean)) | (kLilSpec << kLilSrcShift);
      } else if ((fix[k].flags & kLilHas) && fix[k].ep == w->xp && fix[k].elm == w->xlm) {
        f = fix[k];
        f.flags = (f.flags & (kLilHas | kLilClean)) | (kLilFix << kLilSrcShift);
      } else if ((fin[k].flags >> kLilSrcShift) == kLilRun && fin[k].ep == w->xp && fin[k].elm == w->xlm) {
        f = fin[k];  // the run this walker asked for
      } else if (lil_steps_over(w->xp, c1)) {
        f = lil_skip(w->xp, w->xlm, c1);
        f.flags |= kLilSkip << kLilSrcShift;
      } else {
        todo->u = k;
        todo->p = w->xp;
        todo->lm = w->xlm;
        w->k = k;
        return true;
      }
      fin[k] = f;
      w->xp = f.xp;
      w->xlm = f.xlm;
      w->xclean = lil_clean(f) ? 1 : 0;
      ++k;
      continue;
    }
    k = lil_next_changed(changed, k, nk);
    if (k == nk) break;
    // a changed unit: its fix record is true (what it was entered with is),
    // the units after it were entered otherwise than the passes assumed
    w->active = 1;
    w->xp = fin[k].xp;
    w->xlm = fin[k].xlm;
    w->xclean = lil_clean(fin[k]) ? 1 : 0;
    ++k;
  }
  w->k = nk;
  return false;
}

}  // namespace rure_amd
