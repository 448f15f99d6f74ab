"""Host-side simulation of find_iter over few long haystacks on a regex's
on-demand forward DFA (Regex.lazy_tables / lazy_strip and lazy_build /
lazy_strip_build), mirroring lazy_iter_long_kernel and the passes of
run_lazy_iter_long (regex_amd/csrc/kernels/big_dfa.hip, dispatch.cpp) step
for step.  A batch of fixed-stride haystacks is cut into units of `chunk`
bytes; a unit's iteration runs from an entry state (p, lm) while p is before
its cut c1 and owns the matches that start before c1: every search is
lazy_long_sim's bounded one (through c1 - 1, into strip[state] there, on until
the automaton dies or the text ends), then lazy_iter_sim's start and step
rules.  Pass A runs every unit from (c0, none), pass B every unit whose
predecessor did not leave clean from that exit, pass C resolves (resolve_first
/ resolve_walk: the rule of kernels/lazy_iter_long_device.hpp written out
again, from the queue of changed units as iter_sim.py's walker), the units it
asks for run in resume passes, pass E runs the final entries once more for
the matches.  A lane parks on a row not built yet, or at its cut on a link
not computed; between rounds the host builds what the parked lanes need.
States are the kernel's integers: NONE = 2^64 - 1 for "no last match", and as
p for the stop state.
TEST INFRASTRUCTURE: validates the unit iteration, the records and the
resolve rule on the CPU, and counts the rounds and resume passes a batch
needs."""
from dfa_sim import fwd_flag
from lazy_iter_sim import MATCH, UNKNOWN, rev_scan
from lazy_long_sim import AFTER, AT_CUT, BEFORE, units_of

NONE = (1 << 64) - 1
HAS, CLEAN, SRC = 1, 2, 4
SPEC, FIX, SKIP, RUN = 0, 1, 2, 3
MAX_ROUNDS, MAX_PASSES = 256, 64


def record(ep, elm, xp, xlm, count, clean, src=SPEC):
    return {"ep": ep, "elm": elm, "xp": xp, "xlm": xlm, "count": count,
            "flags": HAS | (CLEAN if clean else 0) | (src << SRC)}


def clean(r):
    return bool(r["flags"] & CLEAN)


def source(r):
    return r["flags"] >> SRC


def with_source(r, src):
    out = dict(r)
    out["flags"] = (r["flags"] & (HAS | CLEAN)) | (src << SRC)
    return out


def equiv(ca, a, cb, b):
    """iter_sim.equiv, not strict"""
    if ca or cb:
        return ca and cb
    return a == b


def steps_over(p, c1):
    return p == NONE or (c1 is not None and p >= c1)


def skipped(p, lm, c1, src=SPEC):
    return record(p, lm, p, lm, 0, p != NONE and p == c1 and lm != c1, src)


def lane(tb, t, c1, st, want=None, out=None):
    """One round of one unit.  st: (ip, lm, count, None) for a fresh lane
    entering with (ip, lm), or the record it parked with, (ip, lm, count,
    (p, s, last, phase)).  want: the write form's match count; out: its
    list.  Returns ("parked", record) or ("done", (xp, xlm, count, clean))."""
    n = len(t)
    ip, lm, cnt, search = st
    while True:
        if search is None:
            if want is not None and cnt >= want:
                return "done", (ip, lm, cnt, True)
            if c1 is not None and ip >= c1:
                return "done", (ip, lm, cnt, ip == c1 and lm != c1)
            if ip > n:
                return "done", (ip, lm, cnt, True)
            s = int(tb.start[fwd_flag(t, ip)]) & ~MATCH
            if s == 0:
                return "done", (ip, lm, cnt, True)  # dead start state
            p, last, phase = ip, None, AFTER if c1 is None else BEFORE
        else:
            p, s, last, phase = search
            search = None
        done = False
        while True:  # lazy_long_sim.lane's walk
            if phase == AT_CUT:
                e = int(tb.strip[s])
                if e == UNKNOWN:
                    return "parked", (ip, lm, cnt, (p, s, last, phase))
                if e == 0:
                    done = True
                    break
                assert not e & MATCH
                s = e
                phase = AFTER
            lim = c1 - 1 if phase == BEFORE else n
            while p < lim:
                e = int(tb.trans[s, tb.colmap[t[p]]])
                if e == UNKNOWN:
                    return "parked", (ip, lm, cnt, (p, s, last, phase))
                if e == 0:
                    done = True
                    break
                s = e & ~MATCH
                if e & MATCH:
                    last = p
                p += 1
            if done or phase == AFTER:
                break
            phase = AT_CUT
        if not done and tb.eof[s]:
            last = n
        if last is None:
            return "done", (ip, lm, cnt, True)  # nothing found: the unit leaves as this search began
        ms = ip
        if last != ip:
            ms = rev_scan(tb.rev, t, ip, last)
            if ms is None:
                return "done", (NONE, NONE, cnt, False)  # exec.rs:656-660: the stop exit
        assert c1 is None or ms < c1  # the unit owns what it finds
        if ms == last:
            ip = last + 1
            if lm == last:
                continue
        else:
            ip = last
        lm = last
        if out is not None:
            out.append((ms, last))
        cnt += 1


class Sim(object):
    """One batched call.  tb: lazy_long_sim.LongTables."""

    def __init__(self, tb, texts, start, chunk, ahead=0):
        self.tb, self.texts, self.start, self.chunk, self.ahead = tb, texts, start, chunk, ahead
        self.units = [(h, c0, c1) for h, t in enumerate(texts) for c0, c1 in units_of(len(t), start, chunk)]
        self.nk = len(self.units) // max(len(texts), 1)
        assert self.nk * len(texts) == len(self.units)  # fixed stride: one length
        self.rounds = self.passes = self.repaired = 0
        self.spec = self.fix = self.fin = None

    def rounds_of(self, lanes, want=None, outs=None):
        """lanes: [(u, ip, lm)].  The records {u: (xp, xlm, count, clean)}, or
        None once the budget is spent or MAX_ROUNDS rounds did not finish."""
        todo = [(u, (ip, lm, 0, None)) for u, ip, lm in lanes]
        res = {}
        rounds = 0
        while todo:
            rounds += 1
            self.rounds += 1
            parked = []
            for u, st in todo:
                h, _, c1 = self.units[u]
                r = lane(self.tb, self.texts[h], c1, st, None if want is None else want[u],
                         None if outs is None else outs[u])
                if r[0] == "parked":
                    parked.append((u, r[1]))
                else:
                    res[u] = r[1]
            if not parked:
                break
            assert want is None  # the write form never parks
            if rounds >= MAX_ROUNDS:
                return None
            links = sorted({st[3][1] for _, st in parked if st[3][3] == AT_CUT})
            rows = {st[3][1] for _, st in parked if st[3][3] != AT_CUT}
            if links:
                if not self.tb.link(links):
                    return None
                strip = self.tb.re.lazy_strip()
                rows |= {int(strip[s]) for s in links}
            if not self.tb.build(sorted(rows), self.ahead):
                return None
            todo = parked
        return res

    def pass_a(self):
        res = self.rounds_of([(u, c0, NONE) for u, (_, c0, _) in enumerate(self.units)])
        if res is None:
            return False
        self.spec = [record(self.units[u][1], NONE, *res[u]) for u in range(len(self.units))]
        return True

    def pass_b(self):
        self.fix = [{"ep": 0, "elm": 0, "xp": 0, "xlm": 0, "count": 0, "flags": 0} for _ in self.units]
        lanes = []
        for u, (h, c0, c1) in enumerate(self.units):
            if u % self.nk == 0 or clean(self.spec[u - 1]):
                continue
            self.repaired += 1
            E = (self.spec[u - 1]["xp"], self.spec[u - 1]["xlm"])
            if steps_over(E[0], c1):
                self.fix[u] = skipped(E[0], E[1], c1)
            else:
                lanes.append((u, E[0], E[1]))
        res = self.rounds_of(lanes)
        if res is None:
            return False
        for u, ip, lm in lanes:
            self.fix[u] = record(ip, lm, *res[u])
        return True

    def resolve_first(self):
        """The parallel pass: the queue of changed units per haystack."""
        n = len(self.units)
        self.fin = [with_source(self.fix[u], FIX) if self.fix[u]["flags"] & HAS else with_source(self.spec[u], SPEC)
                    for u in range(n)]
        self.changed = [bool(self.fix[u]["flags"] & HAS) and
                        not equiv(clean(self.fix[u]), (self.fix[u]["xp"], self.fix[u]["xlm"]),
                                  clean(self.spec[u]), (self.spec[u]["xp"], self.spec[u]["xlm"])) for u in range(n)]
        # per haystack: the queue, how far a walk has come, and a suspended walk (unit, X, X clean)
        self.walkers = [{"queue": [u for u in range(h * self.nk, (h + 1) * self.nk) if self.changed[u]],
                         "walked": h * self.nk, "held": None} for h in range(len(self.texts))]

    def resolve_walk(self):
        """The walkers, each until it needs a unit run or its queue is empty.
        Returns the to-do list [(unit, p, lm)] in haystack order."""
        todo = []
        for h, w in enumerate(self.walkers):
            end = (h + 1) * self.nk
            while w["held"] is not None or w["queue"]:
                if w["held"] is not None:
                    u, X, xc = w["held"]
                    w["held"] = None
                else:
                    j = w["queue"].pop(0)
                    if j < w["walked"]:
                        continue  # a walk went over it
                    u, X, xc = j + 1, (self.fin[j]["xp"], self.fin[j]["xlm"]), clean(self.fin[j])
                asked = False
                while u < end:
                    P = self.spec[u - 1]
                    if equiv(xc, X, clean(P), (P["xp"], P["xlm"])):
                        break
                    c1 = self.units[u][2]
                    F, R = self.fix[u], self.fin[u]
                    if xc:
                        new = with_source(self.spec[u], SPEC)
                    elif F["flags"] & HAS and (F["ep"], F["elm"]) == X:
                        new = with_source(F, FIX)
                    elif source(R) == RUN and (R["ep"], R["elm"]) == X:
                        new = R
                    elif steps_over(X[0], c1):
                        new = skipped(X[0], X[1], c1, SKIP)
                    else:
                        todo.append((u, X[0], X[1]))
                        w["held"] = (u, X, xc)
                        asked = True
                        break
                    self.fin[u] = new
                    X, xc = (new["xp"], new["xlm"]), clean(new)
                    u += 1
                if asked:
                    break
                w["walked"] = u
        return todo

    def run_todo(self, todo):
        self.passes += 1
        self.repaired += len(todo)
        res = self.rounds_of(todo)
        if res is None:
            return False
        for u, ip, lm in todo:
            self.fin[u] = record(ip, lm, *res[u], src=RUN)
        return True

    def write(self, cap=None):
        """Passes D and E: (matches per haystack, total); the flat list is cut
        at cap records, in unit order."""
        n = len(self.units)
        lanes = [(u, self.fin[u]["ep"], self.fin[u]["elm"]) for u in range(n) if self.fin[u]["count"]]
        outs = {u: [] for u, _, _ in lanes}
        res = self.rounds_of(lanes, {u: self.fin[u]["count"] for u in outs}, outs)
        assert res is not None and all(len(outs[u]) == self.fin[u]["count"] for u in outs)
        per = [[] for _ in self.texts]
        off = 0
        for u in range(n):
            for k, m in enumerate(outs.get(u, [])):
                if cap is None or off + k < cap:
                    per[self.units[u][0]].append(m)
            off += self.fin[u]["count"]
        return per, off


def lazy_iter_long(tb, texts, start, chunk, ahead=0, cap=None, check=None, max_passes=MAX_PASSES):
    """The batched call: (matches per haystack, info), or (None, info) where
    the call gives the batch up (a spent budget, MAX_ROUNDS rounds in a pass,
    more than max_passes resume passes; None: the algorithm without that cap).  info: units, rounds, resume passes,
    repaired units, total.  check(sim, first, todo) is called after every
    resolve step."""
    sim = Sim(tb, texts, start, chunk, ahead)

    def info(total=None):
        return {"units": len(sim.units), "rounds": sim.rounds, "resume_passes": sim.passes,
                "repaired": sim.repaired, "total": total}
    if not sim.pass_a() or not sim.pass_b():
        return None, info()
    sim.resolve_first()
    first = True
    while True:
        todo = sim.resolve_walk()
        if check:
            check(sim, first, todo)
        first = False
        if not todo:
            break
        if max_passes is not None and sim.passes + 1 > max_passes:
            sim.passes += 1
            return None, info()
        if not sim.run_todo(todo):
            return None, info()
    per, total = sim.write(cap)
    return per, info(total)
