"""Host-side simulation of the chunked scan of long haystacks on a regex's
on-demand forward DFA (Regex.lazy_tables / lazy_strip and lazy_build /
lazy_strip_build), mirroring lazy_long_kernel and the rounds of run_lazy_long
(regex_amd/csrc/kernels/big_dfa.hip, dispatch.cpp) step for step.  A batch of
fixed-stride haystacks is cut into units of `chunk` bytes; unit [c0, c1) takes
the start state at c0, walks through c1 - 1, steps into strip[state] there
and walks on until the automaton dies or the text ends; the unit that owns
the end has no cut.  A lane parks on a row not built yet, or at its cut on a
link not computed; between rounds the host builds what the parked lanes need
(a link's twin gets its row at once) and `ahead` more rows, the tables are
exported again and the parked lanes resume in the phase they were in.  The
units' results are combined by the kernel's rule: is_match any, shortest_match
the smallest end, find the smallest unit with a match, its start from the
reverse DFA over text[start..end].
TEST INFRASTRUCTURE: validates the links, the walk and the combination on
the CPU, and counts the rounds a batch needs."""
from dfa_sim import fwd_flag
from lazy_iter_sim import MATCH, UNKNOWN, Tables, rev_scan

BEFORE, AT_CUT, AFTER = 0, 1, 2


class LongTables(Tables):
    """lazy_iter_sim.Tables with the strip links, exported again after every
    build."""

    def load(self):
        Tables.load(self)
        self.strip = self.re.lazy_strip()
        assert len(self.strip) == self.info["states"]

    def link(self, states):
        ok = self.re.lazy_strip_build(states)
        self.builds += 1
        return ok


def units_of(n, start, chunk):
    """long_scan_m's geometry: [(c0, c1)], c1 None for the unit that owns the end."""
    span = n - start if n > start else 0
    nk = 1 if span <= chunk else (span + chunk - 1) // chunk
    return [(start + k * chunk, None if k + 1 == nk else start + (k + 1) * chunk) for k in range(nk)]


def lane(tb, t, c0, c1, mode, rec):
    """One round of one unit.  rec: None (fresh) or the record it parked with,
    (p, s, last, phase).  Returns ("parked", record) or ("done", last)."""
    n = len(t)
    cut = c1 is not None and c1 > c0 and c1 - 1 <= n
    if rec is None:
        if c0 > n:
            return "done", None
        s = int(tb.start[fwd_flag(t, c0)]) & ~MATCH
        if s == 0:
            return "done", None  # dead start state
        p, last, phase = c0, None, BEFORE if cut else AFTER
    else:
        p, s, last, phase = rec
    while True:
        if phase == AT_CUT:
            e = int(tb.strip[s])
            if e == UNKNOWN:
                return "parked", (p, s, last, phase)
            if e == 0:
                return "done", last
            assert not e & MATCH
            s = e
            phase = AFTER
        lim = c1 - 1 if phase == BEFORE else n
        while p < lim:
            e = int(tb.trans[s, tb.colmap[t[p]]])
            if e == UNKNOWN:
                return "parked", (p, s, last, phase)
            if e == 0:
                return "done", last
            s = e & ~MATCH
            if e & MATCH:
                last = p
                if mode != "find":
                    return "done", last  # quit_after_match
            p += 1
        if phase == AFTER:
            break
        phase = AT_CUT
    if tb.eof[s]:
        last = n
    return "done", last


def lazy_long(tb, texts, start, chunk, mode, ahead=0, max_rounds=None):
    """The batched call: (results per haystack, rounds), or (None, rounds)
    once the memory budget is spent or max_rounds rounds did not finish (the
    batch would go to the Pike VM).  mode: "find" -> (start, end) or None,
    "is_match" -> bool, "shortest" -> end or None."""
    units = [(h, c0, c1) for h, t in enumerate(texts) for c0, c1 in units_of(len(t), start, chunk)]
    last = [None] * len(units)
    todo = [(u, None) for u in range(len(units))]
    rounds = 0
    while todo:
        rounds += 1
        parked = []
        for u, rec in todo:
            h, c0, c1 = units[u]
            r = lane(tb, texts[h], c0, c1, mode, rec)
            if r[0] == "parked":
                parked.append((u, r[1]))
            else:
                last[u] = r[1]
        if not parked:
            break
        if max_rounds is not None and rounds >= max_rounds:
            return None, rounds
        links = sorted({rec[1] for _, rec in parked if rec[3] == AT_CUT})
        rows = {rec[1] for _, rec in parked if rec[3] != AT_CUT}
        if links:
            if not tb.link(links):
                return None, rounds
            strip = tb.re.lazy_strip()
            rows |= {int(strip[s]) for s in links}
        if not tb.build(sorted(rows), ahead):
            return None, rounds
        for _, rec in parked:
            assert tb.built[rec[1]] if rec[3] != AT_CUT else tb.strip[rec[1]] != UNKNOWN
        todo = parked
    out = []
    for h, t in enumerate(texts):
        mine = [u for u in range(len(units)) if units[u][0] == h]
        hit = [u for u in mine if last[u] is not None]
        if mode == "is_match":
            out.append(bool(hit))
        elif mode == "shortest":
            out.append(min(last[u] for u in hit) if hit else None)
        elif not hit:
            out.append(None)
        else:
            me = last[hit[0]]  # the smallest unit that matched
            if me == start:
                out.append((me, me))
            else:
                ms = rev_scan(tb.rev, t, start, me)
                out.append(None if ms is None else (ms, me))
    return out, rounds


def crossing(exp, start, chunk):
    """Whether the match `exp` of a search from `start` starts in another
    unit than the one it ends in."""
    return exp is not None and exp[1] > exp[0] and (exp[0] - start) // chunk != (exp[1] - 1 - start) // chunk
