"""Host-side simulation of RegexSet matches over few long haystacks on the
set's on-demand DFA (RegexSet.lazy_tables / lazy_strip / lazy_reach and
lazy_build / lazy_strip_build), mirroring lazy_set_long_kernel and the rounds
of run_lazy_set_long (regex_amd/csrc/kernels/big_dfa.hip, dispatch.cpp) step
for step.  Every haystack is cut into units of `chunk` bytes; unit [c0, c1)
takes the start state at c0, walks through c1 - 1 ORing now[] of the states
it enters with the match bit, steps into strip[state] there and walks on
until the automaton dies or the text ends (then eof_mask[] of its state); the
unit that owns the end has no cut.  A unit ORs its mask into its haystack's
word where it finishes, and at every poll (a 16-byte block whose address is a
multiple of 512) it ORs in what the word lacks, reads the word back and leaves
when the word holds every pattern of the set or, past its cut, all of
reach[state].  A lane parks on a row not built yet, or at its cut on a link
not computed; between rounds the host builds what the parked lanes need (a
link's twin gets its row at once) and `ahead` more rows, and the parked lanes
resume in the phase they were in with the mask they had.  The word is zeroed
once, before the first round.
TEST INFRASTRUCTURE: validates the links, reach, the walk and the OR on the
CPU, and counts the rounds and the steps a batch needs."""
from dfa_sim import fwd_flag
from lazy_long_sim import AFTER, AT_CUT, BEFORE, units_of
from lazy_set_sim import MATCH, UNKNOWN, Tables


class SetLongTables(Tables):
    """lazy_set_sim.Tables with the strip links and reach, exported again
    after every build."""

    def load(self):
        Tables.load(self)
        self.strip = self.rs.lazy_strip()
        self.reach = self.rs.lazy_reach()
        assert len(self.strip) == len(self.reach) == self.info["states"]

    def link(self, states):
        ok = self.rs.lazy_strip_build(states)
        self.builds += 1
        self.load()
        return ok


class Stats(object):
    """What a simulated call did: the table reads of the byte loop (steps),
    the polls, the units that left at a poll, each unit's own mask, and per
    unit the states it passed and the patterns it reported, in order."""

    def __init__(self, trace=False):
        self.steps = self.polls = self.left = 0
        self.unit_masks = {}
        self.trace = {} if trace else None

    def note(self, u, kind, v):
        if self.trace is not None:
            self.trace.setdefault(u, []).append((kind, v))


def lane(tb, t, c0, c1, rec, word, use_reach, use_all, base, st, u):
    """One round of one unit.  rec: None (fresh) or the record it parked with,
    (p, s, mask, phase); word: the haystack's mask word (a one-element list);
    base: the address of the haystack's byte 0 modulo 512.  Returns
    ("parked", record) or ("done", mask)."""
    n = len(t)
    cut = c1 is not None and c1 > c0 and c1 - 1 <= n
    if rec is None:
        if c0 > n:
            return "done", 0
        s = int(tb.start[fwd_flag(t, c0)]) & ~MATCH
        if s == 0:
            return "done", 0  # dead start state
        p, mask, phase = c0, 0, BEFORE if cut else AFTER
        st.note(u, "state", s)
    else:
        p, s, mask, phase = rec
    while True:
        if phase == AT_CUT:
            e = int(tb.strip[s])
            if e == UNKNOWN:
                return "parked", (p, s, mask, phase)
            if e == 0:
                word[0] |= mask
                return "done", mask
            assert not e & MATCH
            s = e
            st.note(u, "state", s)
            phase = AFTER
        lim = c1 - 1 if phase == BEFORE else n
        while p < lim:
            a = base + p
            if a & 0x1F0 == 0:
                st.polls += 1
                word[0] |= mask
                seen = word[0]
                if (use_all and tb.full & ~seen == 0) or (use_reach and phase == AFTER and int(tb.reach[s]) & ~seen == 0):
                    st.left += 1
                    return "done", mask
            for p in range(p, min(lim, p + 16 - (a & 15))):
                e = int(tb.trans[s, tb.colmap[t[p]]])
                st.steps += 1
                if e == UNKNOWN:
                    return "parked", (p, s, mask, phase)
                if e == 0:
                    word[0] |= mask
                    return "done", mask  # dead: no EOF step
                s = e & ~MATCH
                if e & MATCH:
                    assert int(tb.now[s]) != 0
                    mask |= int(tb.now[s])
                    st.note(u, "report", int(tb.now[s]))
                else:
                    assert int(tb.now[s]) == 0
                st.note(u, "state", s)
            p += 1
        if phase == AFTER:
            break
        phase = AT_CUT
    mask |= int(tb.eof[s])
    st.note(u, "report", int(tb.eof[s]))
    word[0] |= mask
    return "done", mask


def lazy_set_long(tb, texts, start, chunk, ahead=0, max_rounds=None, use_reach=True, use_all=True, bases=None,
                  stats=None):
    """The batched call: (masks per haystack, rounds), or (None, rounds) once
    the memory budget is spent or max_rounds rounds did not finish (the batch
    would go to the Pike VM).  use_reach / use_all = False: units do not leave
    at a poll on reach / on a full word (with both off every unit walks as far
    as it can: the most rows and rounds a call can need, whatever the order in
    which the device's units see each other's bits).  bases: per haystack, the
    address of its byte 0 modulo 512."""
    st = stats if stats is not None else Stats()
    units = [(h, c0, c1) for h, t in enumerate(texts) for c0, c1 in units_of(len(t), start, chunk)]
    words = [[0] for _ in texts]
    todo = [(u, None) for u in range(len(units))]
    rounds = 0
    while todo:
        rounds += 1
        parked = []
        for u, rec in todo:
            h, c0, c1 = units[u]
            r = lane(tb, texts[h], c0, c1, rec, words[h], use_reach, use_all, bases[h] if bases else 0, st, u)
            if r[0] == "parked":
                parked.append((u, r[1]))
            else:
                st.unit_masks[u] = r[1]
        if not parked:
            break
        if max_rounds is not None and rounds >= max_rounds:
            return None, rounds
        links = sorted({rec[1] for _, rec in parked if rec[3] == AT_CUT})
        rows = {rec[1] for _, rec in parked if rec[3] != AT_CUT}
        if links:
            if not tb.link(links):
                return None, rounds
            rows |= {int(tb.strip[s]) for s in links}
        if not tb.build(sorted(rows), ahead):
            return None, rounds
        for _, rec in parked:
            assert tb.built[rec[1]] if rec[3] != AT_CUT else tb.strip[rec[1]] != UNKNOWN
        todo = parked
    st.units = units
    return [w[0] for w in words], rounds


def check_reach(tb, stats):
    """Every pattern a unit reports after passing a state is in that state's
    reach.  Returns the number of (state, later report) pairs checked."""
    pairs = 0
    for u, evs in stats.trace.items():
        later = 0
        for kind, v in reversed(evs):
            if kind == "report":
                later |= v
            else:
                assert later & ~int(tb.reach[v]) == 0, (u, v, later, int(tb.reach[v]))
                pairs += later != 0
    return pairs
