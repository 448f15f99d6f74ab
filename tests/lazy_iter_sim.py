"""Host-side simulation of find_iter on a regex's on-demand forward DFA
(Regex.lazy_tables / lazy_build), mirroring lazy_iter_kernel
(regex_amd/csrc/kernels/big_dfa.hip) step for step: the whole iteration of
re_trait.rs:197-221 for one haystack, every search a forward walk to the
last match end and a reverse scan (the eager reverse DFA, dfa_tables(1))
over text[p..end] for its start.  The park and resume protocol included: a
lane that meets a row not built yet stops with the iteration's state
(ip, lm, matches so far) and the search's (position, state, last end), the
host builds that row and `ahead` more, the tables are exported again and the
lane resumes inside that search.
TEST INFRASTRUCTURE: validates the automaton's entries, EOF flags and start
flags, and the kernel's stop and step rules, on the CPU."""
from dfa_sim import fwd_flag, rev_flag

MATCH, UNKNOWN = 0x80000000, 0x7FFFFFFF

HUGE = r"(?:a|b)*a(?:a|b){20}"  # ~2^21 states: past the eager budgets
# ordinary regexes pushed through the same walk (GPU: knobs lazy=1, lazy_rows=1)
PLAIN = [r"x*", r"[a-z]+ing", r"\d{4}-\d{2}-\d{2}", r"(?s).{3}$|^Th", r"(?-u)\bthe\b"]
# tests/test_gpu_iter_looks.py's ASCII look-around regexes with reverse
# NoMatches (\B at a search start) and skipped empty matches
LOOKS = [r"(?-u)\B[ab]+", r"(?-u)\b|\B[ab]", r"(?m)^$", r"(?-u)\B"]


class Tables(object):
    """The exported automata of one regex, the forward one exported again
    after every build."""

    def __init__(self, re):
        self.re = re
        self.builds = 0
        self.rev = re.dfa_tables(1)
        assert self.rev is not None and self.rev[0]["quit"] < 0
        self.load()

    def load(self):
        self.info, self.trans, self.eof, self.built, self.start, self.colmap = self.re.lazy_tables()

    def build(self, states, ahead):
        ok = self.re.lazy_build(states, ahead)
        self.builds += 1
        self.load()
        return ok


def rev_scan(rev, t, lo, me):
    """dfa_device.hpp rev_scan over t[lo..me): the smallest start, or None."""
    info, tr, eof, st = rev
    s = int(st[rev_flag(t, lo, me)])
    if s == info["dead"]:
        return None
    rs = None
    a = me
    while a > lo:
        a -= 1
        s = int(tr[s, t[a]])
        if s >= info["normal"]:
            if s < info["match_end"]:
                rs = a + 1
            else:
                assert s == info["dead"]
                return rs
    if eof[s]:
        rs = lo
    return rs


def lane(tb, t, st):
    """One round of one lane.  st: None (a fresh lane searching from `ip`) or
    the record it parked with.  Returns ("parked", record) or ("done",
    matches); a record is (ip, lm, matches, p, s, last)."""
    n = len(t)
    ip, lm, out, p, s, last = st
    resume = p is not None
    while True:
        if not resume:
            if ip > n:
                break
            s = int(tb.start[fwd_flag(t, ip)]) & ~MATCH
            if s == 0:
                break  # dead start state
            p, last = ip, None
        resume = False
        done = False
        while p < n:
            e = int(tb.trans[s, tb.colmap[t[p]]])
            if e == UNKNOWN:
                return "parked", (ip, lm, out, p, s, last)
            if e == 0:
                done = True
                break
            s = e & ~MATCH
            if e & MATCH:
                last = p
            p += 1
        if not done and tb.eof[s]:
            last = n
        if last is None:
            break
        assert last >= ip
        ms = ip
        if last != ip:
            ms = rev_scan(tb.rev, t, ip, last)
            if ms is None:
                break  # exec.rs:656-660: NoMatch ends the iteration
        before = ip
        if ms == last:
            ip = last + 1
            if lm == last:
                assert ip > before
                continue
        else:
            ip = last
        assert ip > before  # every pass advances
        lm = last
        out = out + [(ms, last)]
    return "done", out


def lazy_find_iter(tb, t, start=0, ahead=0):
    """find_iter of haystack t from `start`, or None once the memory budget
    is spent (the batch would go to the other engines)."""
    r = lane(tb, t, (start, None, [], None, None, None))
    while r[0] == "parked":
        s = r[1][4]
        if not tb.build([s], ahead):
            return None
        assert tb.built[s]
        r = lane(tb, t, r[1])
    return r[1]
