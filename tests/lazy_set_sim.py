"""Host-side simulation of RegexSet matches on the set's on-demand DFA
(RegexSet.lazy_tables / lazy_build), mirroring lazy_set_kernel
(regex_amd/csrc/kernels/big_dfa.hip) step for step, the park and resume
protocol included: a lane that meets a row not built yet stops with
(position, state, mask), the host builds that row and `ahead` more, the
tables are exported again and the lane resumes where it stopped.
TEST INFRASTRUCTURE: validates the automaton's entries, now / eof_mask
arrays and start flags on the CPU."""
from dfa_sim import fwd_flag

MATCH, UNKNOWN = 0x80000000, 0x7FFFFFFF

# the sets of the CPU and GPU tests beside set_long_data's
NO_DFA = [r"(?-u:[ab])*a(?-u:[ab]){17}", r"bb", r"^a"]  # test_gpu_nfa.py's: past 65536 raw states
FLAGS = [r"^[a-z]+ ", r"(?m)\d$", r"(?-u)\bERROR\b"]    # the start flags: ^, $, (?m), an ASCII \b


class Tables(object):
    """The exported automaton of one set, exported again after every build."""

    def __init__(self, rs):
        self.rs = rs
        self.full = (1 << len(rs)) - 1
        self.builds = 0
        self.load()

    def load(self):
        self.info, self.trans, self.now, self.eof, self.built, self.start, self.colmap = self.rs.lazy_tables()

    def build(self, states, ahead):
        ok = self.rs.lazy_build(states, ahead)
        self.builds += 1
        self.load()
        return ok


def walk(tb, t, p, s, mask):
    """One round of one lane from byte p in state s: ("parked", p, s, mask)
    or ("done", mask)."""
    n = len(t)
    while p < n:
        e = int(tb.trans[s, tb.colmap[t[p]]])
        if e == UNKNOWN:
            return "parked", p, s, mask
        if e == 0:
            return "done", mask  # dead: no EOF step
        s = e & ~MATCH
        if e & MATCH:
            assert int(tb.now[s]) != 0
            mask |= int(tb.now[s])
            if mask & tb.full == tb.full:
                return "done", mask
        else:
            assert int(tb.now[s]) == 0
        p += 1
    return "done", mask | int(tb.eof[s])


def lazy_set_matches(tb, t, start=0, ahead=0):
    """The mask of haystack t searched from `start`, or None once the memory
    budget is spent (the batch would go to the Pike VM)."""
    if start > len(t):
        return 0
    s = int(tb.start[fwd_flag(t, start)]) & ~MATCH
    if s == 0:
        return 0
    r = walk(tb, t, start, s, 0)
    while r[0] == "parked":
        _, p, s, mask = r
        if not tb.build([s], ahead):
            return None
        assert tb.built[s]
        r = walk(tb, t, p, s, mask)
    return r[1]
