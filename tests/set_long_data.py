"""The pattern sets of the chunked RegexSet scan's tests (CPU simulation and
GPU), and which of them have the strip-built automaton.

C4_PATTERNS has four members with a Unicode `\\b` (`\\.js\\b`, `\\bkernel\\b`,
`=null\\b`, `\\bnil\\b`): its DFA can quit, so it keeps one lane per haystack
like every quit-capable set, and so do the 64-pattern groups that contain it
(the first group of the 65- and 130-pattern sets; the second group of the
130-pattern set has no DFA at all).  C4_ASCII_WB is the same set with those
boundaries ASCII (`(?-u:\\b)`): the large set (37110 states with the stripped
twins, 64 patterns, mask `all` = every bit) on the chunked path."""
from bigset_data import SETS
from regex_amd.workloads import C4_PATTERNS

MIXED = [r"^abc", r"abc$", r"(?m)^\d+", r"", r"(?-u:\b)foo(?-u:\b)", r"x*", r"(?s)a.*z", r"$"]
LITERALS = ["ERROR", "status=404", "oom", "kernel"]
C4_ASCII_WB = [p.replace(r"\b", r"(?-u:\b)") for p in C4_PATTERNS]


def groups(k):
    """The 64-pattern groups of SETS[k] with two patterns or more (a
    one-pattern group is a single regex)."""
    pats = SETS[k]
    return [(lo, pats[lo:lo + 64]) for lo in range(0, k, 64) if len(pats[lo:lo + 64]) > 1]


# name -> (patterns, chunked: the set has the strip-built automaton)
CASES = {
    "mixed": (MIXED, True),
    "literals": (LITERALS, True),
    "c4": (C4_PATTERNS, False),
    "c4_ascii_wb": (C4_ASCII_WB, True),
}
for _k in (65, 130):
    for _lo, _p in groups(_k):
        if _p != C4_PATTERNS:  # (the first group of either is the "c4" case)
            # 130's last group: `ERROR.*INFO`, `(?i)WARN\w*`
            CASES["set%d_group%d" % (_k, _lo // 64)] = (_p, (_k, _lo) == (130, 128))
