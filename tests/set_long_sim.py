"""Host-side simulation of the chunked RegexSet scan over the exported
strip-built set automaton (RegexSet.long_dfa_tables), mirroring the kernel's
unit algorithm (regex_amd/csrc/kernels/set_long.hip) step for step.
TEST INFRASTRUCTURE: validates the automaton, its strip and reach arrays and
the unit geometry on the CPU."""
from dfa_sim import fwd_flag


def tables(rs):
    t = rs.long_dfa_tables()
    if t is not None:
        t[0]["n"] = len(rs)
    return t


STEPS = [0]  # bytes stepped by every unit since the caller last reset it


def _run(tb, t, s, mask, at, end):
    """The byte loop over t[at:end): (state, mask, done)."""
    info, tr, _, now = tb[:4]
    full = (1 << info["n"]) - 1
    while at < end:
        s = int(tr[s, t[at]])
        at += 1
        STEPS[0] += 1
        if s >= info["normal"]:
            if s < info["match_end"]:
                mask |= int(now[s])
                if mask == full:
                    return s, mask, True
            else:
                assert s == info["dead"]  # (no quit state in this automaton)
                return s, mask, True
    return s, mask, False


def unit_mask(tb, t, c0, c1, published=lambda: 0, poll=8):
    """One unit: threads started in [c0, c1) (c1 None: the unit owns the end
    of the text and a start at len(t)).  published(): the haystack's mask
    word as the unit would read it, every `poll` bytes past the cut."""
    info, tr, eof, now, st, strip, reach = tb
    n = len(t)
    if c0 > n:
        return 0
    s = int(st[fwd_flag(t, c0)])
    if s == info["dead"]:
        return 0
    cut = c1 is not None and c1 > c0 and c1 - 1 <= n
    at = c1 - 1 if cut else n
    s, mask, done = _run(tb, t, s, 0, c0, at)
    if not done and cut:
        s = int(strip[s])
        done = s == info["dead"]
        while not done:
            if int(reach[s]) & ~(mask | published()) == 0:
                done = True
            if done or at >= n:
                break
            to = min(n, at + poll)
            s, mask, done = _run(tb, t, s, mask, at, to)
            at = to
    if not done:
        mask |= int(eof[s])
    return mask


def units_of(n, start, chunk):
    """The host's geometry (launch_set_long): [(c0, c1)], c1 None for the
    last unit."""
    span = n - start if n > start else 0
    nk = 1 if span <= chunk else (span + chunk - 1) // chunk
    return [(start + k * chunk, None if k + 1 == nk else start + (k + 1) * chunk) for k in range(nk)]


def set_long_matches(tb, t, start, chunk, reverse=False, share=True):
    """The OR of the units' masks; the units run one after another (in
    reverse order with `reverse`), each seeing what the earlier ones published
    (share=False: nothing, so no unit leaves early on another's account)."""
    word = [0]
    us = units_of(len(t), start, chunk)
    for c0, c1 in (reversed(us) if reverse else us):
        word[0] |= unit_mask(tb, t, c0, c1, (lambda: word[0]) if share else (lambda: 0))
    return word[0]
