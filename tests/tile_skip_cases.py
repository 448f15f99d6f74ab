"""Inputs shared by the tile-skip tests (host simulation and GPU parity): for
each eligible pattern a sample match, the adversarial haystack rows built
from it, and those rows laid out in the 64-haystack groups a wave owns."""
import numpy as np

# pattern -> (a match, bytes that fit no position of the sequence)
ELIGIBLE = {
    r"\d{4}-\d{2}-\d{2}": (b"1234-56-78", b"x", 10),
    r"\d\d:\d\d:\d\d": (b"12:34:56", b"x", 8),
    r"[0-9a-f]{8}-[0-9a-f]{4}": (b"0123abcd-89ef", b"x", 13),
    r"(?i)id=[A-Z]{3}-\d{4}": (b"iD=aBc-1234", b"_", 11),
    # anchors that are byte ranges, not single bytes: the same range twice, and two ranges
    r"[#-&]{2}\d{4}": (b"#$1234", b"x", 6),
    r"[#-&]\d{2}[<->]": (b"#12=", b"x", 4),
}
# the patterns whose anchors are rare enough for the kernel to use the rule
USED = [r"\d{4}-\d{2}-\d{2}", r"(?i)id=[A-Z]{3}-\d{4}", r"[#-&]{2}\d{4}", r"[#-&]\d{2}[<->]"]
INELIGIBLE = [r"\d{2,5}-x", r"a|b", r"\bfoo", r"^\d{4}-\d{2}", r"\w{8}", "\u00e9\\d\\d", "a" * 17]


def _fill(rng, n):
    """Printable filler that cannot complete a match of any of the patterns: no
    '-', ':', '=' or other punctuation of theirs."""
    alpha = np.frombuffer(b"abcdefxyz 0123456789ABCXYZ_.,;", dtype=np.uint8)
    return alpha[rng.integers(0, len(alpha), size=n)].tobytes()


def rows(pat, L, seed=1):
    """Adversarial haystacks of L bytes (L >= 128) for an eligible pattern."""
    match, miss, m = ELIGIBLE[pat]
    assert len(match) == m
    rng = np.random.default_rng(seed)
    anchors = {r"\d{4}-\d{2}-\d{2}": b"-", r"\d\d:\d\d:\d\d": b":", r"[0-9a-f]{8}-[0-9a-f]{4}": b"-",
               r"(?i)id=[A-Z]{3}-\d{4}": b"-", r"[#-&]{2}\d{4}": b"#", r"[#-&]\d{2}[<->]": b"#"}[pat]
    out = []

    def put(base, at, what):
        b = bytearray(base)
        if 0 <= at and at + len(what) <= L:
            b[at:at + len(what)] = what
        return bytes(b)

    printable = bytes(rng.integers(0x20, 0x7F, size=L, dtype=np.uint8))
    out.append(printable)
    out.append(anchors * L)                               # tiles full of the anchor byte
    out.append(bytes(rng.integers(0x30, 0x3A, size=L, dtype=np.uint8)))  # all digits
    base = _fill(rng, L)
    for j in range(m):                                    # a near-miss at every single position
        nm = bytearray(match)
        nm[j:j + 1] = miss
        out.append(put(base, 40, bytes(nm)))
        out.append(put(base, 128 - m // 2 if L >= 128 + m else 40, bytes(nm)))
    bare = bytes(c if not chr(c).isalnum() else miss[0] for c in match)
    for at in (3, 17, 31, 45, 59, 73, 87, 101, 115, 128 - m):  # the anchor bytes alone: candidates that fail
        out.append(put(base, at, bare))
    for at in range(118, 138):                            # every straddle of the first tile cut
        if at + m <= L:
            out.append(put(base, at, match))
    out.append(put(base, 0, match))                       # a match at offset 0
    out.append(put(base, L - m, match))                   # a match ending at len
    out.append(put(base, 128 - m, match))                 # a window ending on a tile's last byte
    out.append(put(base, 50, b"123456789" + match[4:] if pat == r"\d{4}-\d{2}-\d{2}" else b"9" * 9 + match))
    uni = "\u0663".encode()                               # a Unicode digit inside an ASCII match
    d = next(i for i, c in enumerate(match) if chr(c).isdigit())
    out.append(put(base, 30, match[:d] + uni + match[d + 1:]))
    out.append(put(base, 125, match[:d] + uni + match[d + 1:]))
    out.append(put(put(base, 100, "\u00e9".encode()), 130, match))  # non-ASCII in the tile before
    out.append(put(base, 77, b"\xff"))                    # a lone 0xFF
    out.append(put(put(base, 77, b"\xff"), 200, match))
    return [r for r in out if len(r) == L]


def block(pat, L, seed=1):
    """The adversarial rows as a batch block [64 g, L] of whole wave groups (a
    wave of the tile kernel owns 64 consecutive haystacks, and skips a tile
    only when none of its lanes finds it dirty).  Every pure-ASCII row gets a
    group of its own, in three lanes among match-free ASCII filler, so the
    wave's answer for that row comes from the skip rule alone; the rows with
    non-ASCII bytes get groups of their own too.  Then four groups of the
    date recipe's random printable text (2 % with a date) and four of it with
    unicode_mix tokens."""
    from regex_amd.workloads import date_haystacks_host
    from unicode_mix import unicode_mix
    rng = np.random.default_rng(seed ^ 0xB10C)
    groups = []
    for i, r in enumerate(rows(pat, L, seed)):
        g = np.stack([np.frombuffer(_fill(rng, L), dtype=np.uint8) for _ in range(64)])
        for lane in {(7 * i) % 64, (7 * i + 29) % 64, 63}:
            g[lane] = np.frombuffer(r, dtype=np.uint8)
        groups.append(g)
    text, _ = date_haystacks_host(256, L, seed=seed + 11, frac=0.02)
    groups.append(text.reshape(256, L))
    mix, _ = date_haystacks_host(256, L, seed=seed + 12, frac=0.3)
    unicode_mix(mix, 256, L, L, seed + 13, per_hay=2, frac=0.5)
    groups.append(mix.reshape(256, L))
    return np.concatenate(groups)


def clean_share(re, blk):
    """The share of the block's wave-tiles (a group of 64 rows x one 128-byte
    tile) that no lane finds dirty, by the host simulation of each row."""
    k, L = blk.shape
    nt = L // 128
    dirty = np.zeros((k, nt), dtype=bool)
    for i in range(k):
        dirty[i] = re.tile_skip_simulate(blk[i].tobytes())[2] != 0
    return float((~dirty.reshape(k // 64, 64, nt).any(axis=1)).mean())
