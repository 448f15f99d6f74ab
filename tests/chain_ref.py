"""Chains of one-byte-class replace_all steps for the tests of
rure_amd_replace_all_chain, and their plain-Python restatement.

A step is (pattern, byte set, replacement): the byte set is written out here
as a literal, so the expected text never passes through the product's parser
(tests/test_chain_map.py checks each set once against
rure_amd_class_one_export).  The rule is exact: a byte of the set becomes the
replacement, any other byte stays."""

ALL = frozenset(range(256))


def span(lo, hi):
    return frozenset(range(lo, hi + 1))


def lit(s):
    return frozenset(s)


def apply_step(t, cset, rep):
    return b"".join(rep if c in cset else bytes((c,)) for c in t)


def apply_chain(steps, t):
    """[t, the text after step 0, after step 1, ...]"""
    texts = [bytes(t)]
    for _, cset, rep in steps:
        texts.append(apply_step(texts[-1], cset, rep))
    return texts


# tests/test_gpu_replace_class.py's chains (CHAINS there)
CHAINS = [
    # the IUB substitutions' shape: one byte each, the next step's byte counted as written
    [(r"B", lit(b"B"), b"(c|g|t)"), (r"D", lit(b"D"), b"(a|g|t)"), (r"N", lit(b"N"), b"(a|c|g|t)")],
    # two-byte classes (SWAR), a wide class (the count pass), a 64-byte replacement
    [(r"[KM]", lit(b"KM"), b"<km>"), (r"[a-c]", lit(b"abc"), b"Q"), (r"Q", lit(b"Q"), b"<" + b"q" * 62 + b">"),
     (r"[<>]", lit(b"<>"), b"D")],
    # replacements that create the next step's bytes, and a one-step chain
    [(r"x", lit(b"x"), b"yxy"), (r"y", lit(b"y"), b"xx")],
    [(r"(?-u)\xff", lit(b"\xff"), b"\xff\xfe\xff")],
]

# The limits of the composed byte map (REPLACE_HMAP): name -> (steps,
# mappable, changed byte values, sum of the image lengths or None when an
# image is too long to compose)
LIMITS = {
    # all 256 byte values change: byte 0xFF's index would be the "unchanged" mark
    "all256": ([(r"(?s-u:.)", ALL, b"xx")], False, 256, 512),
    # 255 change (everything becomes 0x01, which maps to itself): the largest index
    "c255": ([(r"(?-u)[\x00-\x7f]", span(0x00, 0x7F), b"\x80"), (r"(?-u)[\x80-\xff]", span(0x80, 0xFF), b"\x01")],
             True, 255, 256),
    # 16 / 17 changed bytes: lane-register counters / LDS atomics
    "c16": ([(r"[a-h]", lit(b"abcdefgh"), b"AB"), (r"[i-p]", lit(b"ijklmnop"), b"CDE")], True, 16, 256 + 8 + 16),
    "c17": ([(r"[a-h]", lit(b"abcdefgh"), b"AB"), (r"[i-q]", lit(b"ijklmnopq"), b"CDE")], True, 17, 256 + 8 + 18),
    # 154 changed bytes: deep in the LDS-atomic histogram (0x80.. -> ab -> (z)(z))
    "c154": ([(r"(?-u)[\x80-\xff]", span(0x80, 0xFF), b"ab"), (r"[a-z]", span(0x61, 0x7A), b"(z)")],
             True, 154, 102 + 128 * 6 + 26 * 3),
    # the pool limit: 64 images of 61 bytes + 192 of one = 4096; of 62: 4160
    "pool4096": ([(r"(?-u)[\x40-\x7f]", span(0x40, 0x7F), b"<" + b"p" * 59 + b">")], True, 64, 4096),
    "pool4160": ([(r"(?-u)[\x40-\x7f]", span(0x40, 0x7F), b"<" + b"p" * 60 + b">")], False, 64, 4160),
    # the image limit: x -> 32 x -> 64 x; 33 x -> 66 x
    "img64": ([(r"x", lit(b"x"), b"x" * 32), (r"x", lit(b"x"), b"xx")], True, 1, 255 + 64),
    "img66": ([(r"x", lit(b"x"), b"x" * 33), (r"x", lit(b"x"), b"xx")], False, 0, None),
}
