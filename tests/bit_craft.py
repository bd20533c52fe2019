"""Position-crafted bit flips for the Hamming, CRC and parity codecs -- TEST ONLY (numpy and the
oracle, no engine import).

The bit codecs' kernels have special code at a few places of a block: the interleaved parity
positions of the Hamming head, bit 0, the last used bit L and the unused tail behind it, the owner
lane and LDS word of a correction, the 16-byte pieces and 1 KiB rows of the streaming kernels, the
kept low bits after a CRC field, the parity byte's fix bit.  Flips drawn uniformly over a block of
1-4 KiB almost never land there, so this module aims them, class by class, and takes every expected
result from the oracle (the payload of an undetected or miscorrected block included).

  ham_layout(bs)                              the reference's Hamming bit iterators, walked in Python
  bit_set(oracle, codec, bs, poly=0, seed=0)  the block set of one code with the oracle's results

codec is "ham", "crc" or "par"; poly is the CRC polynomial in the implicit form the GPU tests'
case lists use (oracle.crc_explicit(poly) is the explicit one).  The recipes only propose flips;
what a class means in the oracle's output is pinned by tests/test_bit_craft.py.

Classes (labels; kinds holds a finer name per block, flips the flipped raw bit positions):
  Hamming  clean, single, tail, tail+single, double, triple->payload, triple->parity, triple->bit0,
           triple->tail, quad0, quad
  CRC      clean, single, tail, tail+single, double, poly@s
  parity   clean, single, double, triple
A class that a code cannot hold (a CRC of whole bytes has no tail; a 1-byte Hamming block has three
used bits) is listed in not_applicable with the reason.
"""
from __future__ import annotations

import itertools
import zlib

import numpy as np

_SETS = {}
_LAYOUTS = {}

HAM_CLASSES = ("clean", "single", "tail", "tail+single", "double", "triple->payload", "triple->parity",
               "triple->bit0", "triple->tail", "quad0", "quad")
CRC_CLASSES = ("clean", "single", "tail", "tail+single", "double", "poly@s")
PAR_CLASSES = ("clean", "single", "double", "triple")
CLASSES = {"ham": HAM_CLASSES, "crc": CRC_CLASSES, "par": PAR_CLASSES}

# the codes whose sets the tests pin and run, (codec, implicit polynomial, block size): Hamming on
# the thread-per-block kernels (1, 2, 4), the wave-per-block kernel (8, 64, 512) and the streaming
# kernels of 1, 2 and 4 rows; CRC on the generic and on the streaming kernels (degrees 3, 8, 20, 62 /
# 20, 29, 25, 32); parity on both
HAM_CODES = [("ham", 0, bs) for bs in (1, 2, 4, 8, 64, 512, 1024, 2048, 4096)]
CRC_CODES = [("crc", 0x5, 64), ("crc", 0xea, 256), ("crc", 0xc1acf, 512), ("crc", 0x42F0E1EBA9EA3693 >> 1, 1024),
             ("crc", 0xc1acf, 1024), ("crc", 0x1EDC6F41, 2048), ("crc", 0x1000003, 4096), ("crc", 0x9960034c, 4096)]
PAR_CODES = [("par", 0, bs) for bs in (2, 255, 256, 1024, 4096)]
CODES = HAM_CODES + CRC_CODES + PAR_CODES


def code_id(c):
    return f"{c[0]}-{c[2]}" + (f"-{c[1]:x}" if c[1] else "")


def _pow2(x):
    return x != 0 and (x & (x - 1)) == 0


class HamLayout:
    """The bit layout of one Hamming block size, from the reference's two iterators
    (oracle/ppfs_oracle.c ham_data_next / ham_used_next, walked literally):
    data_pos  raw position of payload bit i;  L  the last of them (None without a payload)
    used      the positions the decode reads, ascending;  tail  every other position of the block
    parity    the positions 2^j < bits;  top  the largest position a flip may take where a class keeps
              its flips "at or below L" (L, or the largest used bit where there is no payload)."""

    def __init__(self, block_size):
        p = 0
        while (1 << (p + 1)) <= block_size:
            p += 1
        self.bs = bs = 1 << p
        self.ds = ds = bs - (p * 3 + 1 + 7) // 8
        self.bits = bits = 8 * bs
        # HammingDataBitsIterator
        data_pos, cur = [], 0
        for _ in range(8 * ds):
            while (cur & (cur - 1)) == 0:
                cur += 1
            data_pos.append(cur)
            cur += 1
        # HammingUsedBitsIterator
        used, cur, next_parity, returned, limit = [], 0, 1, 0, 8 * ds
        while True:
            if returned >= limit and next_parity >= bits:
                break
            if returned >= limit:
                cur = next_parity
                next_parity <<= 1
                used.append(cur)
                continue
            if _pow2(cur):
                next_parity = cur << 1
            if cur and not _pow2(cur):
                returned += 1
            used.append(cur)
            cur += 1
        self.data_pos = np.array(data_pos, np.int64)
        self.L = int(data_pos[-1]) if data_pos else None
        self.used = sorted(set(used))
        self.used_set = set(used)
        self.tail = [q for q in range(bits) if q not in self.used_set]
        self.parity = [1 << j for j in range(bits.bit_length()) if (1 << j) < bits]
        self.top = self.L if self.L is not None else max(self.used)
        self.data_set = set(data_pos)


def ham_layout(bs) -> HamLayout:
    if bs not in _LAYOUTS:
        _LAYOUTS[bs] = HamLayout(bs)
    return _LAYOUTS[bs]


def _xor(ps):
    x = 0
    for p in ps:
        x ^= int(p)
    return x


def _find(rng, pool, k, ok, tries=20000):
    """k distinct positions of pool for which ok(tuple) holds: seeded draws, then (small pools only) an
    exhaustive walk.  None where there is none."""
    pool = list(pool)
    if len(pool) < k:
        return None
    for _ in range(tries if len(pool) > 24 else 0):
        c = tuple(sorted(int(pool[i]) for i in rng.choice(len(pool), k, replace=False)))
        if ok(c):
            return c
    if len(pool) <= 64:
        for c in itertools.combinations(pool, k):
            if ok(c):
                return tuple(int(x) for x in c)
    return None


def _completing(rng, pool, k, target, extra=lambda c: True):
    """k distinct positions of pool whose XOR is target: k - 1 drawn, the last one solved for."""
    pool = [int(x) for x in pool]
    pset = set(pool)
    if len(pool) < k:
        return None
    for _ in range(20000 if len(pool) > 24 else 0):
        head = [pool[i] for i in rng.choice(len(pool), k - 1, replace=False)]
        last = target ^ _xor(head)
        c = tuple(sorted(head + [last]))
        if last in pset and last not in head and extra(c):
            return c
    if len(pool) <= 64:
        for c in itertools.combinations(pool, k):
            if _xor(c) == target and extra(c):
                return c
    return None


# ------------------------------------------------------------------------------------
# recipes: [(label, kind, flipped positions)] and {label: why it cannot exist}
# ------------------------------------------------------------------------------------
def _ham_recipes(rng, lay):
    bits, L, top = lay.bits, lay.L, lay.top
    used, tail, data = lay.used_set, lay.tail, lay.data_pos
    low = [q for q in lay.used if q <= top]  # "at or below L"
    out, na = [], {}

    def add(label, kind, flips):
        out.append((label, kind, tuple(int(f) for f in flips)))

    # single
    seen = set()

    def single(kind, q):
        if q in used and q not in seen and (q <= top or _pow2(q)):
            seen.add(q)
            add("single", kind, (q,))

    single("bit0", 0)
    for q in lay.parity:
        single("parity", q)
    for q in range(3, 73):
        if not _pow2(q):
            single("head", q)
    for q in (127, 128, 129):
        single("piece16", q)
    for q in (8191, 8192, 8193, 16383, 16385, 24575, 24577):
        single("piece1k", q)
    if lay.bs >= 4:
        single("lastword", 32 * (lay.bs // 4 - 1))
    if L is not None:
        single("L-1", L - 1)
        single("L", L)
        fresh = [int(q) for q in data if int(q) not in seen]
        for q in rng.choice(fresh, min(16, len(fresh)), replace=False) if fresh else ():
            single("payload", int(q))
    # tail, exhaustively
    for q in tail:
        add("tail", "tail", (q,))
    # tail + one used bit (a payload bit where there is a payload)
    partners = [int(data[0]), int(L), int(data[data.size // 2])] if L is not None else list(lay.used)
    for i, q in enumerate([tail[0], tail[-1], tail[len(tail) // 2]]):
        add("tail+single", "tail+single", (q, partners[i % len(partners)]))
    # double
    if L is not None and data.size >= 2:
        if bits > 8192:
            lo, hi = data[data < 8192], data[data >= 8192]
            pairs = [(int(rng.choice(lo)), int(rng.choice(hi))), (int(lo[0]), int(hi[-1])), (int(lo[-1]), int(hi[0]))]
        else:
            pairs = [(int(data[0]), int(data[-1])), (int(data[1]), int(data[data.size // 2]))]
        for pr in pairs:
            add("double", "pieces", pr)
        same = [(a, b) for a, b in zip(data[:-1], data[1:]) if a // 8 == b // 8]
        for j in sorted({0, len(same) // 2, len(same) - 1}):
            add("double", "byte", same[j])
        if 0 in used:
            add("double", "bit0+payload", (0, int(data[0])))
            add("double", "bit0+payload", (0, L))
    if 0 in used:
        add("double", "bit0+parity", (0, 1))
        add("double", "bit0+parity", (0, lay.parity[-1]))
    add("double", "parity+parity", (1, 2))
    add("double", "parity+parity", (lay.parity[0], lay.parity[-1]))
    add("double", "parity+parity", (lay.parity[-2], lay.parity[-1]))

    # triples, all three flips at or below L
    def triples(label, targets, want):
        got = 0
        for tg in targets:
            if got >= want:
                break
            c = _completing(rng, low, 3, tg)
            if c is not None:
                add(label, f"->{tg}", c)
                got += 1
        return got

    if L is not None:
        cand = [int(data[0])] + [int(q) for q in data if q < 72][-1:] + [q for q in (129, 8193) if q in lay.data_set] \
            + [L - 1, L] + [int(q) for q in rng.choice(data, min(4, data.size), replace=False)]
        if not triples("triple->payload", list(dict.fromkeys(cand)), 6):
            na["triple->payload"] = "no three used bits XOR to a payload position"
    else:
        na["triple->payload"] = "no payload bits"
    par = lay.parity
    if not triples("triple->parity", list(dict.fromkeys([1, par[len(par) // 2], par[-1], 2, 4])), 3):
        na["triple->parity"] = "no three used bits XOR to a parity position"
    n0 = 0
    if 0 in used:
        if all(q in used and q <= top for q in (3, 5, 6)):
            add("triple->bit0", "->0", (3, 5, 6))
            n0 += 1
        for _ in range(2):
            c = _completing(rng, [q for q in low if q], 3, 0)
            if c is not None:
                add("triple->bit0", "->0", c)
                n0 += 1
    if not n0:
        na["triple->bit0"] = "bit 0 is not a used bit" if 0 not in used else "no three used bits XOR to 0"
    spread = [tail[i] for i in sorted({0, len(tail) // 3, 2 * len(tail) // 3, len(tail) - 1})]
    triples("triple->tail", spread + [q for q in tail if q not in spread], min(4, len(tail)))
    # four flips
    nz = [q for q in low if q]
    nq = 0
    for _ in range(3):
        c = _completing(rng, nz, 4, 0, extra=lambda c: any(q in lay.data_set for q in c))
        if c is not None and ("quad0", "quad0", c) not in out:
            add("quad0", "quad0", c)
            nq += 1
    if not nq:
        na["quad0"] = "fewer than four used bits XOR to 0 with a payload bit among them"
    nq = 0
    for j in range(3):
        pool = lay.used if j == 0 else nz
        c = _find(rng, pool, 4, lambda c: _xor(c) != 0)
        if c is not None:
            add("quad", "quad", c)
            nq += 1
    if not nq:
        na["quad"] = "fewer than four used bits"
    return out, na


def _crc_recipes(rng, bs, P):
    n = P.bit_length() - 1
    ds = bs - (n + 7) // 8
    end = 8 * ds + n
    lim = end - (n + 1)  # the reference's division stops here: offsets below it go undetected
    out, na = [], {}

    def add(label, kind, flips):
        out.append((label, kind, tuple(int(f) for f in flips)))

    for q in (0, 127, 128, 8191, 8192):
        if q < 8 * ds - 2:
            add("single", "payload", (q,))
    add("single", "payload", (8 * ds - 2,))
    add("single", "last-payload-bit", (8 * ds - 1,))
    for q in range(8 * ds, end):
        add("single", "field", (q,))
    tail = list(range(end, 8 * bs))
    for q in tail:
        add("tail", "tail", (q,))
    if tail:
        for i, q in enumerate([tail[0], tail[-1]]):
            add("tail+single", "tail+single", (q, (0, 8 * ds - 2)[i]))
        add("tail+single", "tail+field", (tail[0], end - 1))
    else:
        na["tail"] = na["tail+single"] = "the CRC field ends on a byte boundary"
    add("double", "double", (127, 128) if 8 * ds - 2 > 128 else (3, 4))
    add("double", "double", (0, 8 * ds - 2))
    # a seeded pair 2..n bits apart.  The stored field drops the remainder's top bit, so a short
    # polynomial lets some pairs through (degree 3: bits 127 and 128): the oracle decides
    a = int(rng.integers(0, 8 * ds - 2 - n))
    add("double", "double", (a, a + 1 + int(rng.integers(1, n))))
    offs = [0, 1, 7]
    for edge in (128, 8192):
        s = edge - (n + 1) // 2
        if 0 <= s < lim - 1 and s + n >= edge:
            offs.append(s)
    offs += [lim - 1, lim]
    for s in dict.fromkeys(offs):
        add("poly@s", f"poly@{s}", [s + j for j in range(n + 1) if (P >> (n - j)) & 1])
    return out, na


def _par_recipes(rng, bs):
    out = []

    def add(label, kind, flips):
        out.append((label, kind, tuple(int(f) for f in flips)))

    pay = 8 * (bs - 1)  # first bit of the parity byte
    seen = set()
    for kind, q in (("payload", 0), ("payload", 127), ("payload", 128), ("last-byte-msb", pay - 8), ("last-byte-lsb", pay - 1),
                    ("parity-msb", pay), ("fix-bit", pay + 7)):
        if (q < pay or kind in ("parity-msb", "fix-bit")) and q not in seen:
            seen.add(q)
            add("single", kind, (q,))
    add("double", "payload+payload", (0, pay - 1))
    add("double", "payload+fix-bit", (int(rng.integers(0, pay)), pay + 7))
    add("double", "parity-byte", (pay, pay + 7))
    add("double", "same-byte", (pay - 8, pay - 1))
    add("triple", "payload", (0, 1, pay - 1))
    add("triple", "payload+parity-byte", (int(rng.integers(0, pay)), pay, pay + 7))
    add("triple", "parity-byte", (pay + 5, pay + 6, pay + 7))
    return out, {}


# ------------------------------------------------------------------------------------
# the block set of one code
# ------------------------------------------------------------------------------------
class BitSet:
    """words (nb, bs) with one label, kind and flip tuple per block; clean (nb, bs) and payloads
    (nb, ds) they were made from; the oracle's decode of words: o_st (nb,), o_fixed (nb, bs: the
    image after the write-back; CRC and parity never write) and o_data (nb, ds; zeros at status 5)."""

    @property
    def nb(self):
        return self.words.shape[0]

    def census(self):
        """{class: block count}, every class of the codec listed (0 where not applicable)."""
        out = {c: 0 for c in CLASSES[self.codec]}
        for l in self.labels:
            out[l] += 1
        return out

    def of(self, label, kind=None):
        return np.array([b for b in range(self.nb) if self.labels[b] == label and (kind is None or self.kinds[b] == kind)],
                        np.int64)

    def batches(self):
        """{name: block indices}, each the whole set: "interleaved" deals the classes round-robin
        (one wave or workgroup meets them all), "sorted" keeps each class together.  The count is
        above 64 and no multiple of 4 (so of 32 neither)."""
        groups = {}
        for b, l in enumerate(self.labels):
            groups.setdefault(l, []).append(b)
        a = [g[i] for i in range(max(len(g) for g in groups.values())) for g in groups.values() if i < len(g)]
        out = {"interleaved": np.array(a, np.int64),
               "sorted": np.array(sorted(range(self.nb), key=lambda i: (self.labels[i], i)), np.int64)}
        for v in out.values():
            assert v.size == self.nb and v.size > 64 and v.size % 4 != 0
        return out

    def encode(self, oracle, data, raw_old):
        if self.codec == "ham":
            return oracle.ham_encode(self.bs, data, raw_old=raw_old)
        if self.codec == "crc":
            return oracle.crc_encode(self.bs, self.P, data, raw_old=raw_old)
        return oracle.parity_encode(self.bs, data, raw_old=raw_old)

    def decode(self, oracle, raw):
        """-> (data, status, fixed) of the oracle."""
        raw = np.ascontiguousarray(raw, np.uint8).reshape(-1)
        if self.codec == "ham":
            d, st, fixed, _ = oracle.ham_decode(self.bs, raw)
            return d, st, fixed
        if self.codec == "crc":
            d, st = oracle.crc_check(self.bs, self.P, raw)
        else:
            d, st = oracle.parity_check(self.bs, raw)
        return d, st, raw.copy()


def _flip(words, b, flips):
    for f in flips:
        words[b, f // 8] ^= 0x80 >> (f % 8)


def bit_set(oracle, codec, bs, poly=0, seed=0) -> BitSet:
    """The crafted block set of one code with the oracle's expectations; cached per argument tuple.
    Every block starts from a valid codeword that the oracle encoded over random old contents (so the
    unused tail bits are random); the first clean block has an all-zero payload, the second all 0xFF.
    Clean blocks fill the set up until at most a third of it has oracle status 5, it holds more than
    64 blocks and the count is no multiple of 4; a code with few recipes repeats them on fresh
    codewords."""
    key = (codec, bs, poly, seed)
    if key in _SETS:
        return _SETS[key]
    rng = np.random.default_rng(zlib.crc32(repr(("bit_craft",) + key).encode()))
    s = BitSet()
    s.codec, s.bs, s.poly = codec, bs, poly
    if codec == "ham":
        s.layout = ham_layout(bs)
        assert s.layout.bs == bs, "Hamming block sizes are powers of two"
        s.P, s.ds = 0, s.layout.ds
        assert s.ds == oracle.ham_data_size(bs)
        recipes, na = _ham_recipes(rng, s.layout)
    elif codec == "crc":
        s.P = oracle.crc_explicit(poly)
        s.deg = s.P.bit_length() - 1
        s.ds = oracle.crc_data_size(bs, s.P)
        s.end = 8 * s.ds + s.deg
        recipes, na = _crc_recipes(rng, bs, s.P)
    else:
        assert codec == "par"
        s.P, s.ds = 0, bs - 1
        recipes, na = _par_recipes(rng, bs)
    recipes = recipes * max(1, -(-48 // len(recipes)))
    m, ds = len(recipes), s.ds

    def build(nclean):
        nb = m + nclean
        pay = rng.integers(0, 256, (nb, ds), dtype=np.uint8)
        pay[m:m + 1] = 0
        pay[m + 1:m + 2] = 0xFF
        old = rng.integers(0, 256, nb * bs, dtype=np.uint8)
        clean = s.encode(oracle, pay.reshape(-1), old).reshape(nb, bs)
        words = clean.copy()
        for b, (_, _, flips) in enumerate(recipes):
            _flip(words, b, flips)
        return pay, clean, words

    # the oracle decides how many recipes end in status 5; the clean count follows from that
    _, _, words = build(0)
    n5 = int((s.decode(oracle, words)[1] == 5).sum())
    nclean = max(4, 3 * n5 - m)
    while m + nclean <= 64 or (m + nclean) % 4 == 0:
        nclean += 1
    s.payloads, s.clean, s.words = build(nclean)
    s.labels = [r[0] for r in recipes] + ["clean"] * nclean
    s.kinds = [r[1] for r in recipes] + ["clean"] * nclean
    s.flips = [r[2] for r in recipes] + [()] * nclean
    s.not_applicable = na
    d, st, fixed = s.decode(oracle, s.words)
    s.o_data, s.o_st, s.o_fixed = d.reshape(s.nb, ds), st, fixed.reshape(s.nb, bs)
    for a in (s.words, s.clean, s.payloads, s.o_data, s.o_st, s.o_fixed):
        a.setflags(write=False)
    _SETS[key] = s
    return s
