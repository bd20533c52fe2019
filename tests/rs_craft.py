"""Syndrome-crafted Reed-Solomon words -- TEST ONLY (pure numpy / Python, no engine import).

The RS decoders take shortcuts (geometric syndromes, S2/S1 pairs, closed forms for sigma of
degree 1 and 2, a root search from degree 3 up) that must equal the reference's literal
Berlekamp-Massey / root scan / Forney.  "Codeword plus random byte errors" reaches most of those
branches only by luck, so this module builds words with chosen syndromes instead.

The syndrome map restricted to any 2t distinct byte positions p_j < n is an invertible Vandermonde
system: S_i = sum_j e_j alpha^(i p_j), i = 1..2t.  For any target vector S there is therefore a word
"codeword + 2t chosen bytes" with exactly those syndromes (word_with_syndromes).  Conventions are the
oracle's: alpha = 2, S_i = c(alpha^i), word byte m is the coefficient of x^m, parity in bytes
0..2t-1; the field tables come from Oracle.gf_dump().

  field(oracle)                         the field tables (cached)
  syndromes(words, two_t)               table model of S_1..S_2t
  word_with_syndromes(cw, S, support)   the word on `cw` with syndromes S, changed on `support` only
  lfsr_syndromes(sigma, first_L, two_t) first_L free syndromes extended by sigma's recurrence
  classify(S, n)                        literal BM + root scan: what the reference does with S
  classes_of(info, two_t, n)            the decode-branch classes a word belongs to
  branch_set(oracle, bs, t, seed)       the block set of one code with the oracle's expectations

The recipes of branch_set only propose inputs; classify decides which class a word belongs to
(tests/test_rs_craft.py pins, per t, the classes the set must hold).
"""
from __future__ import annotations

import zlib

import numpy as np

_FIELD = None
_INVERSES = {}
_SETS = {}


class Field:
    def __init__(self, oracle):
        g = oracle.gf_dump()
        self.mul = g["mul"]  # mul[a, b]
        self.div = g["div"]  # div[a, b] = a / b (0 when either is 0)
        self.mul_rows = [bytes(r) for r in self.mul]  # scalar lookups: mul_rows[a][b]
        self.div_rows = [bytes(r) for r in self.div]
        ap = [1]
        for _ in range(254):
            ap.append(self.mul_rows[ap[-1]][2])
        assert len(set(ap)) == 255 and self.mul_rows[ap[-1]][2] == 1, "alpha = 2 must be primitive"
        self.apow_list = ap
        self.apow = np.array(ap, np.uint8)  # alpha^i, i = 0..254


def field(oracle=None) -> Field:
    global _FIELD
    if _FIELD is None:
        assert oracle is not None, "field(oracle) must be called once before the oracle-free helpers"
        _FIELD = Field(oracle)
    return _FIELD


def syndromes(words, two_t):
    """S[b, i-1] = sum_m words[b, m] alpha^(i m), i = 1..2t (the table model)."""
    f = field()
    w = np.atleast_2d(np.asarray(words, np.uint8))
    nb, n = w.shape
    S = np.zeros((nb, two_t), np.uint8)
    m = np.arange(n)
    for i in range(1, two_t + 1):
        S[:, i - 1] = np.bitwise_xor.reduce(f.mul[w, f.apow[(i * m) % 255][None, :]], axis=1)
    return S


def _inverse(two_t, support):
    """Inverse of V[i, j] = alpha^((i+1) p_j) over GF(256) by Gauss-Jordan, cached per (t, support)."""
    key = (two_t, tuple(int(p) for p in support))
    inv = _INVERSES.get(key)
    if inv is not None:
        return inv
    f = field()
    p = np.asarray(key[1], np.int64)
    assert p.size == two_t and np.unique(p).size == two_t and p.min() >= 0 and p.max() < 255
    A = np.concatenate([f.apow[(np.arange(1, two_t + 1)[:, None] * p[None, :]) % 255],
                        np.eye(two_t, dtype=np.uint8)], axis=1)
    for c in range(two_t):
        piv = c + int(np.nonzero(A[c:, c])[0][0])  # a Vandermonde system of distinct points: always found
        if piv != c:
            A[[c, piv]] = A[[piv, c]]
        A[c] = f.div[A[c], A[c, c]]
        rows = np.nonzero(A[:, c])[0]
        rows = rows[rows != c]
        A[rows] ^= f.mul[A[rows, c][:, None], A[c][None, :]]
    inv = np.ascontiguousarray(A[:, two_t:])
    _INVERSES[key] = inv
    return inv


def word_with_syndromes(codeword, S, support):
    """codeword(s) XOR the error on `support` (2t distinct positions < n) that has syndromes S.
    codeword: (n,) or (nb, n); S: (2t,) or (nb, 2t).  The codeword must be valid (zero syndromes)."""
    f = field()
    cw = np.array(codeword, np.uint8, copy=True)
    S2 = np.atleast_2d(np.asarray(S, np.uint8))
    two_t = S2.shape[1]
    if two_t == 0:
        return cw
    w = cw.reshape(S2.shape[0], -1)
    support = np.asarray(support, np.int64)
    assert support.max() < w.shape[1]
    inv = _inverse(two_t, support)
    e = np.bitwise_xor.reduce(f.mul[inv[None, :, :], S2[:, None, :]], axis=2)  # e_j = sum_i inv[j, i] S_i
    w[:, support] ^= e
    return cw


def lfsr_syndromes(sigma, first_L, two_t):
    """first_L free syndromes, then S_n = sum_{i>=1} sigma_i S_{n-i} (sigma[0] = 1)."""
    mul = field().mul_rows
    S = [int(x) for x in first_L][:two_t]
    for n in range(len(S), two_t):
        s = 0
        for i in range(1, len(sigma)):
            if n - i >= 0:
                s ^= mul[sigma[i]][S[n - i]]
        S.append(s)
    return S


def is_geometric(S):
    """All S_i non-zero with a constant ratio S_{i+1} / S_i."""
    f = field()
    S = [int(x) for x in S]
    if not S or any(s == 0 for s in S):
        return False
    if len(S) == 1:
        return True
    r = f.div_rows[S[1]][S[0]]
    return all(f.mul_rows[S[i]][r] == S[i + 1] for i in range(len(S) - 1))


def classify(S, n=255):
    """What the reference's decode does with syndromes S: Berlekamp-Massey as
    rs_block_device.cpp:234-269 states it (tests/ref_model.py rs_decode), then the root scan over
    v = alpha^m, m = 0..254.  A root alpha^m corrects byte 0 for m = 0, else byte 255 - m."""
    f = field()
    mul, div = f.mul_rows, f.div_rows
    S = [int(x) for x in S]
    two_t = len(S)
    sigma, B = [1], [1]
    b, L, m = 1, 0, 1
    for nn in range(two_t):
        d = S[nn]
        for i in range(1, L + 1):
            if i < len(sigma):
                d ^= mul[sigma[i]][S[nn - i]]
        if d:
            T = sigma[:]
            c = div[d][b]
            diff = [0] * m + [mul[c][x] for x in B]
            ln = max(len(sigma), len(diff))
            sigma = [(sigma[i] if i < len(sigma) else 0) ^ (diff[i] if i < len(diff) else 0) for i in range(ln)]
            if 2 * L <= nn:
                L = nn + 1 - L
                B, b, m = T, d, 1
            else:
                m += 1
        else:
            m += 1
    while len(sigma) > 1 and sigma[-1] == 0:
        sigma.pop()
    deg = len(sigma) - 1
    ms = np.arange(255)
    val = np.zeros(255, np.uint8)
    dval = np.zeros(255, np.uint8)
    for i, c in enumerate(sigma):
        if c:
            val ^= f.mul[c, f.apow[(i * ms) % 255]]
            if i & 1:
                dval ^= f.mul[c, f.apow[((i - 1) * ms) % 255]]
    roots = [int(x) for x in np.nonzero(val == 0)[0]]
    positions = [0 if r == 0 else 255 - r for r in roots]
    return {
        "deg": deg,
        "L": L,
        "sigma": sigma,
        "roots": roots,
        "positions": positions,
        "clean": not any(S),
        "geometric": is_geometric(S),
        "geometric_but_last": two_t >= 3 and is_geometric(S[:-1]) and not is_geometric(S),
        "sig1_zero": deg >= 1 and sigma[1] == 0,
        "dsig_zero_at_root": any(dval[r] == 0 for r in roots),
        "zero_syndromes": sum(1 for s in S if s == 0),
        "root_beyond_n": any(p >= n for p in positions),
    }


def classes_of(info, two_t, n=255):
    """The decode-branch classes of a word, from classify's result alone."""
    c = set()
    if info["clean"]:
        return {"clean"}
    deg, L, nr = info["deg"], info["L"], len(info["roots"])
    if info["geometric"]:
        c.add("geometric")
    if info["geometric_but_last"]:
        c.add("geometric_but_last")
    if info["zero_syndromes"]:
        c.add("some_S_zero")
    if deg == 0:
        c.add("deg0")
    if deg == 1 and not info["geometric"]:
        c.add("deg1_not_geometric")
    if deg == 1 and L > 1:
        c.add("deg1_L_gt_1")
    if deg == 2:
        if info["sig1_zero"]:
            c.add("deg2_double_root")
        elif nr == 0:
            c.add("deg2_no_roots")
        else:
            c.add("deg2_two_roots")
            if set(info["roots"]) == {0, 1}:
                c.add("deg2_roots_byte0_byte254")
    if deg >= 3:
        if info["dsig_zero_at_root"]:
            c.add("deg3p_repeated_root")
        if 0 < nr < deg:
            c.add("deg3p_fewer_roots")
        if nr == 0:
            c.add("deg3p_no_roots")
        if nr == deg:
            c.add("deg3p_all_roots")
        if deg < L:
            c.add("deg3p_lt_L")
    if deg < L:
        c.add("deg_lt_L")
    if deg == two_t:
        c.add("deg_2t")
    if info["dsig_zero_at_root"]:
        c.add("dsig_zero_at_root")
    if 0 in info["roots"]:
        c.add("root_m0_byte0")
    if info["root_beyond_n"]:
        c.add("root_beyond_n")
    return c


# ------------------------------------------------------------------------------------
# the block set of one code
# ------------------------------------------------------------------------------------
def _rootless(rng, deg, tries=4000):
    """A random monic-at-zero polynomial 1 + ... of exactly this degree without a root in GF(256)*."""
    f = field()
    ms = np.arange(255)
    for _ in range(tries):
        sig = [1] + [int(x) for x in rng.integers(0, 256, deg - 1)] + [int(rng.integers(1, 256))]
        val = np.zeros(255, np.uint8)
        for i, c in enumerate(sig):
            if c:
                val ^= f.mul[c, f.apow[(i * ms) % 255]]
        if val.all():
            return sig
    raise AssertionError("no rootless polynomial found")


def _pmul(a, b):
    mul = field().mul_rows
    r = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            r[i + j] ^= mul[x][y]
    return r


def _locator(positions):
    """prod (1 + alpha^p x): the locator of errors at these byte positions."""
    ap = field().apow_list
    s = [1]
    for p in positions:
        s = _pmul(s, [1, ap[p % 255]])
    return s


def _recipes(rng, n, t):
    """-> (syndrome entries [(label, S)], error entries [(label, {position: value})])."""
    f = field()
    ap, mul = f.apow_list, f.mul_rows
    two_t = 2 * t
    syn, err = [], []

    def nz(k=None):
        return int(rng.integers(1, 256)) if k is None else [int(x) for x in rng.integers(1, 256, k)]

    def rnd(k):
        return [int(x) for x in rng.integers(0, 256, k)]

    def geo(s1, p):
        return [mul[s1][ap[(p * i) % 255]] for i in range(two_t)]

    # single error, exhaustively: every position with 0x01, 0x80, 0xFF (every XP row; positions
    # < 2t are the rows full of 0xFF markers)
    for p in range(n):
        for v in (0x01, 0x80, 0xFF):
            err.append(("single", {p: v}))
    for _ in range(8):
        err.append(("clean", {}))
    if two_t == 0:
        return syn, err

    # geometric, broken once at S_i (1-based): i = 2t (the shortcut's loop bound), 3, t, t + 1, the
    # 2t = 32 pair's lane boundary 16 | 17, and i = 1 (S_1 zeroed gives sigma of degree 1 with L = 2)
    where = [two_t, 3, t, t + 1, 1, 2] + ([16, 17] if two_t == 32 else [])
    where = sorted({i for i in where if 1 <= i <= two_t})
    for i in where:
        for p in (0, 1, 2 * t, 100 % max(n, 1), 254):
            S0 = geo(nz(), p)
            for v in (0x01, nz(), S0[i - 1]):  # the last one zeroes S_i
                S = list(S0)
                S[i - 1] ^= v
                syn.append((f"geo_broken@{'last' if i == two_t else i}", S))
    # virtual single errors at every "position" class: for n < 255 the roots land past the block
    for p in sorted({n % 255, (n + 1) % 255, 254, 200, 128}):
        for _ in range(2):
            syn.append(("geo_virtual", geo(nz(), p)))

    # zero syndromes
    for _ in range(4):
        syn.append(("only_S1", [nz()] + [0] * (two_t - 1)))
        syn.append(("only_S2t", [0] * (two_t - 1) + [nz()]))
        syn.append(("S1_zero", [0] + rnd(two_t - 1)))
        syn.append(("S2_zero", [nz(), 0] + rnd(two_t - 2)))
        if two_t >= 4:
            syn.append(("S1_S2_zero", [0, 0] + rnd(two_t - 2)))

    if t >= 2:
        # deg 2, double root: sigma = 1 + c x^2 (c = 1: the root is v = 1, byte 0)
        for c in (1, 2, ap[254], nz(), nz(), nz()):
            syn.append(("deg2_double", lfsr_syndromes([1, 0, c], nz(2), two_t)))
        # deg 2 without roots
        for _ in range(6):
            syn.append(("deg2_rootless", lfsr_syndromes(_rootless(rng, 2), nz(2), two_t)))
        # deg 2, two roots: v = 1 (m = 0, byte 0) and v = alpha (m = 1, byte 254); other pairs
        for pair in ((0, 254), (0, 254), (0, 254), (0, 1), (254, 253), (2 * t - 1, 2 * t), (7, 130), (n - 1, 0)):
            syn.append(("deg2_two_roots", lfsr_syndromes(_locator(pair), nz(2), two_t)))
        # deg < L: a recurrence that starts one syndrome late
        for _ in range(4):
            syn.append(("deg1_late", lfsr_syndromes([1, nz()], nz(2), two_t)))
    if t >= 3:
        for _ in range(6):
            a, b2 = rng.choice(255, 2, replace=False)
            syn.append(("deg3_repeated", lfsr_syndromes(_pmul(_pmul([1, ap[a]], [1, ap[a]]), [1, ap[b2]]), nz(3), two_t)))
            syn.append(("deg3_fewer_roots", lfsr_syndromes(_pmul([1, ap[a]], _rootless(rng, 2)), nz(3), two_t)))
            syn.append(("deg3_rootless", lfsr_syndromes(_rootless(rng, 3), nz(3), two_t)))
            syn.append(("deg2_late", lfsr_syndromes(_locator((int(a), int(b2))), nz(3), two_t)))
    if t >= 4:
        for _ in range(6):
            pos = [int(x) for x in rng.choice(255, 3, replace=False)]
            syn.append(("deg3_late", lfsr_syndromes(_locator(pos), nz(4), two_t)))
            pos = [int(x) for x in rng.choice(255, t, replace=False)]
            syn.append(("degt_locator", lfsr_syndromes(_locator(pos), nz(t), two_t)))
            syn.append(("degt_rootless", lfsr_syndromes(_rootless(rng, t), nz(t), two_t)))
    # structured families whose BM result is not fixed in advance (L > t): leading zeros
    for z in range(1, min(two_t, 6)):
        for _ in range(3):
            syn.append((f"lead_zeros_{z}", [0] * z + nz(two_t - z)))

    # genuine t-error patterns whose positions include 0, n - 1 (254), 2t - 1 and 2t
    special = [p for p in (0, n - 1, two_t - 1, two_t) if 0 <= p < n]
    for r in range(8):
        want = [special[(r + j) % len(special)] for j in range(min(t, len(special)))]
        pos = list(dict.fromkeys(want))
        while len(pos) < min(t, n):
            p = int(rng.integers(0, n))
            if p not in pos:
                pos.append(p)
        err.append(("t_errors", {p: nz() for p in pos}))

    # uniform random syndromes
    for _ in range(512):
        syn.append(("random", rnd(two_t)))
    return syn, err


class BranchSet:
    """words (nb, n), one label per block, the target syndromes, and the oracle's decode of the words:
    o_data (nb, k), o_st (nb,), o_fixed (nb, n), o_wbl (nb,), and for n < 255 o_spill (nb, 256 - n):
    the engine's spill record [bytes past the block, those bytes, zeros]."""

    def __init__(self, bs, t, n, k):
        self.bs, self.t_arg, self.n, self.k = bs, t, n, k
        self.two_t = n - k
        self.t = self.two_t // 2
        self._info = None

    @property
    def nb(self):
        return self.words.shape[0]

    def info(self):
        """classify() of every block's actual syndromes (cached)."""
        if self._info is None:
            self._info = [classify(s, self.n) for s in self.S]
        return self._info

    def census(self):
        """{class: block count} by classify."""
        out = {}
        for i in self.info():
            for c in classes_of(i, self.two_t, self.n):
                out[c] = out.get(c, 0) + 1
        return out

    def general(self):
        """Indices of the blocks that take the general path: neither clean nor geometric."""
        return np.array([b for b in range(self.nb) if self.S[b].any() and not is_geometric(self.S[b])], np.int64)

    def clean(self):
        return np.array([b for b in range(self.nb) if not self.S[b].any()], np.int64)

    def batches(self):
        """{name: block indices}.  Each batch ends on a ragged 64-block tile.
        a: classes interleaved (seeded shuffle); b: sorted by label (whole tiles of one class);
        c: tiles of clean blocks with exactly one general-path block, at lane 0, 31, 32, 63 in turn."""
        rng = np.random.default_rng(zlib.crc32(repr(("batches", self.bs, self.t_arg)).encode()))
        a = rng.permutation(self.nb)
        b = np.array(sorted(range(self.nb), key=lambda i: (self.labels[i], i)), np.int64)
        cl, gen = self.clean(), self.general()
        out = {"interleaved": a, "sorted": b}
        if gen.size:
            tiles = []
            for j, lane in enumerate((0, 31, 32, 63) * 2):
                tile = cl[(np.arange(64) + j) % cl.size].copy()
                tile[lane] = gen[(j * max(1, gen.size // 8)) % gen.size]
                tiles.append(tile)
            tiles.append(cl[:5])
            out["lone_general"] = np.concatenate(tiles)
        for v in out.values():
            assert v.size % 64 != 0
        return out


def branch_set(oracle, bs, t, seed=0, max_blocks=None) -> BranchSet:
    """The crafted block set of RS(bs, t) with the oracle's expectations; cached per (bs, t, seed,
    max_blocks).  Every class sits on a random valid codeword.  Supports: the parity bytes 0..2t-1
    (any n >= 2t), and for n = 255 also 2t random payload positions that include byte 254.
    max_blocks: an even subsample of the recipes (for 2t near 254, where each block is expensive).
    Words for which the reference's behaviour is undefined (its fixed 256-entry polynomial buffers
    overflow: possible only when 2t + deg(sigma) > 256) have no expectation and are left out; for
    every other code the whole set must decode with rc == 0."""
    key = (bs, t, seed, max_blocks)
    if key in _SETS:
        return _SETS[key]
    field(oracle)
    n, k, tt = oracle.rs_sizes(bs, t)
    two_t = 2 * tt
    rng = np.random.default_rng(zlib.crc32(repr(("rs_craft", bs, t, seed)).encode()))
    syn, err = _recipes(rng, n, tt)
    entries = [("E", l, e) for l, e in err] + [("S", l, s) for l, s in syn]
    if max_blocks is not None and len(entries) > max_blocks:
        # an even subsample per label, so no recipe is dropped before the block budget allows
        by = {}
        for e in entries:
            by.setdefault(e[1], []).append(e)
        share = max(1, max_blocks // len(by))
        entries = []
        for group in by.values():
            picks = np.unique(np.linspace(0, len(group) - 1, min(share, len(group))).astype(int))
            entries += [group[i] for i in picks]
        entries = entries[:max_blocks]
    nb = len(entries)
    if nb % 64 == 0:
        entries.append(("E", "clean", {}))
        nb += 1
    data = rng.integers(0, 256, nb * k, dtype=np.uint8)
    words = oracle.rs_encode(bs, t, data).reshape(nb, n)
    par = np.arange(two_t)
    sup2 = None
    if n == 255 and two_t and two_t < 255 - two_t:
        sup2 = np.sort(np.concatenate([[254], two_t + rng.choice(254 - two_t, two_t - 1, replace=False)]))
    S = np.zeros((nb, two_t), np.uint8)
    which = np.zeros(nb, np.int64)  # 0: direct error, 1: parity support, 2: payload support
    ns = 0
    for b, (kind, _, x) in enumerate(entries):
        if kind == "E":
            for p, v in x.items():
                words[b, p] ^= v
        else:
            S[b] = x
            which[b] = 1 if (sup2 is None or ns % 2 == 0) else 2
            ns += 1
    for w, sup in ((1, par), (2, sup2)):
        rows = np.nonzero(which == w)[0]
        if rows.size:
            words[rows] = word_with_syndromes(words[rows], S[rows], sup)
    direct = np.nonzero(which == 0)[0]
    if two_t:
        S[direct] = syndromes(words[direct], two_t)
    labels = [e[1] for e in entries]

    o = oracle.rs_decode(bs, t, words.reshape(-1))
    if o[4] != 0:
        assert two_t + 3 > 256, "reference-undefined behaviour in a code whose buffers cannot overflow"
        keep = np.array([oracle.rs_decode(bs, t, words[b])[4] == 0 for b in range(nb)])
        if keep.sum() % 64 == 0:
            keep[np.nonzero(keep)[0][-1]] = False
        words, S, which = words[keep], S[keep], which[keep]
        labels = [l for l, kp in zip(labels, keep) if kp]
        nb = words.shape[0]
        o = oracle.rs_decode(bs, t, words.reshape(-1))
    assert o[4] == 0, "reference-undefined behaviour hit"

    s = BranchSet(bs, t, n, k)
    s.words, s.labels, s.S, s.support = words, labels, S, which
    s.supports = {1: par, 2: sup2}
    s.o_data, s.o_st, s.o_fixed, s.o_wbl = o[0].reshape(nb, k), o[1], o[2].reshape(nb, n), o[3]
    s.o_spill = np.zeros((nb, 256 - n), np.uint8)
    if n < 255:
        for b in np.nonzero(s.o_wbl > n)[0]:
            _, _, fixed, wl, _ = oracle.rs_decode_one_full(bs, t, words[b])
            s.o_spill[b, 0] = wl - n
            s.o_spill[b, 1:1 + wl - n] = fixed[n:wl]
    for a in (s.words, s.S, s.o_data, s.o_st, s.o_fixed, s.o_wbl, s.o_spill):
        a.setflags(write=False)
    _SETS[key] = s
    return s
