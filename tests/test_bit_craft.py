"""CPU tests of the position-crafted bit-codec sets (tests/bit_craft.py) that
tests/test_gpu_bit_branches.py rests on: every class a code can hold is present in its set (so the GPU
comparison cannot pass vacuously), at most a third of a set has status 5, and each class means in the
oracle's output what its name says -- checked from the flips and the oracle's results, so a change of
the oracle cannot quietly empty a class."""
import numpy as np
import pytest

from tests import bit_craft
from tests.bit_craft import CODES, code_id

# classes a code cannot hold, as literals: a silently dropped class fails here
NOT_APPLICABLE = {
    # a 1-byte Hamming block has no payload and the used bits 1, 2, 4: one triple (-> bit 7), no quad
    ("ham", 0, 1): {"triple->payload", "triple->parity", "triple->bit0", "quad0", "quad"},
    # CRC fields of whole bytes have no kept bits behind them
    ("crc", 0xea, 256): {"tail", "tail+single"},
    ("crc", 0x9960034c, 4096): {"tail", "tail+single"},
}


def diffbits(a, b):
    """MSB-first bit positions at which two byte rows differ."""
    return [int(q) for q in np.nonzero(np.unpackbits(np.asarray(a) ^ np.asarray(b)))[0]]


def the_set(oracle, code):
    codec, poly, bs = code
    return bit_craft.bit_set(oracle, codec, bs, poly)


@pytest.mark.parametrize("bs", [c[2] for c in bit_craft.HAM_CODES])
def test_ham_layout_is_the_oracles(oracle, bs):
    """The Python walk of the reference's iterators against the oracle itself: a payload with one
    bit set puts exactly that raw bit (besides parity positions and bit 0) into the codeword, and
    the sizes agree.  Known layouts of the small blocks as literals."""
    lay = bit_craft.ham_layout(bs)
    assert lay.ds == oracle.ham_data_size(bs) and lay.data_pos.size == 8 * lay.ds
    for i in sorted({0, 1, 25, 26, 56, 57, 8 * lay.ds // 2, 8 * lay.ds - 2, 8 * lay.ds - 1}):
        if not 0 <= i < 8 * lay.ds:
            continue
        pay = np.zeros(lay.ds, np.uint8)
        pay[i // 8] = 0x80 >> (i % 8)
        cw = oracle.ham_encode(bs, pay)
        assert [q for q in diffbits(cw, np.zeros(bs, np.uint8)) if q and q & (q - 1)] == [int(lay.data_pos[i])]
    assert set(lay.parity) <= lay.used_set
    assert sorted(lay.used_set | set(lay.tail)) == list(range(8 * bs)) and not lay.used_set & set(lay.tail)
    known = {1: (None, [0, 3, 5, 6, 7]), 2: (12, [13, 14, 15]), 4: (29, [30, 31]), 8: (54, list(range(55, 64))),
             1024: (8173, list(range(8174, 8192))), 4096: (32743, list(range(32744, 32768)))}
    if bs in known:
        assert (lay.L, lay.tail) == known[bs]
    if bs > 1:
        assert lay.tail == list(range(lay.L + 1, 8 * bs)) and lay.used == list(range(lay.L + 1))


@pytest.mark.parametrize("code", CODES, ids=code_id)
def test_census_and_cap(oracle, code):
    s = the_set(oracle, code)
    codec, poly, bs = code
    census = s.census()
    print(f"{code_id(code)} blocks={s.nb} status5={int((s.o_st == 5).sum())}: "
          + ", ".join(f"{c} {census[c]}" for c in bit_craft.CLASSES[codec])
          + (f"; not applicable: {', '.join(sorted(s.not_applicable))}" if s.not_applicable else ""))
    assert set(s.not_applicable) == NOT_APPLICABLE.get(code, set())
    for c in bit_craft.CLASSES[codec]:
        assert (census[c] == 0) == (c in s.not_applicable), c
    assert 3 * int((s.o_st == 5).sum()) <= s.nb
    # a few hundred blocks, under about 3 MB
    assert 64 < s.nb <= 800 and s.words.nbytes <= 3 << 20
    b = s.batches()
    assert set(b) == {"interleaved", "sorted"}
    for idx in b.values():
        assert idx.size > 64 and idx.size % 4 and idx.size % 32
        assert sorted(idx) == list(range(s.nb))
    lab = [s.labels[i] for i in b["sorted"]]
    assert lab == sorted(lab)
    first = [s.labels[i] for i in b["interleaved"][:len(set(s.labels))]]
    assert len(set(first)) == len(first)  # round-robin: one of every class first
    # the flips are what changed, nothing else; the codewords are valid and carry random tails
    for i in range(s.nb):
        assert diffbits(s.words[i], s.clean[i]) == sorted(s.flips[i])
    d, st, _ = s.decode(oracle, s.clean)
    assert not st.any() and np.array_equal(d.reshape(s.nb, -1), s.payloads)
    if s.ds:
        cl = s.of("clean")
        assert not s.payloads[cl[0]].any() and (s.payloads[cl[1]] == 0xFF).all()


@pytest.mark.parametrize("code", bit_craft.HAM_CODES, ids=code_id)
def test_hamming_positions(oracle, code):
    """The places where the Hamming kernels have special code, computed here from the layout, are
    all aimed at."""
    s = the_set(oracle, code)
    lay, bs = s.layout, s.bs
    L, bits = lay.L, lay.bits
    single = {s.flips[i][0] for i in s.of("single")}
    want = set(lay.parity)
    if bs > 1:
        want |= {0, L - 1, L}
        want |= {q for q in range(3, 73) if q & (q - 1) and q <= L}
        want |= {q for q in (127, 128, 129, 8191, 8192, 8193, 16383, 16385, 24575, 24577) if q <= L}
        if bs >= 4:
            want.add(32 * (bs // 4 - 1))
    assert want <= single, sorted(want - single)
    # and 16 seeded payload positions besides (fewer where the block has no other payload bits)
    assert len(s.of("single", "payload")) == min(16, len(lay.data_set - want))
    assert all(q in lay.used_set for q in single)
    assert sorted({s.flips[i][0] for i in s.of("tail")}) == lay.tail
    kinds = {s.kinds[i] for i in s.of("double")}
    assert kinds == ({"parity+parity"} if bs == 1 else {"pieces", "byte", "bit0+payload", "bit0+parity", "parity+parity"})
    if bits > 8192:
        assert any(s.flips[i][0] // 8192 != s.flips[i][1] // 8192 for i in s.of("double", "pieces"))
    assert all(s.flips[i][0] // 8 == s.flips[i][1] // 8 for i in s.of("double", "byte"))
    # three flips at or below L that the reference corrects into the tail: four places of it, or
    # all three tail bits; a 1-byte block has the one triple 1, 2, 4 -> 7
    targets = {bit_craft._xor(s.flips[i]) for i in s.of("triple->tail")}
    assert len(targets) >= (1 if bs == 1 else min(4, len(lay.tail)))
    assert targets <= set(lay.tail)
    for i in s.of("triple->tail"):
        assert all(q <= lay.top and q in lay.used_set for q in s.flips[i])
    for i in s.of("quad0"):
        assert len(set(s.flips[i])) == 4 and 0 not in s.flips[i] and bit_craft._xor(s.flips[i]) == 0
        assert all(q in lay.used_set for q in s.flips[i])
    for i in s.of("quad"):
        assert len(set(s.flips[i])) == 4 and bit_craft._xor(s.flips[i]) != 0


@pytest.mark.parametrize("code", bit_craft.CRC_CODES + bit_craft.PAR_CODES, ids=code_id)
def test_crc_and_parity_positions(oracle, code):
    s = the_set(oracle, code)
    bs, ds = s.bs, s.ds
    single = {s.flips[i][0] for i in s.of("single")}
    if s.codec == "par":
        want = {0, 8 * (bs - 2), 8 * (bs - 1) - 1, 8 * (bs - 1), 8 * bs - 1} | ({127, 128} if bs > 17 else set())
        assert want <= single
        assert {s.kinds[i] for i in s.of("double")} >= {"payload+payload", "payload+fix-bit", "parity-byte"}
        return
    n, end = s.deg, s.end
    assert (n, ds) == (s.P.bit_length() - 1, bs - (n + 7) // 8)
    want = {0, 127, 128, 8 * ds - 2, 8 * ds - 1} | set(range(8 * ds, end)) | ({8191, 8192} if 8 * ds - 2 > 8192 else set())
    assert want <= single, sorted(want - single)
    assert sorted({s.flips[i][0] for i in s.of("tail")}) == list(range(end, 8 * bs))
    offs = sorted(int(s.kinds[i].split("@")[1]) for i in s.of("poly@s"))
    lim = end - (n + 1)
    assert {0, 1, 7, lim - 1, lim} <= set(offs)
    assert any(o < 128 <= o + n for o in offs)  # across a 16-byte piece boundary
    if lim - 1 > 8192:
        assert any(o < 8192 <= o + n for o in offs)  # across a 1 KiB row boundary
    for i in s.of("poly@s"):
        o = int(s.kinds[i].split("@")[1])
        assert list(s.flips[i]) == [o + j for j in range(n + 1) if (s.P >> (n - j)) & 1] and s.flips[i][-1] == o + n


@pytest.mark.parametrize("code", CODES, ids=code_id)
def test_classes_mean_what_they_say(oracle, code):
    s = the_set(oracle, code)
    codec = s.codec
    st, fixed, data, words, clean, pay = s.o_st, s.o_fixed, s.o_data, s.words, s.clean, s.payloads
    same = lambda a, b: np.array_equal(a, b)  # noqa: E731
    if codec != "ham":
        assert same(fixed, words)  # CRC and parity never write
    for i in s.of("clean"):
        assert st[i] == 0 and same(fixed[i], clean[i]) and same(data[i], pay[i]) and same(words[i], clean[i])
    for i in s.of("tail"):
        assert st[i] == 0 and same(data[i], pay[i]) and same(fixed[i], words[i])
    if codec == "ham":
        lay = s.layout
        dpos = {int(q): j for j, q in enumerate(lay.data_pos)}
        for i in s.of("single"):
            assert st[i] == 1 and same(fixed[i], clean[i]) and same(data[i], pay[i])
        for i in s.of("tail+single"):
            t = [q for q in s.flips[i] if q in lay.tail]
            assert len(t) == 1 and st[i] == 1 and diffbits(fixed[i], clean[i]) == t and same(data[i], pay[i])
        for i in list(s.of("double")) + list(s.of("quad")):
            assert st[i] == 5
        for lab in ("triple->payload", "triple->parity", "triple->bit0", "triple->tail"):
            for i in s.of(lab):
                ch = diffbits(fixed[i], words[i])
                assert st[i] == 1 and len(ch) == 1 and ch[0] not in s.flips[i]
                q = ch[0]
                if lab == "triple->payload":
                    assert q in dpos
                elif lab == "triple->parity":
                    assert q & (q - 1) == 0 and q
                elif lab == "triple->bit0":
                    assert q == 0
                else:
                    assert q in lay.tail and (lay.L is None or q > lay.L)
                # the payload carries the flipped payload bits (and the miscorrected one)
                wrong = sorted(dpos[p] for p in list(s.flips[i]) + [q] if p in dpos)
                assert diffbits(data[i], pay[i]) == wrong
        for i in s.of("quad0"):
            assert st[i] == 0 and not same(data[i], pay[i]) and same(fixed[i], words[i])
            assert diffbits(data[i], pay[i]) == sorted(dpos[p] for p in s.flips[i] if p in dpos)
    elif codec == "crc":
        last = 8 * s.ds - 1
        for i in s.of("single"):
            if s.flips[i] == (last,):  # the reference's division stops one step early
                assert st[i] == 0 and diffbits(data[i], pay[i]) == [last]
            else:
                assert st[i] == 5
        assert len(s.of("single", "last-payload-bit")) >= 1
        for i in s.of("tail+single"):
            assert st[i] == 5
        # two payload flips: the stored field drops the remainder's top bit, so a short polynomial lets
        # some pairs through (degree 3: bits 127 and 128); the oracle decides, most are rejected
        dbl = s.of("double")
        assert 2 * int((st[dbl] == 5).sum()) > dbl.size
        for i in dbl:
            assert st[i] in (0, 5) and diffbits(data[i], pay[i]) == sorted(s.flips[i])
        lim = s.end - (s.deg + 1)
        for i in s.of("poly@s"):
            o = int(s.kinds[i].split("@")[1])
            if o < lim:  # a multiple of the polynomial the division still reduces: undetected
                assert st[i] == 0 and not same(data[i], pay[i])
                assert diffbits(data[i], pay[i]) == [q for q in s.flips[i] if q <= last]
            else:
                assert o == lim and st[i] == 5
    else:
        for i in list(s.of("single")) + list(s.of("triple")):
            assert st[i] == 5
        for i in s.of("double"):
            assert st[i] == 0 and same(data[i], words[i][:s.ds])
            assert diffbits(data[i], pay[i]) == [q for q in s.flips[i] if q < 8 * s.ds]
    if codec == "ham":  # status 5 has no defined payload: the oracle's row stays zero
        assert not data[st == 5].any()
