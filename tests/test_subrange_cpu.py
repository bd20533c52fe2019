"""The inputs of tests/test_gpu_subrange.py without a GPU: every case's deal, the share of a batch the
oracle leaves without a defined payload, and the frame's own arithmetic (tests/subrange.py)."""
import numpy as np
import pytest

from tests import subrange as sr

CASES = sr.all_cases()


def case_id(c):
    return f"{sr.code_id(c[0])}-{c[1]}+{c[2]}of{c[3]}"


@pytest.mark.parametrize("spec", CASES, ids=case_id)
def test_case_inputs(oracle, spec):
    code, first, count, nblocks = spec
    cs = sr.case(oracle, code, first, count, nblocks)
    assert first + count <= nblocks and cs.image.size == nblocks * cs.row and cs.new.size == nblocks * cs.ds
    # at most 30 % of a batch has no defined payload
    assert cs.left_out() <= 0.30, (cs.left_out(), cs.st.tolist())
    assert np.array_equal(cs.defined, cs.st != 5)
    # a batch of five blocks or more holds every status of the codec's deal
    if count >= 5:
        assert sr.DEAL_STATUSES[code[0]] <= set(cs.st.tolist()), (sorted(set(cs.st.tolist())), cs.classes[first:first + count])
    # the deal starts its turn at the range's first block, and the rows outside carry faults too
    assert cs.classes[first] == 0 and cs.classes.size == nblocks
    # what the clean blocks decode to is what was encoded; a block with a defined payload that is not
    # the encoded one can only be an RS block beyond t errors
    same = (cs.data == cs.payload.reshape(nblocks, cs.ds)[first:first + count]).all(axis=1)
    cls = cs.classes[first:first + count]
    if code[0] == "rs":
        assert same[cls <= code[1]].all()
    else:
        assert same[cs.defined].all()
    # encode keeps what the codec does not own of the old image: the expectations differ from an encode over zeros
    assert cs.encoded.shape == cs.written.shape == cs.fixed.shape == (count, cs.row)
    if cs.spill is not None:
        assert cs.spill.shape == (count, 256 - cs.row) and (cs.spill[:, 0] <= 255 - cs.row).all()
    else:
        assert code not in sr.RS_GENERIC


@pytest.mark.parametrize("code", [c for c in sr.STREAMING + sr.GENERIC if c[0] != "par"], ids=sr.code_id)
def test_encode_over_noise_keeps_bits(oracle, code):
    """The encode cases check kept bits only if the codec has some: Hamming's tail, a CRC field that ends inside
    a byte.  (Parity keeps the upper seven bits of its last byte: test below.)"""
    cs = sr.case(oracle, code, 0, 67)
    zeros = sr.o_encode(oracle, code, cs.new, np.zeros_like(cs.noise)).reshape(sr.N, cs.row)[:67]
    whole_bytes = code[0] == "crc" and (oracle.crc_explicit(code[1]).bit_length() - 1) % 8 == 0
    assert np.array_equal(zeros, cs.encoded) == whole_bytes


@pytest.mark.parametrize("bs", [255, 256, 1024, 4096])
def test_parity_encode_over_noise_keeps_the_last_byte(oracle, bs):
    cs = sr.case(oracle, ("par", 0, bs), 0, 67)
    old = cs.noise.reshape(sr.N, bs)[:67]
    assert np.array_equal(cs.encoded[:, -1] & 0xFE, old[:, -1] & 0xFE) and (old[:, -1] & 0xFE).any()


def test_lists_are_the_issue():
    assert sr.N == 80 and sr.GUARD == 256
    assert sr.SKEWS == [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 3), (3, 5, 1), (4, 8, 2), (8, 4, 0), (15, 15, 15)]
    assert sr.RANGES == [(0, 1), (3, 5), (0, 67), (13, 67)]
    assert len(sr.CALLS) == 6 and len(set(sr.STREAMING + sr.GENERIC + sr.RS_GENERIC + sr.RS_FAST)) == 20
    f, n = sr.RS_FAST_RANGE
    for code in sr.RS_FAST:  # first = 16: the three offsets are multiples of 16
        assert (f * 255) % 16 == 0 and (f * (255 - 2 * code[1])) % 16 == 0 and f % 16 == 0 and f + n <= sr.RS_FAST_N


@pytest.mark.parametrize("skew", sorted({s for t in sr.SKEWS for s in t}))
@pytest.mark.parametrize("n", [1, 80, 80 * 4091])
def test_frame_arithmetic(skew, n):
    rng = sr.rng_for("frame", skew, n)
    content = rng.integers(0, 256, n, dtype=np.uint8)
    a, b = sr.Frame("x", content, skew, sr.rng_for("g", 1)), sr.Frame("x", content, skew, sr.rng_for("g", 2))
    assert a.host.size == sr.GUARD + skew + n + sr.GUARD and a.off == sr.GUARD + skew
    assert np.array_equal(a.host[a.off:a.off + n], content)
    for base in (0, 256, 7 << 20):  # a 256-byte aligned allocation: the view's address modulo 16 is the skew's
        assert a.address(base) % 16 == skew % 16 and a.address(base, n) + sr.GUARD == base + a.host.size
    # guards and skew bytes are seeded random, not a constant
    ga, gb = np.delete(a.host, np.s_[a.off:a.off + n]), np.delete(b.host, np.s_[b.off:b.off + n])
    assert ga.size == 2 * sr.GUARD + skew and len(set(ga.tolist())) > 64 and not np.array_equal(ga, gb)


def test_frame_comparison_names_the_byte():
    row, first, count = 7, 3, 5
    fr = sr.Frame("x", np.arange(10 * row, dtype=np.uint8), 5, sr.rng_for("cmp"))
    new = np.full((count, row), 0xEE, np.uint8)
    exp, mask = fr.expected(first, count, row, new, defined=[True, False, True, True, True])
    assert fr.mismatch(exp, exp, mask, first, count, row) is None
    assert np.array_equal(exp[fr.off + first * row:fr.off + (first + count) * row], new.reshape(-1))
    assert np.array_equal(np.delete(exp, np.s_[fr.off + first * row:fr.off + (first + count) * row]),
                          np.delete(fr.host, np.s_[fr.off + first * row:fr.off + (first + count) * row]))
    for at, what in ((fr.off - 1, "guard/skew"), (0, "guard/skew"), (fr.off + fr.n, "guard/skew"),
                     (fr.off + 2 * row + 6, "neighbour row 2"), (fr.off + 8 * row, "neighbour row 8"),
                     (fr.off + 3 * row, "range row 3"), (fr.off + 7 * row + 6, "range row 7")):
        got = exp.copy()
        got[at] ^= 0x10
        bad = fr.mismatch(got, exp, mask, first, count, row)
        assert bad == (what, at - fr.off, int(got[at]), int(exp[at])), (at, bad)
    got = exp.copy()
    got[fr.off + 4 * row + 2] ^= 1  # the row that is left out
    assert fr.mismatch(got, exp, mask, first, count, row) is None


def test_rule():
    r = sr.rejects
    for call in sr.CALLS:
        has_data, has_status = sr.uses(call)
        for code in sr.GENERIC + sr.STREAMING:
            if code[0] == "ham":
                assert r(code, call, 16, 1, 3) is False
                assert r(code, call, 8, 0, 0) is (code[2] >= 8)
            else:
                assert r(code, call, 1, 5, 3) is False
        for code in sr.RS_GENERIC:
            assert r(code, call, 15, 15, 15) is False
        for code in sr.RS_FAST:
            assert r(code, call, 32, 48, 64) is False
            assert r(code, call, 33, 48, 64) is True
            assert r(code, call, 32, 49, 64) is has_data
            assert r(code, call, 32, 48, 67) is has_status
