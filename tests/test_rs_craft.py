"""CPU tests of the syndrome-crafting helper (tests/rs_craft.py) that tests/test_gpu_rs_branches.py
rests on: the crafted words have the syndromes they were built for, every decode-branch class a
code's t allows is present in its block set (so the GPU comparison cannot pass vacuously), and the
oracle agrees with the literal Python restatement of the reference on one word per class."""
import numpy as np
import pytest

from tests import ref_model
from tests import rs_craft

FAST = [(255, 1), (255, 2), (512, 3), (256, 4), (1024, 5), (4096, 8), (4096, 16)]
GENERIC = [(255, 6), (255, 9), (255, 20)]
SHORT = [(64, 3), (128, 10), (32, 1), (3, 1)]
CODES = FAST + GENERIC + SHORT

# Classes by classify() that a code's set must hold.  What 2t allows:
#   2t = 2   sigma is 1 + (S2/S1) x, 1 (S2 = 0: degree 0 < L) or 1 + S2 x^2 (S1 = 0: the double root,
#            which is also degree 2t); no other degree-2 form and nothing of degree >= 3 exists
#   2t >= 4  every degree-1 and degree-2 form, "geometric but for the last syndrome", and (L > t)
#            sigma of degree >= 3 with all / some / none of its roots and with a repeated root
#   2t >= 8  also degree >= 3 below L (a degree-3 recurrence that starts one syndrome late needs
#            L = 4 <= t to be the unique BM result)
#   n < 255  roots at positions past the block (a non-empty spill)
T1 = {"clean", "geometric", "deg0", "deg2_double_root", "deg_2t", "deg_lt_L", "dsig_zero_at_root", "root_m0_byte0",
      "some_S_zero"}
T2 = T1 | {"deg1_not_geometric", "deg1_L_gt_1", "deg2_no_roots", "deg2_two_roots", "deg2_roots_byte0_byte254",
           "deg3p_all_roots", "deg3p_fewer_roots", "deg3p_no_roots", "deg3p_repeated_root", "geometric_but_last"}
T4 = T2 | {"deg3p_lt_L"}


def required(n, t):
    req = T1 if t == 1 else (T2 if t < 4 else T4)
    return req | ({"root_beyond_n"} if n < 255 else set())


# the number of required classes as literals, so a silently dropped class fails here
REQUIRED_COUNT = {(255, 1): 9, (255, 2): 19, (512, 3): 19, (256, 4): 20, (1024, 5): 20, (4096, 8): 20, (4096, 16): 20,
                  (255, 6): 20, (255, 9): 20, (255, 20): 20, (64, 3): 20, (128, 10): 21, (32, 1): 10, (3, 1): 10}


@pytest.mark.parametrize("bs,t", CODES, ids=lambda x: str(x))
def test_crafted_words_have_their_syndromes(oracle, bs, t):
    """word_with_syndromes round-trips on both supports: S recomputed from the words with the table
    model equals the targets; the words differ from their codewords on the support only."""
    s = rs_craft.branch_set(oracle, bs, t)
    assert np.array_equal(rs_craft.syndromes(s.words, s.two_t), s.S)
    rng = np.random.default_rng(bs * 131 + t)
    n, k = s.n, s.k
    cw = oracle.rs_encode(bs, t, rng.integers(0, 256, 40 * k, dtype=np.uint8)).reshape(40, n)
    assert not rs_craft.syndromes(cw, s.two_t).any()
    for w, sup in s.supports.items():
        if sup is None:
            continue
        assert n < 255 or w == 1 or 254 in sup
        target = rng.integers(0, 256, (40, s.two_t), dtype=np.uint8)
        target[0] = 0
        words = rs_craft.word_with_syndromes(cw, target, sup)
        assert np.array_equal(rs_craft.syndromes(words, s.two_t), target)
        changed = np.nonzero((words != cw).any(axis=0))[0]
        assert set(changed) <= set(int(p) for p in sup)
        assert np.array_equal(words[0], cw[0])
    if n == 255:
        assert s.supports[2] is not None and (s.support == 2).any() and (s.support == 1).any()


@pytest.mark.parametrize("bs,t", CODES, ids=lambda x: str(x))
def test_census_holds_every_required_class(oracle, bs, t):
    s = rs_craft.branch_set(oracle, bs, t)
    census = s.census()
    print(f"RS({bs},{t}) n={s.n} blocks={s.nb}: " + ", ".join(f"{c} {census[c]}" for c in sorted(census)))
    req = required(s.n, s.t)
    assert len(req) == REQUIRED_COUNT[(bs, t)]
    missing = sorted(c for c in req if census.get(c, 0) < 1)
    assert not missing, missing
    assert s.nb % 64 != 0
    assert sum(1 for l in s.labels if l == "random") >= 512
    assert sum(1 for l in s.labels if l == "single") == 3 * s.n
    # the three batches: ragged, the lone-general tiles hold one general-path block at the lane asked
    b = s.batches()
    assert set(b) == {"interleaved", "sorted", "lone_general"}
    assert sorted(b["interleaved"]) == list(range(s.nb)) and sorted(b["sorted"]) == list(range(s.nb))
    gen = set(int(x) for x in s.general())
    lone = b["lone_general"]
    for j, lane in enumerate((0, 31, 32, 63) * 2):
        tile = lone[64 * j:64 * j + 64]
        assert [i for i, x in enumerate(tile) if int(x) in gen] == [lane]
        assert all(not s.S[x].any() for i, x in enumerate(tile) if i != lane)
    if s.n < 255:
        assert (s.o_spill[:, 0] > 0).any()


@pytest.mark.parametrize("bs,t", [(255, 2), (512, 3), (64, 3)], ids=lambda x: str(x))
def test_oracle_matches_ref_model_on_one_word_per_class(oracle, bs, t):
    """The checker itself at the inputs the reference's own tests never used: status, payload and
    written-back bytes of the oracle against the statement-by-statement Python restatement."""
    s = rs_craft.branch_set(oracle, bs, t)
    picks = {}
    for b, i in enumerate(s.info()):
        for c in rs_craft.classes_of(i, s.two_t, s.n):
            picks.setdefault(c, b)
    for b, l in enumerate(s.labels):
        picks.setdefault("label:" + l, b)
    blocks = sorted(set(picks.values()))
    assert len(blocks) <= 120
    for b in blocks:
        st, data, wb = ref_model.rs_decode(bs, t, s.words[b].tobytes())
        assert st == s.o_st[b], (b, s.labels[b])
        assert data == s.o_data[b].tobytes(), (b, s.labels[b])
        assert len(wb) == s.o_wbl[b], (b, s.labels[b])
        assert wb[:s.n] == s.o_fixed[b].tobytes()[:len(wb)], (b, s.labels[b])
        if len(wb) > s.n:
            assert s.o_spill[b, 0] == len(wb) - s.n
            assert wb[s.n:] == s.o_spill[b, 1:1 + len(wb) - s.n].tobytes()
        else:
            assert s.o_spill[b, 0] == 0


def test_classify_on_known_words(oracle):
    """classify against hand-built cases: a single error is geometric with the one root at its
    position; two errors give their locator; lfsr_syndromes follows sigma's recurrence."""
    f = rs_craft.field(oracle)
    n, k, _ = oracle.rs_sizes(512, 3)
    cw = oracle.rs_encode(512, 3, np.arange(k, dtype=np.uint8))
    for p in (0, 1, 5, 6, 254):
        w = cw.copy()
        w[p] ^= 0x5A
        i = rs_craft.classify(rs_craft.syndromes(w, 6)[0])
        assert (i["deg"], i["L"], i["positions"], i["geometric"]) == (1, 1, [p], True)
    w = cw.copy()
    w[0] ^= 1
    w[254] ^= 7
    i = rs_craft.classify(rs_craft.syndromes(w, 6)[0])
    assert (i["deg"], i["L"], sorted(i["roots"]), sorted(i["positions"])) == (2, 2, [0, 1], [0, 254])
    assert not i["geometric"] and not i["dsig_zero_at_root"]
    S = rs_craft.lfsr_syndromes([1, 0, 9], [3, 200], 6)
    assert S[:2] == [3, 200] and all(S[j] == f.mul_rows[9][S[j - 2]] for j in range(2, 6))
    i = rs_craft.classify(S)
    assert i["deg"] == 2 and i["sig1_zero"] and len(i["roots"]) == 1 and i["dsig_zero_at_root"]
    assert rs_craft.classify([0] * 6)["clean"]
