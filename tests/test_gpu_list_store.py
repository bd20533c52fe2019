"""GPU tests of the direct list encode and write (paritypartyfs_amd/csrc/rs_wg_list.hpp
rs_wg_encode_list_kernel; csrc/list_store.hpp): RS(255, 255-2t), 2t <= 8 encodes a block list in one kernel
that stores codeword i at image + index[i] * 255 itself, and writes a list as the list decode (the old
blocks' statuses) followed by that encode.  The CPU oracle is the checker throughout; the staged path of
the same build (an engine created under PPFS_ECC_LIST_DIRECT=0) is the second opinion of the differential
test.

Geometry of the small cases: tests/test_gpu_list.py's image of 96 blocks inside guard bytes at base skews
0, 1, 2, 3 and 61.  Row b of a 255-byte-block image sits at alignment (skew - b) mod 16, so 16 consecutive
blocks cover every alignment of the store plan; lists of 1, 63, 64, 65 and 96 entries are a partial tile
alone, a tile less one, one tile, a tile and one entry, a tile and half a tile.  The payload arrays have
exactly the list's size: the partial tile must not read past its last payload."""
import numpy as np
import pytest

from tests.conftest import gpu_available
from tests.test_gpu_extents import Walk, extents
from tests.test_gpu_list import BLOCKS, Codec, _rs_errors, d_index, dev, host, rng_for
from tests.test_gpu_list_direct import Skewed, leveled_image, staged_engine

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch

from paritypartyfs_amd import ECC_CRC, ECC_HAMMING, ECC_REED_SOLOMON, EccEngine
from paritypartyfs_amd._native import EccError
from paritypartyfs_amd.block_device import file_extents

DIRECT, STAGED = "rs255-wg-list-store-lds", "gather-stage-scatter"
SKEWS = (0, 1, 2, 3, 61)
LENGTHS = (1, 63, 64, 65)
WPC = 3  # workgroups per CU of the list encode's persistent grid (csrc/rs_fast_inst.hip LIST_ENC_WPC)


# ------------------------------------------------------------------------------------
# 1. which contexts encode lists directly
# ------------------------------------------------------------------------------------
def test_list_encode_kernel_name(oracle):
    for t in (1, 2, 3, 4):
        assert EccEngine(ECC_REED_SOLOMON, 512, t).list_encode_kernel_name() == DIRECT
    assert EccEngine(ECC_REED_SOLOMON, 4096, 16).list_encode_kernel_name() == STAGED
    assert EccEngine(ECC_REED_SOLOMON, 64, 3).list_encode_kernel_name() == STAGED
    assert EccEngine(ECC_HAMMING, 256).list_encode_kernel_name() == STAGED
    assert EccEngine(ECC_CRC, 64, crc_polynomial_explicit=oracle.crc_explicit(0x9960034c)).list_encode_kernel_name() == STAGED
    assert staged_engine(ECC_REED_SOLOMON, 512, 3).list_encode_kernel_name() == STAGED
    assert EccEngine(ECC_REED_SOLOMON, 512, 3).list_encode_kernel_name() == DIRECT


# ------------------------------------------------------------------------------------
# 2. encode against the oracle
# ------------------------------------------------------------------------------------
def distinct_list(rng, n, blocks=BLOCKS):
    """n distinct blocks that always hold blocks 0..15 and the last block where n allows (shorter lists
    take the first n of those, the last block first), in a seeded order."""
    must = np.concatenate([[blocks - 1], np.arange(16)])
    rest = rng.permutation(np.arange(16, blocks - 1))
    ix = np.concatenate([must, rest])[:n]
    assert ix.size == n and np.unique(ix).size == n
    return rng.permutation(ix).astype(np.uint32)


def payloads(rng, c, n):
    """n random payloads and their codewords by the oracle, (n x ds, n x 255)."""
    data = rng.integers(0, 256, n * c.ds, dtype=np.uint8)
    return data.reshape(n, c.ds), c.encode(data, None).reshape(n, c.raw)


def exact(a):
    """A device array of exactly a's size (no guard bytes behind it)."""
    d = dev(np.ascontiguousarray(a).reshape(-1))
    assert d.numel() == a.size and d.data_ptr() % 16 == 0
    return d


def expect_rows(image, ix, cw):
    """The image with row ix[i] replaced by cw[i] for every in-range entry."""
    blocks = image.size // 255
    exp = image.reshape(blocks, 255).copy()
    ok = ix < blocks
    exp[ix[ok].astype(np.int64)] = cw[:ix.size][ok]
    return exp.reshape(-1)


@pytest.mark.parametrize("t", [1, 2, 3, 4])
def test_encode_list_against_the_oracle(oracle, t):
    c = Codec(oracle, "rs", 512, t)
    assert c.eng.list_encode_kernel_name() == DIRECT
    rng = rng_for("store", t)
    image = rng.integers(0, 256, BLOCKS * c.raw, dtype=np.uint8)
    data, cw = payloads(rng, c, BLOCKS)  # one reference for every list: entry i carries payload i
    for n in LENGTHS + (BLOCKS,):  # 96: the whole image permuted, a full tile and a partial one
        for skew in SKEWS:
            ix = distinct_list(rng, n)
            assert n < 17 or ({*range(16), BLOCKS - 1} <= set(ix.tolist()))
            g = Skewed(image, skew)
            c.eng.encode_list(exact(data[:n]), g.image, d_index(ix))
            torch.cuda.synchronize()
            assert np.array_equal(g.result(), expect_rows(image, ix, cw)), (n, skew)


# ------------------------------------------------------------------------------------
# 3. neighbouring rows written by different workgroups
# ------------------------------------------------------------------------------------
def test_neighbours_from_different_workgroups(oracle):
    """All even blocks, then all odd blocks of a 130-block image (65 + 65 entries, three tiles): every
    16-byte window and cache line that two rows share has its two writers in different tiles.  Then the
    even blocks alone: every odd row stays byte for byte."""
    c = Codec(oracle, "rs", 512, 3)
    rng = rng_for("store-neigh")
    blocks = 130
    image = rng.integers(0, 256, blocks * c.raw, dtype=np.uint8)
    data, cw = payloads(rng, c, blocks)
    ix = np.concatenate([np.arange(0, blocks, 2), np.arange(1, blocks, 2)]).astype(np.uint32)
    even = ix[:65]
    for skew in (0, 3):
        g = Skewed(image, skew)
        c.eng.encode_list(exact(data), g.image, d_index(ix))
        torch.cuda.synchronize()
        assert np.array_equal(g.result(), expect_rows(image, ix, cw))
        g = Skewed(image, skew)
        c.eng.encode_list(exact(data[:65]), g.image, d_index(even))
        torch.cuda.synchronize()
        got = g.result()
        assert np.array_equal(got, expect_rows(image, even, cw))
        assert np.array_equal(got.reshape(blocks, c.raw)[1::2], image.reshape(blocks, c.raw)[1::2])


# ------------------------------------------------------------------------------------
# 4. out-of-range entries
# ------------------------------------------------------------------------------------
def test_out_of_range_entries(oracle):
    """Entries equal to image_blocks, past it, 1 << 31 and 0xFFFFFFFF at a tile's first and last row, as
    a whole tile of 64 and in the partial tile: they store nothing, and write_list gives them status 9."""
    t = 3
    c = Codec(oracle, "rs", 512, t)
    rng = rng_for("store-oob")
    level = np.arange(BLOCKS) % (t + 2)
    image = c.corrupt(rng, c.valid_image(rng, BLOCKS), level)
    _, o_st, _, _ = c.decode(image)
    bad = np.array([BLOCKS, BLOCKS + 7, 0xFFFFFFFF, 1 << 31], np.uint32)
    inside = rng.permutation(BLOCKS).astype(np.uint32)
    tile0 = np.concatenate([[BLOCKS], inside[:62], [0xFFFFFFFF]])
    tile1 = bad[np.arange(64) % bad.size]
    tile2 = np.concatenate([[BLOCKS + 7], inside[62:94], bad[np.arange(30) % bad.size], [BLOCKS]])
    part = np.concatenate([[0xFFFFFFFF], inside[94:96], [BLOCKS]])
    ix = np.concatenate([tile0, tile1, tile2, part]).astype(np.uint32)
    assert ix.size == 3 * 64 + 4
    oob = ix >= BLOCKS
    assert np.unique(ix[~oob]).size == BLOCKS and oob[64:128].all()
    data, cw = payloads(rng, c, ix.size)
    exp = expect_rows(image, ix, cw)
    for skew in (0, 61):
        g = Skewed(image, skew)
        c.eng.encode_list(exact(data), g.image, d_index(ix))
        torch.cuda.synchronize()
        assert np.array_equal(g.result(), exp)
        g = Skewed(image, skew)
        st = torch.full((ix.size + 48,), 77, dtype=torch.uint8, device="cuda")
        c.eng.write_list(exact(data), g.image, d_index(ix), st[:ix.size])
        st = host(st)
        assert np.array_equal(st[:ix.size], np.where(oob, 9, o_st[np.where(oob, 0, ix)])) and (st[ix.size:] == 77).all()
        assert np.array_equal(g.result(), exp)
        # an image of no whole block: every entry is out of range and nothing is stored
        g = Skewed(image, skew)
        s8 = torch.full((8,), 77, dtype=torch.uint8, device="cuda")
        c.eng.encode_list(exact(data[:8]), g.image[:100], d_index(np.arange(8)))
        c.eng.write_list(exact(data[:8]), g.image[:100], d_index(np.arange(8)), s8)
        assert (host(s8) == 9).all()
        assert np.array_equal(g.result(), image)
    torch.cuda.synchronize()  # no fault behind any of it


# ------------------------------------------------------------------------------------
# 5. write list
# ------------------------------------------------------------------------------------
def run_write_list(eng, image, skew, ix, data, status):
    """-> ("ok", status or None, image afterwards), or ("refused", error code, image afterwards).
    status: None, "aligned" or "misaligned" (3 bytes past a 16-byte boundary)."""
    g = Skewed(image, skew)
    buf = torch.full((ix.size + 64,), 77, dtype=torch.uint8, device="cuda")
    st = None if status is None else buf[:ix.size] if status == "aligned" else buf[3:3 + ix.size]
    assert st is None or (st.data_ptr() % 16 == 0) == (status == "aligned")
    try:
        eng.write_list(exact(data), g.image, d_index(ix), st)
    except EccError as e:
        torch.cuda.synchronize()
        assert (host(buf) == 77).all()
        return "refused", e.code, g.result()
    torch.cuda.synchronize()
    b = host(buf)
    lo = 0 if status != "misaligned" else 3
    if st is None:
        assert (b == 77).all()
    else:
        assert (b[:lo] == 77).all() and (b[lo + ix.size:] == 77).all(), "status store outside the list"
    return "ok", None if st is None else b[lo:lo + ix.size].copy(), g.result()


@pytest.mark.parametrize("t", [1, 2, 3, 4])
def test_write_list(oracle, t):
    """Old blocks with 0 .. t + 1 byte errors: the statuses are the oracle's decode statuses in list order,
    and every listed row becomes the new codeword whatever the old block's status was."""
    c = Codec(oracle, "rs", 512, t)
    staged = staged_engine(ECC_REED_SOLOMON, 512, t)
    rng = rng_for("store-write", t)
    image, level = leveled_image(c, rng)
    _, o_st, _, _ = c.decode(image)
    assert set(o_st.tolist()) == {0, 1} and (level == t + 1).any()
    data, cw = payloads(rng, c, BLOCKS)
    for n in (65, BLOCKS):
        ix = distinct_list(rng, n)
        exp = expect_rows(image, ix, cw)
        for skew in (0, 61):
            kind, st, img = run_write_list(c.eng, image, skew, ix, data[:n], "aligned")
            assert kind == "ok" and np.array_equal(st, o_st[ix]) and np.array_equal(img, exp)
            kind, st, img = run_write_list(c.eng, image, skew, ix, data[:n], None)
            assert kind == "ok" and np.array_equal(img, exp)
        # a status array that breaks the 16-byte rule: the staged path, byte for byte
        a = run_write_list(c.eng, image, 61, ix, data[:n], "misaligned")
        b = run_write_list(staged, image, 61, ix, data[:n], "misaligned")
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------
# 6. more tiles than the persistent grid holds workgroups
# ------------------------------------------------------------------------------------
def test_multi_tile_walk(oracle):
    """Three tiles per workgroup of the persistent grid and a partial tile: every workgroup runs its
    prologue, steady-state iterations and its last tile, and one of them the partial tile.  A seeded
    permutation of an image 50 blocks larger; one encode_list and one write_list over it."""
    c = Codec(oracle, "rs", 512, 3)
    rng = rng_for("store-walk")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nb = 3 * WPC * cus * 64 + 37
    blocks = nb + 50
    image = _rs_errors(rng, c.valid_image(rng, blocks), c.raw, c.t, blocks)
    ix = rng.permutation(blocks)[:nb].astype(np.uint32)
    _, o_st, _, _ = c.decode(image)
    data, cw = payloads(rng, c, nb)
    exp = expect_rows(image, ix, cw)
    data_d, ix_d = exact(data), d_index(ix)
    image_d = dev(image)
    c.eng.encode_list(data_d, image_d, ix_d)
    assert np.array_equal(host(image_d), exp)
    image_d = dev(image)
    st = torch.full((nb + 48,), 77, dtype=torch.uint8, device="cuda")
    c.eng.write_list(data_d, image_d, ix_d, st[:nb])
    st = host(st)
    assert np.array_equal(st[:nb], o_st[ix]) and (st[nb:] == 77).all()
    assert np.array_equal(host(image_d), exp)


# ------------------------------------------------------------------------------------
# 7. the staged path of the same build as a second opinion
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 3, 4])
def test_direct_equals_staged(oracle, t):
    c = Codec(oracle, "rs", 512, t)
    staged = staged_engine(ECC_REED_SOLOMON, 512, t)
    assert (c.eng.list_encode_kernel_name(), staged.list_encode_kernel_name()) == (DIRECT, STAGED)
    rng = rng_for("store-diff", t)
    image, level = leveled_image(c, rng)
    perm = rng.permutation(BLOCKS).astype(np.uint32)
    ix = np.concatenate([perm[:40], [BLOCKS, 0xFFFFFFFF], perm[40:90]]).astype(np.uint32)  # no repeats
    data, cw = payloads(rng, c, ix.size)
    res = []
    for eng in (c.eng, staged):
        g = Skewed(image, 61)  # result() checks the guard bytes
        eng.encode_list(exact(data), g.image, d_index(ix))
        torch.cuda.synchronize()
        res.append((g.result(),) + run_write_list(eng, image, 61, ix, data, "aligned"))
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    assert np.array_equal(res[0][0], expect_rows(image, ix, cw))
    assert (res[0][2] == 9).sum() == 2 and (res[0][2] == 1).any()
    # write_extents, the file shape with a non-zero first offset, a zero-length and an invalid entry
    blocks = perm[:41]
    off0 = 7
    nbytes = (c.ds - off0) + 39 * c.ds + 5
    ext = file_extents(blocks, off0, nbytes, c.ds)
    assert int(ext["offset"][0]) == off0 and int(ext["length"].astype(np.int64).sum()) == nbytes
    more = extents([(0, int(perm[50]), 9, 0), (0, BLOCKS + 1, 0, 4)])  # (pos, block, offset, length)
    ext = np.concatenate([ext, more])
    buf = rng.integers(0, 256, nbytes, dtype=np.uint8)
    w = Walk(c, image)
    o_st = w.write(ext, buf)
    assert o_st[-1] == 9 and o_st[-2] in (0, 1) and (o_st == 1).any()
    res = []
    for eng in (c.eng, staged):
        g = Skewed(image, 61)
        src = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        src[3:3 + nbytes] = dev(buf)
        st = torch.full((len(ext) + 48,), 77, dtype=torch.uint8, device="cuda")
        eng.write_extents(src[3:3 + nbytes], g.image, ext, st[:len(ext)])
        torch.cuda.synchronize()
        res.append((g.result(), host(st)))
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    img, st = res[0]
    assert np.array_equal(st[:len(ext)], o_st) and (st[len(ext):] == 77).all()
    assert np.array_equal(img, w.image())


# ------------------------------------------------------------------------------------
# 8. repeated indices stay memory-safe
# ------------------------------------------------------------------------------------
def test_repeats_stay_safe(oracle):
    """A block listed three times inside one tile, and once in each of three tiles, with different
    payloads: no byte outside the listed rows changes, each byte of the repeated row is that byte of one
    of its candidates' codewords, every other row is exact."""
    c = Codec(oracle, "rs", 512, 3)
    rng = rng_for("store-rep")
    image = rng.integers(0, 256, BLOCKS * c.raw, dtype=np.uint8)
    A = 5
    clean = np.array([b for b in range(BLOCKS) if b != A and b < 91], np.uint32)  # 90 blocks; 91..95 stay unlisted
    one_tile = clean[:64].copy()
    one_tile[[0, 17, 63]] = A
    three_tiles = np.full(3 * 64, 0xFFFFFFFF, np.uint32)  # 30 distinct blocks per tile, the rest no block
    for k in range(3):
        three_tiles[64 * k:64 * k + 30] = clean[30 * k:30 * k + 30]
    three_tiles[[3, 64 + 60, 128 + 29]] = A
    for ix in (one_tile, three_tiles):
        copies = np.nonzero(ix == A)[0]
        others = np.nonzero((ix != A) & (ix < BLOCKS))[0]
        assert copies.size == 3 and np.unique(ix[others]).size == others.size
        data, cw = payloads(rng, c, ix.size)
        for skew in (0, 3):
            g = Skewed(image, skew)  # result() checks the guard bytes
            c.eng.encode_list(exact(data), g.image, d_index(ix))
            torch.cuda.synchronize()
            got = g.result().reshape(BLOCKS, c.raw)
            exp = image.reshape(BLOCKS, c.raw).copy()
            exp[ix[others].astype(np.int64)] = cw[others]
            rest = np.arange(BLOCKS) != A
            assert np.array_equal(got[rest], exp[rest])
            assert (got[A][None, :] == cw[copies]).any(axis=0).all()


# ------------------------------------------------------------------------------------
# 9. two calls side by side
# ------------------------------------------------------------------------------------
def test_two_streams_encode_interleaved_rows(oracle):
    """Two direct list encodes of one engine on two streams over the even and the odd blocks of one image:
    interleaved neighbours, no ordering between the calls (there is no staging to protect)."""
    c = Codec(oracle, "rs", 512, 3)
    assert c.eng.list_encode_kernel_name() == DIRECT
    rng = rng_for("store-streams")
    blocks = 4000
    image = rng.integers(0, 256, blocks * c.raw, dtype=np.uint8)
    data, cw = payloads(rng, c, blocks)
    half = blocks // 2
    lists = [rng.permutation(np.arange(0, blocks, 2)).astype(np.uint32), rng.permutation(np.arange(1, blocks, 2)).astype(np.uint32)]
    parts = [data[:half], data[half:]]
    exp = image.reshape(blocks, c.raw).copy()
    exp[lists[0].astype(np.int64)] = cw[:half]
    exp[lists[1].astype(np.int64)] = cw[half:]
    image_d = dev(image)
    ix_d = [d_index(ix) for ix in lists]
    data_d = [exact(p) for p in parts]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for k, s in enumerate(streams):
        c.eng.encode_list(data_d[k], image_d, ix_d[k], stream=s)
    for s in streams:
        s.synchronize()
    assert np.array_equal(host(image_d), exp.reshape(-1))
