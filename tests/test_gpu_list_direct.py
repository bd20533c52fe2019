"""GPU tests of the direct list decode (paritypartyfs_amd/csrc/rs_wg_list.hpp): RS(255, 255-2t), 2t <= 8
decodes a block list in one kernel that fetches the listed rows from the image itself, corrects them in
place and emits payloads and statuses in list order.  The CPU oracle is the checker throughout; the
staged path of the same build (an engine created under PPFS_ECC_LIST_DIRECT=0) is the second opinion of
the differential test.

Geometry of the small cases: tests/test_gpu_list.py's image of 96 blocks inside guard bytes, here at base
skews 0, 1, 2, 3 and 61, so the loader's aligned reads meet both ends of the image at every dword phase;
lists of 1, 63, 64, 65 and 200 entries (a partial tile alone, a tile less one, one tile, a tile and one
entry, three tiles and a partial one).  The payload and status arrays carry guard bytes behind their
ends: the partial tile's last 16-byte piece must stop at the list's last payload byte."""
import os

import numpy as np
import pytest

from tests.conftest import gpu_available
from tests.test_gpu_list import BLOCKS, GUARD, Codec, _rs_errors, d_index, dev, host, rng_for

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch

from paritypartyfs_amd import ECC_CRC, ECC_HAMMING, ECC_REED_SOLOMON, EccEngine
from paritypartyfs_amd.block_device import file_extents

DIRECT, STAGED = "rs255-wg-list-lds", "gather-stage-scatter"
SKEWS = (0, 1, 2, 3, 61)
LENGTHS = (1, 63, 64, 65, 200)
TAIL = 48  # guard bytes behind the payload and status arrays


def staged_engine(*args, **kw):
    """An engine whose list decodes take the staged path: PPFS_ECC_LIST_DIRECT=0 around its constructor."""
    old = os.environ.get("PPFS_ECC_LIST_DIRECT")
    os.environ["PPFS_ECC_LIST_DIRECT"] = "0"
    try:
        return EccEngine(*args, **kw)
    finally:
        if old is None:
            del os.environ["PPFS_ECC_LIST_DIRECT"]
        else:
            os.environ["PPFS_ECC_LIST_DIRECT"] = old


class Skewed:
    """A device image `skew` bytes past a 256-byte aligned address, inside guard bytes."""

    def __init__(self, image, skew):
        self.n, self.lo = image.size, GUARD + skew
        buf = np.full(self.lo + self.n + GUARD, 0xA5, np.uint8)
        buf[self.lo:self.lo + self.n] = image
        self.buf = dev(buf)
        self.image = self.buf[self.lo:self.lo + self.n]
        assert self.image.data_ptr() % 16 == skew % 16

    def result(self):
        b = host(self.buf)
        assert (b[:self.lo] == 0xA5).all() and (b[self.lo + self.n:] == 0xA5).all(), "write outside the image"
        return b[self.lo:self.lo + self.n].copy()


class Outputs:
    """Payload, status and spill arrays of a list decode, preset and with guard bytes behind them."""

    def __init__(self, n, ds):
        self.n, self.ds = n, ds
        self.data = torch.full((n * ds + TAIL,), 0x77, dtype=torch.uint8, device="cuda")
        self.st = torch.full((n + TAIL,), 77, dtype=torch.uint8, device="cuda")
        self.spill = torch.full((n + TAIL,), 0x55, dtype=torch.uint8, device="cuda")

    def views(self):
        return self.data[:self.n * self.ds], self.st[:self.n], self.spill[:self.n]

    def result(self):
        d, s, sp = host(self.data), host(self.st), host(self.spill)
        assert (d[self.n * self.ds:] == 0x77).all(), "payload store past the list's end"
        assert (s[self.n:] == 77).all() and (sp[self.n:] == 0x55).all(), "status / spill store past the list's end"
        return d[:self.n * self.ds].reshape(self.n, self.ds), s[:self.n], sp[:self.n]


def decode_list(eng, g, ix, ds, write_back=True):
    out = Outputs(len(ix), ds)
    data, st, spill = out.views()
    eng.decode_list(g.image, d_index(ix), data, st, write_back=write_back, spill=spill)
    torch.cuda.synchronize()
    return out.result()


# ------------------------------------------------------------------------------------
# which contexts decode lists directly
# ------------------------------------------------------------------------------------
def test_list_kernel_name(oracle):
    for t in (1, 2, 3, 4):
        assert EccEngine(ECC_REED_SOLOMON, 512, t).list_kernel_name() == DIRECT
    assert EccEngine(ECC_REED_SOLOMON, 4096, 16).list_kernel_name() == STAGED
    assert EccEngine(ECC_REED_SOLOMON, 64, 3).list_kernel_name() == STAGED
    assert EccEngine(ECC_HAMMING, 256).list_kernel_name() == STAGED
    assert EccEngine(ECC_CRC, 64, crc_polynomial_explicit=oracle.crc_explicit(0x9960034c)).list_kernel_name() == STAGED
    before = os.environ.get("PPFS_ECC_LIST_DIRECT")
    assert staged_engine(ECC_REED_SOLOMON, 512, 3).list_kernel_name() == STAGED
    assert os.environ.get("PPFS_ECC_LIST_DIRECT") == before  # restored
    assert EccEngine(ECC_REED_SOLOMON, 512, 3).list_kernel_name() == DIRECT


# ------------------------------------------------------------------------------------
# decode against the oracle
# ------------------------------------------------------------------------------------
def leveled_image(c, rng):
    """96 valid blocks, block b with b % (t + 2) byte errors (0 .. t + 1) -> (image, errors per block)."""
    level = np.arange(BLOCKS) % c.levels
    return c.corrupt(rng, c.valid_image(rng, BLOCKS), level), level


def listed(rng, n, level, t):
    """n entries that always hold blocks 0..15 and the last block where n allows (shorter lists take the
    first n of those, the last block first).  A list longer than the image repeats blocks, but none with
    more than t errors: the copies of such a block may differ (include/ppfs_ecc.h), the others' may not."""
    must = np.concatenate([[BLOCKS - 1], np.arange(16)])
    if n <= must.size:
        return rng.permutation(must[:n]).astype(np.uint32)
    rest = rng.permutation(np.arange(16, BLOCKS - 1))
    ix = np.concatenate([must, rest])[:n]
    if n > ix.size:
        again = np.nonzero(level <= t)[0]
        ix = np.concatenate([ix, rng.choice(again, n - ix.size, replace=True)])
    return rng.permutation(ix).astype(np.uint32)


def check_against_oracle(c, ix, got, image_after, image, o, write_back):
    """Entries of a block listed once: exactly the oracle's payload, status and image row.  Copies of a
    block listed more than once (at most t errors): the oracle's payload each, statuses in {0, 1} with at
    least one 1 where the block had errors and write-back is on; without write-back every copy's status
    is the oracle's."""
    o_data, o_st, o_fixed, _ = o
    data, st, spill = got
    assert np.array_equal(data, o_data[ix])
    assert not spill.any()  # n = 255: a write-back never passes the block's end
    counts = np.bincount(ix, minlength=BLOCKS)
    once = counts[ix] == 1
    if not write_back:
        once[:] = True
    assert np.array_equal(st[once], o_st[ix][once])
    for b in np.nonzero(counts > 1)[0] if write_back else ():
        s = st[ix == b]
        assert set(s) <= {0, 1} and (s == 1).any() == bool(o_st[b]), (b, s)
    exp = image.reshape(BLOCKS, c.raw).copy()
    if write_back:
        exp[ix] = o_fixed[ix]
    assert np.array_equal(image_after, exp.reshape(-1))


@pytest.mark.parametrize("t", [1, 2, 3, 4])
def test_decode_list_against_the_oracle(oracle, t):
    c = Codec(oracle, "rs", 512, t)
    assert c.eng.list_kernel_name() == DIRECT
    rng = rng_for("direct", t)
    image, level = leveled_image(c, rng)
    o = c.decode(image)
    assert (o[1] == 1).any() and (level == t + 1).any()
    for n in LENGTHS:
        for skew in SKEWS:
            ix = listed(rng, n, level, t)
            assert n < 17 or ({*range(16), BLOCKS - 1} <= set(ix.tolist()))
            for wb in (True, False):
                g = Skewed(image, skew)
                got = decode_list(c.eng, g, ix, c.ds, write_back=wb)
                check_against_oracle(c, ix, got, g.result(), image, o, wb)


def test_out_of_range_entries(oracle):
    """Entries equal to image_blocks, past it and 0xFFFFFFFF at a tile's first and last row and as a
    whole tile of 64: status 9, a zero payload, nothing read or written for them."""
    t = 3
    c = Codec(oracle, "rs", 512, t)
    rng = rng_for("direct-oob")
    level = np.arange(BLOCKS) % (t + 1)  # at most t errors
    image = c.corrupt(rng, c.valid_image(rng, BLOCKS), level)
    o_data, o_st, o_fixed, _ = c.decode(image)
    bad = np.array([BLOCKS, BLOCKS + 7, 0xFFFFFFFF, 1 << 31], np.uint32)
    inside = rng.permutation(BLOCKS).astype(np.uint32)
    tile0 = np.concatenate([[BLOCKS], inside[:62], [0xFFFFFFFF]])
    tile1 = bad[np.arange(64) % bad.size]
    tile2 = np.concatenate([[BLOCKS + 7], inside[62:94], bad[np.arange(30) % bad.size], [BLOCKS]])
    part = np.concatenate([[0xFFFFFFFF], inside[94:96], [BLOCKS]])
    ix = np.concatenate([tile0, tile1, tile2, part]).astype(np.uint32)
    assert ix.size == 3 * 64 + 4
    oob = ix >= BLOCKS
    valid = ix[~oob].astype(np.int64)
    assert np.unique(valid).size == valid.size == BLOCKS and oob[64:128].all()
    for skew in (0, 61):
        g = Skewed(image, skew)
        data, st, spill = decode_list(c.eng, g, ix, c.ds, write_back=True)
        assert np.array_equal(st, np.where(oob, 9, o_st[np.where(oob, 0, ix)]))
        assert not data[oob].any() and np.array_equal(data[~oob], o_data[valid])
        assert not spill.any()
        assert np.array_equal(g.result(), o_fixed.reshape(-1))  # every block listed once: all corrected
        # an image of no whole block: every entry is out of range and nothing is dereferenced
        out = Outputs(8, c.ds)
        d8, s8, _ = out.views()
        c.eng.decode_list(g.image[:100], d_index(np.arange(8)), d8, s8, write_back=True)
        d8, s8, _ = out.result()
        assert (s8 == 9).all() and not d8.any()
    torch.cuda.synchronize()  # no fault behind any of it


def test_multi_tile_walk(oracle):
    """More tiles than the persistent grid holds workgroups, three times over, and a partial tile: every
    workgroup runs its prologue, steady-state iterations, its last tile, and one of them the partial
    tile.  A seeded permutation of an image 50 blocks larger."""
    c = Codec(oracle, "rs", 512, 3)
    rng = rng_for("direct-walk")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nb = 3 * 3 * cus * 64 + 37
    blocks = nb + 50
    image = _rs_errors(rng, c.valid_image(rng, blocks), c.raw, c.t, blocks)
    ix = rng.permutation(blocks)[:nb].astype(np.uint32)
    o_data, o_st, o_fixed, _ = c.decode(image)
    exp = image.reshape(blocks, c.raw).copy()
    exp[ix] = o_fixed[ix]
    image_d = dev(image)
    out = Outputs(nb, c.ds)
    data, st, spill = out.views()
    c.eng.decode_list(image_d, d_index(ix), data, st, write_back=True, spill=spill)
    data, st, spill = out.result()
    assert np.array_equal(st, o_st[ix])
    assert np.array_equal(data, o_data[ix])
    assert np.array_equal(host(image_d), exp.reshape(-1))


def test_repeated_blocks(oracle):
    """A block with 2 and one with 3 error bytes (t = 3), each listed three times inside one tile, and
    once in each of three tiles (three workgroups, whose reads may see another's write-back partly
    applied): every copy gets the oracle's payload, statuses are 0 or 1 with at least one 1 per block,
    and the image ends corrected."""
    c = Codec(oracle, "rs", 512, 3)
    rng = rng_for("direct-rep")
    level = np.zeros(BLOCKS, np.int64)
    A, B = 5, 77
    level[A], level[B] = 2, 3
    image = c.corrupt(rng, c.valid_image(rng, BLOCKS), level)
    o_data, o_st, o_fixed, _ = c.decode(image)
    assert o_st[A] == 1 and o_st[B] == 1 and o_st.sum() == 2
    clean = np.array([b for b in range(BLOCKS) if b not in (A, B)], np.uint32)
    one_tile = clean[:64].copy()
    one_tile[[0, 17, 63]] = A
    one_tile[[1, 40, 62]] = B
    three_tiles = np.concatenate([clean[:64], clean[20:84], clean[30:94]])
    three_tiles[[3, 64 + 60, 128 + 31]] = A
    three_tiles[[63, 64, 128 + 32]] = B
    for ix in (one_tile, three_tiles):
        for skew in (0, 3):
            g = Skewed(image, skew)
            data, st, _ = decode_list(c.eng, g, ix, c.ds, write_back=True)
            assert np.array_equal(data, o_data[ix])
            for b in (A, B):
                s = st[ix == b]
                assert s.size == 3 and set(s) <= {0, 1} and (s == 1).any(), (b, s)
            assert not st[(ix != A) & (ix != B)].any()
            assert np.array_equal(g.result(), o_fixed.reshape(-1))


# ------------------------------------------------------------------------------------
# the staged path of the same build as a second opinion
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 3, 4])
def test_direct_equals_staged(oracle, t):
    c = Codec(oracle, "rs", 512, t)
    staged = staged_engine(ECC_REED_SOLOMON, 512, t)
    assert (c.eng.list_kernel_name(), staged.list_kernel_name()) == (DIRECT, STAGED)
    rng = rng_for("direct-diff", t)
    image, level = leveled_image(c, rng)  # 0 .. t + 1 errors: the blocks beyond capability included
    perm = rng.permutation(BLOCKS).astype(np.uint32)
    ix = np.concatenate([perm[:40], [BLOCKS, 0xFFFFFFFF], perm[40:90]]).astype(np.uint32)  # no repeats
    for wb in (True, False):
        res = []
        for eng in (c.eng, staged):
            g = Skewed(image, 61)
            data, st, spill = decode_list(eng, g, ix, c.ds, write_back=wb)
            res.append((data, st, spill, g.result()))
        for a, b in zip(*res):
            assert np.array_equal(a, b)
        assert (res[0][1] == 9).sum() == 2 and (res[0][1] == 1).any()
    # read_extents, the file shape with a non-zero first offset
    blocks = perm[:41]
    off0 = 7
    nbytes = (c.ds - off0) + 39 * c.ds + 5
    ext = file_extents(blocks, off0, nbytes, c.ds)
    assert int(ext["offset"][0]) == off0 and int(ext["length"].astype(np.int64).sum()) == nbytes
    for wb in (True, False):
        res = []
        for eng in (c.eng, staged):
            g = Skewed(image, 61)
            out = torch.full((nbytes + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
            st = torch.full((len(ext) + TAIL,), 77, dtype=torch.uint8, device="cuda")
            eng.read_extents(g.image, ext, out[3:3 + nbytes], st[:len(ext)], write_back=wb)
            torch.cuda.synchronize()
            res.append((host(out), host(st), g.result()))
        for a, b in zip(*res):
            assert np.array_equal(a, b)
        out, st, img = res[0]
        assert (out[:3] == 0xA5).all() and (out[3 + nbytes:] == 0xA5).all() and (st[len(ext):] == 77).all()
        o_data, o_st, o_fixed, _ = c.decode(image)
        payload = o_data[blocks].reshape(-1)
        assert np.array_equal(out[3:3 + nbytes], payload[off0:off0 + nbytes])
        assert np.array_equal(st[:len(ext)], o_st[blocks[:len(ext)]])


def test_two_streams_decode_disjoint_halves(oracle):
    """Two direct list decodes of one engine on two streams, side by side on disjoint halves of one image
    (no ordering between them: there is no staging to protect)."""
    c = Codec(oracle, "rs", 512, 3)
    assert c.eng.list_kernel_name() == DIRECT
    rng = rng_for("direct-streams")
    blocks = 4000
    image = _rs_errors(rng, c.valid_image(rng, blocks), c.raw, c.t, blocks)
    half = blocks // 2
    lists = [rng.permutation(half).astype(np.uint32), (half + rng.permutation(half)).astype(np.uint32)]
    o_data, o_st, o_fixed, _ = c.decode(image)
    image_d = dev(image)
    ix_d = [d_index(ix) for ix in lists]
    data_d = [torch.zeros(half * c.ds, dtype=torch.uint8, device="cuda") for _ in lists]
    st_d = [torch.full((half,), 77, dtype=torch.uint8, device="cuda") for _ in lists]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for k, s in enumerate(streams):
        c.eng.decode_list(image_d, ix_d[k], data_d[k], st_d[k], write_back=True, stream=s)
    for s in streams:
        s.synchronize()
    for k, ix in enumerate(lists):
        assert np.array_equal(host(st_d[k]), o_st[ix])
        assert np.array_equal(host(data_d[k]).reshape(half, c.ds), o_data[ix])
    assert np.array_equal(host(image_d), o_fixed.reshape(-1))
