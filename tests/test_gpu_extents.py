"""GPU tests of the byte-extent calls (include/ppfs_ecc.h ppfs_ecc_*_extents_*; EccEngine.read_extents /
write_extents, their host forms, IBlockDevice.read_extents / write_extents) against the CPU oracle:
entry i of a batch gets exactly what the reference's readBlock({block, offset}, length) /
writeBlock(bytes, {block, offset}) gives, the entries taken in list order, and nothing outside the
named bytes and blocks changes.

The geometry is that of tests/test_gpu_list.py: an image of 96 blocks at an odd offset inside a guarded
buffer, a list of 41 distinct blocks, blocks corrupted at levels 0..t+1 (RS) or 0..3 bit flips.  The
packed buffer sits at an odd offset inside guards of 0xA5 as well.  The small cases take their expected
values from an OracleDevice over a copy of the image, one read / write per entry in list order; the long
case from the batch oracle and numpy slicing."""
import numpy as np
import pytest

from tests.conftest import gpu_available
from tests.oracle_lib import OracleDevice
from tests.test_gpu_list import (BLOCKS, GUARD, LISTED, Codec, Guarded, _rs_errors, corrupted_image, dev, host, rng_for,
                                 small_list)
from tests.test_gpu_list_direct import staged_engine

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch

from paritypartyfs_amd import ECC_REED_SOLOMON, EccEngine
from paritypartyfs_amd._native import EXTENT_DTYPE, EccError
from paritypartyfs_amd.block_device import (DataLocation, ECCType, HeapDisk, Logger, create_block_device, file_extents)

PSKEW = 45  # the packed buffer's odd offset inside its guards

CODECS = [("rs", 512, 3), ("rs", 4096, 16), ("rs", 255, 6), ("rs", 64, 3),
          ("crc", 64, 0x9960034c), ("crc", 5, 0xc1acf),
          ("ham", 2, 0), ("ham", 256, 0), ("ham", 4096, 0),
          ("par", 1, 0), ("par", 3, 0), ("par", 4096, 0),  # par-1: dataSize() == 0, every entry is zero-length
          ("none", 255, 0)]
CODEC_IDS = [f"{k}-{bs}-{x:x}" if k == "crc" else f"{k}-{bs}-{x}" for k, bs, x in CODECS]
FORMS = ["device", "host"]
TYPE_OF = {"none": 0, "crc": 1, "ham": 2, "par": 3, "rs": 4}


def extents(rows):
    return np.array([tuple(int(v) for v in r) for r in rows], dtype=EXTENT_DTYPE).reshape(-1)


# ------------------------------------------------------------------------------------
# the expected values: the reference's per-block calls, entry by entry
# ------------------------------------------------------------------------------------
def is_valid(e, blocks, ds, nbytes):
    """The three rules of include/ppfs_ecc.h, restated."""
    blk, off, ln, pos = int(e["block"]), int(e["offset"]), int(e["length"]), int(e["pos"])
    return blk < blocks and off <= ds and pos + min(ln, ds - off) <= nbytes


class Walk:
    """An OracleDevice over a copy of the image.  A shortened RS code's write-back may run past its
    block on the reference's disk; the engine reports such a spill and never applies it (and the extent
    calls take no spill argument), so for those codes the bytes outside the entry's block are put back
    after every call."""

    def __init__(self, c, image):
        self.c = c
        self.od = OracleDevice(c.o, TYPE_OF[c.kind], c.bs, c.x if c.kind == "rs" else 3, getattr(c, "P", 0), image.size)
        self.od.disk[:] = image
        assert (self.od.raw_block_size(), self.od.data_size()) == (c.raw, c.ds)
        self.confine = c.kind == "rs" and c.raw < 255

    def _call(self, block, fn):
        before = self.od.disk.copy() if self.confine else None
        n0 = self.od.o.L.oracle_dev_log_len(self.od.h)
        rc, val = fn()
        if before is not None:
            lo, hi = block * self.c.raw, (block + 1) * self.c.raw
            self.od.disk[:lo] = before[:lo]
            self.od.disk[hi:] = before[hi:]
        corrected = self.od.o.L.oracle_dev_log_len(self.od.h) > n0
        return (rc if rc else (1 if corrected else 0)), val

    def read(self, ext, nbytes, fill=0xA5):
        """(packed buffer, status per entry) of readBlock per entry in list order."""
        out = np.full(nbytes, fill, np.uint8)
        st = np.zeros(len(ext), np.uint8)
        for k, e in enumerate(ext):
            if not is_valid(e, BLOCKS, self.c.ds, nbytes):
                st[k] = 9
                continue
            blk, off, ln, pos = int(e["block"]), int(e["offset"]), int(e["length"]), int(e["pos"])
            st[k], data = self._call(blk, lambda: self.od.read(blk, off, ln))
            n = min(ln, self.c.ds - off)
            if st[k] == 5:
                out[pos:pos + n] = 0
            else:
                assert len(data) == n
                out[pos:pos + n] = np.frombuffer(data, np.uint8)
        return out, st

    def write(self, ext, data):
        st = np.zeros(len(ext), np.uint8)
        for k, e in enumerate(ext):
            if not is_valid(e, BLOCKS, self.c.ds, data.size):
                st[k] = 9
                continue
            blk, off, ln, pos = int(e["block"]), int(e["offset"]), int(e["length"]), int(e["pos"])
            n = min(ln, self.c.ds - off)
            st[k], wrote = self._call(blk, lambda: self.od.write(blk, off, data[pos:pos + n].tobytes()))
            assert st[k] == 5 or wrote == n
        return st

    def image(self):
        return self.od.disk.copy()


# ------------------------------------------------------------------------------------
# the two forms of the calls behind one face: numpy in, numpy out, guards checked
# ------------------------------------------------------------------------------------
class GuardedBuf:
    """The packed buffer at an odd offset inside guard bytes, on the device or on the host."""

    def __init__(self, form, content):
        self.form, self.n = form, content.size
        buf = np.full(GUARD + PSKEW + self.n + GUARD, 0xA5, np.uint8)
        buf[GUARD + PSKEW:GUARD + PSKEW + self.n] = content
        self.buf = dev(buf) if form == "device" else buf
        self.view = self.buf[GUARD + PSKEW:GUARD + PSKEW + self.n]

    def result(self):
        b = host(self.buf) if self.form == "device" else self.buf
        assert (b[:GUARD + PSKEW] == 0xA5).all() and (b[GUARD + PSKEW + self.n:] == 0xA5).all(), "write outside the buffer"
        return b[GUARD + PSKEW:GUARD + PSKEW + self.n].copy()


class HostImage:
    """Guarded's face for a host image."""

    def __init__(self, image):
        self.n = image.size
        self.buf = np.full(GUARD + 61 + self.n + GUARD, 0xA5, np.uint8)
        self.image = self.buf[GUARD + 61:GUARD + 61 + self.n]
        self.image[:] = image

    def result(self):
        b = self.buf
        assert (b[:GUARD + 61] == 0xA5).all() and (b[GUARD + 61 + self.n:] == 0xA5).all(), "write outside the image"
        return self.image.copy()


def status_buffer(form, n, aligned=True):
    """n status bytes preset to 77; with aligned=False at an odd address."""
    if form == "device":
        t = torch.full((n + 16,), 77, dtype=torch.uint8, device="cuda")
        return t[:n] if aligned else t[3:3 + n]
    a = np.full(n + 16, 77, np.uint8)
    return a[:n] if aligned else a[3:3 + n]


def to_np(form, x):
    return host(x) if form == "device" else np.array(x, copy=True)


def run_read(form, c, image, ext, nbytes, write_back=True, with_status=True, aligned_status=True):
    """-> (packed buffer, status or None, image afterwards)"""
    g = Guarded(image) if form == "device" else HostImage(image)
    out = GuardedBuf(form, np.full(nbytes, 0xA5, np.uint8))
    st = status_buffer(form, len(ext), aligned_status) if with_status else None
    if form == "device":
        c.eng.read_extents(g.image, ext, out.view, st, write_back=write_back)
        torch.cuda.synchronize()
    else:
        c.eng.read_extents_host(g.image, ext, out.view, st, write_back=write_back)
    return out.result(), None if st is None else to_np(form, st), g.result()


def run_write(form, c, image, ext, data, with_status=True, aligned_status=True):
    """-> (status or None, image afterwards)"""
    g = Guarded(image) if form == "device" else HostImage(image)
    buf = GuardedBuf(form, data)
    st = status_buffer(form, len(ext), aligned_status) if with_status else None
    if form == "device":
        c.eng.write_extents(buf.view, g.image, ext, st)
        torch.cuda.synchronize()
    else:
        c.eng.write_extents_host(buf.view, g.image, ext, st)
    assert np.array_equal(buf.result(), data)  # the caller's bytes are only read
    return None if st is None else to_np(form, st), g.result()


# ------------------------------------------------------------------------------------
# 1. segment shapes
# ------------------------------------------------------------------------------------
def shape_cycle(ds):
    """The (offset, length) shapes, their offsets brought into [0, ds] where ds is tiny (the lengths
    are left to the call's own clamp)."""
    raw = [(0, ds), (0, 0), (ds, 0), (0, 1), (ds - 1, 1), (ds - 1, 5), (1, ds - 1), (3, 16), (5, 17), (7, 15), (0, ds + 9),
           (ds // 2, 33)]
    return [(min(max(o, 0), ds), max(n, 0)) for o, n in raw]


def shaped_extents(ix, ds):
    """One entry per listed block, the shapes in a cycle.  The first segment starts at pos 0, 1-7 byte
    gaps lie between the segments -- chosen so that the segments' starts meet all 16 residues mod 16 --
    and the last segment ends exactly at the buffer's end.  Returns (extents, bytes of the buffer)."""
    shapes = shape_cycle(ds)
    rows, pos, seen = [], 0, set()
    for k, blk in enumerate(ix):
        off, ln = shapes[k % len(shapes)]
        n = min(ln, ds - off)
        if k:
            gaps = [g for g in range(1, 8) if n and (pos + g) % 16 not in seen] or [1 + k % 7]
            pos += gaps[0]
        if n:
            seen.add(pos % 16)
        rows.append((pos, int(blk), off, ln))
        pos += n
    assert ds == 0 or len(seen) == 16
    return extents(rows), pos


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,bs,x", CODECS, ids=CODEC_IDS)
def test_read_segment_shapes(oracle, kind, bs, x, form):
    c = Codec(oracle, kind, bs, x)
    rng = rng_for("xr", kind, bs, x)
    ix = small_list(rng)
    image = corrupted_image(c, rng, ix)
    ext, nbytes = shaped_extents(ix, c.ds)
    assert ext["pos"][0] == 0
    w = Walk(c, image)
    exp_out, exp_st = w.read(ext, nbytes)
    exp_image = w.image()
    assert not (exp_st == 9).any()
    if c.write_back:
        assert (exp_st == 1).any() and not np.array_equal(exp_image, image)
    else:
        assert np.array_equal(exp_image, image)
    out, st, img = run_read(form, c, image, ext, nbytes, write_back=True)
    assert np.array_equal(st, exp_st)
    assert np.array_equal(out, exp_out)  # the gaps still 0xA5
    assert np.array_equal(img, exp_image)  # the listed blocks written back, every other byte as it was
    # write_back = 0: the same bytes and statuses, the image untouched; no status array: the same bytes
    out, st, img = run_read(form, c, image, ext, nbytes, write_back=False, aligned_status=False)
    assert np.array_equal(st, exp_st) and np.array_equal(out, exp_out) and np.array_equal(img, image)
    out, st, img = run_read(form, c, image, ext, nbytes, write_back=True, with_status=False)
    assert st is None and np.array_equal(out, exp_out) and np.array_equal(img, exp_image)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,bs,x", CODECS, ids=CODEC_IDS)
def test_write_segment_shapes(oracle, kind, bs, x, form):
    c = Codec(oracle, kind, bs, x)
    rng = rng_for("xw", kind, bs, x)
    ix = small_list(rng)
    image = corrupted_image(c, rng, ix)
    ext, nbytes = shaped_extents(ix, c.ds)
    data = rng.integers(0, 256, nbytes, dtype=np.uint8)
    w = Walk(c, image)
    exp_st = w.write(ext, data)
    exp_image = w.image()
    st, img = run_write(form, c, image, ext, data)
    assert np.array_equal(st, exp_st)
    assert np.array_equal(img, exp_image)  # unlisted blocks and the guards untouched
    failed = ix[exp_st == 5]
    rows_before, rows_after = image.reshape(BLOCKS, c.raw), img.reshape(BLOCKS, c.raw)
    assert np.array_equal(rows_after[failed], rows_before[failed])  # status 5: byte-identical to before
    if kind in ("crc", "par"):
        assert failed.size
    # no status array, and one at an odd address: the context's own selects the rows
    st, img = run_write(form, c, image, ext, data, with_status=False)
    assert st is None and np.array_equal(img, exp_image)
    st, img = run_write(form, c, image, ext, data, aligned_status=False)
    assert np.array_equal(st, exp_st) and np.array_equal(img, exp_image)


# ------------------------------------------------------------------------------------
# 2. the file shape
# ------------------------------------------------------------------------------------
def file_cases(ds):
    """(off0, nbytes) over the whole 41-block list for off0 in {0, 1, ds-1} x tail in {1, ds-1, ds}."""
    out = []
    for off0 in sorted({0, 1, ds - 1}):
        for tail in sorted({1, ds - 1, ds}):
            if 0 <= off0 < ds and tail > 0:
                out.append((off0, (ds - off0) + (LISTED - 2) * ds + tail))
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,bs,x", CODECS, ids=CODEC_IDS)
def test_file_shape(oracle, kind, bs, x, form):
    c = Codec(oracle, kind, bs, x)
    rng = rng_for("xf", kind, bs, x)
    ix = small_list(rng)
    image = corrupted_image(c, rng, ix)
    # the list decode's payload array (failed blocks read as zeros) and the image after its write-back
    o_data, o_st, o_fixed, _ = c.decode(image)
    payload = o_data[ix].copy()
    payload[o_st[ix] == 5] = 0
    payload = payload.reshape(-1)
    exp_read_image = image.reshape(BLOCKS, c.raw).copy()
    if c.write_back:
        exp_read_image[ix] = o_fixed[ix]
    if c.ds == 0:
        assert len(file_extents(ix, 0, 10, c.ds)) == 0  # nothing to walk, and nothing divides by ds
        out, st, img = run_read(form, c, image, file_extents(ix, 0, 10, c.ds), 10)
        assert (out == 0xA5).all() and np.array_equal(img, image)
        return
    cases = [(ix, off0, nbytes) for off0, nbytes in file_cases(c.ds)]
    if c.ds >= 8:
        cases.append((ix[:1], 3, 5))  # a file inside one block: head = tail
    for blocks, off0, nbytes in cases:
        ext = file_extents(blocks, off0, nbytes, c.ds)
        assert int(ext["length"].astype(np.int64).sum()) == nbytes and int(ext["offset"][0]) == off0
        out, st, img = run_read(form, c, image, ext, nbytes)
        assert np.array_equal(out, payload[off0:off0 + nbytes]), (off0, nbytes)
        assert np.array_equal(st, o_st[blocks[:len(ext)]])
        exp = image.reshape(BLOCKS, c.raw).copy()
        exp[blocks[:len(ext)]] = exp_read_image[blocks[:len(ext)]]
        assert np.array_equal(img, exp.reshape(-1))
        # the same walk as writeFile makes it
        data = rng.integers(0, 256, nbytes, dtype=np.uint8)
        w = Walk(c, image)
        exp_st = w.write(ext, data)
        st, img = run_write(form, c, image, ext, data)
        assert np.array_equal(st, exp_st) and np.array_equal(img, w.image()), (off0, nbytes)


# ------------------------------------------------------------------------------------
# 3. invalid entries
# ------------------------------------------------------------------------------------
def mixed_extents(c, ix):
    """Valid entries with the four kinds of invalid ones between them; -> (extents, bytes, invalid mask)."""
    ds = c.ds
    n = min(7, ds)
    rows, pos = [], 0
    for k in range(6):
        rows.append((pos, int(ix[k]), min(2, ds), n))
        pos += min(n, ds - min(2, ds)) + 3
    nbytes = pos + 40
    victim = int(ix[10])
    rows.insert(1, (pos, BLOCKS, 0, n))                # block = image_blocks
    rows.insert(3, (pos + 8, 0xFFFFFFFF, 0, n))        # block = 0xFFFFFFFF
    rows.insert(5, (pos + 16, victim, ds + 1, n))      # offset = ds + 1
    rows.append((nbytes + 1 - min(n, ds), victim, 0, n))  # pos + len = out_bytes + 1
    rows.append((nbytes - min(n, ds), int(ix[11]), 0, n))  # ... and = out_bytes: valid
    ext = extents(rows)
    invalid = np.array([not is_valid(e, BLOCKS, ds, nbytes) for e in ext])
    return ext, nbytes, invalid


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,bs,x", [("rs", 512, 3), ("rs", 64, 3), ("crc", 5, 0xc1acf), ("ham", 256, 0), ("par", 1, 0),
                                       ("none", 255, 0)], ids=["rs255", "rs64", "crc5", "ham256", "par1", "none"])
def test_invalid_entries(oracle, kind, bs, x, form):
    c = Codec(oracle, kind, bs, x)
    rng = rng_for("xi", kind, bs, x)
    ix = small_list(rng)
    image = corrupted_image(c, rng, ix)
    ext, nbytes, invalid = mixed_extents(c, ix)
    assert list(np.nonzero(invalid)[0]) == [1, 3, 5, 9]
    w = Walk(c, image)
    exp_out, exp_st = w.read(ext, nbytes)
    assert list(exp_st[invalid]) == [9] * int(invalid.sum())
    out, st, img = run_read(form, c, image, ext, nbytes)
    assert np.array_equal(st, exp_st) and np.array_equal(out, exp_out) and np.array_equal(img, w.image())
    data = rng.integers(0, 256, nbytes, dtype=np.uint8)
    w = Walk(c, image)
    exp_st = w.write(ext, data)
    st, img = run_write(form, c, image, ext, data)
    assert np.array_equal(st, exp_st) and np.array_equal(img, w.image())
    # an empty packed buffer, passed as NULL: every entry with bytes is invalid, the others still run
    w = Walk(c, image)
    exp_out, exp_st = w.read(ext, 0)
    g = Guarded(image) if form == "device" else HostImage(image)
    st = status_buffer(form, len(ext))
    if form == "device":
        c.eng.read_extents(g.image, ext, None, st)
    else:
        c.eng.read_extents_host(g.image, ext, None, st)
    assert np.array_equal(to_np(form, st), exp_st) and np.array_equal(g.result(), w.image())


# ------------------------------------------------------------------------------------
# 4. more than one piece
# ------------------------------------------------------------------------------------
def test_extents_longer_than_one_piece(oracle):
    c = Codec(oracle, "rs", 512, 3)
    rng = rng_for("xpiece")
    n = c.eng.host_chunk_blocks() + 37
    blocks = n + 50
    image = _rs_errors(rng, c.valid_image(rng, blocks), c.raw, c.t, blocks)
    ix = rng.permutation(blocks)[:n].astype(np.uint32)
    off, ln = 11, 7
    ext = np.zeros(n, EXTENT_DTYPE)
    ext["pos"], ext["block"], ext["offset"], ext["length"] = np.arange(n, dtype=np.uint64) * ln, ix, off, ln
    o_data, o_st, o_fixed, _ = c.decode(image)
    assert not (o_st == 5).any()
    exp_image = image.reshape(blocks, c.raw).copy()
    exp_image[ix] = o_fixed[ix]
    image_d = dev(image)
    out_d = torch.full((n * ln,), 0xA5, dtype=torch.uint8, device="cuda")
    st_d = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    c.eng.read_extents(image_d, ext, out_d, st_d, write_back=True)
    assert np.array_equal(host(st_d), o_st[ix])
    assert np.array_equal(host(out_d).reshape(n, ln), o_data[ix][:, off:off + ln])
    assert np.array_equal(host(image_d), exp_image.reshape(-1))
    # write: the old payloads with 7 new bytes each, encoded again
    new = rng.integers(0, 256, n * ln, dtype=np.uint8)
    payload = o_data[ix].copy()
    payload[:, off:off + ln] = new.reshape(n, ln)
    exp_image = image.reshape(blocks, c.raw).copy()
    exp_image[ix] = c.encode(payload.reshape(-1), None).reshape(n, c.raw)
    image_d = dev(image)
    st_d.fill_(77)
    c.eng.write_extents(dev(new), image_d, ext, st_d)
    assert np.array_equal(host(st_d), o_st[ix])
    assert np.array_equal(host(image_d), exp_image.reshape(-1))


def test_extents_direct_equals_staged(oracle):
    """RS(255, 249) over two pieces, the second shorter than one 64-row tile, through the direct engine
    and through one created under PPFS_ECC_LIST_DIRECT=0 (the staged piece loop, which no other extent
    test runs for a 255-byte RS code): packed bytes, statuses and the whole image are byte-identical, with
    the status array 16-byte aligned, 3 bytes past a boundary (the copy out of the context's own array)
    and absent; the aligned leg equals the oracle too.  1 .. t byte errors in every seventh block, five
    invalid entries of each of test_invalid_entries' four kinds, in both pieces."""
    c = Codec(oracle, "rs", 512, 3)
    staged = staged_engine(ECC_REED_SOLOMON, 512, 3)
    assert (c.eng.list_kernel_name(), staged.list_kernel_name()) == ("rs255-wg-list-lds", "gather-stage-scatter")
    rng = rng_for("xdiff")
    piece = c.eng.host_chunk_blocks() & ~1023
    n = c.eng.host_chunk_blocks() + 37
    assert piece < n < 2 * piece and n - piece < 64
    blocks = n + 50
    rows = c.valid_image(rng, blocks).reshape(blocks, c.raw).copy()
    hit = np.arange(0, blocks, 7)
    ne, start = 1 + np.arange(hit.size) % c.t, rng.integers(0, c.raw, hit.size)
    for j in range(c.t):  # 37 is a unit mod 255: distinct positions per block
        rows[hit[ne > j], (start[ne > j] + 37 * j) % c.raw] ^= rng.integers(1, 256, int((ne > j).sum()), dtype=np.uint8)
    image = rows.reshape(-1)
    ix = rng.permutation(blocks)[:n].astype(np.uint32)
    off, ln = 11, 7
    nbytes = n * ln
    ext = np.zeros(n, EXTENT_DTYPE)
    ext["pos"], ext["block"], ext["offset"], ext["length"] = np.arange(n, dtype=np.uint64) * ln, ix, off, ln
    for k, (field, value) in enumerate((("block", blocks), ("block", 0xFFFFFFFF), ("offset", c.ds + 1),
                                        ("pos", nbytes + 1 - ln))):
        at = np.array([5 + k, 1000 + k, piece - 1 - k, piece + 3 + 8 * k, piece + 7 + 8 * k])
        ext[field][at] = value
    valid = (ext["block"] < blocks) & (ext["offset"] <= c.ds) & (ext["pos"] + ln <= nbytes)
    assert (~valid).sum() == 20 and (~valid)[:piece].sum() == 12 and valid[-1]
    ixv = ix[valid]
    o_data, o_st, o_fixed, _ = c.decode(image)
    assert not (o_st == 5).any() and {1, 2, 3} <= set(ne) and (o_st[hit] == 1).all()
    exp_st = np.where(valid, o_st[ix], 9).astype(np.uint8)
    exp_out = np.full((n, ln), 0xA5, np.uint8)
    exp_out[valid] = o_data[ixv][:, off:off + ln]
    exp_read = rows.copy()
    exp_read[ixv] = o_fixed[ixv]
    new = rng.integers(0, 256, nbytes, dtype=np.uint8)
    payload = o_data[ixv].copy()
    payload[:, off:off + ln] = new.reshape(n, ln)[valid]
    exp_write = rows.copy()
    exp_write[ixv] = c.encode(payload.reshape(-1), None).reshape(-1, c.raw)
    new_d = dev(new)

    def status(leg):
        """(the whole guarded buffer, the n bytes the call gets)"""
        if leg == "absent":
            return None, None
        t = torch.full((n + 48,), 77, dtype=torch.uint8, device="cuda")
        lo = 16 if leg == "aligned" else 19
        assert t.data_ptr() % 16 == 0
        return t, t[lo:lo + n]

    def status_of(t, leg):
        if t is None:
            return None
        b, lo = host(t), 16 if leg == "aligned" else 19
        assert (b[:lo] == 77).all() and (b[lo + n:] == 77).all(), "write outside the status array"
        return b[lo:lo + n]

    for leg in ("aligned", "skewed", "absent"):
        res = []
        for eng in (c.eng, staged):
            image_d = dev(image)
            out_d = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
            t, st = status(leg)
            eng.read_extents(image_d, ext, out_d, st, write_back=True)
            read = (host(out_d), status_of(t, leg), host(image_d))
            image_d = dev(image)
            t, st = status(leg)
            eng.write_extents(new_d, image_d, ext, st)
            res.append(read + (status_of(t, leg), host(image_d)))
        for a, b in zip(*res):
            assert (a is None and b is None) or np.array_equal(a, b), leg
        if leg == "aligned":
            out, r_st, r_img, w_st, w_img = res[0]
            assert np.array_equal(out, exp_out.reshape(-1)) and np.array_equal(r_st, exp_st)
            assert np.array_equal(r_img, exp_read.reshape(-1))
            assert np.array_equal(w_st, exp_st) and np.array_equal(w_img, exp_write.reshape(-1))


# ------------------------------------------------------------------------------------
# 5. / 6. repeated blocks
# ------------------------------------------------------------------------------------
def _image_with_damage(c, rng, damaged):
    level = np.zeros(BLOCKS, np.int64)
    level[damaged] = 2
    return c.corrupt(rng, c.valid_image(rng, BLOCKS), level)


def test_repeated_block_in_a_device_read(oracle):
    c = Codec(oracle, "rs", 512, 3)
    rng = rng_for("xrep")
    image = _image_with_damage(c, rng, [5])
    o_data, o_st, o_fixed, _ = c.decode(image)
    assert o_st[5] == 1
    ext = extents([(0, 5, 10, 20), (20, 9, 0, 4), (24, 5, 10, 20), (44, 5, 0, 249), (293, 3, 248, 9)])
    nbytes = 294
    exp = np.concatenate([o_data[5][10:30], o_data[9][:4], o_data[5][10:30], o_data[5], o_data[3][248:]])
    exp_image = image.reshape(BLOCKS, c.raw).copy()
    exp_image[5] = o_fixed[5]
    out, st, img = run_read("device", c, image, ext, nbytes, write_back=True)
    assert np.array_equal(out, exp)  # every copy gets the same bytes
    # the rule of decode_list: a copy reads the block before or after another copy's write-back
    assert set(st[[0, 2, 3]]) <= {0, 1} and (st[[0, 2, 3]] == 1).any() and st[1] == 0 and st[4] == 0
    assert np.array_equal(img, exp_image.reshape(-1))


def test_host_forms_take_repeated_blocks_in_list_order(oracle):
    c = Codec(oracle, "rs", 512, 3)
    rng = rng_for("xhrep")
    image = _image_with_damage(c, rng, [5, 7])
    # two writes into one block, bytes [0, 8) then [4, 12): both land, the second wins where they overlap
    ext = extents([(0, 5, 0, 8), (8, 9, 4, 8), (16, 5, 4, 8), (24, 7, 100, 8)])
    data = rng.integers(0, 256, 32, dtype=np.uint8)
    w = Walk(c, image)
    exp_st = w.write(ext, data)
    assert list(exp_st) == [1, 0, 0, 1]
    st, img = run_write("host", c, image, ext, data)
    assert np.array_equal(st, exp_st) and np.array_equal(img, w.image())
    got, _, _ = run_read("host", c, img, extents([(0, 5, 0, 12)]), 12)
    assert np.array_equal(got, np.concatenate([data[0:4], data[16:24]]))
    # a corrupted block read twice with write-back: status 1, then 0
    ext = extents([(0, 5, 3, 9), (9, 5, 3, 9), (18, 7, 0, 1)])
    w = Walk(c, image)
    exp_out, exp_st = w.read(ext, 19)
    assert list(exp_st) == [1, 0, 1]
    out, st, img = run_read("host", c, image, ext, 19)
    assert np.array_equal(st, exp_st) and np.array_equal(out, exp_out) and np.array_equal(img, w.image())


# ------------------------------------------------------------------------------------
# 7. a capturing stream
# ------------------------------------------------------------------------------------
def test_extent_call_refuses_a_capturing_stream():
    eng = EccEngine(ECC_REED_SOLOMON, 512, 3)
    image = torch.zeros(8 * 255, dtype=torch.uint8, device="cuda")
    ext = dev(extents([(0, 1, 3, 5), (5, 2, 0, 7)]).view(np.uint8))
    out = torch.zeros(12, dtype=torch.uint8, device="cuda")
    st = torch.zeros(16, dtype=torch.uint8, device="cuda")
    eng.read_extents(image, ext, out, st)  # the staging exists before the capture
    torch.cuda.synchronize()
    codes = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # captured and never replayed
        eng.decode(image, None, st, write_back=False, nblocks=4)  # a contiguous call may be captured
        for call in (lambda: eng.read_extents(image, ext, out, st), lambda: eng.write_extents(out, image, ext, st)):
            try:
                call()
                codes.append(0)
            except EccError as e:
                codes.append(e.code)
    assert codes == [-95, -95]  # PPFS_ECC_ENOTSUP
    st.fill_(77)
    eng.write_extents(out, image, ext, st)  # a later eager call works
    eng.read_extents(image, ext, out, st)
    assert list(host(st)[:2]) == [0, 0] and not host(out).any()


# ------------------------------------------------------------------------------------
# 8. the Python block devices
# ------------------------------------------------------------------------------------
DEVICES = [("rs", ECCType.ReedSolomon, 255, 0, 3), ("crc", ECCType.Crc, 64, 0x9960034c, 0),
           ("hamming", ECCType.Hamming, 256, 0, 0), ("parity", ECCType.Parity, 3, 0, 0)]


def _device(oracle, typ, bs, imp, t, disk_bytes):
    disk, log = HeapDisk(disk_bytes), Logger()
    poly = oracle.crc_explicit(imp) if imp else 0
    return create_block_device(disk, bs, typ, crc_polynomial_explicit=poly, rs_correctable_bytes=t, logger=log), disk, log


@pytest.mark.parametrize("name,typ,bs,imp,t", DEVICES, ids=[d[0] for d in DEVICES])
def test_block_device_extents_equal_the_per_block_loop(oracle, name, typ, bs, imp, t):
    rng = rng_for("xbd", name)
    probe, _, _ = _device(oracle, typ, bs, imp, t, 4096 * 4)
    raw, ds = probe.rawBlockSize(), probe.dataSize()
    size = BLOCKS * raw + 7  # a ragged disk end
    a, disk_a, log_a = _device(oracle, typ, bs, imp, t, size)
    b, disk_b, log_b = _device(oracle, typ, bs, imp, t, size)
    assert not a.writeBlocks(0, rng.integers(0, 256, (BLOCKS, ds), dtype=np.uint8)).any()

    def damage():
        for blk in range(0, BLOCKS, 3):
            for _ in range(1 + blk % 3):
                disk_a.buf[blk * raw + int(rng.integers(0, raw))] ^= 1 << int(rng.integers(0, 8))
        disk_b.buf[:] = disk_a.buf
        log_a.corrections.clear()
        log_b.corrections.clear()

    ix = small_list(rng)
    ext, nbytes = shaped_extents(ix, ds)
    # a block listed again (read after the first entry's write-back), one off the disk, an offset past ds
    more = extents([(0, int(ix[0]), 0, 1), (1, BLOCKS, 0, 1), (2, int(ix[1]), ds + 1, 1)])
    ext = np.concatenate([ext, more])
    damage()
    out = np.full(nbytes, 0xA5, np.uint8)
    err = a.read_extents(ext, out)
    exp = np.full(nbytes, 0xA5, np.uint8)
    for k, e in enumerate(ext):  # the same object's per-block calls on the twin disk
        off, n = int(e["offset"]), int(e["length"])
        if off > ds:
            assert err[k] == 9
            continue
        r = b.readBlock(DataLocation(int(e["block"]), off), n)
        assert (int(r.error()) if not r else 0) == err[k], (k, e)
        n = min(n, ds - off)
        if r:
            exp[int(e["pos"]):int(e["pos"]) + n] = np.frombuffer(r.value(), np.uint8)
        elif err[k] == 5:
            exp[int(e["pos"]):int(e["pos"]) + n] = 0
    assert np.array_equal(out, exp)
    assert np.array_equal(disk_a.buf, disk_b.buf)
    assert log_a.corrections == log_b.corrections  # length and order
    if name in ("rs", "hamming"):
        assert log_a.corrections
    damage()
    data = rng.integers(0, 256, nbytes, dtype=np.uint8)
    err = a.write_extents(ext, data)
    for k, e in enumerate(ext):
        off, n = int(e["offset"]), int(e["length"])
        if off > ds:
            assert err[k] == 9
            continue
        n = min(n, ds - off)
        r = b.writeBlock(data[int(e["pos"]):int(e["pos"]) + n].tobytes(), DataLocation(int(e["block"]), off))
        assert (int(r.error()) if not r else 0) == err[k], (k, e)
    assert np.array_equal(disk_a.buf, disk_b.buf)
    assert log_a.corrections == log_b.corrections
