"""GPU tests of the inode reads (include/ppfs_ecc.h ppfs_ecc_inode_span, ppfs_ecc_read_inodes_*; EccEngine.inode_span /
read_inodes / read_inodes_host; IBlockDevice.read_inodes) against the CPU oracle.

Expected values come from the per-inode loop -- InodeManager::get: Bitmap::getBit, then _readInode -- over the oracle's
device model (tests/oracle_lib.py OracleDevice), in the calls' batch form: every piece of an inode whose bit allows the
read is attempted, the first failing one gives the status.  Nothing expected comes from the engine.  The loop tells
which reads corrected a block; from that follow the three flavours of the repeat rule: the loop's own (the first
toucher reports 1: the host form), every sharer reports 1 (the device form without write-back), and each sharer 0 or
1 with at least one 1 (the device form with write-back).

Images are small: about 200 inodes, a bitmap with free and allocated bits, a table of random records, spare blocks
around both regions."""
import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch

from paritypartyfs_amd import _native
from paritypartyfs_amd._native import FILE_DTYPE, INODE_TABLE_DTYPE, EccError
from paritypartyfs_amd.block_device import (INODE_DTYPE, ECCType, FsError, HeapDisk, IBlockDevice, IDisk, Logger,
                                            create_block_device)
from paritypartyfs_amd.ecc import InodeCounts
from tests.oracle_lib import OracleDevice
from tests.test_gpu_file import flip, make_engine, oracle_encode, rng_for
from tests.test_gpu_files import FilesImage
from tests.test_gpu_list import Guarded, dev, host

PIECE = 16384  # PPFS_ECC_INODE_PIECE
# name, ECCType, block size, t, explicit CRC polynomial, unused: the tuples tests/test_gpu_file.py's helpers take.
# rs255: ds 249, every fourth inode straddles; rs64: a shortened code, ds 58, two or three pieces; parity32: ds 31,
# K = 4, three and four pieces
CFG = {c[0]: c for c in [("rs255_t3", 4, 255, 3, 0, 0), ("rs64_t3", 4, 64, 3, 0, 0), ("hamming512", 2, 512, 0, 0, 0),
                         ("crc512", 1, 512, 0, 0x104C11DB7, 0), ("parity32", 3, 32, 0, 0, 0)]}
NAMES = list(CFG)
FIXES = ["rs255_t3", "rs64_t3", "hamming512"]  # a single error is corrected and written back
FAILS = ["crc512", "parity32", "hamming512"]   # detection only, or a double flip


class InodeImage:
    """An inode bitmap and an inode table of `total` random inodes in one image."""

    def __init__(self, oracle, name, total=200, free=0.3, allocated=(), freed=()):
        self.oracle, self.cfg, self.total = oracle, CFG[name], total
        self.eng = make_engine(self.cfg)
        self.raw, self.ds = raw, ds = self.eng.raw_block_size, self.eng.data_size
        self.K = 2 + 79 // ds
        rng = rng_for("inodes", name, total)
        bm_bytes = (total + 7) // 8
        self.bitmap_block, self.bm_blocks = 2, -(-bm_bytes // ds)
        self.table_block = self.bitmap_block + self.bm_blocks + 5  # a shortened code's write-back runs into these
        self.t_blocks = -(-81 * total // ds)
        self.blocks = self.table_block + self.t_blocks + 6
        payload = rng.integers(0, 256, (self.blocks, ds), dtype=np.uint8)
        self.free = rng.random(total) < free
        self.free[list(allocated)] = False
        self.free[list(freed)] = True
        bits = np.zeros(self.bm_blocks * ds * 8, np.uint8)
        bits[:] = rng.integers(0, 2, bits.size)  # the bits past total are noise
        bits[:total] = self.free
        self.records = rng.integers(0, 256, (total, 81), dtype=np.uint8)
        self.records[:, 80] = rng.integers(0, 2, total)
        stream = payload[self.bitmap_block:self.bitmap_block + self.bm_blocks].reshape(-1)
        stream[:] = np.packbits(bits)
        stream = payload[self.table_block:self.table_block + self.t_blocks].reshape(-1)
        stream[:81 * total] = self.records.reshape(-1)
        self.clean = oracle_encode(oracle, self.cfg, payload).reshape(-1)
        assert self.clean.size == self.blocks * raw

    def table(self, check=1, table_block=None):
        t = np.zeros(1, INODE_TABLE_DTYPE)
        t["table_block"], t["bitmap_block"] = self.table_block if table_block is None else table_block, self.bitmap_block
        t["total_inodes"], t["check_bitmap"] = self.total, check
        return t

    def rows(self, image):
        return image.reshape(-1, self.raw)

    def blocks_of(self, i):
        """The table blocks inode i has bytes in."""
        return list(range(self.table_block + 81 * i // self.ds, self.table_block + (81 * i + 80) // self.ds + 1))

    def batch(self, extra=(), n=64):
        """About n numbers: straddling and non-straddling, free and allocated, three past the table, one repeated, the
        last inode; `extra` first."""
        rng = rng_for("batch", self.cfg[0], self.total, tuple(extra))
        least = len(self.blocks_of(0))
        straddler = next(i for i in range(self.total) if len(self.blocks_of(i)) > least and not self.free[i])
        nums = list(extra) + [self.total - 1, self.total, self.total + 5, 0xFFFFFFFF, 0, straddler]
        nums += rng.choice(self.total, n - len(nums) - 1, replace=False).tolist()
        nums.append(nums[len(extra) + 6])  # a number twice
        nums = np.array(nums, np.uint32)
        ok = nums[nums < self.total]
        assert self.free[ok].any() and not self.free[ok].all()
        assert len({len(self.blocks_of(int(i))) for i in ok}) >= 2
        return nums

    # ---- the per-inode loop over the oracle's device model ----
    def loop(self, image, numbers, check=1, table_block=None, nblocks=None):
        """Per inode the reads the loop makes and what they gave; the disk afterwards; the log."""
        _, typ, bs, t, poly, _ = self.cfg
        nblocks = self.blocks if nblocks is None else nblocks
        od = OracleDevice(self.oracle, typ, bs, t, poly, nblocks * self.raw)
        od.disk[:] = image[:nblocks * self.raw]
        L, ds = self.oracle.L, self.ds
        tb = self.table_block if table_block is None else table_block

        def read(block, offset, nbytes):
            n0 = L.oracle_dev_log_len(od.h)
            rc, data = od.read(block, offset, nbytes)
            return (rc if rc else int(L.oracle_dev_log_len(od.h) > n0)), data

        out = []
        for i in (int(x) for x in numbers):
            r = dict(ino=i, bit=None, pieces=[], rec=None, verdict=0)
            if i >= self.total:
                r["verdict"] = 9
            elif check:
                byte = i // 8
                st, data = read(self.bitmap_block + byte // ds, byte % ds, 1)
                r["bit"] = (self.bitmap_block + byte // ds, st)
                if st in (5, 9):
                    r["verdict"] = st
                elif data[0] & (0x80 >> (i % 8)):
                    r["verdict"] = 255
            if r["verdict"] == 0:
                got, block, off = bytearray(), tb + 81 * i // ds, 81 * i % ds
                while len(got) < 81:
                    want = 81 - len(got)
                    st, data = read(block, off, want)
                    r["pieces"].append((block, st))
                    got += data if st in (0, 1) else bytes(min(want, ds - off))
                    block, off = block + 1, 0
                r["rec"] = bytes(got)
            out.append(r)
        return out, od.disk.copy(), od.log_entries()

    def expect(self, reads, mode):
        """files, meta, status, piece_status, counts from the loop's reads.  mode "first": as the loop saw them; "all":
        every read of a block that some read corrected reports 1."""
        fixed = {b for r in reads for b, st in ([r["bit"]] if r["bit"] else []) + r["pieces"] if st == 1}

        def seen(b, st):
            return 1 if mode == "all" and st == 0 and b in fixed else st

        n, W = len(reads), 1 + self.K
        files, meta = np.zeros((n, 64), np.uint8), np.zeros((n, 24), np.uint8)
        status, pieces = np.zeros(n, np.uint8), np.full((n, W), 255, np.uint8)
        for j, r in enumerate(reads):
            sts = [seen(*r["bit"])] if r["bit"] else []
            if r["bit"]:
                pieces[j, 0] = sts[0]
            ps = [seen(b, st) for b, st in r["pieces"]]
            pieces[j, 1:1 + len(ps)] = ps
            bad = [s for s in ps if s in (5, 9)]
            status[j] = r["verdict"] if r["verdict"] else bad[0] if bad else int(1 in sts + ps)
            if status[j] in (0, 1):
                rec = np.frombuffer(r["rec"], np.uint8)
                files[j], meta[j, :16], meta[j, 16] = rec[16:80], rec[:16], rec[80]
        counts = InodeCounts(*[int((status == s).sum()) for s in (0, 1, 5, 9, 255)], 0, 0, 0)
        return dict(files=files, meta=meta, status=status, pieces=pieces, counts=counts, fixed=fixed)

    def sharers(self, reads, fixed):
        return np.array([any(b in fixed for b, _ in ([r["bit"]] if r["bit"] else []) + r["pieces"]) for r in reads])

    # ---- the engine ----
    def run(self, form, image, numbers, check=1, write_back=True, table_block=None, nblocks=None, src=None, stride=None,
            null=(), stream=None, eng=None, guarded=None):
        eng, n, W = eng or self.eng, len(numbers), 1 + self.K
        table = self.table(check, table_block)
        nblocks = self.blocks if nblocks is None else nblocks
        img = np.ascontiguousarray(image[:nblocks * self.raw])
        if form == "host":
            img = img.copy()
            o = dict(files=np.full(64 * n + 8, 0x5A, np.uint8), meta=np.full(24 * n + 8, 0x5A, np.uint8),
                     status=np.full(n + 8, 0x5A, np.uint8), piece_status=np.full(n * W + 8, 0x5A, np.uint8))
            kw = {k: (None if k in null else v[:v.size - 8]) for k, v in o.items()}
            nums = np.ascontiguousarray(numbers, np.uint32) if src is None else src
            counts = eng.read_inodes_host(img, table, nums, n=n if src is not None else None, stride=stride,
                                          write_back=write_back, **kw)
            for k, v in o.items():
                assert (v[v.size - 8:] == 0x5A).all(), k
            got = {k: (None if k in null else v[:v.size - 8]) for k, v in o.items()}
            got.update(counts=counts, image=img)
        else:
            at = dict(files=(4, 64 * n), meta=(8, 24 * n), status=(5, n), piece_status=(3, n * W))
            with torch.cuda.stream(stream):  # the buffers are filled on the stream the call runs on (None: the current one)
                g = guarded or Guarded(img)
                o = {k: torch.full((a + b + 37,), 0x5A, dtype=torch.uint8, device="cuda") for k, (a, b) in at.items()}
                cn = torch.full((10,), -7, dtype=torch.int64, device="cuda")
                kw = {k: (None if k in null else o[k][a:a + b]) for k, (a, b) in at.items()}
                nums = dev(np.ascontiguousarray(numbers, np.uint32).view(np.int32)) if src is None else src
                eng.read_inodes(g.image, table, nums, n=n if src is not None else None, stride=stride,
                                counts=None if "counts" in null else cn[1:9], write_back=write_back, stream=stream, **kw)
            if stream is not None:
                return lambda: self._finish(g, o, at, cn, null)
            got = self._finish(g, o, at, cn, null)
        for k, shape in (("files", (n, 64)), ("meta", (n, 24)), ("piece_status", (n, W))):
            if got[k] is not None:
                got[k] = got[k].reshape(shape)
        return got

    @staticmethod
    def _finish(g, o, at, cn, null):
        got = {}
        for k, (a, b) in at.items():
            h = host(o[k])
            assert (h[:a] == 0x5A).all() and (h[a + b:] == 0x5A).all(), f"{k} written outside its array"
            assert k not in null or (h == 0x5A).all()
            got[k] = None if k in null else h[a:a + b]
        c = host(cn)
        assert c[0] == -7 and c[9] == -7, "counts written outside the record"
        got["counts"] = None if "counts" in null else InodeCounts(*c[1:9].tolist())
        got["image"] = g.result()
        n = at["status"][1]
        for k, shape in (("files", (n, 64)), ("meta", (n, 24)), ("piece_status", (n, -1))):
            if got[k] is not None:
                got[k] = got[k].reshape(shape)
        return got


def same(got, e, tag=None, only=None):
    for k, ek in (("files", "files"), ("meta", "meta"), ("status", "status"), ("piece_status", "pieces"), ("counts", "counts")):
        if got[k] is None or (only and k not in only):
            continue
        assert np.array_equal(got[k], e[ek]) if k != "counts" else got[k] == e[ek], (k, tag)


@pytest.fixture(scope="module")
def images(oracle):
    cache = {}

    def get(name, **kw):
        key = (name, tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items())))
        if key not in cache:
            cache[key] = InodeImage(oracle, name, **kw)
        return cache[key]
    return get


# ------------------------------------------------------------------------------------
# the closed form, the base batch on every codec, both forms, with and without the bitmap
# ------------------------------------------------------------------------------------
def test_inode_span_against_the_closed_form(images):
    for name in NAMES:
        im = images(name)
        ds, table = im.ds, im.table()
        for i in range(im.total):
            assert im.eng.inode_span(table, i) == (im.table_block + 81 * i // ds, 81 * i % ds, (81 * i % ds + 80) // ds + 1)
        assert im.eng.inode_max_pieces == im.K
        with pytest.raises(EccError):
            im.eng.inode_span(table, im.total)
    assert images("parity32").K == 4 and images("rs255_t3").K == 2
    assert {images("parity32").eng.inode_span(images("parity32").table(), i)[2] for i in range(200)} == {3, 4}


@pytest.mark.parametrize("check", [1, 0])
@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("name", NAMES)
def test_read_inodes(images, name, form, check):
    im = images(name)
    nums = im.batch()
    reads, disk, _ = im.loop(im.clean, nums, check)
    e = im.expect(reads, "first")
    assert e["counts"].ok > 0 and e["counts"].out_of_range == 3 and (e["counts"].not_allocated > 0) == bool(check)
    got = im.run(form, im.clean, nums, check)
    same(got, e, (name, form, check))
    assert np.array_equal(got["image"], im.clean) and np.array_equal(disk, im.clean)


def test_rs255_staged_list_path_gives_the_same(images, monkeypatch):
    im = images("rs255_t3")
    nums = im.batch()
    e = im.expect(im.loop(im.clean, nums)[0], "first")
    monkeypatch.setenv("PPFS_ECC_LIST_DIRECT", "0")
    staged = make_engine(im.cfg)
    monkeypatch.delenv("PPFS_ECC_LIST_DIRECT")
    assert staged.list_kernel_name() != im.eng.list_kernel_name()
    same(im.run("device", im.clean, nums, eng=staged), e)


@pytest.mark.parametrize("form", ["device", "host"])
def test_every_output_null_in_turn(images, form):
    im = images("rs255_t3")
    nums = im.batch()
    e = im.expect(im.loop(im.clean, nums)[0], "first")
    for null in ("files", "meta", "status", "piece_status", "counts"):
        same(im.run(form, im.clean, nums, null=(null,)), e, null)
    got = im.run(form, im.clean, nums, null=("files", "meta", "status", "piece_status", "counts"))
    assert np.array_equal(got["image"], im.clean)


@pytest.mark.parametrize("form", ["device", "host"])
def test_strided_source_at_an_odd_address(images, form):
    """The numbers as the first four bytes of 128-byte DirectoryEntry records that start at an odd address, and at
    stride 4 from an odd address: the same results as from the packed array."""
    im = images("parity32")
    nums = im.batch()
    e = im.expect(im.loop(im.clean, nums)[0], "first")
    for stride in (128, 4, 7):
        buf = rng_for("stride", stride).integers(0, 256, 3 + stride * len(nums) + 9, dtype=np.uint8)
        for j, v in enumerate(nums):
            buf[3 + stride * j:3 + stride * j + 4] = np.frombuffer(np.uint32(v).tobytes(), np.uint8)
        buf = buf[:3 + stride * (len(nums) - 1) + 4]  # ends with the last number
        src = dev(buf)[3:] if form == "device" else buf[3:]
        same(im.run(form, im.clean, nums, src=src, stride=stride), e, stride)


# ------------------------------------------------------------------------------------
# damage
# ------------------------------------------------------------------------------------
def damaged(im, region, kind):
    """(image, the damaged block, numbers): one error the code corrects (kind "fix") or one beyond it ("fail") in a
    bitmap block or in a table block that three allocated inodes of the batch share (a shortened code: the table's
    last block, so that the reference's write-back runs into spare blocks only)."""
    typ = im.cfg[1]
    rng = rng_for("damage", im.cfg[0], region, kind)
    if region == "bitmap":
        block, extra = im.bitmap_block + im.bm_blocks - 1, []
    elif im.raw < 255 and typ == 4:
        block = im.table_block + im.t_blocks - 1
        extra = [i for i in range(im.total) if block in im.blocks_of(i)]
    else:
        block = im.table_block + 5
        extra = [i for i in range(im.total) if block in im.blocks_of(i)][:3]
    image = im.clean.copy()
    flip(rng, im.cfg, im.rows(image)[block], 1 if kind == "fix" or typ != 2 else 2)
    return image, block, im.batch(extra=extra)


def sharing_image(images, name):
    """ds = 249: inodes 15 .. 18 have bytes in table block + 5, and the last inodes in the last block; all allocated."""
    im = images(name)
    keep = sorted({i for b in (im.table_block + 5, im.table_block + im.t_blocks - 1) for i in range(im.total) if b in im.blocks_of(i)})
    return images(name, allocated=keep)


@pytest.mark.parametrize("region", ["bitmap", "table"])
@pytest.mark.parametrize("name", FIXES + ["rs255_staged"])
def test_one_corrected_block(images, monkeypatch, name, region):
    eng = None
    if name == "rs255_staged":
        name = "rs255_t3"
        monkeypatch.setenv("PPFS_ECC_LIST_DIRECT", "0")
        eng = make_engine(CFG[name])
        monkeypatch.delenv("PPFS_ECC_LIST_DIRECT")
    im = sharing_image(images, name)
    image, block, nums = damaged(im, region, "fix")
    reads, disk, log = im.loop(image, nums)
    first, every = im.expect(reads, "first"), im.expect(reads, "all")
    assert first["fixed"] == {block} and log == [block]
    share = im.sharers(reads, first["fixed"])
    need = 3 if im.ds >= 162 or region == "bitmap" else 2  # ds 58: a block has bytes of at most two inodes
    assert share.sum() >= need and first["counts"].corrected == 1 and every["counts"].corrected >= need
    if im.raw == 255 or im.cfg[1] != 4:
        assert np.array_equal(disk, im.clean)  # the loop ends with the block corrected (a shortened code also spills)
    tag = (name, region)
    # the host form is the loop
    got = im.run("host", image, nums, eng=eng)
    same(got, first, tag)
    assert np.array_equal(got["image"], im.clean)
    got = im.run("host", image, nums, write_back=False, eng=eng)
    same(got, every, tag)
    assert np.array_equal(got["image"], image)
    # the device form without write-back: every sharer reports 1
    got = im.run("device", image, nums, write_back=False, eng=eng)
    same(got, every, tag)
    assert np.array_equal(got["image"], image)
    # ... with it: exact outside the sharers, among them 0 or 1 and at least one 1; the image ends corrected
    got = im.run("device", image, nums, eng=eng)
    same(got, first, tag, only=("files", "meta"))
    assert np.array_equal(got["status"][~share], first["status"][~share])
    assert np.array_equal(got["piece_status"][~share], first["pieces"][~share])
    read = share & (first["status"] <= 1)  # a sharer of the bitmap block may be free: its status is the loop's
    assert np.array_equal(got["status"][share & ~read], first["status"][share & ~read])
    assert set(got["status"][read].tolist()) <= {0, 1}
    lo, hi = first["pieces"][share], every["pieces"][share]
    assert ((got["piece_status"][share] == lo) | (got["piece_status"][share] == hi)).all()
    assert (got["piece_status"][share] == 1).any()  # at least one sharer saw the block before its correction landed
    if region == "table":
        assert (got["status"][read] == 1).any()
    assert got["counts"].ok + got["counts"].corrected == first["counts"].ok + first["counts"].corrected
    assert got["counts"][2:] == first["counts"][2:] and (got["counts"].corrected >= 1 or region == "bitmap")
    assert np.array_equal(got["image"], im.clean)


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("region", ["bitmap", "table"])
@pytest.mark.parametrize("name", FAILS)
def test_one_failed_block(images, name, region, form):
    im = sharing_image(images, name)
    image, block, nums = damaged(im, region, "fail")
    reads, disk, log = im.loop(image, nums)
    e = im.expect(reads, "first")
    assert e["counts"].failed >= (3 if region == "table" else 10) and log == [] and np.array_equal(disk, image)
    failed = e["status"] == 5
    assert not e["files"][failed].any() and not e["meta"][failed].any()
    got = im.run(form, image, nums)
    same(got, e, (name, region, form))
    assert np.array_equal(got["image"], image)


@pytest.mark.parametrize("form", ["device", "host"])
def test_block_only_free_inodes_touch_stays_damaged(images, form):
    im = images("rs255_t3")
    block = im.table_block + 9
    inodes = [i for i in range(im.total) if block in im.blocks_of(i)]
    im = images("rs255_t3", freed=inodes, allocated=[199])
    image = im.clean.copy()
    im.rows(image)[block, 17] ^= 0x41
    nums = np.array(inodes + [im.total - 1], np.uint32)
    reads, disk, log = im.loop(image, nums)
    e = im.expect(reads, "first")
    assert e["counts"].not_allocated == len(inodes) >= 3 and e["counts"].ok == 1 and log == [] and np.array_equal(disk, image)
    got = im.run(form, image, nums, write_back=True)
    same(got, e)
    assert np.array_equal(got["image"], image)
    got = im.run(form, image, nums, check=0)  # without the bitmap the block is read, and corrected
    same(got, im.expect(im.loop(image, nums, check=0)[0], "first" if form == "host" else "all"), only=("files", "meta"))
    assert np.array_equal(got["image"], im.clean)


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("name", ["rs255_t3", "parity32"])
def test_pieces_past_the_image(images, name, form):
    """An image that ends inside the table: the pieces past it read as 9, nothing outside the image is touched."""
    im = images(name, allocated=range(150, 200))
    nblocks = im.table_block + im.t_blocks - 3
    cut = [i for i in range(im.total) if im.blocks_of(i)[-1] >= nblocks]
    nums = np.array(cut + [0, 1, 2, cut[0] - 1], np.uint32)
    reads, _, _ = im.loop(im.clean, nums, nblocks=nblocks)
    e = im.expect(reads, "first")
    assert e["counts"].out_of_range == len(cut) and e["counts"].ok >= 1
    assert any(p[0][1] == 0 and p[-1][1] == 9 for p in (r["pieces"] for r in reads) if p)  # one that straddles the end
    got = im.run(form, im.clean, nums, nblocks=nblocks)
    same(got, e, (name, form))
    assert np.array_equal(got["image"], im.clean[:nblocks * im.raw])
    # a table block that puts every piece past the image
    got = im.run(form, im.clean, nums, table_block=im.blocks + 40)
    assert (got["status"][im.expect(reads, "first")["status"] != 255] == 9).all() and not got["files"].any()


# ------------------------------------------------------------------------------------
# pieces, refusals, streams
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["device", "host"])
def test_batch_crosses_the_piece_size(oracle, form):
    n = PIECE + 5
    im = InodeImage(oracle, "rs255_t3", total=n + 3, free=0.1)
    assert im.t_blocks > 5000
    image = im.clean.copy()
    fixed = im.table_block + 81 * (2 + PIECE) // im.ds  # the block in which the second piece's first inode begins
    im.rows(image)[fixed, 100] ^= 0x10
    nums = np.arange(2, 2 + n, dtype=np.uint32)
    reads, disk, _ = im.loop(image, nums)
    e = im.expect(reads, "first")
    assert np.array_equal(disk, im.clean) and e["counts"].corrected == 1
    got = im.run(form, image, nums)
    same(got, e, only=("files", "meta"))
    share = im.sharers(reads, e["fixed"])
    assert np.array_equal(got["status"][~share], e["status"][~share]) and (got["status"][share] == 1).any()
    assert np.array_equal(got["image"], im.clean)
    if form == "host":
        same(got, e)


def test_rejected_calls_touch_nothing(images):
    im = images("rs255_t3")
    nums = im.batch()
    eng, table, n = im.eng, im.table(), len(nums)
    g = Guarded(im.clean)
    d_nums = dev(nums.view(np.int32))
    out = torch.full((64 * n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    L, h = _native.lib(), eng._h
    img, blocks, st = g.image.data_ptr(), im.blocks, torch.cuda.current_stream().cuda_stream
    p = out.data_ptr()
    bad = [
        (None, img, blocks, table.ctypes.data, d_nums.data_ptr(), 4, n, p, None, None, None, None),      # null context
        (h, img, blocks, None, d_nums.data_ptr(), 4, n, p, None, None, None, None),                       # null table
        (h, None, blocks, table.ctypes.data, d_nums.data_ptr(), 4, n, p, None, None, None, None),         # null image
        (h, img, blocks, table.ctypes.data, None, 4, n, p, None, None, None, None),                       # null numbers
        (h, img, blocks, table.ctypes.data, d_nums.data_ptr(), 3, n, p, None, None, None, None),          # stride below 4
        (h, img, blocks, table.ctypes.data, d_nums.data_ptr(), 4, n, p + 2, None, None, None, None),      # misaligned files
        (h, img, blocks, table.ctypes.data, d_nums.data_ptr(), 4, n, None, p + 4, None, None, None),      # misaligned meta
        (h, img, blocks, table.ctypes.data, d_nums.data_ptr(), 4, n, None, None, None, None, p + 4),      # misaligned counts
    ]
    for args in bad:
        assert L.ppfs_ecc_read_inodes_device(*args, 1, st) == -22, args
        assert L.ppfs_ecc_read_inodes_host(*args, 1) == -22, args
    assert (host(out) == 0x5A).all() and np.array_equal(g.result(), im.clean)
    with pytest.raises(ValueError):
        eng.read_inodes(g.image, table, d_nums, stride=2)
    with pytest.raises(ValueError):
        eng.read_inodes(g.image, table, d_nums, status=out[:n - 1])
    # nothing to read: zeroed counts
    cn = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    eng.read_inodes(g.image, table, d_nums[:0], counts=cn)
    assert host(cn).tolist() == [0] * 8
    assert eng.read_inodes_host(im.clean.copy(), table, nums[:0]) == InodeCounts(*[0] * 8)


def test_inode_call_refuses_a_capturing_stream(images):
    im = images("rs255_t3")
    nums, table = dev(im.batch().view(np.int32)), im.table()
    image = torch.from_numpy(im.clean).cuda()
    st = torch.zeros(64, dtype=torch.uint8, device="cuda")
    im.eng.read_inodes(image, table, nums, status=st)  # whatever the call sets up exists before the capture
    torch.cuda.synchronize()
    codes = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # captured and never replayed
        try:
            im.eng.read_inodes(image, table, nums, status=st)
            codes.append(0)
        except EccError as e:
            codes.append(e.code)
    assert codes == [-95]  # PPFS_ECC_ENOTSUP


def test_back_to_back_and_on_two_streams(images):
    im = sharing_image(images, "rs255_t3")
    image, block, nums = damaged(im, "table", "fix")
    other = nums[::-1].copy()
    clean_a, clean_b = (im.expect(im.loop(im.clean, x)[0], "first") for x in (nums, other))
    first = im.expect(im.loop(image, nums)[0], "first")
    # one stream: the first call corrects the block, the second reads it clean
    s, g = torch.cuda.Stream(), Guarded(image)
    torch.cuda.synchronize()  # the image was copied on the default stream
    a = im.run("device", image, nums, stream=s, guarded=g)
    b = im.run("device", image, other, stream=s, guarded=g)
    torch.cuda.synchronize()
    a, b = a(), b()
    same(a, first, only=("files", "meta"))
    assert a["counts"].corrected >= 1
    same(b, clean_b, "second call")
    assert np.array_equal(b["image"], im.clean)
    # two streams, one context, an image each
    runs = [im.run("device", im.clean, x, stream=torch.cuda.Stream()) for x in (nums, other)]
    torch.cuda.synchronize()
    same(runs[0](), clean_a, "stream 0")
    same(runs[1](), clean_b, "stream 1")


# ------------------------------------------------------------------------------------
# a directory level end to end: read_file, read_inodes at stride 128, read_files
# ------------------------------------------------------------------------------------
def test_directory_level_end_to_end(oracle):
    """A directory of 40 entries in an image that also holds its children's files, the inode bitmap and the inode
    table: the directory's payload stays in device memory, the children's inode numbers are read out of it at stride
    128, the 64-byte records go to the host and into read_files.  The bytes of all 40 files against the oracle's walk
    of each file."""
    rng = rng_for("directory")
    sizes = [21] + [int(x) for x in rng.choice([1, 2, 3, 5, 13, 14, 30], 40)]  # the directory: 40 * 128 = 5,120 bytes
    fi = FilesImage(oracle, "rs512_t3", sizes, damage_data=False, one_index_error=True)
    ds, raw, cfg = fi.ds, fi.raw, fi.cfg
    assert (raw, ds) == (255, 249) and -(-5120 // ds) == 21
    fi.files["file_size"][0] = 5120
    total = 200
    inos = rng.permutation(total)[:41].astype(np.uint32)  # the directory's own inode, then its children's
    entries = rng.integers(1, 256, (40, 128), dtype=np.uint8)
    entries[:, :4] = inos[1:].astype("<u4").view(np.uint8).reshape(40, 4)
    rows = fi.image.reshape(fi.blocks, raw)
    dir_payload = rng.integers(0, 256, (21, ds), dtype=np.uint8)
    dir_payload.reshape(-1)[:5120] = entries.reshape(-1)
    rows[fi.data_blk[0]] = oracle_encode(oracle, cfg, dir_payload)
    # the bitmap and the table behind the files' blocks
    bm_block, tb_block = fi.blocks + 1, fi.blocks + 3
    t_blocks = -(-81 * total // ds)
    extra = rng.integers(0, 256, (tb_block + t_blocks + 2 - fi.blocks, ds), dtype=np.uint8)
    bits = np.ones(ds * 8, np.uint8)
    bits[inos] = 0
    extra[bm_block - fi.blocks] = np.packbits(bits)
    records = rng.integers(0, 256, (total, 81), dtype=np.uint8)
    records[inos, 16:80] = fi.files.view(np.uint8).reshape(41, 64)
    extra[tb_block - fi.blocks:tb_block - fi.blocks + t_blocks].reshape(-1)[:81 * total] = records.reshape(-1)
    extra_rows = oracle_encode(oracle, cfg, extra)
    extra_rows[tb_block - fi.blocks + 4, 33] ^= 0x77  # one table block to correct on the way
    image = np.concatenate([rows.reshape(-1), extra_rows.reshape(-1)])
    fi.image, fi.blocks = image, image.size // raw
    expected = [fi.per_file(f, 0, int(fi.files["file_size"][f]), True)["out"] for f in range(1, 41)]
    assert all(e.size == int(fi.files["file_size"][f + 1]) for f, e in enumerate(expected))

    eng = fi.eng
    table = np.zeros(1, INODE_TABLE_DTYPE)
    table["table_block"], table["bitmap_block"], table["total_inodes"], table["check_bitmap"] = tb_block, bm_block, total, 1
    g = Guarded(image)
    # the directory's own record, as a directory level starts: out of the table, one inode
    root = np.zeros(1, FILE_DTYPE)
    eng.read_inodes_host(g.result(), table, inos[:1], files=root)
    assert root.tobytes() == fi.files[:1].tobytes()
    d_out = torch.zeros(5120 + 5, dtype=torch.uint8, device="cuda")[5:]
    d_files = torch.zeros(40 * 64, dtype=torch.uint8, device="cuda")
    d_status = torch.full((40,), 77, dtype=torch.uint8, device="cuda")
    eng.read_file(g.image, root, 0, 5120, d_out)
    eng.read_inodes(g.image, table, d_out, n=40, stride=128, files=d_files, status=d_status)
    files = host(d_files).view(FILE_DTYPE)  # 64 bytes per child to the host
    assert set(host(d_status).tolist()) <= {0, 1} and files.tobytes() == fi.files[1:].tobytes()
    nbytes = int(files["file_size"].sum())
    out = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    eng.read_files(g.image, files, None, out)
    assert np.array_equal(host(out), np.concatenate(expected))


# ------------------------------------------------------------------------------------
# the block-device mirror: the engine override against the per-inode loop, which is the definition
# ------------------------------------------------------------------------------------
class PlainDisk(IDisk):
    """A disk the engine cannot map: the device keeps the per-inode loop."""

    def __init__(self, image):
        self._d = HeapDisk(image.size)
        self._d.buf[:] = image

    def read(self, address, size):
        return self._d.read(address, size)

    def write(self, address, data):
        return self._d.write(address, data)

    def size(self):
        return self._d.size()

    @property
    def contents(self):
        return self._d.buf


def mirror(im, image, mapped=True):
    _, typ, bs, t, poly, _ = im.cfg
    logger = Logger()
    if mapped:
        disk = HeapDisk(image.size)
        disk.buf[:] = image
    else:
        disk = PlainDisk(image)
    d = create_block_device(disk, bs, ECCType(typ), crc_polynomial_explicit=poly, rs_correctable_bytes=t, logger=logger)
    return d, (disk.buf if mapped else disk.contents), logger


MIRROR = [("rs255_t3", "fix"), ("hamming512", "fix"), ("hamming512", "fail"), ("crc512", "fail"), ("parity32", "fail"),
          ("rs64_t3", "clean")]


@pytest.mark.parametrize("mapped", [True, False], ids=["mapped", "unmapped"])
@pytest.mark.parametrize("name,kind", MIRROR, ids=[f"{a}-{b}" for a, b in MIRROR])
def test_block_device_read_inodes_matches_the_loop(images, name, kind, mapped):
    im = sharing_image(images, name)
    image, nums = im.clean.copy(), im.batch()
    if kind != "clean":  # a shared table block damaged, and with it a bitmap block where the code corrects
        image, _, nums = damaged(im, "table", kind)
        if kind == "fix":
            b, bb, _ = damaged(im, "bitmap", "fix")
            im.rows(image)[bb] = im.rows(b)[bb]
    for check in (1, 0):
        d, disk, logger = mirror(im, image, mapped)
        ref, ref_disk, ref_logger = mirror(im, image, True)
        got = d.read_inodes(im.table(check), nums)
        want = IBlockDevice.read_inodes(ref, im.table(check), nums)  # the per-inode loop
        assert len(got) == len(want) == len(nums)
        errors = set()
        for j, ((g_rec, g_err), (w_rec, w_err)) in enumerate(zip(got, want)):
            assert g_err == w_err and (g_rec is None) == (w_rec is None), (name, kind, check, j)
            if w_rec is not None:
                assert g_rec.dtype == INODE_DTYPE and g_rec.tobytes() == w_rec.tobytes(), (name, kind, check, j)
            errors.add(w_err)
        assert FsError.Bitmap_IndexOutOfRange in errors and None in errors
        assert (FsError.InodeManager_NotFound in errors) == bool(check)
        if kind == "fail":
            assert FsError.BlockDevice_CorrectionError in errors
        if kind == "fix":
            assert len(ref_logger.corrections) == (2 if check else 1)
        assert logger.corrections == ref_logger.corrections, (name, kind, check)
        assert np.array_equal(disk, ref_disk), (name, kind, check)
    # the loop itself against the oracle's device model
    reads, o_disk, o_log = im.loop(image, nums)
    e = im.expect(reads, "first")
    for j, (rec, err) in enumerate(IBlockDevice.read_inodes(mirror(im, image)[0], im.table(1), nums)):
        st = int(e["status"][j])
        if st in (0, 1):
            assert err is None and rec.tobytes() == reads[j]["rec"]
        else:
            assert rec is None and err == (FsError.Bitmap_IndexOutOfRange if int(nums[j]) >= im.total else
                                           FsError.InodeManager_NotFound if st == 255 else FsError(st))
