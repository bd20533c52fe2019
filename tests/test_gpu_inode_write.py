"""GPU tests of the inode writes (include/ppfs_ecc.h ppfs_ecc_write_inodes_*; EccEngine.write_inodes /
write_inodes_host; IBlockDevice.write_inodes) against the CPU oracle.

Expected values come only from the per-inode loop -- InodeManager::update: Bitmap::getBit, then _writeInode, one
writeBlock per piece -- over the oracle's device model (tests/oracle_lib.py OracleDevice.read / .write), in the calls'
batch form: every piece of an inode whose bit allows the write is attempted, the first failing one gives the status.
The loop tells which access corrected a block, and that is the first toucher rule: the table statuses are exact in both
forms.  Only the bitmap byte's read on the device with write-back keeps the reads' latitude (each sharer of a corrected
bitmap block 0 or 1, at least one 1).  Every case compares the whole raw image, status, piece_status and counts.

Images are those of tests/test_gpu_inodes.py: about 200 inodes, batches of about 64."""
import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch

from paritypartyfs_amd import _native
from paritypartyfs_amd._native import EXTENT_DTYPE, INODE_META_DTYPE, EccError
from paritypartyfs_amd.block_device import FsError, IBlockDevice
from paritypartyfs_amd.ecc import InodeCounts
from tests.oracle_lib import OracleDevice
from tests.test_gpu_file import make_engine, rng_for
from tests.test_gpu_inodes import CFG, FAILS, NAMES, PIECE, InodeImage, damaged, mirror, sharing_image
from tests.test_gpu_list import Guarded, dev, host

CFG.setdefault("crc100_deg3", ("crc100_deg3", 1, 100, 0, 0xB, 0))  # a CRC whose last byte is partly undefined


def records(n, *tag):
    """n random 81-byte inodes."""
    return rng_for("records", n, tag).integers(0, 256, (n, 81), dtype=np.uint8)


def split(recs):
    """The calls' inputs: the 64-byte file records and the metadata, its padding filled with noise."""
    n = len(recs)
    meta = np.zeros(n, INODE_META_DTYPE)
    meta["time_creation"] = np.ascontiguousarray(recs[:, 0:8]).view("<u8").reshape(n)
    meta["time_modified"] = np.ascontiguousarray(recs[:, 8:16]).view("<u8").reshape(n)
    meta["type"], meta["pad"] = recs[:, 80], 0xEE
    return np.ascontiguousarray(recs[:, 16:80]).reshape(-1), meta.view(np.uint8).reshape(-1)


# ---- the per-inode loop over the oracle's device model ----
def loop(im, image, numbers, recs, check=1, table_block=None, nblocks=None):
    """Per inode what getBit and the writeBlocks gave; the disk afterwards; the correction log."""
    _, typ, bs, t, poly, _ = im.cfg
    nblocks = im.blocks if nblocks is None else nblocks
    od = OracleDevice(im.oracle, typ, bs, t, poly, nblocks * im.raw)
    od.disk[:] = image[:nblocks * im.raw]
    L, ds, raw = im.oracle.L, im.ds, im.raw
    tb = im.table_block if table_block is None else table_block
    confine = typ == 4 and raw < 255  # the engine keeps a shortened code's codeword inside its block

    def call(block, fn):
        before = od.disk.copy() if confine and block < nblocks else None
        n0 = L.oracle_dev_log_len(od.h)
        rc, val = fn()
        if before is not None:
            lo, hi = block * raw, (block + 1) * raw
            od.disk[:lo], od.disk[hi:] = before[:lo], before[hi:]
        return (rc if rc else int(L.oracle_dev_log_len(od.h) > n0)), val

    out = []
    for j, i in enumerate(int(x) for x in numbers):
        r = dict(ino=i, bit=None, pieces=[], verdict=0)
        if i >= im.total:
            r["verdict"] = 9
        elif check:
            byte = i // 8
            b = im.bitmap_block + byte // ds
            st, data = call(b, lambda: od.read(b, byte % ds, 1))
            r["bit"] = (b, st)
            if st in (5, 9):
                r["verdict"] = st
            elif data[0] & (0x80 >> (i % 8)):
                r["verdict"] = 255
        if r["verdict"] == 0:
            block, off, pos = tb + 81 * i // ds, 81 * i % ds, 0
            while pos < 81:
                n = min(81 - pos, ds - off)
                st, wrote = call(block, lambda: od.write(block, off, recs[j, pos:pos + n].tobytes()))
                assert (st == 9) == (block >= nblocks) and (st in (5, 9) or wrote == n)
                r["pieces"].append((block, st))
                block, off, pos = block + 1, 0, pos + n
        out.append(r)
    return out, od.disk.copy(), od.log_entries()


def expect(im, reads):
    n, W = len(reads), 1 + im.K
    status, pieces = np.zeros(n, np.uint8), np.full((n, W), 255, np.uint8)
    for j, r in enumerate(reads):
        sts = [r["bit"][1]] if r["bit"] else []
        if r["bit"]:
            pieces[j, 0] = sts[0]
        ps = [st for _, st in r["pieces"]]
        pieces[j, 1:1 + len(ps)] = ps
        bad = [s for s in ps if s in (5, 9)]
        status[j] = r["verdict"] if r["verdict"] else bad[0] if bad else int(1 in sts + ps)
    counts = InodeCounts(*[int((status == s).sum()) for s in (0, 1, 5, 9, 255)], 0, 0, 0)
    return dict(status=status, pieces=pieces, counts=counts)


# ---- the engine ----
def run(im, form, image, numbers, recs, check=1, write_back=True, table_block=None, nblocks=None, src=None, stride=None, null=(),
        stream=None, eng=None, guarded=None):
    eng, n, W = eng or im.eng, len(numbers), 1 + im.K
    table = im.table(check, table_block)
    nblocks = im.blocks if nblocks is None else nblocks
    img = np.ascontiguousarray(image[:nblocks * im.raw])
    files, meta = split(recs)
    if form == "host":
        img = img.copy()
        o = dict(status=np.full(n + 8, 0x5A, np.uint8), piece_status=np.full(n * W + 8, 0x5A, np.uint8))
        kw = {k: (None if k in null else v[:v.size - 8]) for k, v in o.items()}
        nums = np.ascontiguousarray(numbers, np.uint32) if src is None else src
        f0, m0 = files.copy(), meta.copy()
        counts = eng.write_inodes_host(img, table, nums, files, meta, n=n if src is not None else None, stride=stride,
                                       write_back=write_back, **kw)
        assert np.array_equal(files, f0) and np.array_equal(meta, m0)
        for k, v in o.items():
            assert (v[v.size - 8:] == 0x5A).all(), k
        got = {k: (None if k in null else v[:v.size - 8]) for k, v in o.items()}
        got.update(counts=counts, image=img)
        if got["piece_status"] is not None:
            got["piece_status"] = got["piece_status"].reshape(n, W)
        return got
    at = dict(status=(5, n), piece_status=(3, n * W))
    with torch.cuda.stream(stream):  # the buffers are filled on the stream the call runs on (None: the current one)
        g = guarded or Guarded(img)
        o = {k: torch.full((a + b + 37,), 0x5A, dtype=torch.uint8, device="cuda") for k, (a, b) in at.items()}
        cn = torch.full((10,), -7, dtype=torch.int64, device="cuda")
        kw = {k: (None if k in null else o[k][a:a + b]) for k, (a, b) in at.items()}
        nums = dev(np.ascontiguousarray(numbers, np.uint32).view(np.int32)) if src is None else src
        # the inputs at their least alignment inside guard bytes: files 4, meta 8
        d_files = dev(np.concatenate([np.full(4, 0xC3, np.uint8), files, np.full(9, 0xC3, np.uint8)]))
        d_meta = dev(np.concatenate([np.full(8, 0xC3, np.uint8), meta, np.full(9, 0xC3, np.uint8)]))
        eng.write_inodes(g.image, table, nums, d_files[4:4 + files.size], d_meta[8:8 + meta.size], n=n if src is not None else None,
                         stride=stride, counts=None if "counts" in null else cn[1:9], write_back=write_back, stream=stream, **kw)

    def finish():
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
        assert np.array_equal(host(d_files)[4:4 + files.size], files) and np.array_equal(host(d_meta)[8:8 + meta.size], meta)
        if got["piece_status"] is not None:
            got["piece_status"] = got["piece_status"].reshape(n, W)
        return got
    return finish if stream is not None else finish()


def same(got, e, disk, tag=None):
    for k, ek in (("status", "status"), ("piece_status", "pieces"), ("counts", "counts")):
        if got[k] is None:
            continue
        assert np.array_equal(got[k], e[ek]) if k != "counts" else got[k] == e[ek], (k, tag)
    assert np.array_equal(got["image"], disk), ("image", tag)


def check_all(im, forms, image, nums, recs, tag=None, **kw):
    """Both forms against the loop, exactly; -> (reads, expectation, disk, log)."""
    run_kw = {k: kw.pop(k) for k in ("eng",) if k in kw}
    reads, disk, log = loop(im, image, nums, recs, **kw)
    e = expect(im, reads)
    for form in forms:
        same(run(im, form, image, nums, recs, **kw, **run_kw), e, disk, (tag, form))
    return reads, e, disk, log


@pytest.fixture(scope="module")
def images(oracle):
    cache = {}

    def get(name, **kw):
        key = (name, tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple, range)) else v) for k, v in kw.items())))
        if key not in cache:
            cache[key] = InodeImage(oracle, name, **kw)
        return cache[key]
    return get


def staged_engine(monkeypatch, im):
    monkeypatch.setenv("PPFS_ECC_LIST_DIRECT", "0")
    eng = make_engine(im.cfg)
    monkeypatch.delenv("PPFS_ECC_LIST_DIRECT")
    assert eng.list_kernel_name() != im.eng.list_kernel_name()
    return eng


# ------------------------------------------------------------------------------------
# the base batch on every codec, both forms, with and without the bitmap
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("check", [1, 0])
@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("name", NAMES)
def test_write_inodes(images, name, form, check):
    """Free inodes and numbers past the table are left alone, straddling inodes land in both blocks, three or four inodes
    of one block all land, the number that appears twice ends with its later record."""
    im = images(name)
    nums = im.batch()
    recs = records(len(nums), name)
    reads, e, disk, log = check_all(im, [form], im.clean, nums, recs, (name, check), check=check)
    assert e["counts"].ok > 0 and e["counts"].out_of_range == 3 and (e["counts"].not_allocated > 0) == bool(check)
    assert e["counts"].ok + e["counts"].out_of_range + e["counts"].not_allocated == len(nums) and log == []
    assert not np.array_equal(disk, im.clean)
    touched = [b for r in reads for b, _ in r["pieces"]]
    assert len(touched) > len(set(touched)) and len({len(r["pieces"]) for r in reads if r["pieces"]}) >= 2  # sharers, a straddler
    # read back through the engine: every inode that was written holds its LAST record of the batch
    last = {int(i): j for j, i in enumerate(nums) if e["status"][j] == 0}
    assert len(set(nums.tolist())) < len(nums)  # a number appears twice
    back = np.array(sorted(last), np.uint32)
    files, meta = np.zeros((len(back), 64), np.uint8), np.zeros((len(back), 24), np.uint8)
    im.eng.read_inodes_host(disk.copy(), im.table(0), back, files=files, meta=meta)
    for row, i in enumerate(back):
        rec = recs[last[int(i)]]
        assert files[row].tobytes() == rec[16:80].tobytes() and meta[row, :16].tobytes() == rec[:16].tobytes() and meta[row, 16] == rec[80]


def test_rs255_staged_list_path_gives_the_same(images, monkeypatch):
    im = images("rs255_t3")
    nums = im.batch()
    check_all(im, ["device"], im.clean, nums, records(len(nums), "staged"), eng=staged_engine(monkeypatch, im))


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("name", ["rs255_t3", "parity32"])
def test_sharers_of_one_block_and_a_whole_batch_aimed_at_it(images, name, form):
    im = sharing_image(images, name)
    block = im.table_block + 5
    inodes = [i for i in range(im.total) if block in im.blocks_of(i)]
    inside = [i for i in inodes if im.blocks_of(i) == [block]]
    assert len(inodes) >= (4 if name == "rs255_t3" else 2) and len(inodes) > len(inside)
    # every inode of the block, the straddlers among them, last to first, and one of them again
    nums = np.array(inodes[::-1] + [inodes[1]], np.uint32)
    check_all(im, [form], im.clean, nums, records(len(nums), name, "sharers"))
    # 64 entries, all at the same block: its inodes over and over
    rng = rng_for("one block", name)
    pool = inside or inodes
    nums = np.array(rng.choice(pool, 64), np.uint32)
    reads, e, disk, _ = check_all(im, [form], im.clean, nums, records(64, name, "one block"))
    assert e["counts"].ok == 64
    changed = np.flatnonzero((im.rows(disk) != im.rows(im.clean)).any(axis=1))
    assert set(changed) <= set(b for i in pool for b in im.blocks_of(i)) and block in changed


# ------------------------------------------------------------------------------------
# damage
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("name", ["rs255_t3", "rs255_staged", "hamming512"])
def test_one_corrected_table_block(images, monkeypatch, name, form):
    """The first toucher -- the lowest entry, its lowest piece -- reports 1, every later one 0; all their bytes land."""
    eng = None
    if name == "rs255_staged":
        name, eng = "rs255_t3", staged_engine(monkeypatch, images("rs255_t3"))
    im = sharing_image(images, name)
    image, block, nums = damaged(im, "table", "fix")
    recs = records(len(nums), name, "fix")
    kw = dict(eng=eng) if eng else {}
    reads, e, disk, log = check_all(im, [form], image, nums, recs, name, **kw)
    assert log == [block] and e["counts"].corrected == 1
    touchers = [(j, k) for j, r in enumerate(reads) for k, (b, _) in enumerate(r["pieces"]) if b == block]
    assert len(touchers) >= 3 and [reads[j]["pieces"][k][1] for j, k in touchers] == [1] + [0] * (len(touchers) - 1)
    # the block ends clean, with every toucher's bytes: the loop over the result reads all of them without a correction
    assert loop(im, disk, nums, recs)[2] == []


@pytest.mark.parametrize("name", ["rs255_t3", "hamming512"])
def test_one_corrected_bitmap_block(images, name):
    im = sharing_image(images, name)
    image, block, nums = damaged(im, "bitmap", "fix")
    recs = records(len(nums), name, "bitmap fix")
    reads, e, disk, log = check_all(im, ["host"], image, nums, recs, name)
    assert log == [block] and e["counts"].corrected == 1
    # without write-back the host form sees the correction at every read of the block, and leaves it damaged
    share = np.array([bool(r["bit"]) and r["bit"][0] == block for r in reads])
    got = run(im, "host", image, nums, recs, write_back=False)
    assert (got["piece_status"][share, 0] == 1).all() and np.array_equal(got["piece_status"][:, 1:], e["pieces"][:, 1:])
    assert np.array_equal(im.rows(got["image"])[block], im.rows(image)[block])
    # the device form with write-back: the reads' latitude for the bitmap byte, everything else exact
    got = run(im, "device", image, nums, recs)
    assert np.array_equal(got["image"], disk)
    assert np.array_equal(got["piece_status"][:, 1:], e["pieces"][:, 1:])
    assert np.array_equal(got["piece_status"][~share], e["pieces"][~share]) and np.array_equal(got["status"][~share], e["status"][~share])
    assert set(got["piece_status"][share, 0].tolist()) <= {0, 1} and (got["piece_status"][share, 0] == 1).any()
    written = share & (e["status"] <= 1)
    assert set(got["status"][written].tolist()) <= {0, 1}
    assert np.array_equal(got["status"][share & ~written], e["status"][share & ~written])
    assert got["counts"].ok + got["counts"].corrected == e["counts"].ok + e["counts"].corrected and got["counts"][2:] == e["counts"][2:]


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("region", ["bitmap", "table"])
@pytest.mark.parametrize("name", FAILS)
def test_one_failed_block(images, name, region, form):
    """A table block whose old contents fail stays byte-identical and its touchers report 5; the inodes whose bitmap
    byte cannot be read are not written at all."""
    im = sharing_image(images, name)
    image, block, nums = damaged(im, region, "fail")
    recs = records(len(nums), name, region)
    reads, e, disk, log = check_all(im, [form], image, nums, recs, (name, region))
    assert e["counts"].failed >= (3 if region == "table" else 10) and log == []
    assert np.array_equal(im.rows(disk)[block], im.rows(image)[block])
    if region == "table":
        assert not np.array_equal(disk, image)
        for j, r in enumerate(reads):
            hit = [st for b, st in r["pieces"] if b == block]
            assert not hit or (hit == [5] and e["status"][j] == 5)
    else:
        assert all(not r["pieces"] for r in reads if r["bit"] and r["bit"][0] == block)


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("name", ["rs255_t3", "parity32"])
def test_table_blocks_past_the_image(images, name, form):
    im = images(name, allocated=range(150, 200))
    nblocks = im.table_block + im.t_blocks - 3
    cut = [i for i in range(im.total) if im.blocks_of(i)[-1] >= nblocks]
    nums = np.array(cut + [0, 1, 2, cut[0] - 1], np.uint32)
    recs = records(len(nums), name, "cut")
    reads, e, disk, _ = check_all(im, [form], im.clean, nums, recs, name, nblocks=nblocks)
    assert e["counts"].out_of_range == len(cut) and e["counts"].ok >= 1
    assert any(p[0][1] == 0 and p[-1][1] == 9 for p in (r["pieces"] for r in reads) if p)  # one that straddles the end
    # a table block that puts every piece past the image: nothing is written
    got = run(im, form, im.clean, nums, recs, table_block=im.blocks + 40)
    assert (got["status"][e["status"] != 255] == 9).all() and np.array_equal(got["image"], im.clean)


@pytest.mark.parametrize("name", ["hamming512", "crc100_deg3"])
def test_undefined_bits_are_kept(images, oracle, name):
    """Hamming-512's tail bits and the low bits of a degree-3 CRC's last byte keep whatever they held."""
    im = images(name)
    _, typ, bs, _, poly, _ = im.cfg
    rng = rng_for("tail", name)
    od = OracleDevice(oracle, typ, bs, 0, poly, im.clean.size)
    od.disk[:] = im.clean
    image = im.clean.copy()
    for b in range(im.table_block, im.table_block + im.t_blocks):  # the same payloads encoded onto random old contents
        rc, payload = od.read(b, 0, im.ds)
        assert rc == 0
        old = rng.integers(0, 256, im.raw, dtype=np.uint8)
        payload = np.frombuffer(payload, np.uint8)
        im.rows(image)[b] = oracle.ham_encode(bs, payload, raw_old=old) if typ == 2 else oracle.crc_encode(bs, poly, payload, raw_old=old)
    assert not np.array_equal(image, im.clean), "this configuration leaves no bit undefined"
    nums = im.batch()
    recs = records(len(nums), name, "tail")
    _, e, disk, _ = check_all(im, ["device", "host"], image, nums, recs, name)
    assert e["counts"].failed == 0 and e["counts"].corrected == 0
    assert not np.array_equal(disk, loop(im, im.clean, nums, recs)[1])  # the same bytes onto zeroed tails give another image


# ------------------------------------------------------------------------------------
# arguments
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["device", "host"])
def test_every_output_null_in_turn(images, form):
    im = images("rs255_t3")
    nums = im.batch()
    recs = records(len(nums), "null")
    reads, disk, _ = loop(im, im.clean, nums, recs)
    e = expect(im, reads)
    for null in (("status",), ("piece_status",), ("counts",), ("status", "piece_status", "counts")):
        same(run(im, form, im.clean, nums, recs, null=null), e, disk, null)


@pytest.mark.parametrize("form", ["device", "host"])
def test_strided_source_at_an_odd_address(images, form):
    im = images("parity32")
    nums = im.batch()
    recs = records(len(nums), "stride")
    reads, disk, _ = loop(im, im.clean, nums, recs)
    e = expect(im, reads)
    for stride in (128, 4, 7):
        buf = rng_for("stride", stride).integers(0, 256, 3 + stride * len(nums) + 9, dtype=np.uint8)
        for j, v in enumerate(nums):
            buf[3 + stride * j:3 + stride * j + 4] = np.frombuffer(np.uint32(v).tobytes(), np.uint8)
        buf = buf[:3 + stride * (len(nums) - 1) + 4]  # ends with the last number
        src = dev(buf)[3:] if form == "device" else buf[3:]
        same(run(im, form, im.clean, nums, recs, src=src, stride=stride), e, disk, stride)


def test_rejected_calls_touch_nothing(images):
    im = images("rs255_t3")
    nums = im.batch()
    eng, table, n = im.eng, im.table(), len(nums)
    g = Guarded(im.clean)
    d_nums = dev(nums.view(np.int32))
    buf = torch.full((64 * n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    L, h = _native.lib(), eng._h
    img, blocks, st = g.image.data_ptr(), im.blocks, torch.cuda.current_stream().cuda_stream
    p, t, d = buf.data_ptr(), table.ctypes.data, d_nums.data_ptr()
    bad = [
        (None, img, blocks, t, d, 4, n, p, p, None, None, None),      # null context
        (h, img, blocks, None, d, 4, n, p, p, None, None, None),      # null table
        (h, None, blocks, t, d, 4, n, p, p, None, None, None),        # null image
        (h, img, blocks, t, None, 4, n, p, p, None, None, None),      # null numbers
        (h, img, blocks, t, d, 3, n, p, p, None, None, None),         # stride below 4
        (h, img, blocks, t, d, 4, n, p + 2, p, None, None, None),     # misaligned files
        (h, img, blocks, t, d, 4, n, p, p + 4, None, None, None),     # misaligned meta
        (h, img, blocks, t, d, 4, n, p, p, None, None, p + 4),        # misaligned counts
        (h, img, blocks, t, d, 4, n, None, p, None, None, None),      # no file records
        (h, img, blocks, t, d, 4, n, p, None, None, None, None),      # no metadata
    ]
    for args in bad:
        assert L.ppfs_ecc_write_inodes_device(*args, 1, st) == -22, args
        assert L.ppfs_ecc_write_inodes_host(*args, 1) == -22, args
    assert (host(buf) == 0x5A).all() and np.array_equal(g.result(), im.clean)
    with pytest.raises(ValueError):
        eng.write_inodes(g.image, table, d_nums, buf, buf, stride=2)
    with pytest.raises(ValueError):
        eng.write_inodes(g.image, table, d_nums, buf[:64 * n - 1], buf)
    with pytest.raises(ValueError):
        eng.write_inodes(g.image, table, d_nums, None, buf)
    # nothing to write: zeroed counts, also without records
    cn = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    eng.write_inodes(g.image, table, d_nums[:0], buf, buf, counts=cn)
    assert host(cn).tolist() == [0] * 8
    assert L.ppfs_ecc_write_inodes_device(h, img, blocks, t, d, 4, 0, None, None, None, None, cn.data_ptr(), 1, st) == 0
    files, meta = split(records(1, "none"))
    assert eng.write_inodes_host(im.clean.copy(), table, nums[:0], files, meta) == InodeCounts(*[0] * 8)
    assert np.array_equal(g.result(), im.clean)


def test_inode_write_refuses_a_capturing_stream(images):
    im = images("rs255_t3")
    nums, table = dev(im.batch().view(np.int32)), im.table()
    image = torch.from_numpy(im.clean).cuda()
    files, meta = (dev(x) for x in split(records(64, "capture")))
    st = torch.zeros(64, dtype=torch.uint8, device="cuda")
    im.eng.write_inodes(image, table, nums, files, meta, status=st)  # whatever the call sets up exists before the capture
    torch.cuda.synchronize()
    before = host(image)
    codes = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # captured and never replayed
        try:
            im.eng.write_inodes(image, table, nums, files, meta, status=st)
            codes.append(0)
        except EccError as e:
            codes.append(e.code)
    assert codes == [-95]  # PPFS_ECC_ENOTSUP
    assert np.array_equal(host(image), before)


# ------------------------------------------------------------------------------------
# pieces and the election table at its limit
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["device", "host"])
def test_batch_crosses_the_piece_size(images, form):
    """More numbers than a piece holds over the 200-inode table: every inode many times, in both pieces; one block to
    correct, which the first piece's first toucher reports."""
    im = sharing_image(images, "rs255_t3")
    n = PIECE + 37
    nums = rng_for("pieces").integers(0, im.total + 4, n).astype(np.uint32)
    image = im.clean.copy()
    im.rows(image)[im.table_block + 5, 100] ^= 0x10
    recs = records(n, "pieces")
    reads, e, disk, log = check_all(im, [form], image, nums, recs)
    assert log == [im.table_block + 5] and e["counts"].corrected == 1 and e["counts"].ok > PIECE // 2
    assert {int(i) for i in nums[PIECE:]} & {int(i) for i in nums[:PIECE]}


def test_a_full_piece_of_distinct_inodes(oracle):
    """16,384 distinct inodes of a table of 16,500 in one batch: the election table at the load it is sized for."""
    im = InodeImage(oracle, "rs255_t3", total=16500, free=0.05)
    assert im.K == 2 and im.t_blocks > 5000
    nums = rng_for("full piece").permutation(im.total)[:PIECE].astype(np.uint32)
    recs = records(PIECE, "full piece")
    reads, e, disk, _ = check_all(im, ["device", "host"], im.clean, nums, recs)
    assert e["counts"].ok > 15000 and e["counts"].ok + e["counts"].not_allocated == PIECE
    assert len({b for r in reads for b, _ in r["pieces"]}) > 5000


# ------------------------------------------------------------------------------------
# streams, and the extent write around an inode write
# ------------------------------------------------------------------------------------
def test_write_then_read_on_one_stream_and_on_two(images):
    im = sharing_image(images, "rs255_t3")
    image, block, nums = damaged(im, "table", "fix")
    recs = records(len(nums), "streams")
    reads, disk, _ = loop(im, image, nums, recs)
    e = expect(im, reads)
    back = im.expect(im.loop(disk, nums)[0], "first")  # what read_inodes finds afterwards
    s, g = torch.cuda.Stream(), Guarded(image)
    torch.cuda.synchronize()  # the image was copied on the default stream
    a = run(im, "device", image, nums, recs, stream=s, guarded=g)
    b = im.run("device", image, nums, stream=s, guarded=g)
    torch.cuda.synchronize()
    same(a(), e, disk, "write")
    b = b()
    assert np.array_equal(b["files"], back["files"]) and np.array_equal(b["meta"], back["meta"])
    assert np.array_equal(b["status"], back["status"]) and np.array_equal(b["image"], disk)
    # two streams, one context, an image each
    other = nums[::-1].copy()
    reads2, disk2, _ = loop(im, im.clean, other, recs)
    reads1, disk1, _ = loop(im, im.clean, nums, recs)
    runs = [run(im, "device", im.clean, x, recs, stream=torch.cuda.Stream()) for x in (nums, other)]
    torch.cuda.synchronize()
    same(runs[0](), expect(im, reads1), disk1, "stream 0")
    same(runs[1](), expect(im, reads2), disk2, "stream 1")


@pytest.mark.parametrize("name", ["rs255_t3", "parity32"])  # K = 2 on the direct list path; ds = 31, K = 4, staged
def test_reads_and_writes_alternate_on_one_stream(images, name):
    """read, write, read, write, read queued on one stream of one context with nothing in between, every batch one
    piece of its call plus 3 inodes: the two calls share their frame and the scratch's layout, and the second piece of
    each starts in what the piece before left there.  Every output, the counts and the final image equal those of the
    same five calls through the host forms, which the tests above hold to the loop."""
    im = images(name)
    K, eng = im.K, im.eng
    staged = max(1024, min(eng.host_chunk_blocks() & ~1023, max(1024, ((1 << 31) // im.raw) & ~1023)))  # list_plan.hpp piece_blocks
    piece = dict(read=2 * PIECE // K, write=min(2 * PIECE // K, max(staged // K, 1)))
    assert (K, eng.list_kernel_name()) == dict(rs255_t3=(2, "rs255-wg-list-lds"), parity32=(4, "gather-stage-scatter"))[name]
    calls = []
    for step, kind in enumerate(["read", "write", "read", "write", "read"]):
        n = piece[kind] + 3
        nums = rng_for("alternate", name, step).integers(0, im.total, n).astype(np.uint32)
        nums[[5, n - 1]] = nums[2]  # a number in both pieces
        nums[[7, n - 2]] = im.total, 0xFFFFFFFF
        assert im.free[nums[nums < im.total]].any()
        calls.append((kind, nums, records(n, "alternate", name, step)))
    image, want = im.clean, []
    for kind, nums, recs in calls:
        want.append(im.run("host", image, nums) if kind == "read" else run(im, "host", image, nums, recs))
        image = want[-1]["image"]
    assert not np.array_equal(image, im.clean)
    s, g = torch.cuda.Stream(), Guarded(im.clean)
    torch.cuda.synchronize()  # the image was copied on the default stream
    got = [im.run("device", im.clean, nums, stream=s, guarded=g) if kind == "read"
           else run(im, "device", im.clean, nums, recs, stream=s, guarded=g) for kind, nums, recs in calls]
    torch.cuda.synchronize()
    for step, ((kind, nums, _), finish, w) in enumerate(zip(calls, got, want)):
        a = finish()
        for k in ("files", "meta") if kind == "read" else ():
            assert np.array_equal(a[k], w[k]), (k, step)
        assert np.array_equal(a["status"], w["status"]) and np.array_equal(a["piece_status"], w["piece_status"]), step
        assert a["counts"] == w["counts"] and sum(a["counts"][:5]) == len(nums), step
        assert a["counts"].out_of_range == 2 and a["counts"].not_allocated > 0 and a["counts"].ok > 0, step
        assert np.array_equal(a["image"], image), step  # the image after all five


def test_extent_write_before_and_after_an_inode_write(images):
    """ppfs_ecc_write_extents_device on the same context gives what it gives on a context that never wrote an inode."""
    im = images("rs255_t3")
    rng = rng_for("extents around")
    blocks = rng.permutation(im.blocks)[:40].astype(np.uint32)
    ext = np.zeros(41, EXTENT_DTYPE)
    ext["block"][:40], ext["offset"][:40], ext["length"][:40] = blocks, rng.integers(0, 100, 40), rng.integers(0, 150, 40)
    ext["block"][40], ext["length"][40] = im.blocks + 3, 5  # one past the image
    ext["pos"] = np.concatenate([[0], np.cumsum(ext["length"][:-1])])
    data = rng.integers(0, 256, int(ext["length"].sum()), dtype=np.uint8)
    image = im.clean.copy()
    im.rows(image)[blocks[3], 9] ^= 0x22

    def extents(eng):
        g, st = Guarded(image), torch.full((41,), 0x5A, dtype=torch.uint8, device="cuda")
        eng.write_extents(dev(data), g.image, ext, st)
        return g.result(), host(st)

    alone = extents(make_engine(im.cfg))
    assert alone[1][3] == 1 and alone[1][40] == 9 and not np.array_equal(alone[0], image)
    before = extents(im.eng)
    nums = im.batch()
    check_all(im, ["device"], im.clean, nums, records(len(nums), "between"))
    after = extents(im.eng)
    for got in (before, after):
        assert np.array_equal(got[0], alone[0]) and np.array_equal(got[1], alone[1])


# ------------------------------------------------------------------------------------
# the block-device mirror: the engine override against the per-inode loop, which is the definition
# ------------------------------------------------------------------------------------
MIRROR = [("rs255_t3", "fix"), ("hamming512", "fix"), ("hamming512", "fail"), ("crc512", "fail"), ("parity32", "fail"),
          ("rs64_t3", "clean")]


@pytest.mark.parametrize("mapped", [True, False], ids=["mapped", "unmapped"])
@pytest.mark.parametrize("name,kind", MIRROR, ids=[f"{a}-{b}" for a, b in MIRROR])
def test_block_device_write_inodes_matches_the_loop(images, name, kind, mapped):
    im = sharing_image(images, name)
    image, nums = im.clean.copy(), im.batch()
    if kind != "clean":  # a shared table block damaged, and with it a bitmap block where the code corrects
        image, block, nums = damaged(im, "table", kind)
        if kind == "fix":
            b, bb, _ = damaged(im, "bitmap", "fix")
            im.rows(image)[bb] = im.rows(b)[bb]
    recs = records(len(nums), name, kind, "mirror")
    files, meta = split(recs)
    for check in (1, 0):
        d, disk, logger = mirror(im, image, mapped)
        ref, ref_disk, ref_logger = mirror(im, image, True)
        got = d.write_inodes(im.table(check), nums, files.view(_native.FILE_DTYPE), meta.view(INODE_META_DTYPE))
        want = IBlockDevice.write_inodes(ref, im.table(check), nums, files.view(_native.FILE_DTYPE), meta.view(INODE_META_DTYPE))
        assert len(got) == len(want) == len(nums) and got == want, (name, kind, check)
        errors = set(want)
        assert FsError.Bitmap_IndexOutOfRange in errors and None in errors
        assert (FsError.InodeManager_NotFound in errors) == bool(check)
        if kind == "fail":
            assert FsError.BlockDevice_CorrectionError in errors
        if kind == "fix":
            assert len(ref_logger.corrections) == (2 if check else 1)
        assert logger.corrections == ref_logger.corrections, (name, kind, check)
        if kind != "fail":
            assert np.array_equal(disk, ref_disk), (name, kind, check)
        else:  # the loop stops an inode at its first failing piece, the one call writes its other pieces too
            assert np.array_equal(im.rows(disk)[block], im.rows(image)[block]) and not np.array_equal(disk, image)
    # the loop itself against the oracle's device model: errors, and the image where no piece failed
    reads, o_disk, o_log = loop(im, image, nums, recs)
    e = expect(im, reads)
    ref, ref_disk, _ = mirror(im, image, True)
    for j, err in enumerate(IBlockDevice.write_inodes(ref, im.table(1), nums, files.view(_native.FILE_DTYPE), meta.view(INODE_META_DTYPE))):
        st = int(e["status"][j])
        assert err == (None if st in (0, 1) else FsError.Bitmap_IndexOutOfRange if int(nums[j]) >= im.total else
                       FsError.InodeManager_NotFound if st == 255 else FsError(st))
    if kind != "fail" and (im.raw == 255 or im.cfg[1] != 4):
        assert np.array_equal(ref_disk, o_disk)
