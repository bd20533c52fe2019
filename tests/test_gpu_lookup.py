"""GPU tests of the directory lookups (include/ppfs_ecc.h ppfs_ecc_lookup_*; EccEngine.lookup_plan / lookup /
lookup_host; IBlockDevice.lookup) against the CPU oracle.

Expected values come from IBlockDevice.lookup, the loop of DirectoryManager::getInodeByName (and of removeEntry's
search) restated over read_file in 256-entry batches, run on a device whose readBlock is the oracle's device model
(tests/oracle_lib.py OracleDevice).  Nothing expected comes from the engine.  The loop also gives the disk it leaves
and its correction log; the engine reads every directory whole, so with write-back its image is the loop's plus the
corrected blocks the loop did not reach: the oracle's own correction of every block the engine can reach.

Images are small: three directories of 0, 5 and 300 entries (at ds = 249 the last is 155 blocks: the indirect block,
the doubly indirect tree and both batch boundaries are in play, and no entry is block-aligned), fragmented over one
image by a seeded permutation, as tests/test_gpu_files.py builds its files."""
import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch

from paritypartyfs_amd import _native
from paritypartyfs_amd._native import FILE_DTYPE, LOOKUP_HIT_DTYPE, LOOKUP_QUERY_DTYPE, EccError
from paritypartyfs_amd.block_device import DataLocation, ECCType, Expected, FsError, HeapDisk, IBlockDevice, IDisk, Logger, create_block_device
from paritypartyfs_amd.ecc import EccEngine, LookupCounts
from tests.oracle_lib import OracleDevice
from tests.test_gpu_file import flip, make_engine, oracle_encode, path_of, rng_for, tree_ids
from tests.test_gpu_list import Guarded, dev, host

NONE = 0xFFFFFFFF
NOT_FOUND = 2  # PPFS_ECC_NOT_FOUND
# name, ECCType, block size, t, explicit CRC polynomial, the directories' entries.  rs255: ds 249; hamming1024: a
# payload near a power of two (ds 1,020); rs64: a shortened code, ds 58; parity32: ds 31, whose tree holds 411 blocks
CFG = {c[0]: c for c in [("rs255_t3", 4, 255, 3, 0, (0, 5, 300)), ("hamming1024", 2, 1024, 0, 0, (0, 5, 300)),
                         ("rs64_t3", 4, 64, 3, 0, (0, 5, 300)), ("hamming512", 2, 512, 0, 0, (0, 5, 300)),
                         ("crc512", 1, 512, 0, 0x104C11DB7, (0, 5, 300)), ("parity32", 3, 32, 0, 0, (0, 5, 70))]}
PATHS = ["rs255_t3", "rs64_t3", "hamming512", "crc512", "parity32"]  # with the staged list path of rs255: six
TRAILING = (100, 0, 77)  # bytes behind the last entry, never read


class OracleBlockDevice(IBlockDevice):
    """The reference's device model behind the IBlockDevice interface: what the defining loops run on."""

    def __init__(self, od, ds):
        self.od, self._ds = od, ds

    def dataSize(self):
        return self._ds

    def readBlock(self, loc: DataLocation, bytes_to_read: int, capacity=None):
        rc, data = self.od.read(loc.block_index, loc.offset, bytes_to_read)
        return Expected(data) if rc == 0 else Expected.unexpected(FsError(rc))


class DirImage:
    """Directories of counts[d] entries, fragmented over one image."""

    def __init__(self, oracle, name):
        self.oracle, self.cfg = oracle, CFG[name]
        self.counts = counts = self.cfg[5]
        self.eng = make_engine(self.cfg)
        self.raw, self.ds = raw, ds = self.eng.raw_block_size, self.eng.data_size
        self.I = I = ds // 4
        rng = rng_for("dirs", name, counts)
        nbytes = [128 * n + (TRAILING[d] if n else 100) for d, n in enumerate(counts)]
        self.sizes = sizes = [-(-b // ds) if counts[d] else 1 for d, b in enumerate(nbytes)]  # an empty directory keeps a block
        ids = [[i for lv in tree_ids(0, n, I) for i in lv] for n in sizes]
        self.blocks = blocks = sum(sizes) + sum(len(x) for x in ids) + 7
        perm = rng.permutation(blocks).astype(np.uint32)
        self.files = np.zeros(len(counts), FILE_DTYPE)
        self.data_blk, self.node_blk, self.node_entries, at = [], {}, {}, 0
        for f, n in enumerate(sizes):
            self.data_blk.append(perm[at:at + n].copy())
            at += n
            for i in ids[f]:
                self.node_blk[f, i] = int(perm[at])
                self.node_entries[f, i] = np.zeros(I, np.uint32)
                at += 1
            self.files["file_size"][f] = nbytes[f]
        self.spare = [int(b) for b in perm[at:]]
        for f, n in enumerate(sizes):
            for i in ids[f]:
                self._set_pointer(f, i[:-1], i[-1] if len(i) > 1 else 11 + i[0], self.node_blk[f, i])
            for j in range(n):
                p = path_of(j, I)
                self._set_pointer(f, p[:-1] if p[0] else (), p[-1], int(self.data_blk[f][j]))
        # the entries: names that mostly agree in their first 12 bytes, so that the kernel's second step decides
        self.entries = [np.full((n, 128), 0xEE, np.uint8) for n in counts]  # 0xEE: garbage behind every NUL
        self.names = []
        for d, n in enumerate(counts):
            names = [b"common_prefix_%d_%03d" % (d, i) if i % 3 else b"e%d_%d" % (d, i) for i in range(n)]
            if n >= 300:
                names[10] = names[200] = b"twice"  # the first wins
                names[280] = b""
                names[260] = b"L" * 123
                names[255], names[256] = b"last_of_batch_0", b"first_of_batch_1"
                names[150] = names[20] + b"x"  # an existing name is its proper prefix
            self.names.append(names)
            for i, nm in enumerate(names):
                self.entries[d][i, :4] = np.frombuffer(np.uint32(7000 * (d + 1) + i).tobytes(), np.uint8)
                self.entries[d][i, 4:4 + len(nm)] = np.frombuffer(nm, np.uint8)
                self.entries[d][i, 4 + len(nm)] = 0
            if n >= 300:
                self.entries[d][50, 4:] = np.frombuffer(b"U" * 124, np.uint8)  # unterminated: matches nothing
                self.entries[d][201, :4] = self.entries[d][11, :4]  # an inode number twice
        payload = rng.integers(0, 256, (blocks, ds), dtype=np.uint8)
        for f, n in enumerate(sizes):
            stream = payload[self.data_blk[f]].reshape(-1)
            stream[:128 * counts[f]] = self.entries[f].reshape(-1)
            payload[self.data_blk[f]] = stream.reshape(n, ds)
        self.payload = payload
        self.clean = self.encoded().reshape(-1)

    def _set_pointer(self, f, parent, slot, value):
        if parent == ():
            if slot < 12:
                self.files["direct"][f, slot] = value
            else:
                self.files[("indirect", "doubly_indirect", "trebly_indirect")[slot - 12]][f] = value
        else:
            self.node_entries[f, parent][slot] = value

    def encoded(self):
        payload = self.payload.copy()
        for key, blk in self.node_blk.items():
            payload[blk] = 0
            payload[blk, :4 * self.I] = self.node_entries[key].astype("<u4").view(np.uint8)
        return oracle_encode(self.oracle, self.cfg, payload)

    def block_of_entry(self, d, e, last=False):
        """The file block that holds entry e's first (last) byte."""
        return (128 * e + (127 if last else 0)) // self.ds

    # ---- queries ----
    def queries(self):
        """About 40 (dir, name): several per directory, repeats, every special entry, names that match nothing."""
        big = len(self.counts) - 1
        n = self.counts[big]
        nm = self.names[big]
        ask = [(big, nm[0]), (big, nm[1]), (big, nm[n - 1]), (big, nm[n // 2]), (big, nm[n // 2 + 1]), (big, b"nope"),
               (big, nm[1][:-1]), (big, nm[1] + b"0"), (big, nm[n - 1]), (big, nm[0]), (big, b"U" * 123), (big, b"e"),
               (1, self.names[1][0]), (1, self.names[1][4]), (1, self.names[1][2]), (1, b"nope"), (1, self.names[1][4]),
               (1, nm[0]), (0, b"anything"), (0, b""), (0, nm[0]), (big, b"common_prefix_"), (big, b"common_prefix_%d_" % big)]
        if n >= 300:
            ask += [(big, b"twice"), (big, b""), (big, b"L" * 123), (big, b"L" * 122), (big, nm[255]), (big, nm[256]), (big, nm[20]),
                    (big, nm[150]), (big, nm[10 + 1]), (big, nm[199]), (big, nm[257]), (big, nm[299]), (big, b"twice"),
                    (big, nm[201]), (big, nm[130]), (big, nm[131])]
        q = np.zeros(len(ask) + 2, LOOKUP_QUERY_DTYPE)
        q["dir"][:len(ask)] = [d for d, _ in ask]
        q["dir"][len(ask):] = big
        q["key"] = 0xABCD0000 + np.arange(q.size)  # not read in name mode
        rec = np.full((q.size, 128), 0xC3, np.uint8)  # garbage behind every query's NUL
        for k, (_, name) in enumerate(ask):
            rec[k, :len(name)] = np.frombuffer(name, np.uint8)
            rec[k, len(name)] = 0
        rec[len(ask)] = np.frombuffer(b"U" * 128, np.uint8)  # no NUL
        rec[len(ask) + 1, :124] = np.frombuffer(b"U" * 124, np.uint8)  # L = 124
        rec[len(ask) + 1, 124] = 0
        return q, rec

    def inode_queries(self):
        big = len(self.counts) - 1
        n = self.counts[big]
        base = 7000 * (big + 1)
        keys = [(big, base), (big, base + n - 1), (big, base + 11), (big, base + n // 2), (big, 5), (big, base + n), (1, 14000),
                (1, 14004), (1, 14005), (0, 7000), (big, base + n - 1), (big, base + 10)]
        if n >= 300:
            keys += [(big, base + 255), (big, base + 256), (big, base + 201), (big, base + 200), (big, base + 131), (big, base + 270)]
        q = np.zeros(len(keys), LOOKUP_QUERY_DTYPE)
        q["dir"], q["key"] = [d for d, _ in keys], [k for _, k in keys]
        return q

    # ---- the loop over the oracle's device model ----
    def oracle_device(self, image, nblocks=None):
        _, typ, bs, t, poly, _ = self.cfg
        nblocks = self.blocks if nblocks is None else nblocks
        od = OracleDevice(self.oracle, typ, bs, t, poly, nblocks * self.raw)
        od.disk[:] = image[:nblocks * self.raw]
        return od

    def loop(self, image, q, rec, mode, files=None, nblocks=None):
        """(the loop's answers as hit records, its disk, its log)."""
        od = self.oracle_device(image, nblocks)
        res = OracleBlockDevice(od, self.ds).lookup(self.files if files is None else files, q, rec, mode)
        hits = np.zeros(len(res), LOOKUP_HIT_DTYPE)
        for k, (inode, entry, err) in enumerate(res):
            if err is None:
                hits[k] = (inode, entry, 0, 0)
            else:
                status = NOT_FOUND if err in (FsError.PpFS_NotFound, FsError.DirectoryManager_NotFound) else int(err)
                assert status in (NOT_FOUND, 5, 9) and (err == FsError.DirectoryManager_NotFound) <= (mode == 1)
                hits[k] = (NONE, NONE, status, 0)
        return hits, od.disk.copy(), od.log_entries()

    def reach(self, image, skip_under=(), skip_data=(), nblocks=None):
        """The image after the oracle has read -- and corrected -- every block of every directory that a whole read can
        reach: all of them, except what lies under the index blocks skip_under (directory, id) and the data blocks
        skip_data (directory, file block)."""
        od = self.oracle_device(image, nblocks)
        for (f, i), blk in self.node_blk.items():
            if not any(f == sf and i[:len(si)] == si and i != si for sf, si in skip_under):
                od.read(blk, 0, 1)
        for f, n in enumerate(self.sizes):
            if self.counts[f] == 0:
                continue
            for j in range(n):
                p = path_of(j, self.I)
                under = any(f == sf and p[:len(si)] == si for sf, si in skip_under)
                if not under and (f, j) not in skip_data:
                    od.read(int(self.data_blk[f][j]), 0, 1)
        return od.disk.copy()

    # ---- the engine ----
    def run(self, form, image, q, rec, mode, write_back=True, files=None, eng=None, null=(), nblocks=None):
        eng, files = eng or self.eng, self.files if files is None else files
        nblocks = self.blocks if nblocks is None else nblocks
        img = np.ascontiguousarray(image[:nblocks * self.raw])
        slots, totals = eng.lookup_plan(files)
        nb, nbytes, nq, nd = int(totals["blocks"]), int(totals["bytes"]), len(q), len(files)
        if form == "host":
            img = img.copy()
            ent, st, fl = np.full(nbytes + 8, 0x5A, np.uint8), np.full(nb + 8, 77, np.uint8), np.full(nd, 0x77777777, np.uint32)
            hits, counts, fcounts = eng.lookup_host(img, files, q, rec if mode == 0 else None, mode,
                                                    None if "entries" in null else ent[:nbytes],
                                                    None if "block_status" in null else st[:nb],
                                                    None if "dir_flags" in null else fl, write_back=write_back)
            assert (ent[nbytes:] == 0x5A).all() and (st[nb:] == 77).all()
            return dict(hits=hits, counts=counts, fcounts=fcounts, image=img, entries=ent[:nbytes], st=st[:nb], flags=fl,
                        slots=slots, totals=totals)
        g = Guarded(img)
        ent = torch.full((7 + nbytes + 40,), 0x5A, dtype=torch.uint8, device="cuda")  # the entries start at an odd address
        st = torch.full((5 + nb + 40,), 77, dtype=torch.uint8, device="cuda")
        fl = dev(np.full(nd + 2, 0x77777777, np.uint32).view(np.int32))
        hi = dev(np.full(4 * nq + 8, 0x5A5A5A5A, np.uint32).view(np.int32))
        names = torch.full((3 + 128 * nq + 5,), 0x11, dtype=torch.uint8, device="cuda")
        if mode == 0:
            names[3:3 + 128 * nq] = dev(rec.reshape(-1))
        cn = torch.full((10,), -7, dtype=torch.int64, device="cuda")
        eng.lookup(g.image, files, q, names[3:3 + 128 * nq] if mode == 0 else None, mode, ent[7:7 + nbytes], st[5:5 + nb], hi[4:4 + 4 * nq],
                   dir_flags=None if "dir_flags" in null else fl[1:1 + nd], counts=None if "counts" in null else cn[1:9],
                   file_counts=None if "file_counts" in null else True, write_back=write_back)
        e, s, h, c, f = host(ent), host(st), host(hi).view(np.uint32), host(cn), host(fl).view(np.uint32)
        assert (e[:7] == 0x5A).all() and (e[7 + nbytes:] == 0x5A).all(), "entries written outside the directories' bytes"
        assert (s[:5] == 77).all() and (s[5 + nb:] == 77).all(), "block statuses written outside their array"
        assert (h[:4] == 0x5A5A5A5A).all() and (h[4 + 4 * nq:] == 0x5A5A5A5A).all(), "hits written outside their array"
        assert c[0] == -7 and c[9] == -7 and f[0] == 0x77777777 and f[1 + nd] == 0x77777777
        return dict(hits=h[4:4 + 4 * nq].copy().view(LOOKUP_HIT_DTYPE), counts=None if "counts" in null else LookupCounts(*c[1:9].tolist()),
                    image=g.result(), entries=e[7:7 + nbytes], st=s[5:5 + nb], flags=f[1:1 + nd], slots=slots, totals=totals)

    def read_whole(self, image, write_back=True, files=None, eng=None, nblocks=None):
        """EccEngine.read_files_host over the ranges (0, 128 n_d): what the lookup's working buffers must hold."""
        eng, files = eng or self.eng, self.files if files is None else files
        nblocks = self.blocks if nblocks is None else nblocks
        ranges = np.stack([np.zeros(len(files), np.uint64), (files["file_size"] // 128 * 128).astype(np.uint64)], axis=1)
        _, totals = eng.files_plan(files, ranges)
        out, st = np.zeros(int(totals["bytes"]), np.uint8), np.zeros(int(totals["blocks"]), np.uint8)
        fl = np.zeros(len(files), np.uint32)
        img = np.ascontiguousarray(image[:nblocks * self.raw]).copy()
        eng.read_files_host(img, files, ranges, out, st, fl, write_back=write_back)
        return out, st, fl, img


def counts_of(hits):
    return LookupCounts(*[int((hits["status"] == s).sum()) for s in (0, NOT_FOUND, 5, 9)], 0, 0, 0, 0)


def same_hits(got, want, tag):
    for field in LOOKUP_HIT_DTYPE.names:
        assert np.array_equal(got[field], want[field]), (tag, field, got[field].tolist(), want[field].tolist())


def check(im, image, q, rec, mode, write_back, expect_image, tag, forms=("device", "host"), **kw):
    """Both forms against the loop: hits field by field, counts, the working buffers against read_files, the image."""
    want, loop_disk, _ = im.loop(image, q, rec, mode, files=kw.get("files"), nblocks=kw.get("nblocks"))
    ent, st, fl, _ = im.read_whole(image, write_back, files=kw.get("files"), nblocks=kw.get("nblocks"))
    for form in forms:
        got = im.run(form, image, q, rec, mode, write_back, **kw)
        same_hits(got["hits"], want, (tag, form))
        assert got["counts"] == counts_of(want), (tag, form)
        assert np.array_equal(got["st"], st) and np.array_equal(got["flags"], fl), (tag, form)
        good = np.ones(ent.size, bool)  # the bytes of a block that failed or lies past the image are not defined
        for s in got["slots"]:
            pos, end = int(s["out_pos"]), int(s["out_pos"]) + int(s["bytes"])
            for j in np.nonzero(np.isin(st[int(s["block_pos"]):int(s["block_pos"]) + int(s["blocks"])], (5, 9)))[0]:
                good[pos + int(j) * im.ds:min(pos + (int(j) + 1) * im.ds, end)] = False
        assert np.array_equal(got["entries"][good], ent[good]), (tag, form)
        if expect_image is not None:
            assert np.array_equal(got["image"], expect_image if write_back else image[:got["image"].size]), (tag, form)
    if expect_image is not None:  # the loop's disk is the engine's minus the blocks the loop did not reach
        rows_l, rows_e = loop_disk.reshape(-1, im.raw), expect_image.reshape(-1, im.raw)
        rows_0 = image[:loop_disk.size].reshape(-1, im.raw)
        untouched, as_engine = (rows_l == rows_0).all(axis=1), (rows_l == rows_e).all(axis=1)
        assert (untouched | as_engine).all(), tag
    return want


@pytest.fixture(scope="module")
def images(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = DirImage(oracle, name)
        return cache[name]
    return get


# ------------------------------------------------------------------------------------
# clean images: every codec path, both modes, both forms
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", PATHS + ["hamming1024"])
def test_lookup_on_a_clean_image(images, name, mode):
    im = images(name)
    q, rec = im.queries() if mode == 0 else (im.inode_queries(), None)
    want = check(im, im.clean, q, rec, mode, True, im.clean, name)
    assert (want["status"] == 0).sum() >= 8 and (want["status"] == NOT_FOUND).sum() >= 4
    if mode == 0 and im.counts[-1] >= 300:
        found = {bytes(rec[k][:list(rec[k]).index(0)]): int(want["entry"][k]) for k in np.nonzero(want["status"] == 0)[0]}
        assert found[b"twice"] == 10 and found[b""] == 280 and found[b"L" * 123] == 260 and found[im.names[-1][256]] == 256
        assert found[im.names[-1][20]] == 20 and found[im.names[-1][150]] == 150


def test_plan_is_files_plan_over_the_entries(images):
    im = images("rs255_t3")
    slots, totals = im.eng.lookup_plan(im.files)
    ranges = np.array([(0, 128 * n) for n in im.counts], np.uint64)
    s2, t2 = im.eng.files_plan(im.files, ranges)
    assert slots.tobytes() == s2.tobytes() and totals.tobytes() == t2.tobytes()
    assert int(totals["bytes"]) == 128 * sum(im.counts) and int(slots["blocks"][0]) == 0 and int(slots["blocks"][2]) == 155
    assert 128 * 300 % im.ds and all((128 * e) % im.ds for e in range(1, 249))  # entries do not start on block boundaries


def test_rs255_staged_list_path_gives_the_same(images, monkeypatch):
    im = images("rs255_t3")
    monkeypatch.setenv("PPFS_ECC_LIST_DIRECT", "0")
    staged = make_engine(im.cfg)
    monkeypatch.delenv("PPFS_ECC_LIST_DIRECT")
    assert staged.list_kernel_name() != im.eng.list_kernel_name()
    q, rec = im.queries()
    check(im, im.clean, q, rec, 0, True, im.clean, "staged", forms=("device",), eng=staged)


@pytest.mark.parametrize("form", ["device", "host"])
def test_optional_outputs_null(images, form):
    im = images("rs255_t3")
    q, rec = im.queries()
    want, _, _ = im.loop(im.clean, q, rec, 0)
    nulls = ("dir_flags", "counts", "file_counts") if form == "device" else ("entries", "block_status", "dir_flags")
    for null in [(n,) for n in nulls] + [nulls]:
        got = im.run(form, im.clean, q, rec, 0, null=null)
        same_hits(got["hits"], want, null)
        if "dir_flags" in null:
            assert (got["flags"] == 0x77777777).all()


# ------------------------------------------------------------------------------------
# damage: the loop's failure rule, write-back on and off
# ------------------------------------------------------------------------------------
def fail_block(im, rng, rows, files, f, j=None, node=None):
    """Make file block j (or the index block `node`) of directory f fail; returns the status it fails with.  Hamming:
    two flips, CRC and parity: one, which the reference answers with a correction error (5).  The reference's
    Reed-Solomon decode never reports a correction error -- errors past t come back as corrected -- so under RS the
    only failing status there is, is 9: the pointer to the block is set past the image instead."""
    if im.cfg[1] != 4:
        blk = int(im.data_blk[f][j]) if node is None else im.node_blk[f, node]
        flip(rng, im.cfg, rows[blk], 2 if im.cfg[1] == 2 else 1)
        assert im.oracle_device(rows.reshape(-1)).read(blk, 0, 1)[0] == 5
        return 5
    point_past(im, rows, files, f, path_of(j, im.I) if node is None else node, data=node is None)
    return 9


def point_past(im, rows, files, f, path, data=True):
    """The pointer at the end of `path` -- a data block's path_of, or an index block's id -- names a block past the image."""
    past = im.blocks + 5
    if data and path[0] == 0:
        files["direct"][f, path[1]] = past
    elif not data and len(path) == 1:
        files[("indirect", "doubly_indirect", "trebly_indirect")[path[0] - 1]][f] = past
    else:
        key = (f, path[:-1])
        entries = im.node_entries[key].copy()
        entries[path[-1]] = past
        payload = np.zeros((1, im.ds), np.uint8)
        payload[0, :4 * im.I] = entries.astype("<u4").view(np.uint8)
        rows[im.node_blk[key]] = oracle_encode(im.oracle, im.cfg, payload)[0]


def damaged(im, case):
    """(image, directory records, the failing status, what a whole read cannot reach: index ids, data blocks) for one
    fault in the large directory."""
    big = len(im.counts) - 1
    rng = rng_for("lookup damage", im.cfg[0], case)
    rows, files = im.clean.reshape(-1, im.raw).copy(), im.files.copy()
    bad, skip_under, skip_data = 0, (), ()
    if case == "correctable":  # one error the code corrects, behind last(0): only batch-1 and not-found loops reach it
        flip(rng, im.cfg, rows[im.data_blk[big][im.block_of_entry(big, 270)]], 1)
    elif case in ("fail_batch0", "fail_batch1", "straddler"):
        # under entry 100: every loop over this directory reads it; under entry 290: a match in batch 0 is found,
        # everything else fails; the block with byte 32,768: the end of batch 0 and the start of batch 1
        j = {"fail_batch0": im.block_of_entry(big, 100), "fail_batch1": im.block_of_entry(big, 290), "straddler": 32768 // im.ds}[case]
        assert case != "straddler" or j * im.ds < 32768 < (j + 1) * im.ds
        bad = fail_block(im, rng, rows, files, big, j)
        skip_data = ((big, j),) if bad == 9 else ()
        if case == "fail_batch1":  # and behind it a block the code corrects: no loop reaches it, the engine does
            assert im.block_of_entry(big, 297) > j
            flip(rng, im.cfg, rows[im.data_blk[big][im.block_of_entry(big, 297)]], 1)
        if case == "fail_batch0":  # the same in the next batch, which no readFile of any loop touches
            flip(rng, im.cfg, rows[im.data_blk[big][im.block_of_entry(big, 270)]], 1)
    elif case == "indirect":  # the single indirect block: file blocks 12 .. 12 + ipb - 1 inherit its failure
        bad = fail_block(im, rng, rows, files, big, node=(1,))
        skip_under = ((big, (1,)),)
    elif case == "past_image":  # the pointer of the block under entry 290 lies past the image: 9
        j = im.block_of_entry(big, 290)
        point_past(im, rows, files, big, path_of(j, im.I))
        bad, skip_data = 9, ((big, j),)
    else:
        raise AssertionError(case)
    return rows.reshape(-1), files, bad, skip_under, skip_data


CASES = ["correctable", "fail_batch0", "fail_batch1", "straddler", "indirect", "past_image"]


@pytest.mark.parametrize("write_back", [True, False])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", ["rs255_t3", "hamming1024"])
def test_lookup_on_a_damaged_image(images, name, case, write_back):
    im = images(name)
    image, files, bad, skip_under, skip_data = damaged(im, case)
    expect_image = im.reach(image, skip_under, skip_data)
    q, rec = im.queries()
    want = check(im, image, q, rec, 0, write_back, expect_image, (name, case, write_back), files=files)
    big = q["dir"] == len(im.counts) - 1
    st = want["status"]
    if case == "correctable":
        assert not np.isin(st, (5, 9)).any() and not np.array_equal(expect_image, image)
    elif case in ("fail_batch0", "straddler", "indirect"):
        assert (st[big] == bad).all() and not np.isin(st[~big], (5, 9)).any()
    elif case == "fail_batch1":
        # found in batch 0 although a block fails behind last(0); everything that reads batch 1 fails
        assert ((st[big] == 0) == (want["entry"][big] < 256)).all() and (st[big] == bad).sum() >= 10 and (st[big] == 0).sum() >= 10
        loop_disk = im.loop(image, q, rec, 0, files=files)[1]
        assert np.array_equal(loop_disk, image) and not np.array_equal(expect_image, image)  # corrected beyond the loop's reach
    else:
        assert ((st[big] == 0) == (want["entry"][big] < 256)).all() and (st[big] == 9).sum() >= 10
    assert (st[~big] == 0).any() and (st[~big] == NOT_FOUND).any()


def test_the_reference_outcomes_cover_every_class(images):
    """Found, not found, 5, 9, and a failure that is ignored because it lies behind last(B): none is silently empty.
    (Hamming: the reference's Reed-Solomon decode has no 5.)"""
    im = images("hamming1024")
    q, rec = im.queries()
    seen = set()
    for case in CASES:
        image, files, *_ = damaged(im, case)
        want, _, _ = im.loop(image, q, rec, 0, files=files)
        clean, _, _ = im.loop(im.clean, q, rec, 0)
        seen |= {int(s) for s in want["status"]}
        if case in ("fail_batch1", "past_image"):
            kept = (want["status"] == 0) & (q["dir"] == 2)
            assert kept.any() and np.array_equal(want[kept], clean[kept])
            seen.add("ignored")
    assert seen == {0, NOT_FOUND, 5, 9, "ignored"}


@pytest.mark.parametrize("write_back", [True, False])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", ["rs255_t3", "hamming1024"])
def test_inode_mode_on_a_damaged_image(images, name, case, write_back):
    im = images(name)
    image, files, _, skip_under, skip_data = damaged(im, case)
    q = im.inode_queries()
    want = check(im, image, q, None, 1, write_back, im.reach(image, skip_under, skip_data), (name, case, write_back), files=files)
    if case != "correctable":
        assert np.isin(want["status"], (5, 9)).any()
    assert (want["status"] == 0).any() and (want["status"] == NOT_FOUND).any()


# ------------------------------------------------------------------------------------
# the block devices
# ------------------------------------------------------------------------------------
class PlainDisk(IDisk):
    """A disk the engine cannot map: the device keeps the loop."""

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


def log_blocks(logger):
    return [b for _, b in logger.corrections]


# a shortened code (rs64) keeps the loop, a detection-only code (crc512) corrects nothing: one case each
DEVICE_CASES = [("rs255_t3", c, 2) for c in ("clean", "correctable", "fail_batch0", "fail_batch1", "indirect", "past_image")] + [
    ("hamming1024", "correctable", 2), ("hamming1024", "fail_batch0", 2), ("hamming1024", "indirect", 2), ("rs64_t3", "clean", 5), ("crc512", "fail_batch1", 2)]


@pytest.mark.parametrize("name,case,every", DEVICE_CASES)
def test_block_device_lookup_equals_the_loop(images, name, case, every):
    """The engine device's one-call lookup against the base-class loop on a copy of the disk, and against the loop on
    the oracle's device model: results, then the adapter contract for the disk and the log."""
    im = images(name)
    image, files, _, skip_under, skip_data = (im.clean, im.files, 0, (), ()) if case == "clean" else damaged(im, case)
    for mode in (0, 1):
        q, rec = im.queries() if mode == 0 else (im.inode_queries(), None)
        q, rec = q[::every].copy(), (None if rec is None else rec[::every].copy())  # the per-block loops run three times
        want, loop_disk, _ = im.loop(image, q, rec, mode, files=files)
        d, disk, logger = mirror(im, image)
        got = d.lookup(files, q, rec, mode)
        ref_dev, ref_disk, ref_logger = mirror(im, image)
        ref = IBlockDevice.lookup(ref_dev, files, q, rec, mode)
        assert got == ref, (name, case, mode)
        for k, (inode, entry, err) in enumerate(got):
            if want["status"][k] == 0:
                assert (inode, entry, err) == (int(want["inode"][k]), int(want["entry"][k]), None)
            else:
                assert inode is None and entry is None and err is not None
        # the loop over the device's own read_file, which corrects what lies behind a failing block of the same batch
        # (readFile's documented deviation): its disk is the oracle loop's or, block by block, the engine's
        rows_r, rows_l = ref_disk.reshape(-1, im.raw), loop_disk.reshape(-1, im.raw)
        rows_e = im.reach(image, skip_under, skip_data).reshape(-1, im.raw)
        assert ((rows_r == rows_l).all(axis=1) | (rows_r == rows_e).all(axis=1)).all(), (name, case, mode)
        mine, theirs = log_blocks(logger), log_blocks(ref_logger)
        if name == "rs64_t3":  # a shortened code keeps the loop
            assert np.array_equal(disk, ref_disk) and mine == theirs
            continue
        expect = im.reach(image, skip_under, skip_data)
        assert np.array_equal(disk, expect), (name, case, mode)
        assert mine[:len(theirs)] == theirs, (name, case, mode)
        extra = mine[len(theirs):]
        changed = np.nonzero((expect.reshape(-1, im.raw) != ref_disk.reshape(-1, im.raw)).any(axis=1))[0]
        assert sorted(extra) == sorted(int(b) for b in changed) and len(set(extra)) == len(extra), (name, case, mode)
    # an unmapped disk keeps the loop, over its own per-block read_file
    q, rec = im.queries()
    q, rec = q[::every].copy(), rec[::every].copy()
    d, disk, logger = mirror(im, image, mapped=False)
    ref_dev, ref_disk, ref_logger = mirror(im, image, mapped=False)
    assert d.lookup(files, q, rec, 0) == IBlockDevice.lookup(ref_dev, files, q, rec, 0)
    assert np.array_equal(disk, ref_disk) and log_blocks(logger) == log_blocks(ref_logger)


# ------------------------------------------------------------------------------------
# error returns, the read_inodes hand-over
# ------------------------------------------------------------------------------------
def test_error_returns(images):
    im = images("rs255_t3")
    eng = im.eng
    q, rec = im.queries()
    _, totals = eng.lookup_plan(im.files)
    nb, nbytes, nq = int(totals["blocks"]), int(totals["bytes"]), len(q)
    g = Guarded(im.clean)
    ent, st = (torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda") for n in (nbytes, nb))
    hi = torch.full((4 * nq,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    names = dev(rec.reshape(-1))
    bad = q.copy()
    bad["dir"][17] = len(im.counts)
    with pytest.raises(EccError) as e:
        eng.lookup(g.image, im.files, bad, names, 0, ent, st, hi)
    assert e.value.code == -22 and "query 17" in str(e.value)
    with pytest.raises(EccError) as e:
        eng.lookup_host(im.clean.copy(), im.files, bad, rec, 0)
    assert e.value.code == -22 and "query 17" in str(e.value)
    for kw in (dict(entries=ent[:nbytes - 1]), dict(block_status=st[:nb - 1]), dict(hits=hi[:4 * nq - 1]), dict(names=names[:-1]),
               dict(names=None), dict(entries=None), dict(mode=2)):
        a = dict(names=names, mode=0, entries=ent, block_status=st, hits=hi)
        a.update(kw)
        with pytest.raises((ValueError, EccError)):
            eng.lookup(g.image, im.files, q, a["names"], a["mode"], a["entries"], a["block_status"], a["hits"])
    # the C ABI itself: short and null buffers, misaligned hits, before anything touches the GPU
    L = _native.lib()
    args = lambda **k: (eng._h, g.image.data_ptr(), im.blocks, im.files.ctypes.data, len(im.files), q.ctypes.data,  # noqa: E731
                        k.get("names", names.data_ptr()), nq, 0, k.get("entries", ent.data_ptr()), k.get("bytes", nbytes),
                        k.get("st", st.data_ptr()), None, k.get("hits", hi.data_ptr()), None, None, 1, None)
    for k in (dict(bytes=nbytes - 1), dict(entries=None), dict(st=None), dict(names=None), dict(hits=hi.data_ptr() + 2), dict(hits=None)):
        assert L.ppfs_ecc_lookup_device(*args(**k)) == -22, k
    torch.cuda.synchronize()
    assert (host(ent) == 0x5A).all() and (host(hi) == 0x5A5A5A5A).all() and np.array_equal(g.result(), im.clean)
    # nothing to look up: zeroed counts, nothing read
    cn = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    eng.lookup(g.image, im.files, q[:0], names[:0], 0, ent, st, hi, counts=cn)
    assert host(cn).tolist() == [0] * 8 and (host(ent) == 0x5A).all()
    hits, counts, _ = eng.lookup_host(im.clean.copy(), im.files, q[:0], rec[:0], 0)
    assert hits.size == 0 and counts == LookupCounts(*[0] * 8)


def test_lookup_refuses_a_capturing_stream(images):
    im = images("rs255_t3")
    q, rec = im.queries()
    _, totals = im.eng.lookup_plan(im.files)
    image, names = torch.from_numpy(im.clean).cuda(), dev(rec.reshape(-1))
    ent = torch.zeros(int(totals["bytes"]), dtype=torch.uint8, device="cuda")
    st = torch.zeros(int(totals["blocks"]), dtype=torch.uint8, device="cuda")
    hi = torch.zeros(4 * len(q), dtype=torch.int32, device="cuda")
    im.eng.lookup(image, im.files, q, names, 0, ent, st, hi)  # whatever the call sets up exists before the capture
    torch.cuda.synchronize()
    codes = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # captured and never replayed
        try:
            im.eng.lookup(image, im.files, q, names, 0, ent, st, hi)
            codes.append(0)
        except EccError as e:
            codes.append(e.code)
    assert codes == [-95]  # PPFS_ECC_ENOTSUP


def test_entries_are_a_ready_source_for_read_inodes(images):
    """After the call the entries buffer holds DirectoryEntry records at stride 128: the hits' entries name the inode
    numbers read_inodes would fetch next."""
    im = images("rs255_t3")
    q, rec = im.queries()
    got = im.run("device", im.clean, q, rec, 0)
    found = got["hits"][got["hits"]["status"] == 0]
    dirs = q["dir"][got["hits"]["status"] == 0]
    at = got["slots"]["out_pos"][dirs].astype(np.int64) + 128 * found["entry"].astype(np.int64)
    numbers = got["entries"][at[:, None] + np.arange(4)].copy().view("<u4").reshape(-1)
    assert np.array_equal(numbers, found["inode"]) and found.size >= 8
