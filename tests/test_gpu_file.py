"""GPU tests of the read-only file walk (include/ppfs_ecc.h ppfs_ecc_file_blocks_*, ppfs_ecc_read_file_*,
ppfs_ecc_file_span, ppfs_ecc_file_tree_blocks; EccEngine.file_blocks / read_file and their host forms)
against the CPU oracle.

This file carries a Python restatement of the read-only BlockIndexIterator walk (file_io.cpp:186-463) and of
FileIO::readFile (:12-44) over the oracle's batch decode, in the calls' batch form: every block of the range
is attempted, an index block that fails hands its status to everything under it.  Nothing expected comes
from the engine.

Images are built as the reference builds them -- an index block is a write of its entries at {block, 0}
onto a zeroed block (_writeIndexBlock), a data block a full write -- but with the oracle's batch encode
(test_batch_built_image_equals_per_block_writes shows the two agree), and placed by a seeded permutation,
so that the file is fragmented and index blocks lie among data blocks."""
import zlib

import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch

from paritypartyfs_amd import EccEngine
from paritypartyfs_amd._native import FILE_DTYPE, EccError
from paritypartyfs_amd.block_device import ECCType, HeapDisk, IBlockDevice, Logger, create_block_device
from paritypartyfs_amd.ecc import FileCounts
from tests.oracle_lib import OracleDevice
from tests.test_gpu_list import Guarded, d_index, host
from tests.test_gpu_scrub_alloc import oracle_decode

NO_BLOCK = 0xFFFFFFFF
PIECE_BLOCKS = 1 << 15  # csrc/file_plan.hpp
# name, ECCType, block size, t, explicit CRC polynomial, file blocks: the smallest files that reach every branch
# of each tree (rs64 / crc100: ipb 14 / 24, past a mid-block boundary of the trebly tree; rs512: ipb 62, into the
# trebly tree; hamming512: ipb 127, into the doubly tree; parity3: dataSize() 2, ipb 0, direct blocks only)
CFGS = [("rs64_t3", 4, 64, 3, 0, 450), ("rs512_t3", 4, 512, 3, 0, 4200), ("hamming512", 2, 512, 0, 0, 400),
        ("crc100_deg3", 1, 100, 0, 0xB, 1250), ("parity3", 3, 3, 0, 0, 9)]
CFG = {c[0]: c for c in CFGS}
NAMES = [c[0] for c in CFGS]


def rng_for(*k):
    return np.random.default_rng(zlib.crc32(repr(k).encode()))


def path_of(j, I):
    """(segment, slots outermost first) of file block j."""
    if j < 12:
        return (0, j)
    s = j - 12
    if s < I:
        return (1, s)
    s -= I
    if s < I * I:
        return (2, s // I, s % I)
    s -= I * I
    assert s < I ** 3
    return (3, s // (I * I), (s // I) % I, s % I)


def tree_ids(j0, cnt, I):
    """The index blocks a walk over [j0, j0 + cnt) needs, per level in level order.  An id is its path from the
    inode: (segment,) a root, (segment, a) a doubly leaf or a trebly mid block, (3, a, b) a trebly leaf."""
    levels = [{}, {}, {}]
    for j in range(j0, j0 + cnt):
        p = path_of(j, I)
        for d in range(p[0]):
            levels[d].setdefault(p[:d + 1])
    return [list(lv) for lv in levels]


def oracle_encode(oracle, cfg, payloads):
    """Rows of the payloads (nb, ds) written onto zeroed blocks."""
    _, typ, bs, t, poly, _ = cfg
    nb = payloads.shape[0]
    flat, zero = np.ascontiguousarray(payloads).reshape(-1), np.zeros(nb * bs, np.uint8)
    if typ == 4:
        raw = oracle.rs_encode(bs, t, flat)
    elif typ == 2:
        raw = oracle.ham_encode(bs, flat, raw_old=zero)
    elif typ == 1:
        raw = oracle.crc_encode(bs, poly, flat, raw_old=zero)
    else:
        raw = oracle.parity_encode(bs, flat, raw_old=zero)
    return raw.reshape(nb, -1)


def make_engine(cfg):
    _, typ, bs, t, poly, _ = cfg
    return EccEngine(typ, bs, t, crc_polynomial_explicit=poly)


def flip(rng, cfg, row, k):
    """k errors at distinct places of one raw block: byte errors for RS, bit flips otherwise."""
    typ = cfg[1]
    for pos in rng.choice(row.size * (1 if typ == 4 else 8), k, replace=False):
        if typ == 4:
            row[pos] ^= np.uint8(rng.integers(1, 256))
        else:
            row[pos // 8] ^= np.uint8(0x80 >> (pos % 8))


class FileImage:
    """One fragmented file in one image, damaged, with the oracle's walk over it.
    fail: the id of an index block damaged beyond the code's capability; oob: an id (or ("data", j)) whose pointer
    is set past the image; dup: (j, k) -- file block k points at file block j's image block."""

    def __init__(self, oracle, name, n=None, fail=None, oob=None, dup=None, damage_data=True):
        self.oracle, self.cfg = oracle, CFG[name]
        _, typ, bs, t, poly, n_default = self.cfg
        self.n = n = n_default if n is None else n
        self.eng = eng = make_engine(self.cfg)
        self.raw, self.ds = raw, ds = eng.raw_block_size, eng.data_size
        self.I = I = ds // 4
        rng = rng_for(name, n, fail, oob, dup)
        ids = [i for lv in tree_ids(0, n, I) for i in lv]
        self.blocks = blocks = n + len(ids) + 5
        perm = rng.permutation(blocks).astype(np.uint32)
        self.data_blk = perm[:n].copy()
        self.node_blk = {i: int(perm[n + k]) for k, i in enumerate(ids)}
        self.file = np.zeros(1, FILE_DTYPE)
        self.file["file_size"] = (n - 1) * ds + (ds + 1) // 2  # the last block is half full
        entries = {i: np.zeros(I, np.uint32) for i in ids}
        past = blocks + 5

        def set_pointer(parent, slot, value):
            if parent == ():
                if slot < 12:
                    self.file["direct"][0, slot] = value
                else:
                    self.file[("indirect", "doubly_indirect", "trebly_indirect")[slot - 12]] = value
            else:
                entries[parent][slot] = value

        for i in ids:
            v = past if oob == i else self.node_blk[i]
            set_pointer(i[:-1], i[-1] if len(i) > 1 else 11 + i[0], v)
        if dup:
            self.data_blk[dup[1]] = self.data_blk[dup[0]]
        for j in range(n):
            p = path_of(j, I)
            set_pointer(p[:-1] if p[0] else (), p[-1], past if oob == ("data", j) else int(self.data_blk[j]))
        payload = rng.integers(0, 256, (blocks, ds), dtype=np.uint8)
        for i in ids:
            payload[self.node_blk[i]] = 0
            payload[self.node_blk[i], :4 * I] = entries[i].astype("<u4").view(np.uint8)
        self.payload = payload
        rows = oracle_encode(oracle, self.cfg, payload)
        self.clean = rows.reshape(-1).copy()
        for k, i in enumerate(ids):  # every index block: errors within the code's capability
            row = rows[self.node_blk[i]]
            if i == fail:  # beyond it: t + 2 bytes for RS, two flips for Hamming, one for CRC and parity
                flip(rng, self.cfg, row, t + 2 if typ == 4 else 2 if typ == 2 else 1)
            else:
                flip(rng, self.cfg, row, 1 + k % t if typ == 4 else 1 if typ == 2 else 0)
        if damage_data:
            for j in range(n):  # 0 .. t + 2 byte errors (RS), 0 .. 3 flips
                flip(rng, self.cfg, rows[self.data_blk[j]], int(rng.integers(0, (t + 3) if typ == 4 else 4)))
        self.image = rows.reshape(-1)

    # ---- the oracle's walk ----
    def walk(self, j0, cnt, write_back=True):
        """index, path status, tree index, tree status, the image afterwards, every block the walk decoded."""
        I, rows = self.I, self.image.reshape(self.blocks, self.raw)
        wb = write_back and self.cfg[1] in (2, 4)
        exp, seen, info = rows.copy(), [], {}
        t_index, t_status = [], []
        f = self.file[0]

        def decode(ptrs):
            """statuses and payloads of the listed blocks; those past the image get 9"""
            ptrs = np.asarray(ptrs, np.int64)
            st, pay = np.full(ptrs.size, 9, np.uint8), np.zeros((ptrs.size, self.ds), np.uint8)
            inr = np.nonzero(ptrs < self.blocks)[0]
            if inr.size:
                d, s, fixed = oracle_decode(self.oracle, self.cfg[:5], rows[ptrs[inr]])
                st[inr], pay[inr] = s, d
                if wb:
                    exp[ptrs[inr]] = fixed
                seen.extend(ptrs[inr].tolist())
            return st, pay

        def pointer_under(parent, slot):
            if parent == ():
                return (int(f["direct"][slot]) if slot < 12 else int(f[("indirect", "doubly_indirect", "trebly_indirect")[slot - 12]])), 0
            _, ps, ent = info[parent]
            return (NO_BLOCK, ps) if ps in (5, 9) else (int(ent[slot]), 0)

        for lv in tree_ids(j0, cnt, I):
            got = [pointer_under(i[:-1], i[-1] if len(i) > 1 else 11 + i[0]) for i in lv]
            live = [k for k, (_, inh) in enumerate(got) if not inh]
            st, pay = decode([got[k][0] for k in live])
            for k, i in enumerate(lv):
                ptr, inh = got[k]
                s, ent = inh, None
                if not inh:
                    q = live.index(k)
                    s, ent = int(st[q]), pay[q, :4 * I].copy().view("<u4")
                info[i] = (ptr, s, ent)
                t_index.append(ptr)
                t_status.append(s)
        index, path = np.zeros(cnt, np.uint32), np.zeros(cnt, np.uint8)
        for k in range(cnt):
            p = path_of(j0 + k, I)
            index[k], path[k] = pointer_under(p[:-1] if p[0] else (), p[-1])
        return index, path, np.array(t_index, np.uint32), np.array(t_status, np.uint8), exp, seen, decode

    def read(self, offset, nbytes, write_back=True, sentinel=0x5A):
        """(first, blocks, clamped), out, status, counts, tree statuses, the image afterwards of a read_file."""
        ds, size = self.ds, int(self.file["file_size"][0])
        assert offset < size or nbytes == 0
        clamped = min(nbytes, size - offset) if nbytes else 0
        first = offset // ds if nbytes else 0
        cnt = (offset % ds + clamped + ds - 1) // ds if nbytes else 0
        index, path, _, t_status, exp, seen, decode = self.walk(first, cnt, write_back)
        live = np.nonzero(path == 0)[0]
        st, pay = decode(index[live])
        assert len(seen) == len(set(seen)), "the expected walk names an image block twice"
        status = path.copy()
        status[live] = st
        out, pos = np.full(clamped, sentinel, np.uint8), 0
        payload = {int(k): pay[q] for q, k in enumerate(live)}
        for k in range(cnt):
            off = offset % ds if k == 0 else 0
            ln = min(ds - off, clamped - pos)
            if status[k] == 5:
                out[pos:pos + ln] = 0
            elif status[k] != 9:
                out[pos:pos + ln] = payload[k][off:off + ln]
            pos += ln
        assert pos == clamped
        counts = FileCounts(*[int((status == v).sum()) for v in (0, 1, 5, 9)], *[int((t_status == v).sum()) for v in (0, 1, 5, 9)])
        return (first, cnt, clamped), out, status, counts, t_status, exp.reshape(-1)

    def expect_blocks(self, j0, cnt, write_back=True):
        index, path, t_index, t_status, exp, seen, _ = self.walk(j0, cnt, write_back)
        assert len(seen) == len(set(seen)), "the expected walk names an image block twice"
        counts = FileCounts(*[int((path == v).sum()) for v in (0, 1, 5, 9)], *[int((t_status == v).sum()) for v in (0, 1, 5, 9)])
        return index, path, t_index, t_status, counts, exp.reshape(-1)

    # ---- the engine ----
    def run_blocks(self, form, j0, cnt, eng=None, write_back=True):
        eng = eng or self.eng
        T = eng.file_tree_blocks(self.file, j0, cnt)
        if form == "host":
            img = self.image.copy()
            ix, ps = np.full(cnt, 0x77777777, np.uint32), np.full(cnt, 77, np.uint8)
            ti, ts = np.full(T, 0x77777777, np.uint32), np.full(T, 77, np.uint8)
            counts = eng.file_blocks_host(img, self.file, j0, cnt, ix, ps, ti, ts, write_back=write_back)
            return ix, ps, ti, ts, counts, img
        g = Guarded(self.image)
        ix, ti = d_index(np.full(cnt + 8, 0x77777777)), d_index(np.full(T + 8, 0x77777777))
        ps, ts = (torch.full((m + 24,), 77, dtype=torch.uint8, device="cuda") for m in (cnt, T))
        counts = eng.file_blocks(g.image, self.file, j0, cnt, ix[3:3 + cnt], ps[5:5 + cnt], ti[1:1 + T], ts[7:7 + T], counts=True,
                                 write_back=write_back)
        ix, ti, ps, ts = host(ix).view(np.uint32), host(ti).view(np.uint32), host(ps), host(ts)
        for a, lo, m, fill in ((ix, 3, cnt, 0x77777777), (ti, 1, T, 0x77777777), (ps, 5, cnt, 77), (ts, 7, T, 77)):
            assert (a[:lo] == fill).all() and (a[lo + m:] == fill).all(), "an output was written outside its array"
        return ix[3:3 + cnt], ps[5:5 + cnt], ti[1:1 + T], ts[7:7 + T], FileCounts(*counts.tolist()), g.result()

    def run_read(self, form, offset, nbytes, eng=None, write_back=True):
        """out (with 64 bytes past the clamped range), status, counts, image"""
        eng = eng or self.eng
        _, cnt, clamped = eng.file_span(self.file, offset, nbytes)
        if form == "host":
            img = self.image.copy()
            out, st = np.full(clamped + 64, 0x5A, np.uint8), np.full(cnt, 77, np.uint8)
            counts = eng.read_file_host(img, self.file, offset, nbytes, out, st, write_back=write_back)
            return out, st, counts, img
        g = Guarded(self.image)
        out = torch.full((7 + clamped + 64 + 32,), 0x5A, dtype=torch.uint8, device="cuda")
        st = torch.full((5 + cnt + 32,), 77, dtype=torch.uint8, device="cuda")
        counts = eng.read_file(g.image, self.file, offset, nbytes, out[7:7 + clamped + 64], st[5:5 + cnt], counts=True,
                               write_back=write_back)
        return self.finish_read(g, out, st, counts, cnt, clamped)

    @staticmethod
    def finish_read(g, out, st, counts, cnt, clamped):
        out, st = host(out), host(st)
        assert (out[:7] == 0x5A).all() and (out[7 + clamped:] == 0x5A).all(), "out written outside the clamped range"
        assert (st[:5] == 77).all() and (st[5 + cnt:] == 77).all(), "status written outside its array"
        return out[7:7 + clamped + 64], st[5:5 + cnt], FileCounts(*counts.tolist()), g.result()

    def check_blocks(self, form, j0, cnt, eng=None, write_back=True):
        e_ix, e_ps, e_ti, e_ts, e_counts, e_img = self.expect_blocks(j0, cnt, write_back)
        ix, ps, ti, ts, counts, img = self.run_blocks(form, j0, cnt, eng, write_back)
        tag = f"{self.cfg[0]} {form} blocks [{j0}, +{cnt})"
        assert np.array_equal(ti, e_ti) and np.array_equal(ts, e_ts), tag
        assert np.array_equal(ix, e_ix) and np.array_equal(ps, e_ps), tag
        assert counts == e_counts, (tag, counts, e_counts)
        assert np.array_equal(img, e_img), tag
        return e_ts, e_ps

    def check_read(self, form, offset, nbytes, eng=None, write_back=True):
        (_, cnt, clamped), e_out, e_st, e_counts, e_ts, e_img = self.read(offset, nbytes, write_back)
        eng_ = eng or self.eng
        assert eng_.file_span(self.file, offset, nbytes)[1:] == (cnt, clamped)
        out, st, counts, img = self.run_read(form, offset, nbytes, eng, write_back)
        tag = f"{self.cfg[0]} {form} read ({offset}, {nbytes})"
        assert np.array_equal(st, e_st), tag
        assert np.array_equal(out[:clamped], e_out) and (out[clamped:] == 0x5A).all(), tag
        assert counts == e_counts, (tag, counts, e_counts)
        assert np.array_equal(img, e_img), tag
        return e_st, e_ts


def block_ranges(n, I):
    """(first, count): the whole file, one block, a start in the middle of each segment, across every segment
    boundary, across a leaf and a mid-block boundary inside the trebly tree, the last block, nothing."""
    S1, S2 = 12 + I, 12 + I + I * I
    want = [(0, n), (5, 1), (3, 0), (4, 5), (11, 2), (12 + I // 2, 3), (S1 - 1, 2), (S1 + I * I // 2 + 1, I + 3), (S2 - 1, 2),
            (S2 + I // 2, 3), (S2 + I - 1, 2), (S2 + I * I - 1, 2), (S2 + I * I - I - 2, 2 * I + 5), (n - 1, 1), (7, n - 7)]
    return sorted({(a, c) for a, c in want if a >= 0 and c >= 0 and a + c <= n and (I or a + c <= 12)})


_images = {}


def image_of(oracle, name):
    if name not in _images:
        _images[name] = FileImage(oracle, name)
    return _images[name]


# ------------------------------------------------------------------------------------
# the walk and the read, device and host forms
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("name", NAMES)
def test_file_blocks(oracle, name, form):
    fi = image_of(oracle, name)
    corrected = 0
    for j0, cnt in block_ranges(fi.n, fi.I):
        ts, _ = fi.check_blocks(form, j0, cnt)
        corrected += int((ts == 1).sum())
        assert not ((ts == 5) | (ts == 9)).any()
    if fi.cfg[1] in (2, 4):
        assert corrected > 0  # every index block carried errors within the capability: status 1, written back


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("name", NAMES)
def test_read_file(oracle, name, form):
    fi = image_of(oracle, name)
    ds, size = fi.ds, int(fi.file["file_size"][0])
    seen = set()
    for j0, cnt in block_ranges(fi.n, fi.I):
        if cnt == 0:
            continue
        offset, nbytes = j0 * ds + min(3, ds - 1), max(1, cnt * ds - 5)  # starts and ends in mid-block
        if offset >= size:
            offset, nbytes = j0 * ds, size
        st, _ = fi.check_read(form, offset, nbytes)
        seen |= set(st.tolist())
    for offset, nbytes in ((0, size), (0, size + 1000), (7 * ds + ds // 2, 1), (size - 1, 1), (size - min(size, 10), 100), (5, 0),
                           (2 * ds, 3 * ds)):
        st, _ = fi.check_read(form, offset, nbytes)
        seen |= set(st.tolist())
    # RS reports 0 / 1 only (the reference's decode never gives 5); CRC and parity 0 / 5; Hamming all three
    assert seen == {4: {0, 1}, 2: {0, 1, 5}, 1: {0, 5}, 3: {0, 5}}[fi.cfg[1]]


def test_rs512_staged_list_path_gives_the_same(oracle, monkeypatch):
    fi = image_of(oracle, "rs512_t3")
    assert fi.eng.list_kernel_name() == "rs255-wg-list-lds"
    monkeypatch.setenv("PPFS_ECC_LIST_DIRECT", "0")
    staged = make_engine(fi.cfg)
    monkeypatch.delenv("PPFS_ECC_LIST_DIRECT")
    assert staged.list_kernel_name() == "gather-stage-scatter"
    size = int(fi.file["file_size"][0])
    fi.check_blocks("device", 0, fi.n, eng=staged)
    fi.check_read("device", 0, size, eng=staged)
    fi.check_read("device", 3 * fi.ds + 3, 4000 * fi.ds, eng=staged)


def test_write_back_off_writes_nothing(oracle):
    for name in ("rs64_t3", "hamming512"):
        fi = image_of(oracle, name)
        size = int(fi.file["file_size"][0])
        for form in ("device", "host"):
            *_, img = fi.run_blocks(form, 0, fi.n, write_back=False)
            assert np.array_equal(img, fi.image)
            fi.check_blocks(form, 0, fi.n, write_back=False)
            *_, img = fi.run_read(form, 0, size, write_back=False)
            assert np.array_equal(img, fi.image)
            fi.check_read(form, 0, size, write_back=False)


def test_crc_and_parity_images_are_untouched(oracle):
    for name in ("crc100_deg3", "parity3"):
        fi = image_of(oracle, name)
        for form in ("device", "host"):
            *_, img = fi.run_read(form, 0, int(fi.file["file_size"][0]))
            assert np.array_equal(img, fi.image)


def test_read_crosses_the_piece_size(oracle):
    """A file of one piece and 300 blocks: the device read runs in two pieces."""
    fi = FileImage(oracle, "rs512_t3", n=PIECE_BLOCKS + 300)
    size = int(fi.file["file_size"][0])
    fi.check_read("device", 5, size)
    fi.check_blocks("device", 1, fi.n - 1)


# ------------------------------------------------------------------------------------
# damage beyond the capability, pointers past the image
# ------------------------------------------------------------------------------------
LEVEL_IDS = {"singly-root": (1,), "doubly-root": (2,), "doubly-leaf": (2, 1), "trebly-root": (3,), "trebly-mid": (3, 0),
             "trebly-leaf": (3, 0, 1)}


def under(fi, node, j0, cnt):
    return np.array([path_of(j, fi.I)[:len(node)] == node for j in range(j0, j0 + cnt)])


# configuration, file blocks: the smallest file of that configuration that has every block of LEVEL_IDS it can have.
# Only codecs that can report a correction error: the reference's Reed-Solomon decode returns 0 or 1, never 5
# (rs_block_device.cpp:119-183), so an RS index block beyond the capability comes back "corrected" with a
# miscorrected payload, which test_read_file's data blocks with t + 1 and t + 2 byte errors already cover.
FAIL_FILES = {"crc100_deg3": 700, "hamming512": 400}
FAIL_CASES = [(name, where) for name in FAIL_FILES for where in LEVEL_IDS
              if not (name == "hamming512" and where.startswith("trebly"))]  # ipb 127: 400 blocks end in the doubly tree


@pytest.mark.parametrize("name,where", FAIL_CASES, ids=[f"{a}-{b}" for a, b in FAIL_CASES])
def test_failed_index_block(oracle, name, where):
    node, n = LEVEL_IDS[where], FAIL_FILES[name]
    fi = FileImage(oracle, name, n=n, fail=node)
    size = int(fi.file["file_size"][0])
    below = under(fi, node, 0, n)
    for form in ("device", "host"):
        ts, ps = fi.check_blocks(form, 0, n)
        t_below = np.array([i[:len(node)] == node for lv in tree_ids(0, n, fi.I) for i in lv])  # the block and what hangs on it
        assert (ts[t_below] == 5).all() and not (ts[~t_below] == 5).any()
        assert (ps[below] == 5).all() and (ps[~below] == 0).all()
        st, _ = fi.check_read(form, 0, size)
        assert (st[below] == 5).all()
        out, *_ = fi.run_read(form, 0, size)
        k = int(np.nonzero(below)[0][0])
        assert not out[k * fi.ds:min((k + 1) * fi.ds, size)].any()  # zero-filled like a failed read


@pytest.mark.parametrize("where", list(LEVEL_IDS) + ["data"])
def test_pointer_past_the_image(oracle, where):
    n = 260
    node = LEVEL_IDS.get(where, ("data", 100))
    fi = FileImage(oracle, "rs64_t3", n=n, oob=node)
    size = int(fi.file["file_size"][0])
    for form in ("device", "host"):
        ts, ps = fi.check_blocks(form, 0, n)
        st, _ = fi.check_read(form, 0, size)
        if where == "data":
            assert not ps.any() and st[100] == 9 and (st == 9).sum() == 1
        else:
            below = under(fi, node, 0, n)
            assert below.any() and (ts == 9).sum() >= 1 and (ps[below] == 9).all() and (ps[~below] == 0).all()
            assert (st[below] == 9).all()


def test_duplicated_pointer_is_memory_safe(oracle):
    """File blocks 20 and 200 name the same clean image block: guards intact, both copies read the same payload."""
    fi = FileImage(oracle, "rs64_t3", n=260, dup=(20, 200), damage_data=False)
    ds, size = fi.ds, int(fi.file["file_size"][0])
    for form in ("device", "host"):
        out, st, _, _ = fi.run_read(form, 0, size)
        assert st[20] == 0 and st[200] == 0
        assert np.array_equal(out[20 * ds:21 * ds], out[200 * ds:201 * ds])
        assert np.array_equal(out[20 * ds:21 * ds], fi.payload[fi.data_blk[20]])
        ix, *_ = fi.run_blocks(form, 0, fi.n)
        assert ix[20] == ix[200] == fi.data_blk[20]


# ------------------------------------------------------------------------------------
# arguments, NULL outputs, streams
# ------------------------------------------------------------------------------------
def test_span_tree_blocks_and_refusals(oracle):
    fi = image_of(oracle, "rs64_t3")
    eng, f, ds, I, n = fi.eng, fi.file, fi.ds, fi.I, fi.n
    size = int(f["file_size"][0])
    assert (ds, I) == (58, 14)
    assert eng.file_span(f, 0, size) == (0, n, size)
    assert eng.file_span(f, 0, 10 ** 12) == (0, n, size)
    assert eng.file_span(f, 57, 2) == (0, 2, 2) and eng.file_span(f, 58, 58) == (1, 1, 58) and eng.file_span(f, 59, 58) == (1, 2, 58)
    assert eng.file_span(f, size - 1, 5) == (n - 1, 1, 1) and eng.file_span(f, 123, 0) == (0, 0, 0)
    assert eng.file_tree_blocks(f, 0, 12) == 0 and eng.file_tree_blocks(f, 0, 13) == 1 and eng.file_tree_blocks(f, 12, 14) == 1
    assert eng.file_tree_blocks(f, 25, 2) == 3  # the last singly block and the first doubly one: two roots, one leaf
    assert eng.file_tree_blocks(f, 0, n) == sum(len(lv) for lv in tree_ids(0, n, I))
    assert eng.file_tree_blocks(f, 221, 2) == 2 + 2 + 1  # the last doubly and the first trebly block
    img = np.zeros(8 * fi.raw, np.uint8)
    out = np.zeros(64, np.uint8)
    for call in (lambda: eng.file_span(f, size, 1), lambda: eng.file_span(f, size + 5, 1),
                 lambda: eng.file_tree_blocks(f, n, 1), lambda: eng.file_tree_blocks(f, 0, n + 1),
                 lambda: eng.file_blocks_host(img, f, n - 1, 2), lambda: eng.read_file_host(img, f, size, 1, out)):
        with pytest.raises(EccError) as e:
            call()
        assert e.value.code == -22
    big = f.copy()
    big["file_size"] = 0xFFFFFFFF  # occupies more blocks than the tree of 2,966 holds
    assert eng.file_tree_blocks(big, 0, 2966) > 0
    for call in (lambda: eng.file_tree_blocks(big, 2966, 1), lambda: eng.file_span(big, 2965 * ds, 2 * ds)):
        with pytest.raises(EccError) as e:
            call()
        assert e.value.code == -22
    tiny = image_of(oracle, "parity3")  # dataSize() 2: no index entry fits a block
    tf = tiny.file.copy()
    tf["file_size"] = 100
    assert tiny.eng.file_tree_blocks(tf, 0, 12) == 0
    with pytest.raises(EccError) as e:
        tiny.eng.file_tree_blocks(tf, 0, 13)
    assert e.value.code == -22
    assert eng.read_file_host(img, f, 5, 0, None) == FileCounts(0, 0, 0, 0, 0, 0, 0, 0)
    assert eng.file_blocks_host(img, f, 5, 0) == FileCounts(0, 0, 0, 0, 0, 0, 0, 0)


def test_null_outputs_in_every_combination(oracle):
    fi = image_of(oracle, "rs64_t3")
    eng, f, j0, cnt = fi.eng, fi.file, 7, 300
    e_ix, e_ps, e_ti, e_ts, e_counts, e_img = fi.expect_blocks(j0, cnt)
    T = e_ti.size
    for mask in range(32):
        g = Guarded(fi.image)
        ix = d_index(np.zeros(cnt)) if mask & 1 else None
        ps = torch.zeros(cnt, dtype=torch.uint8, device="cuda") if mask & 2 else None
        ti = d_index(np.zeros(T)) if mask & 4 else None
        ts = torch.zeros(T, dtype=torch.uint8, device="cuda") if mask & 8 else None
        counts = eng.file_blocks(g.image, f, j0, cnt, ix, ps, ti, ts, counts=bool(mask & 16))
        assert np.array_equal(g.result(), e_img), mask
        for got, want in ((ix, e_ix), (ps, e_ps), (ti, e_ti), (ts, e_ts)):
            if got is not None:
                got = host(got)
                assert np.array_equal(got.view(np.uint32) if got.dtype == np.int32 else got, want), mask
        if counts is not None:
            assert FileCounts(*counts.tolist()) == e_counts, mask
    size = int(f["file_size"][0])
    (_, rc, clamped), e_out, e_st, e_counts, _, e_img = fi.read(9, size)
    for mask in range(4):
        g = Guarded(fi.image)
        out = torch.zeros(clamped, dtype=torch.uint8, device="cuda")
        st = torch.zeros(rc, dtype=torch.uint8, device="cuda") if mask & 1 else None
        counts = eng.read_file(g.image, f, 9, size, out, st, counts=bool(mask & 2))
        assert np.array_equal(g.result(), e_img), mask
        keep = np.repeat(e_st != 9, fi.ds)[9:9 + clamped]
        assert np.array_equal(host(out)[keep], e_out[keep]), mask
        if st is not None:
            assert np.array_equal(host(st), e_st), mask
        if counts is not None:
            assert FileCounts(*counts.tolist()) == e_counts, mask
    # host forms with nothing but the counts
    assert eng.file_blocks_host(fi.image.copy(), f, j0, cnt) == fi.expect_blocks(j0, cnt)[4]


def test_file_calls_refuse_a_capturing_stream(oracle):
    fi = image_of(oracle, "rs64_t3")
    eng, f = fi.eng, fi.file
    image = torch.from_numpy(fi.clean).cuda()
    ix = d_index(np.zeros(40))
    out = torch.zeros(40 * fi.ds, dtype=torch.uint8, device="cuda")
    eng.file_blocks(image, f, 0, 40, ix)  # whatever the calls set up exists before the capture
    eng.read_file(image, f, 0, 40 * fi.ds, out)
    torch.cuda.synchronize()
    codes = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # captured and never replayed
        for call in (lambda: eng.file_blocks(image, f, 0, 40, ix), lambda: eng.read_file(image, f, 0, 40 * fi.ds, out)):
            try:
                call()
                codes.append(0)
            except EccError as e:
                codes.append(e.code)
    assert codes == [-95, -95]  # PPFS_ECC_ENOTSUP


def test_two_reads_of_one_context_on_two_streams(oracle):
    fi = image_of(oracle, "rs64_t3")
    size = int(fi.file["file_size"][0])
    reads = [(3, size), (30 * fi.ds + 7, 200 * fi.ds)]
    expect = [fi.read(o, nb) for o, nb in reads]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = []
    for (_, cnt, clamped), *_ in expect:
        bufs.append((Guarded(fi.image), torch.full((7 + clamped + 64 + 32,), 0x5A, dtype=torch.uint8, device="cuda"),
                     torch.full((5 + cnt + 32,), 77, dtype=torch.uint8, device="cuda"),
                     torch.zeros(8, dtype=torch.int64, device="cuda"), cnt, clamped))
    torch.cuda.synchronize()  # the buffers were filled on the default stream
    for (o, nb), s, (g, out, st, counts, cnt, clamped) in zip(reads, streams, bufs):
        fi.eng.read_file(g.image, fi.file, o, nb, out[7:7 + clamped + 64], st[5:5 + cnt], counts=counts, stream=s)
    torch.cuda.synchronize()
    for b, ((_, cnt, clamped), e_out, e_st, e_counts, _, e_img) in zip(bufs, expect):
        out, st, counts, img = fi.finish_read(*b)
        assert np.array_equal(out[:clamped], e_out) and np.array_equal(st, e_st) and counts == e_counts
        assert np.array_equal(img, e_img)


def test_single_file_calls_between_two_batches_on_one_stream(oracle):
    """read_files, read_file, write_file and read_files again on one stream with nothing in between.  The single-file
    calls run the batch's walk in the same scratch, their record in the kernel arguments where a batch has tables: they
    must neither disturb a batch's tables nor depend on them.  rs64_t3 (ds 58, ipb 14), one file of 12 + 14 + 3 blocks
    (levels A and B), one flipped byte in the doubly root, which the first call corrects and writes back.  Every
    result against the oracle's walk (the reads) and the per-block loop over its device model (the write)."""
    from tests.test_gpu_file_write import Img
    from tests.test_gpu_files import bits

    fi = FileImage(oracle, "rs64_t3", n=12 + 14 + 3, damage_data=False)
    ds, size, f = fi.ds, int(fi.file["file_size"][0]), fi.file
    assert (ds, fi.I) == (58, 14) and [len(lv) for lv in tree_ids(0, fi.n, fi.I)] == [2, 1, 0]
    start = fi.clean.copy()
    start.reshape(fi.blocks, fi.raw)[fi.node_blk[(2,)], 9] ^= 0x5A
    batch = [(0, size), (0, 5 * ds)]  # the file, and its first 5 blocks: no tree
    files, ranges = np.concatenate([f, f]), np.array(batch, np.uint64)
    one = (13 * ds + 5, 12 * ds)  # through both roots and the leaf
    w_off, w_bytes = 20 * ds + 7, 6 * ds + 11  # from the singly into the doubly tree, mid-block at both ends
    data = rng_for("between").integers(0, 256, w_bytes, dtype=np.uint8)

    def expect_batch(image):
        """out, status, flags, counts, the image afterwards of the batch on `image`"""
        fi.image = image
        per = [fi.read(o, nb) for o, nb in batch]
        assert np.array_equal(per[1][5], image)  # five clean direct blocks: nothing to write back
        counts = FileCounts(*np.sum([list(p[3]) for p in per], axis=0).tolist())
        flags = np.array([bits(p[2]) | bits(p[4]) << 8 for p in per], np.uint32)
        return np.concatenate([p[1] for p in per]), np.concatenate([p[2] for p in per]), flags, counts, per[0][5]

    e1 = expect_batch(start)
    assert e1[3].index_corrected == 1 and e1[2].tolist() == [1 << 8, 0] and np.array_equal(e1[4], fi.clean)
    fi.image = e1[4]
    (_, one_cnt, one_bytes), e2_out, e2_st, e2_counts, _, e2_img = fi.read(*one)
    assert np.array_equal(e2_img, e1[4])
    e3 = Img(fi).loop([0], [(w_off, w_bytes)], data)
    assert int(e3["written"][0]) == w_bytes and not np.array_equal(e3["image"], e2_img)
    e4 = expect_batch(e3["image"])
    assert e4[3].index_corrected == 0 and not np.array_equal(e4[0], e1[0])

    g = Guarded(start)
    nb, nbytes = fi.n + 5, size + 5 * ds
    outs = [torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(2)]
    sts = [torch.full((nb,), 77, dtype=torch.uint8, device="cuda") for _ in range(2)]
    fls = [d_index(np.full(2, 0x77777777)) for _ in range(2)]
    out2 = torch.full((one_bytes,), 0x5A, dtype=torch.uint8, device="cuda")
    st2 = torch.full((one_cnt,), 77, dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(data).cuda()
    st3 = torch.full((e3["st"].size,), 77, dtype=torch.uint8, device="cuda")
    wr = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    cn = [torch.full((8,), -1, dtype=torch.int64, device="cuda") for _ in range(4)]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()  # the buffers were filled on the default stream
    fi.eng.read_files(g.image, files, ranges, outs[0], sts[0], fls[0], counts=cn[0], stream=s)
    fi.eng.read_file(g.image, f, *one, out2, st2, counts=cn[1], stream=s)
    fi.eng.write_file(src, g.image, f, w_off, w_bytes, st3, written=wr, counts=cn[2], stream=s)
    fi.eng.read_files(g.image, files, ranges, outs[1], sts[1], fls[1], counts=cn[3], stream=s)
    torch.cuda.synchronize()
    for k, e in ((0, e1), (1, e4)):
        assert np.array_equal(host(outs[k]), e[0]) and np.array_equal(host(sts[k]), e[1]), k
        assert np.array_equal(host(fls[k]).view(np.uint32), e[2]) and FileCounts(*cn[3 * k].tolist()) == e[3], k
    assert np.array_equal(host(out2), e2_out) and np.array_equal(host(st2), e2_st) and FileCounts(*cn[1].tolist()) == e2_counts
    assert np.array_equal(host(st3), e3["st"]) and int(wr[0]) == w_bytes and FileCounts(*cn[2].tolist()) == e3["counts"]
    assert np.array_equal(g.result(), e4[4]) and np.array_equal(e4[4], e3["image"])


def test_batch_built_image_equals_per_block_writes(oracle):
    """The images above come from the oracle's batch encode; the reference writes an index block's entries at
    {block, 0} of a zeroed block and a data block whole.  Both give the same bytes."""
    for name in ("rs64_t3", "hamming512", "crc100_deg3", "parity3"):
        fi = FileImage(oracle, name, n=min(CFG[name][5], 40), damage_data=False)
        _, typ, bs, t, poly, _ = fi.cfg
        od = OracleDevice(oracle, typ, bs, t, poly, fi.blocks * fi.raw)
        nodes = set(fi.node_blk.values())
        for b in range(fi.blocks):
            data = fi.payload[b, :4 * fi.I] if b in nodes else fi.payload[b]
            assert od.write(b, 0, data.tobytes())[0] == 0
        assert np.array_equal(od.disk[:fi.blocks * fi.raw], fi.clean)


# ------------------------------------------------------------------------------------
# the block-device mirror: the engine overrides against the per-block loops, which are the definition
# ------------------------------------------------------------------------------------
def mirror_device(fi):
    _, typ, bs, t, poly, _ = fi.cfg
    disk, logger = HeapDisk(fi.image.size), Logger()
    disk.buf[:] = fi.image
    return create_block_device(disk, bs, ECCType(typ), crc_polynomial_explicit=poly, rs_correctable_bytes=t, logger=logger), disk, logger


# configuration, file blocks, failing index block, pointer past the image: rs64_t3 is a shortened code, whose device
# keeps the per-block loop
MIRROR = [("rs512_t3", 150, None, None), ("hamming512", 300, None, None), ("crc100_deg3", 700, None, None),
          ("rs64_t3", 260, None, None), ("crc100_deg3", 700, (2, 1), None), ("hamming512", 300, (2,), None),
          ("rs512_t3", 150, None, (2, 0)), ("hamming512", 300, None, ("data", 170))]


@pytest.mark.parametrize("name,n,fail,oob", MIRROR, ids=[f"{a}-{b}-fail{c}-oob{d}" for a, b, c, d in MIRROR])
def test_block_device_file_calls_match_the_per_block_loops(oracle, name, n, fail, oob):
    fi = FileImage(oracle, name, n=n, fail=fail, oob=oob)
    ds, size = fi.ds, int(fi.file["file_size"][0])
    before = fi.image.reshape(fi.blocks, fi.raw)
    calls = [("file_blocks", (0, n)), ("file_blocks", (9, n - 20)), ("read_file", (0, size)), ("read_file", (7 * ds + 3, 100 * ds)),
             ("read_file", (size - 5, 50)), ("read_file", (size, 1)), ("file_blocks", (n - 1, 2)), ("read_file", (3, 0))]
    failures = 0
    for method, args in calls:
        dev, disk, logger = mirror_device(fi)
        ref, ref_disk, ref_logger = mirror_device(fi)
        got, got_err = getattr(dev, method)(fi.file, *args)
        want, want_err = getattr(IBlockDevice, method)(ref, fi.file, *args)  # the per-block loop
        tag = (name, method, args)
        assert got_err == want_err, tag
        assert np.array_equal(np.frombuffer(got, np.uint8) if method == "read_file" else got,
                              np.frombuffer(want, np.uint8) if method == "read_file" else want), tag
        a, b = disk.buf.reshape(fi.blocks, fi.raw), ref_disk.buf.reshape(fi.blocks, fi.raw)
        if want_err is None:
            assert logger.corrections == ref_logger.corrections, tag
            assert np.array_equal(a, b), tag
        else:  # everything up to the failing block; the engine may have corrected and logged blocks after it
            failures += 1
            assert logger.corrections[:len(ref_logger.corrections)] == ref_logger.corrections, tag
            touched = np.nonzero((b != before).any(axis=1))[0]
            assert np.array_equal(a[touched], b[touched]), tag
    assert failures >= (3 if fail or oob else 2)  # two of the calls are refused for their range alone
