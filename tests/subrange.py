"""Sub-range calls of the contiguous device entry points, framed in guard bytes -- TEST ONLY (numpy
and the oracle; the device side of a frame imports torch where it is used).

"Decode blocks [first, first + count) of a device image into slots first.. of a packed payload
buffer" is raw + first * raw_size, data + first * data_size, status + first: pointers of any
alignment, neighbours on both sides that the call must leave alone.  This module builds such calls:

  Frame      one buffer of a case as a view into its own allocation [256 guard | skew | n | 256 guard],
             guards and skew bytes seeded random, and the comparison of the whole allocation afterwards
  Case       the inputs of one (code, first, count) and everything the oracle says about them
  rejects    the pointer rule of include/ppfs_ecc.h ("Pointers" in INTEGRATION.md) as a predicate
  run_call   one engine call on the sub-range of freshly uploaded frames, checked byte for byte

A code is (codec, parameter, block size) as in tests/bit_craft.py: ("ham", 0, bs), ("crc", implicit
polynomial, bs), ("par", 0, bs) and ("rs", correctable bytes, bs).

Faults are dealt by block number, counted from the first block of the range so that every batch
starts a full turn of the deal and holds each status the codec can report (block b of the image gets
class (b - first) mod m; the rows outside the range carry the same deal and must come back as
uploaded):
  Hamming      m = 4: clean, one flip of a used bit (status 1), two flips of used bits (5), one tail bit (0)
  CRC, parity  m = 4: classes 0-2 clean, class 3 one flipped payload bit (5)
  RS           m = t + 2: that many byte errors (0 clean, 1 corrected; t + 1 errors: whatever the oracle says)
A block the oracle rejects (status 5) has no defined payload: its payload row is left out of the
comparison, its raw row and status are not.  At most 30 % of a batch may be left out
(tests/test_subrange_cpu.py).
"""
from __future__ import annotations

import functools
import zlib

import numpy as np

from tests import bit_craft

GUARD = 256
N = 80
SKEWS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 3), (3, 5, 1), (4, 8, 2), (8, 4, 0), (15, 15, 15)]  # raw, data, status
RANGES = [(0, 1), (3, 5), (0, 67), (13, 67)]  # (first, count); 67: more than one workgroup of every bit kernel, ragged
CALLS = ("encode", "decode", "decode-status-only", "decode-no-status", "write", "write-no-status")

CRC62 = 0x42F0E1EBA9EA3693 >> 1  # the degree-62 polynomial of test_gpu_parity.CRC_CASES
# 1, 2 and 4 KiB: the streaming kernels for 16-byte aligned payload and raw pointers, else the generic ones
STREAMING = [("ham", 0, 1024), ("ham", 0, 4096), ("crc", 0x9960034c, 1024), ("crc", 0x9960034c, 4096),
             ("crc", 0xc1acf, 2048), ("par", 0, 1024), ("par", 0, 4096)]
GENERIC = [("ham", 0, 64), ("ham", 0, 512), ("ham", 0, 4), ("crc", 0xea, 256), ("crc", CRC62, 1024), ("par", 0, 255),
           ("par", 0, 256)]
RS_GENERIC = [("rs", 3, 64), ("rs", 10, 128), ("rs", 9, 255)]
RS_FAST = [("rs", 3, 512), ("rs", 5, 1024), ("rs", 16, 4096)]
RS_FAST_N, RS_FAST_RANGE = 100, (16, 67)  # first = 16: all three offsets are multiples of 16
KERNEL_NAMES = {("ham", True): ("hamming-stream-wave",), ("crc", True): ("crc-piecemap-wave",),
                ("par", True): ("parity-stream-wave",), ("ham", False): ("hamming-funnel", "hamming-tiny"),
                ("crc", False): ("crc-nibble-shift",), ("par", False): ("parity-popcount",)}
# the statuses a batch of >= 5 blocks must hold
DEAL_STATUSES = {"ham": {0, 1, 5}, "crc": {0, 5}, "par": {0, 5}, "rs": {0, 1}}
EINVAL = -22


def code_id(c):
    return f"{c[0]}-{c[2]}-{c[1]:x}" if c[0] == "crc" else (f"rs-{c[2]}-t{c[1]}" if c[0] == "rs" else f"{c[0]}-{c[2]}")


def skew_id(s):
    return "skew-%d-%d-%d" % s


def rng_for(*k):
    return np.random.default_rng(zlib.crc32(repr(k).encode()))


# ------------------------------------------------------------------------------------
# the frame
# ------------------------------------------------------------------------------------
class Frame:
    """n bytes at [GUARD + skew, +n) of an allocation of GUARD + skew + n + GUARD seeded random bytes."""

    def __init__(self, name, content, skew, rng):
        content = np.ascontiguousarray(content, np.uint8).reshape(-1)
        self.name, self.skew, self.n = name, int(skew), int(content.size)
        self.off = GUARD + self.skew
        self.host = rng.integers(0, 256, self.off + self.n + GUARD, dtype=np.uint8)
        self.host[self.off:self.off + self.n] = content
        self.dev = self.view = None

    def address(self, base, at=0):
        """Address of byte `at` of the view in an allocation at `base`."""
        return base + self.off + at

    def upload(self):
        import torch

        self.dev = torch.from_numpy(self.host.copy()).cuda()
        self.view = self.dev[self.off:self.off + self.n]
        assert self.dev.data_ptr() % 256 == 0, (self.name, "allocation base", self.dev.data_ptr() % 256)
        assert self.view.data_ptr() == self.address(self.dev.data_ptr())
        assert self.view.data_ptr() % 16 == self.skew % 16, (self.name, self.view.data_ptr() % 16, self.skew)
        return self

    def sub(self, first, row):
        """The pointer of a sub-range call: the view from row `first` on.  Its range ends GUARD bytes before
        the end of the allocation at the closest."""
        t = self.view[first * row:]
        assert t.data_ptr() + t.numel() + GUARD <= self.dev.data_ptr() + self.dev.numel()
        return t

    def expected(self, first, count, row, rows=None, defined=None):
        """(the whole allocation as it must read back, the mask of the bytes that are compared): as uploaded,
        rows [first, first + count) replaced by `rows` (None: unchanged); defined: per row of the range,
        False leaves the row out of the comparison."""
        exp, mask = self.host.copy(), np.ones(self.host.size, bool)
        a = self.off + first * row
        if rows is not None:
            exp[a:a + count * row] = np.asarray(rows, np.uint8).reshape(-1)
        if defined is not None:
            mask[a:a + count * row] = np.repeat(np.asarray(defined, bool), row)
        return exp, mask

    def mismatch(self, got, exp, mask, first, count, row):
        """None, or (what, offset relative to the view, got, expected) of the first differing byte."""
        bad = np.flatnonzero((np.asarray(got) != exp) & mask)
        if not bad.size:
            return None
        i = int(bad[0])
        rel = i - self.off
        if rel < 0 or rel >= self.n:
            what = "guard/skew"
        elif first * row <= rel < (first + count) * row:
            what = f"range row {rel // row if row else 0}"
        else:
            what = f"neighbour row {rel // row if row else 0}"
        return what, rel, int(got[i]), int(exp[i])

    def download(self):
        import torch

        torch.cuda.synchronize()
        return self.dev.cpu().numpy()


# ------------------------------------------------------------------------------------
# codecs through the oracle
# ------------------------------------------------------------------------------------
def sizes(oracle, code):
    """(raw row bytes, payload row bytes, spill row bytes or 0)."""
    codec, par, bs = code
    if codec == "rs":
        n, k, _ = oracle.rs_sizes(bs, par)
        return n, k, 256 - n
    if codec == "ham":
        return bs, oracle.ham_data_size(bs), 0
    if codec == "crc":
        return bs, oracle.crc_data_size(bs, oracle.crc_explicit(par)), 0
    return bs, bs - 1, 0


def o_encode(oracle, code, data, old):
    codec, par, bs = code
    if codec == "rs":
        return oracle.rs_encode(bs, par, data)
    if codec == "ham":
        return oracle.ham_encode(bs, data, raw_old=old)
    if codec == "crc":
        return oracle.crc_encode(bs, oracle.crc_explicit(par), data, raw_old=old)
    return oracle.parity_encode(bs, data, raw_old=old)


def o_decode(oracle, code, raw):
    """(payloads, statuses, the image after write-back)."""
    codec, par, bs = code
    if codec == "rs":
        data, st, fixed, _, rc = oracle.rs_decode(bs, par, raw)
        assert rc == 0
        return data, st, fixed
    if codec == "ham":
        data, st, fixed, _ = oracle.ham_decode(bs, raw)
        return data, st, fixed
    if codec == "crc":
        data, st = oracle.crc_check(bs, oracle.crc_explicit(par), raw)
    else:
        data, st = oracle.parity_check(bs, raw)
    return data, st, np.array(raw, np.uint8, copy=True)


def deal(code, first, nblocks):
    """Class of every block of the image."""
    m = code[1] + 2 if code[0] == "rs" else 4
    return (np.arange(nblocks) - first) % m


def inject(code, rng, image, classes, row, ds):
    """The image with each block's class of faults."""
    codec, par, bs = code
    img = image.reshape(classes.size, row).copy()

    def flip(b, q):
        img[b, q // 8] ^= 0x80 >> (q % 8)

    lay = bit_craft.ham_layout(bs) if codec == "ham" else None
    for b, c in enumerate(classes):
        if codec == "rs":
            pos = rng.choice(row, int(c), replace=False)
            img[b, pos] ^= rng.integers(1, 256, pos.size, dtype=np.uint8)
        elif codec == "ham":
            if c == 1 or c == 2:
                for q in rng.choice(lay.used, int(c), replace=False):
                    flip(b, int(q))
            elif c == 3:
                flip(b, int(rng.choice(lay.tail)))
        elif c == 3:
            flip(b, int(rng.integers(0, 8 * ds)))
    return img.reshape(-1)


class Case:
    """One image of `nblocks` blocks with the range [first, first + count) and the oracle's results."""

    def __init__(self, oracle, code, first, count, nblocks=N):
        assert 0 <= first and count >= 1 and first + count <= nblocks
        self.code, self.first, self.count, self.nblocks = code, first, count, nblocks
        self.row, self.ds, self.spill_row = sizes(oracle, code)
        row, ds = self.row, self.ds
        rng = rng_for("subrange", code, first, count, nblocks)
        self.classes = deal(code, first, nblocks)
        self.payload = rng.integers(0, 256, nblocks * ds, dtype=np.uint8)
        self.noise = rng.integers(0, 256, nblocks * row, dtype=np.uint8)  # the old image of an encode
        self.new = rng.integers(0, 256, nblocks * ds, dtype=np.uint8)     # what encode and write store
        self.image = inject(code, rng, o_encode(oracle, code, self.payload, self.noise), self.classes, row, ds)
        for a in (self.payload, self.noise, self.new, self.image):
            a.setflags(write=False)
        r = slice(first, first + count)
        rows = lambda a, w: np.asarray(a).reshape(nblocks, w)[r]  # noqa: E731
        data, st, fixed = o_decode(oracle, code, self.image)
        self.st = st[r].copy()
        self.defined = self.st != 5
        self.data = rows(data, ds).copy()
        self.fixed = rows(fixed, row).copy()
        self.encoded = rows(o_encode(oracle, code, self.new, self.noise), row).copy()
        if code[0] == "rs":  # the new codeword whatever the old block's status (rs_block_device.cpp:61-93)
            self.written = rows(o_encode(oracle, code, self.new, None), row).copy()
        else:  # a rejected block stays, else the new payload over the corrected old block
            over = rows(o_encode(oracle, code, self.new, fixed), row)
            self.written = np.where((self.st == 5)[:, None], rows(self.image, row), over)
        self.spill = None
        if self.spill_row and code in RS_GENERIC:  # [bytes past the block, those bytes, zeros]
            self.spill = np.zeros((count, self.spill_row), np.uint8)
            img = self.image.reshape(nblocks, row)
            for i in range(count):
                _, _, full, wl, _ = oracle.rs_decode_one_full(code[2], code[1], img[first + i])
                extra = max(0, wl - row)
                self.spill[i, 0] = extra
                self.spill[i, 1:1 + extra] = full[row:row + extra]

    def left_out(self):
        """Fraction of the batch without a defined payload."""
        return float((~self.defined).sum()) / self.count


@functools.lru_cache(maxsize=None)
def _case(oracle, code, first, count, nblocks):
    return Case(oracle, code, first, count, nblocks)


def case(oracle, code, first, count, nblocks=N):
    """Computed once and shared: nothing in a Case is written afterwards."""
    return _case(oracle, code, first, count, nblocks)


def all_cases():
    """(code, first, count, nblocks) of every case of tests/test_gpu_subrange.py."""
    out = [(c, f, n, N) for c in STREAMING + GENERIC + RS_GENERIC for f, n in RANGES]
    return out + [(c, RS_FAST_RANGE[0], RS_FAST_RANGE[1], RS_FAST_N) for c in RS_FAST]


# ------------------------------------------------------------------------------------
# the pointer rule
# ------------------------------------------------------------------------------------
def uses(call):
    """(data, status) pointers the call passes."""
    return call not in ("decode-status-only",), call in ("decode", "decode-status-only", "write")


def rejects(code, call, raw_ptr, data_ptr, status_ptr, rs_fast=None):
    """The documented rule: True where the call must return PPFS_ECC_EINVAL with nothing written.
    RS fast paths: raw, and the payload and status pointers the call passes, 16-byte aligned (the
    write call: its decode's and its encode's rule); Hamming blocks >= 8 bytes: raw 16-byte aligned;
    everything else: any address."""
    codec, _, bs = code
    has_data, has_status = uses(call)
    if codec == "rs":
        fast = (code in RS_FAST) if rs_fast is None else rs_fast
        if not fast:
            return False
        return raw_ptr % 16 != 0 or (has_data and data_ptr % 16 != 0) or (has_status and status_ptr % 16 != 0)
    if codec == "ham":
        return bs >= 8 and raw_ptr % 16 != 0
    return False


# ------------------------------------------------------------------------------------
# one call
# ------------------------------------------------------------------------------------
def frames(cs, call, skews, tag):
    """Fresh frames of a call: raw (the old image), data, status, spill (None where the case has none)."""
    rng = rng_for("frames", cs.code, cs.first, cs.count, call, skews, tag)
    sr, sd, ss = skews
    old = cs.noise if call == "encode" else cs.image
    if call in ("encode", "write", "write-no-status"):
        data = cs.new
    else:
        data = rng.integers(0, 256, cs.nblocks * cs.ds, dtype=np.uint8)
    f = {"raw": Frame("raw", old, sr, rng), "data": Frame("data", data, sd, rng),
         "status": Frame("status", rng.integers(0, 256, cs.nblocks, dtype=np.uint8), ss, rng), "spill": None}
    if cs.spill is not None:
        f["spill"] = Frame("spill", rng.integers(0, 256, cs.nblocks * cs.spill_row, dtype=np.uint8), ss, rng)
    return f


def expectations(cs, call, fr, rejected):
    """{buffer: (expected allocation, mask, row bytes)} after the call."""
    f, n = cs.first, cs.count
    raw = data = status = spill = None
    dfn = None
    if not rejected:
        if call == "encode":
            raw = cs.encoded
        elif call == "decode":  # payload, status, write-back (and the spill of a shortened RS code)
            raw, data, status, dfn, spill = cs.fixed, cs.data, cs.st, cs.defined, cs.spill
        elif call == "decode-status-only":  # with write-back
            raw, status = cs.fixed, cs.st
        elif call == "decode-no-status":  # payload only, no write-back: the image stays
            data, dfn = cs.data, cs.defined
        elif call == "write":
            raw, status = cs.written, cs.st
        else:
            raw = cs.written
    out = {"raw": fr["raw"].expected(f, n, cs.row, raw) + (cs.row,),
           "data": fr["data"].expected(f, n, cs.ds, data, dfn) + (cs.ds,),
           "status": fr["status"].expected(f, n, 1, status) + (1,)}
    if fr["spill"] is not None:
        out["spill"] = fr["spill"].expected(f, n, cs.spill_row, spill) + (cs.spill_row,)
    return out


def run_call(eng, cs, call, skews, tag=""):
    """Upload fresh frames, make the call on the sub-range, read the whole allocations back and compare.
    Returns whether the call was (rightly) refused."""
    from paritypartyfs_amd._native import EccError

    fr = frames(cs, call, skews, tag)
    for x in fr.values():
        if x is not None:
            x.upload()
    f, n = cs.first, cs.count
    raw, data, status = fr["raw"].sub(f, cs.row), fr["data"].sub(f, cs.ds), fr["status"].sub(f, 1)
    spill = fr["spill"].sub(f, cs.spill_row) if fr["spill"] is not None else None
    rejected = rejects(cs.code, call, raw.data_ptr(), data.data_ptr(), status.data_ptr(),
                       rs_fast=eng.kernel_name != "rs-generic-lfsr" if cs.code[0] == "rs" else None)
    where = (code_id(cs.code), call, skew_id(skews), "first", f, "count", n, tag)
    try:
        if call == "encode":
            eng.encode(data, raw, nblocks=n)
        elif call == "decode":
            eng.decode(raw, data, status, write_back=True, spill=spill, nblocks=n)
        elif call == "decode-status-only":
            eng.decode(raw, None, status, write_back=True, nblocks=n)
        elif call == "decode-no-status":
            eng.decode(raw, data, None, write_back=False, nblocks=n)
        elif call == "write":
            eng.write(data, raw, status, nblocks=n)
        else:
            eng.write(data, raw, None, nblocks=n)
        assert not rejected, (where, "accepted pointers the documented rule forbids")
    except EccError as e:
        assert rejected and e.code == EINVAL, (where, "refused", e.code, str(e))
    for name, (exp, mask, row) in expectations(cs, call, fr, rejected).items():
        bad = fr[name].mismatch(fr[name].download(), exp, mask, f, n, row)
        assert bad is None, (where, name, "rejected" if rejected else "ran",
                             "%s: offset %d of the view reads %#x, expected %#x" % bad)
    return rejected
