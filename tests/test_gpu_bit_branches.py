"""GPU tests of every Hamming, CRC and parity decode branch against the CPU oracle, bit-exact.

The other tests of the bit codecs flip bits drawn uniformly over the block, which at 1-4 KiB almost
never lands where the kernels have special code: a Hamming syndrome of 0 (bit 0 is the bad one), a
power of two, L, or a position in another 1 KiB row; the owner lane, LDS word and byte of the
correction with a payload output and the separate in-place patch without one; payload extraction
with the corrected bit among the interleaved parity positions of the head; a miscorrection into the
unused tail and the write that must keep that bit; flips of tail bits, which are ignored; four flips
that cancel; the kept bits behind a CRC field, the 16-byte and 1 KiB boundaries of the CRC streaming
kernel, multiples of the polynomial up to the reference's last undetected offset; the parity byte
and its fix bit.  Here the flips are aimed (tests/bit_craft.py; tests/test_bit_craft.py pins the
classes each code's set holds and what they mean in the oracle) and go through every decode entry:
the device calls with and without a payload output, the write call, the resident server, the
chunked host pipeline and the block-list call.  Each set runs as two batches of a ragged count
above 64: classes dealt round-robin, and sorted by class.  A block of status 5 has no defined
payload and is left out of the payload comparison.
"""
import contextlib
import os
import zlib

import numpy as np
import pytest

from tests import bit_craft
from tests.bit_craft import CODES, code_id
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch

from paritypartyfs_amd import ECC_CRC, ECC_HAMMING, ECC_PARITY, EccEngine

# the bit server carries Hamming from 8-byte blocks up
SERVER_CODES = [c for c in CODES if not (c[0] == "ham" and c[2] < 8)]
PIPELINE_CODES = [("ham", 0, 1024), ("ham", 0, 4096), ("crc", 0x9960034c, 4096)]
LIST_CODES = [("ham", 0, 4096), ("crc", 0xc1acf, 1024), ("par", 0, 4096)]


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()  # the sets' arrays are read-only


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def rng_for(*k):
    return np.random.default_rng(zlib.crc32(repr(k).encode()))


def the_set(oracle, code):
    codec, poly, bs = code
    return bit_craft.bit_set(oracle, codec, bs, poly)


def engine(oracle, code, server=None):
    """The code's context; server=True: on the resident server, created as bit_engine of
    tests/test_gpu_server.py creates it (the first small call, where the choice is made, sees
    PPFS_ECC_SERVER=1)."""
    codec, poly, bs = code

    def make():
        if codec == "crc":
            return EccEngine(ECC_CRC, bs, crc_polynomial_explicit=oracle.crc_explicit(poly))
        return EccEngine(ECC_HAMMING if codec == "ham" else ECC_PARITY, bs)

    if server is None:
        return make()
    old = os.environ.get("PPFS_ECC_SERVER")
    os.environ["PPFS_ECC_SERVER"] = "1" if server else "0"
    try:
        eng = make()
        eng.encode_host(np.zeros(eng.data_size, np.uint8), np.zeros(eng.raw_block_size, np.uint8))
    finally:
        if old is None:
            del os.environ["PPFS_ECC_SERVER"]
        else:
            os.environ["PPFS_ECC_SERVER"] = old
    return eng


def batches(s):
    for name, idx in s.batches().items():
        yield name, idx, np.ascontiguousarray(s.words[idx]).reshape(-1)


def where_wrong(s, idx, got, exp):
    """For the assertion message: class and flips of the first blocks whose rows differ."""
    got, exp = np.asarray(got).reshape(idx.size, -1), np.asarray(exp).reshape(idx.size, -1)
    bad = np.nonzero((got != exp).any(axis=1))[0][:6]
    return [(int(i), s.labels[idx[i]], s.kinds[idx[i]], s.flips[idx[i]]) for i in bad]


def same_status(s, idx, st, tag):
    assert np.array_equal(st, s.o_st[idx]), (tag, where_wrong(s, idx, st, s.o_st[idx]))


def same_image(s, idx, img, exp, tag):
    assert np.array_equal(img, np.asarray(exp).reshape(-1)), (tag, where_wrong(s, idx, img, exp))


def same_payload(s, idx, out, tag):
    """Payload rows of the blocks the oracle did not reject."""
    ok = s.o_st[idx] != 5
    got, exp = np.asarray(out).reshape(idx.size, s.ds)[ok], s.o_data[idx][ok]
    assert np.array_equal(got, exp), (tag, where_wrong(s, idx[ok], got, exp))


def written(s, oracle, idx, raw, new):
    """What the write call leaves: a rejected block as it was, else the new payload encoded over the
    old block after its correction (the kept tail bits are the corrected image's)."""
    enc = s.encode(oracle, new, s.o_fixed[idx].reshape(-1)).reshape(idx.size, s.bs)
    return np.where((s.o_st[idx] == 5)[:, None], raw.reshape(idx.size, s.bs), enc).reshape(-1)


@pytest.mark.parametrize("code", CODES, ids=code_id)
def test_decode_payload_and_write_back(oracle, code):
    s = the_set(oracle, code)
    eng = engine(oracle, code)
    assert (eng.raw_block_size, eng.data_size) == (s.bs, s.ds)
    for name, idx, raw in batches(s):
        nb = idx.size
        raw_d = dev(raw)
        data_d = torch.full((nb * s.ds,), 0x77, dtype=torch.uint8, device="cuda")
        st_d = torch.full((nb,), 77, dtype=torch.uint8, device="cuda")
        eng.decode(raw_d, data_d, st_d, write_back=True, nblocks=nb)
        same_status(s, idx, host(st_d), name)
        same_payload(s, idx, host(data_d), name)
        same_image(s, idx, host(raw_d), s.o_fixed[idx], name)  # CRC and parity: untouched
    eng.close()


@pytest.mark.parametrize("code", CODES, ids=code_id)
def test_decode_status_only(oracle, code):
    """Without a payload output there is no LDS image: the Hamming streaming kernel patches the byte
    in place, a statement of its own.  Without write-back the image stays byte for byte."""
    s = the_set(oracle, code)
    eng = engine(oracle, code)
    for name, idx, raw in batches(s):
        for wb in (True, False):
            raw_d = dev(raw)
            st_d = torch.full((idx.size,), 77, dtype=torch.uint8, device="cuda")
            eng.decode(raw_d, None, st_d, write_back=wb, nblocks=idx.size)
            same_status(s, idx, host(st_d), (name, wb))
            same_image(s, idx, host(raw_d), s.o_fixed[idx] if wb else raw, (name, wb))
    eng.close()


@pytest.mark.parametrize("code", CODES, ids=code_id)
def test_write_over_the_corrected_block(oracle, code):
    """The status is the old block's; the new codeword keeps the tail bits of the corrected old
    block, a tail bit that a three-flip miscorrection turned included."""
    s = the_set(oracle, code)
    eng = engine(oracle, code)
    for name, idx, raw in batches(s):
        new = rng_for("bit-branches-write", code, name).integers(0, 256, idx.size * s.ds, dtype=np.uint8)
        raw_d = dev(raw)
        st_d = torch.full((idx.size,), 77, dtype=torch.uint8, device="cuda")
        eng.write(dev(new), raw_d, st_d, nblocks=idx.size)
        same_status(s, idx, host(st_d), name)
        same_image(s, idx, host(raw_d), written(s, oracle, idx, raw, new), name)
    eng.close()


def serve(eng, s, idx, raw, step, tag):
    """The batch through decode_host in slices of `step` blocks (each <= 64: one server request),
    once with write-back and payload, once status-only with write-back."""
    n, k = s.bs, s.ds
    img, out, st = raw.copy(), np.full(idx.size * k, 0x77, np.uint8), np.full(idx.size, 77, np.uint8)
    img2, st2 = raw.copy(), np.full(idx.size, 77, np.uint8)
    for b0 in range(0, idx.size, step):
        b1 = min(idx.size, b0 + step)
        eng.decode_host(img[b0 * n:b1 * n], out[b0 * k:b1 * k], st[b0:b1], write_back=True)
        eng.decode_host(img2[b0 * n:b1 * n], None, st2[b0:b1], write_back=True)
    same_status(s, idx, st, tag)
    same_payload(s, idx, out, tag)
    same_image(s, idx, img, s.o_fixed[idx], tag)
    same_status(s, idx, st2, tag)
    same_image(s, idx, img2, s.o_fixed[idx], tag)


@pytest.mark.parametrize("code", SERVER_CODES, ids=code_id)
def test_resident_server(oracle, code):
    """The server kernel runs the same per-wave bodies on its own request loop; compared with the
    oracle (tests/test_gpu_server.py compares uniform flips with the launch path).  Slices of 64, 17
    and 1 move every class through every wave of a request and through single-block requests."""
    s = the_set(oracle, code)
    eng = engine(oracle, code, server=True)
    idx = s.batches()["interleaved"]
    raw = np.ascontiguousarray(s.words[idx]).reshape(-1)
    for step in (64, 17, 1):
        serve(eng, s, idx, raw, step, step)
    new = rng_for("bit-branches-serve", code).integers(0, 256, idx.size * s.ds, dtype=np.uint8)
    for step in (64, 17):
        img, st = raw.copy(), np.full(idx.size, 77, np.uint8)
        for b0 in range(0, idx.size, step):
            b1 = min(idx.size, b0 + step)
            eng.write_host(new[b0 * s.ds:b1 * s.ds], img[b0 * s.bs:b1 * s.bs], st[b0:b1])
        same_status(s, idx, st, ("write", step))
        same_image(s, idx, img, written(s, oracle, idx, raw, new), ("write", step))
    eng.close()


@pytest.mark.parametrize("kind", ["pageable", "pinned"])
@pytest.mark.parametrize("code", PIPELINE_CODES, ids=code_id)
def test_chunk_pipeline(oracle, code, kind):
    """One decode_host call over each whole batch (> 64 blocks: the chunk pipeline).  Hamming sends
    back a patch list of one slot per block, applied to the caller's image by the host (pageable) or
    written straight into it (page-locked): the caller's image must be the oracle's."""
    from paritypartyfs_amd import pinned

    s = the_set(oracle, code)
    eng = engine(oracle, code)
    for name, idx, raw in batches(s):
        assert idx.size > 64
        img, out, st = raw.copy(), np.full(idx.size * s.ds, 0x77, np.uint8), np.full(idx.size, 77, np.uint8)
        with pinned(img, out, st) if kind == "pinned" else contextlib.nullcontext():
            eng.decode_host(img, out, st, write_back=True)
        same_status(s, idx, st, name)
        same_payload(s, idx, out, name)
        same_image(s, idx, img, s.o_fixed[idx], name)
        img2, st2 = raw.copy(), np.full(idx.size, 77, np.uint8)
        with pinned(img2, st2) if kind == "pinned" else contextlib.nullcontext():
            eng.decode_host(img2, None, st2, write_back=True)
        same_status(s, idx, st2, (name, "status-only"))
        same_image(s, idx, img2, s.o_fixed[idx], (name, "status-only"))
    eng.close()


@pytest.mark.parametrize("code", LIST_CODES, ids=code_id)
def test_decode_list_permuted(oracle, code):
    """The set as one image, listed in a permuted order: entry i gets block index[i]'s results, the
    corrected bytes go back to their rows of the image."""
    s = the_set(oracle, code)
    eng = engine(oracle, code)
    ix = rng_for("bit-branches-list", code).permutation(s.nb).astype(np.uint32)
    idx = ix.astype(np.int64)
    image_d = dev(s.words.reshape(-1))
    data_d = torch.full((s.nb * s.ds,), 0x77, dtype=torch.uint8, device="cuda")
    st_d = torch.full((s.nb,), 77, dtype=torch.uint8, device="cuda")
    eng.decode_list(image_d, dev(ix.view(np.int32)), data_d, st_d, write_back=True)
    same_status(s, idx, host(st_d), "list")
    same_payload(s, idx, host(data_d), "list")
    same_image(s, np.arange(s.nb), host(image_d), s.o_fixed, "list")
    # status only: the image stays
    image_d = dev(s.words.reshape(-1))
    st_d = torch.full((s.nb,), 77, dtype=torch.uint8, device="cuda")
    eng.decode_list(image_d, dev(ix.view(np.int32)), None, st_d, write_back=False)
    same_status(s, idx, host(st_d), "list status-only")
    same_image(s, np.arange(s.nb), host(image_d), s.words, "list status-only")
    eng.close()
