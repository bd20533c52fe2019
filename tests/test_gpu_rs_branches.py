"""GPU tests of every Reed-Solomon decode branch against the CPU oracle, bit-exact.

The other RS tests feed the decoders "codeword plus 0..t+3 random byte errors", which reaches the
shortcuts of the kernels (geometric syndromes, the S2/S1 pair correction, the closed forms for
sigma of degree 1 and 2, the double root whose fix value is 0, the root search from degree 3 up,
degree 0, a root at m = 0, roots past a shortened block) only by luck or not at all.  Here the
inputs are built from chosen syndromes (tests/rs_craft.py; tests/test_rs_craft.py pins the
classes each code's set holds) and go through every decode entry: the device calls, the write
call's status, the resident server, the chunked host pipeline and the block-list call.  Each set
runs as three batches, all ending on a ragged 64-block tile: classes interleaved (one wave holds
geometric, general and clean lanes), sorted by class (whole tiles of one kind), and tiles of clean
blocks with one general-path block at lane 0, 31, 32 or 63.
"""
import contextlib
import os
import zlib

import numpy as np
import pytest

from tests import rs_craft
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch

from paritypartyfs_amd import ECC_REED_SOLOMON, EccEngine

FAST = [(255, 1), (255, 2), (512, 3), (256, 4), (1024, 5), (4096, 8), (4096, 16)]
GENERIC = [(255, 6), (255, 9), (255, 20)]
SHORT = [(64, 3), (128, 10), (32, 1), (3, 1)]
CODES = FAST + GENERIC + SHORT


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()  # the sets' arrays are read-only


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def rng_for(*k):
    return np.random.default_rng(zlib.crc32(repr(k).encode()))


def server_engine(bs, t):
    """A context on the resident server, created as engine() of tests/test_gpu_server.py creates it:
    the first small call (where the choice is made) sees PPFS_ECC_SERVER=1."""
    old = os.environ.get("PPFS_ECC_SERVER")
    os.environ["PPFS_ECC_SERVER"] = "1"
    try:
        eng = EccEngine(ECC_REED_SOLOMON, bs, t)
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


def check_device_decode(eng, s, idx, raw, tag):
    """decode with write-back, payload, status (pre-filled) and spill: all as the oracle."""
    nb = idx.size
    raw_d = dev(raw)
    data_d = torch.full((nb * s.k,), 0x77, dtype=torch.uint8, device="cuda")
    st_d = torch.full((nb,), 77, dtype=torch.uint8, device="cuda")
    spill_d = torch.zeros(nb * eng.spill_bytes_per_block(), dtype=torch.uint8, device="cuda")
    eng.decode(raw_d, data_d, st_d, write_back=True, spill=spill_d, nblocks=nb)
    assert np.array_equal(host(st_d), s.o_st[idx]), tag
    assert np.array_equal(host(data_d), s.o_data[idx].reshape(-1)), tag
    assert np.array_equal(host(raw_d), s.o_fixed[idx].reshape(-1)), tag
    assert np.array_equal(host(spill_d).reshape(nb, -1), s.o_spill[idx]), tag


@pytest.mark.parametrize("bs,t", CODES, ids=lambda x: str(x))
def test_decode_write_back_payload_status_spill(oracle, bs, t):
    s = rs_craft.branch_set(oracle, bs, t)
    eng = EccEngine(ECC_REED_SOLOMON, bs, t)
    assert (eng.raw_block_size, eng.data_size) == (s.n, s.k)
    for name, idx, raw in batches(s):
        check_device_decode(eng, s, idx, raw, name)
    eng.close()


@pytest.mark.parametrize("bs,t", CODES, ids=lambda x: str(x))
def test_decode_status_only_leaves_the_image(oracle, bs, t):
    s = rs_craft.branch_set(oracle, bs, t)
    eng = EccEngine(ECC_REED_SOLOMON, bs, t)
    for name, idx, raw in batches(s):
        raw_d = dev(raw)
        st_d = torch.full((idx.size,), 77, dtype=torch.uint8, device="cuda")
        eng.decode(raw_d, None, st_d, write_back=False, nblocks=idx.size)
        assert np.array_equal(host(st_d), s.o_st[idx]), name
        assert np.array_equal(host(raw_d), raw), name
    eng.close()


@pytest.mark.parametrize("bs,t", CODES, ids=lambda x: str(x))
def test_write_status_of_the_old_block_and_new_codeword(oracle, bs, t):
    s = rs_craft.branch_set(oracle, bs, t)
    eng = EccEngine(ECC_REED_SOLOMON, bs, t)
    for name, idx, raw in batches(s):
        new = rng_for("branches-write", bs, t, name).integers(0, 256, idx.size * s.k, dtype=np.uint8)
        raw_d = dev(raw)
        st_d = torch.full((idx.size,), 77, dtype=torch.uint8, device="cuda")
        eng.write(dev(new), raw_d, st_d, nblocks=idx.size)
        assert np.array_equal(host(st_d), s.o_st[idx]), name
        assert np.array_equal(host(raw_d), oracle.rs_encode(bs, t, new)), name
    eng.close()


def serve(eng, s, idx, raw, step, tag):
    """The batch through decode_host in slices of `step` blocks (each <= 64: one server request),
    once with write-back and payload, once status-only."""
    n, k = s.n, s.k
    img, out, st = raw.copy(), np.full(idx.size * k, 0x77, np.uint8), np.full(idx.size, 77, np.uint8)
    img2, st2 = raw.copy(), np.full(idx.size, 77, np.uint8)
    for b0 in range(0, idx.size, step):
        b1 = min(idx.size, b0 + step)
        eng.decode_host(img[b0 * n:b1 * n], out[b0 * k:b1 * k], st[b0:b1], write_back=True)
        eng.decode_host(img2[b0 * n:b1 * n], None, st2[b0:b1], write_back=False)
    assert np.array_equal(st, s.o_st[idx]), tag
    assert np.array_equal(out, s.o_data[idx].reshape(-1)), tag
    assert np.array_equal(img, s.o_fixed[idx].reshape(-1)), tag
    assert np.array_equal(st2, s.o_st[idx]), tag
    assert np.array_equal(img2, raw), tag


@pytest.mark.parametrize("bs,t", CODES, ids=lambda x: str(x))
def test_resident_server(oracle, bs, t):
    """The server kernels carry their own copies of the correction code.  Slices of 64 keep the
    batches' tile layout (the lone general block at lane 0 / 31 / 32 / 63 of a request); 17 and 1
    move every class through the other lanes and through single-block requests."""
    s = rs_craft.branch_set(oracle, bs, t)
    eng = server_engine(bs, t)
    for name, idx, raw in batches(s):
        serve(eng, s, idx, raw, 64, (name, 64))
        if name == "interleaved":
            serve(eng, s, idx, raw, 17, (name, 17))
            if (bs, t) not in FAST:
                # the generic server kernel takes milliseconds per request whatever its size (one
                # thread per block, a 255-step root scan over 2t + 1 coefficients): single-block
                # requests get every class, but only every 16th of the random-syndrome and
                # exhaustive single-error blocks
                bulk = np.array([s.labels[b] in ("random", "single") for b in idx])
                keep = ~bulk | (np.cumsum(bulk) % 16 == 1)
                idx = idx[keep]
                raw = np.ascontiguousarray(s.words[idx]).reshape(-1)
            serve(eng, s, idx, raw, 1, (name, 1))
    eng.close()


@pytest.mark.parametrize("kind", ["pageable", "pinned"])
@pytest.mark.parametrize("bs,t", [(512, 3), (4096, 16)], ids=lambda x: str(x))
def test_chunk_pipeline_patch_lists(oracle, bs, t, kind):
    """One decode_host call over each whole batch (> 64 blocks: the chunk pipeline).  The patch lists
    must reproduce the oracle's image, double-root fixes of value 0 included."""
    from paritypartyfs_amd import pinned

    s = rs_craft.branch_set(oracle, bs, t)
    eng = EccEngine(ECC_REED_SOLOMON, bs, t)
    for name, idx, raw in batches(s):
        assert idx.size > 64
        img, out, st = raw.copy(), np.full(idx.size * s.k, 0x77, np.uint8), np.full(idx.size, 77, np.uint8)
        with pinned(img, out, st) if kind == "pinned" else contextlib.nullcontext():
            eng.decode_host(img, out, st, write_back=True)
        assert np.array_equal(st, s.o_st[idx]), name
        assert np.array_equal(out, s.o_data[idx].reshape(-1)), name
        assert np.array_equal(img, s.o_fixed[idx].reshape(-1)), name
        img2, st2 = raw.copy(), np.full(idx.size, 77, np.uint8)
        with pinned(img2, st2) if kind == "pinned" else contextlib.nullcontext():
            eng.decode_host(img2, None, st2, write_back=True)
        assert np.array_equal(st2, s.o_st[idx]) and np.array_equal(img2, s.o_fixed[idx].reshape(-1)), name
    eng.close()


@pytest.mark.parametrize("bs,t", [(512, 3), (64, 3)], ids=lambda x: str(x))
def test_decode_list_permuted(oracle, bs, t):
    """The set as one image, listed in a permuted order: entry i gets block index[i]'s results."""
    s = rs_craft.branch_set(oracle, bs, t)
    eng = EccEngine(ECC_REED_SOLOMON, bs, t)
    ix = rng_for("branches-list", bs, t).permutation(s.nb).astype(np.uint32)
    image_d = dev(s.words.reshape(-1))
    data_d = torch.full((s.nb * s.k,), 0x77, dtype=torch.uint8, device="cuda")
    st_d = torch.full((s.nb,), 77, dtype=torch.uint8, device="cuda")
    spill_d = torch.zeros(s.nb * eng.spill_bytes_per_block(), dtype=torch.uint8, device="cuda")
    eng.decode_list(image_d, dev(ix.view(np.int32)), data_d, st_d, write_back=True, spill=spill_d)
    assert np.array_equal(host(st_d), s.o_st[ix])
    assert np.array_equal(host(data_d), s.o_data[ix].reshape(-1))
    assert np.array_equal(host(spill_d).reshape(s.nb, -1), s.o_spill[ix])
    assert np.array_equal(host(image_d), s.o_fixed.reshape(-1))
    # status only: the image stays
    image_d = dev(s.words.reshape(-1))
    st_d = torch.full((s.nb,), 77, dtype=torch.uint8, device="cuda")
    eng.decode_list(image_d, dev(ix.view(np.int32)), None, st_d, write_back=False)
    assert np.array_equal(host(st_d), s.o_st[ix])
    assert np.array_equal(host(image_d), s.words.reshape(-1))
    eng.close()


# ------------------------------------------------------------------------------------
# parameter points of the generic kernel that never ran on the GPU
# ------------------------------------------------------------------------------------
# 2t = 0 (t = 0; n = 1 clamps t to 0): the codeword is the payload, every block is clean.
# (255, 127): the clamp limit, k = 1.  (3, 1): a 3-byte block.  (255, 9), (255, 20): t >= 9 at n = 255.
POINTS = [(255, 0), (1, 3), (255, 127), (3, 1), (255, 9), (255, 20)]


@pytest.mark.parametrize("bs,t", POINTS, ids=lambda x: str(x))
def test_generic_parameter_points(oracle, bs, t):
    n, k, tt = oracle.rs_sizes(bs, t)
    eng = EccEngine(ECC_REED_SOLOMON, bs, t)
    assert (eng.raw_block_size, eng.data_size) == (n, k)
    nb = 100 if tt == 127 else 131
    rng = rng_for("branches-points", bs, t)
    data = rng.integers(0, 256, nb * k, dtype=np.uint8)
    data[:k] = 0
    data[k:2 * k] = 0xFF
    cw = oracle.rs_encode(bs, t, data)
    raw_d = torch.zeros(nb * n, dtype=torch.uint8, device="cuda")
    eng.encode(dev(data), raw_d, nblocks=nb)
    assert np.array_equal(host(raw_d), cw)
    # 0 .. min(t, 3) + 1 random byte errors per block
    bad = cw.reshape(nb, n).copy()
    for b in range(nb):
        pos = rng.choice(n, min(b % (min(tt, 3) + 2), n), replace=False)
        bad[b, pos] ^= rng.integers(1, 256, pos.size, dtype=np.uint8)
    o_data, o_st, o_fixed, o_wbl, rc = oracle.rs_decode(bs, t, bad.reshape(-1))
    if rc != 0:
        # the reference overflows its 256-entry polynomial buffers (S(x) sigma(x) of 2t + deg > 256
        # coefficients): only with 2t = 254 and three or more errors.  Those blocks have no
        # expectation; the ones with <= 2 errors stay
        assert 2 * tt + 3 > 256
        keep = np.array([oracle.rs_decode(bs, t, bad[b])[4] == 0 for b in range(nb)])
        assert keep.sum() >= 3 * (nb // 5)
        bad = bad[keep]
        nb = bad.shape[0]
        o_data, o_st, o_fixed, o_wbl, rc = oracle.rs_decode(bs, t, bad.reshape(-1))
    assert rc == 0
    if tt == 0:
        assert not o_st.any() and np.array_equal(o_data, bad.reshape(-1))
    raw_d = dev(bad.reshape(-1))
    data_d = torch.full((nb * k,), 0x77, dtype=torch.uint8, device="cuda")
    st_d = torch.full((nb,), 77, dtype=torch.uint8, device="cuda")
    spill_d = torch.zeros(nb * eng.spill_bytes_per_block(), dtype=torch.uint8, device="cuda")
    eng.decode(raw_d, data_d, st_d, write_back=True, spill=spill_d, nblocks=nb)
    assert np.array_equal(host(st_d), o_st)
    assert np.array_equal(host(data_d), o_data)
    assert np.array_equal(host(raw_d), o_fixed)
    sp = host(spill_d).reshape(nb, -1)
    for b in range(nb):
        extra = max(0, int(o_wbl[b]) - n)
        assert sp[b, 0] == extra
        if extra:
            fixed = oracle.rs_decode_one_full(bs, t, bad[b])[2]
            assert sp[b, 1:1 + extra].tobytes() == fixed[n:n + extra].tobytes()
    # the crafted set (a single clean class for 2t = 0)
    s = rs_craft.branch_set(oracle, bs, t, max_blocks=128 if tt == 127 else None)
    idx = s.batches()["interleaved"]
    check_device_decode(eng, s, idx, np.ascontiguousarray(s.words[idx]).reshape(-1), "crafted")
    eng.close()
