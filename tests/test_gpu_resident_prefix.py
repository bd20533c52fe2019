"""GPU tests of the resident codeword prefix of the RS 2t <= 8 ticket encode (paritypartyfs_amd/csrc/
rs_wg_tk.hpp, resident_plan.hpp): whatever the prefix, an encode -> inject -> decode pass computes what
the CPU oracle computes, bit for bit.

The batch is 64 * 5 + 7 blocks: five full tiles and a ragged one.  The prefix (PPFS_ECC_RESIDENT_MIB,
read when the context is created) is 0 tiles, 2 and 3 tiles (a boundary inside the batch, on either side
of a tile) and more than the batch.  Every tile -- so the tiles on both sides of each boundary and the
partial tile -- holds codewords with 0, 1 and 2 byte errors.  Each case runs two full passes over the
same buffers (the second pass meets the lines the first one left in the cache), with the decode's
write-back on and off, on the default stream and on a created one.
"""
import contextlib
import os
import zlib

import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch

from paritypartyfs_amd import ECC_REED_SOLOMON, EccEngine

NB = 64 * 5 + 7
NTILES = 6
TILE_BYTES = 64 * 255
CODES = [(255, 1), (255, 2), (512, 3), (256, 4)]  # 2t = 2, 4, 6, 8
PREFIX_TILES = [0, 2, 3, NTILES + 10]
PASSES = 2


def prefix_mib(tiles):
    """A PPFS_ECC_RESIDENT_MIB value that gives exactly `tiles` tiles (half a tile of slack)."""
    return "0" if tiles == 0 else f"{(tiles + 0.5) * TILE_BYTES / 2 ** 20:.9f}"


@contextlib.contextmanager
def resident_env(value):
    old = os.environ.get("PPFS_ECC_RESIDENT_MIB")
    os.environ["PPFS_ECC_RESIDENT_MIB"] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ["PPFS_ECC_RESIDENT_MIB"]
        else:
            os.environ["PPFS_ECC_RESIDENT_MIB"] = old


_REF = {}


def reference(oracle, bs, t):
    """The oracle's results for the code's two passes, computed once: per pass the payloads, the clean
    codewords, the error positions and values, the damaged image and its decode."""
    if (bs, t) in _REF:
        return _REF[(bs, t)]
    n, k, _ = oracle.rs_sizes(bs, t)
    rng = np.random.default_rng(zlib.crc32(repr(("resident-prefix", bs, t)).encode()))
    passes = []
    for _ in range(PASSES):
        data = rng.integers(0, 256, NB * k, dtype=np.uint8)
        cw = oracle.rs_encode(bs, t, data)
        bad = cw.reshape(NB, n).copy()
        pos, val = [], []
        for b in range(NB):
            ne = (b + b // 64) % 3  # 0, 1, 2 errors, every count in every tile (the 7-block one too)
            for p in rng.choice(n, ne, replace=False):
                pos.append(b * n + int(p))
                val.append(int(rng.integers(1, 256)))
        pos, val = np.array(pos, np.int64), np.array(val, np.uint8)
        bad.reshape(-1)[pos] ^= val
        bad = bad.reshape(-1)
        o_data, o_st, o_fixed, _, rc = oracle.rs_decode(bs, t, bad)
        assert rc == 0
        for tile in range(NTILES):  # the placement the test is about
            blocks = np.arange(tile * 64, min(NB, tile * 64 + 64))
            assert {int((b + b // 64) % 3) for b in blocks} == {0, 1, 2}
        passes.append(dict(data=data, cw=cw, pos=pos, val=val, bad=bad, o_data=o_data, o_st=o_st, o_fixed=o_fixed))
    _REF[(bs, t)] = (n, k, passes)
    return _REF[(bs, t)]


def run_passes(eng, ref, write_back, stream):
    n, k, passes = ref
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        cw_d = torch.zeros(NB * n, dtype=torch.uint8, device="cuda")
        out_d = torch.empty(NB * k, dtype=torch.uint8, device="cuda")
        st_d = torch.empty(NB, dtype=torch.uint8, device="cuda")
        for i, p in enumerate(passes):
            tag = (i, write_back, stream is not None)
            data_d = torch.from_numpy(p["data"]).cuda()
            pos_d, val_d = torch.from_numpy(p["pos"]).cuda(), torch.from_numpy(p["val"]).cuda()
            out_d.fill_(0x77)
            st_d.fill_(77)
            eng.encode(data_d, cw_d, nblocks=NB)
            enc = cw_d.clone()
            cw_d[pos_d] = cw_d[pos_d] ^ val_d  # at most one error per byte: plain indexing
            eng.decode(cw_d, out_d, st_d, write_back=write_back, nblocks=NB)
            torch.cuda.current_stream().synchronize()
            assert np.array_equal(enc.cpu().numpy(), p["cw"]), tag
            assert np.array_equal(out_d.cpu().numpy(), p["o_data"]), tag
            assert np.array_equal(st_d.cpu().numpy(), p["o_st"]), tag
            assert np.array_equal(cw_d.cpu().numpy(), p["o_fixed"] if write_back else p["bad"]), tag


@pytest.mark.parametrize("tiles", PREFIX_TILES, ids=lambda x: f"prefix{x}")
@pytest.mark.parametrize("bs,t", CODES, ids=lambda x: str(x))
def test_prefix_keeps_the_oracle_results(oracle, bs, t, tiles):
    ref = reference(oracle, bs, t)
    with resident_env(prefix_mib(tiles)):
        eng = EccEngine(ECC_REED_SOLOMON, bs, t)
    assert eng.kernel_name == "rs255-wg-tk-lds"
    created = torch.cuda.Stream()
    for stream in (None, created):
        assert eng.stream_kernel_name(stream) == "rs255-wg-tk-lds"  # the ticket kernels, not the static walk
        for write_back in (True, False):
            run_passes(eng, ref, write_back, stream)
    eng.close()
