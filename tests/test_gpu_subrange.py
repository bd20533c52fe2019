"""GPU tests of the contiguous device calls on sub-ranges of larger buffers: every pointer alignment,
every buffer inside guard bytes.

ppfs_ecc_encode_device, ppfs_ecc_decode_device and ppfs_ecc_write_device on blocks [first, first + count)
of an image of 80 blocks, i.e. on raw + first * raw_size, data + first * data_size, status + first, with
each buffer skewed against the 16-byte grid on its own.  Every buffer of a call (image, payloads,
statuses, an RS spill) is a view into its own allocation [256 guard | skew | n | 256 guard] of seeded
random bytes (tests/subrange.py); after the call the whole allocations are read back: inside the range
they equal the CPU oracle bit for bit, the rows of the blocks outside the range and the guard and skew
bytes are as uploaded.  An overrun of up to 256 bytes is a failed assertion, not a fault.

The pointer rule is the documented one (include/ppfs_ecc.h): where it forbids a skew (the RS fast paths:
raw, payload, status; Hamming blocks >= 8 bytes: raw) the call must return PPFS_ECC_EINVAL and leave
every buffer as it was.  1, 2 and 4 KiB CRC, Hamming and parity contexts run their streaming kernels on
16-byte aligned payload and raw pointers and the generic kernels on any others; a context's
kernel_name does not change with that.  One test per (code, skew triple) loops the ranges and the six
calls: encode over an old image of random bytes, decode with payload, status and write-back, decode
status-only, decode without a status, write with and without a status.  tests/test_subrange_cpu.py
checks the inputs.
"""
import pytest

from tests import subrange as sr
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch  # noqa: F401

from paritypartyfs_amd import ECC_CRC, ECC_HAMMING, ECC_PARITY, ECC_REED_SOLOMON, EccEngine


def engine(oracle, code):
    codec, par, bs = code
    if codec == "rs":
        return EccEngine(ECC_REED_SOLOMON, bs, par)
    if codec == "crc":
        return EccEngine(ECC_CRC, bs, crc_polynomial_explicit=oracle.crc_explicit(par))
    return EccEngine(ECC_HAMMING if codec == "ham" else ECC_PARITY, bs)


def sweep(oracle, code, skews, ranges, nblocks=sr.N):
    """Every range and call of one code at one skew triple; returns the (call, first) that were refused."""
    eng = engine(oracle, code)
    refused = []
    try:
        for first, count in ranges:
            cs = sr.case(oracle, code, first, count, nblocks)
            assert (eng.raw_block_size, eng.data_size) == (cs.row, cs.ds)
            for call in sr.CALLS:
                if sr.run_call(eng, cs, call, skews):
                    refused.append((call, first))
    finally:
        eng.close()
    return refused


@pytest.mark.parametrize("skews", sr.SKEWS, ids=sr.skew_id)
@pytest.mark.parametrize("code", sr.STREAMING, ids=sr.code_id)
def test_streaming_sizes(oracle, code, skews):
    """1, 2 and 4 KiB blocks: the streaming kernels where the payload and raw pointers of the call are 16-byte
    aligned -- skews (0, 0, 0) or a status skew only, and first * data_size a multiple of 16 (here: the ranges from
    block 0) -- and the generic kernels for any other pointer:
    a payload row of 4091 or 1023 bytes puts the ranges from blocks 3 and 13 there at every skew.  (A build
    whose wave_g2l funnel is wrong by one byte fails exactly the calls whose generic-kernel source rows are
    not 4-byte aligned and none of the aligned ones.)  Hamming refuses a misaligned raw pointer."""
    eng = engine(oracle, code)
    assert eng.kernel_name in sr.KERNEL_NAMES[code[0], True]
    eng.close()
    refused = sweep(oracle, code, skews, sr.RANGES)
    assert bool(refused) == (code[0] == "ham" and skews[0] % 16 != 0)
    assert not refused or len(refused) == len(sr.RANGES) * len(sr.CALLS)


@pytest.mark.parametrize("skews", sr.SKEWS, ids=sr.skew_id)
@pytest.mark.parametrize("code", sr.GENERIC, ids=sr.code_id)
def test_generic_bit_kernels(oracle, code, skews):
    """The wave-per-block kernels (any payload address; CRC and parity: any raw address) and the thread-per-block
    Hamming kernel of 4-byte blocks, where the raw pointer may have any address too."""
    eng = engine(oracle, code)
    assert eng.kernel_name in sr.KERNEL_NAMES[code[0], False]
    eng.close()
    refused = sweep(oracle, code, skews, sr.RANGES)
    assert bool(refused) == (code[0] == "ham" and code[2] >= 8 and skews[0] % 16 != 0)


@pytest.mark.parametrize("skews", sr.SKEWS, ids=sr.skew_id)
@pytest.mark.parametrize("code", sr.RS_GENERIC, ids=sr.code_id)
def test_rs_generic(oracle, code, skews):
    """Shortened codes and 16 < 2t < 32: a thread per block, bytes only -- every skew is allowed; the spill
    records of the decode lie at the status skew."""
    eng = engine(oracle, code)
    assert eng.kernel_name == "rs-generic-lfsr"
    eng.close()
    assert sweep(oracle, code, skews, sr.RANGES) == []


@pytest.mark.parametrize("skews", sr.SKEWS, ids=sr.skew_id)
@pytest.mark.parametrize("code", sr.RS_FAST, ids=sr.code_id)
def test_rs_fast(oracle, code, skews):
    """The fast paths take 16-byte aligned pointers only.  Blocks [16, 83) of an image of 100: first = 16 makes
    the three offsets multiples of 16, so skews (0, 0, 0) is an aligned sub-range, checked against the oracle
    with untouched neighbours, and at any other triple each call is refused exactly when a pointer it passes
    is misaligned (raw, data or status on its own included), with nothing written."""
    eng = engine(oracle, code)
    assert eng.kernel_name != "rs-generic-lfsr"
    eng.close()
    refused = sweep(oracle, code, skews, [sr.RS_FAST_RANGE], sr.RS_FAST_N)
    first = sr.RS_FAST_RANGE[0]
    sr_, sd, ss = (s % 16 != 0 for s in skews)
    want = [(call, first) for call in sr.CALLS
            if sr_ or (sd and sr.uses(call)[0]) or (ss and sr.uses(call)[1])]
    assert refused == want
