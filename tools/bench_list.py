"""bench_list.py -- what a block-list decode costs next to the contiguous call it wraps.

For RS(255,249), RS(255,251) and RS(255,223) at 2^12, 2^16 and 2^20 blocks with one injected byte error
per block, device-resident:
  decode_list, identity index        the rows in image order
  decode_list, seeded permutation    255-byte rows fetched from random places
  decode (contiguous)                ppfs_ecc_decode_device on the same image: the yardstick
  device copy                        ppfs_copy_device of the image's bytes: the HBM ceiling
and the two ratios list / contiguous.  A codec whose list decode is the direct kernel (RS 2t <= 8,
EccEngine.list_kernel_name) is measured a second time in a worker started under PPFS_ECC_LIST_DIRECT=0,
the staged path (gather + decode + scatter) of the same build: the record carries both (staged_*) and
their ratio.  Times are medians of --reps runs between stream events, each with the run's spread
(*_minmax_us), the image re-corrupted (untimed) before every run.  Recorded, not gating: DESIGN.md
"Block lists".

With --extents, for RS(255,249) only, the two byte-extent legs beside their yardsticks of the same build:
  read_extents, file shape           file_extents over the permuted list from byte 100 of the first block
  decode_list, same permutation      the yardstick of the read
  (both again under PPFS_ECC_LIST_DIRECT=0: staged_read_extents_us, staged_decode_list_us)
  device copy of the packed bytes    what the pack's traffic costs as a plain copy
  write_extents, 64 bytes at 32      one 64-byte segment at offset 32 of every permuted block
  write_list, same permutation       the yardstick of the write
  (all four legs again under PPFS_ECC_LIST_DIRECT=0: staged_*_us)
Recorded, not gating: DESIGN.md "Byte extents".

With --writes, the write side: RS(255,249) and RS(255,251) at 2^12, 2^16 and 2^20 blocks, RS(255,223)
(staged only) at 2^20:
  encode_list, identity / permuted   the codewords stored at image + index[i] * 255
  encode (contiguous)                ppfs_ecc_encode_device of the same payloads: the yardstick
  write_list, identity / permuted    old blocks with one byte error each (re-corrupted untimed)
  write (contiguous)                 ppfs_ecc_write_device over the same image
  device copy                        the image's bytes
A codec whose list encode is the direct kernel (EccEngine.list_encode_kernel_name) is measured again in a
worker under PPFS_ECC_LIST_DIRECT=0; the record carries both, their ratio, and per leg whether the direct
median lies below the staged minimum of its runs (direct_below_staged_min_*: the routing rule of
DESIGN.md "Block lists").

Every codec is measured in a child process of its own under a time limit; the first child that
fails ends the run.

    python tools/bench_list.py [--blocks 4096,65536,1048576 --reps 7 --out profiles/list_io.json]
    python tools/bench_list.py --extents [--out profiles/extent_io.json]
    python tools/bench_list.py --writes [--out profiles/list_write_io.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CODECS = [("RS(255,249)", 512, 3), ("RS(255,251)", 512, 2), ("RS(255,223)", 512, 16)]
SIZES = "4096,65536,1048576"
STEP_TIMEOUT_S = 240


def worker(bs: int, t: int, blocks: int, reps: int) -> dict:
    import numpy as np
    import torch

    from paritypartyfs_amd import ECC_REED_SOLOMON, EccEngine, device_copy, inject_bytes

    torch.cuda.set_device(0)
    eng = EccEngine(ECC_REED_SOLOMON, bs, t)
    n, k = eng.raw_block_size, eng.data_size
    g = torch.Generator(device="cuda").manual_seed(20240611)
    data = torch.randint(0, 256, (blocks * k,), dtype=torch.uint8, device="cuda", generator=g)
    image = torch.empty(blocks * n, dtype=torch.uint8, device="cuda")
    eng.encode(data, image)
    pos = torch.randint(0, n, (blocks,), dtype=torch.uint8, device="cuda", generator=g)
    val = torch.randint(1, 256, (blocks,), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty_like(data)
    st = torch.empty(blocks, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(image)
    ident = torch.arange(blocks, dtype=torch.int32, device="cuda")
    perm = torch.from_numpy(np.random.default_rng(7).permutation(blocks).astype(np.int32)).cuda()

    spread = {}

    def timed(name, fn, corrupt=True):
        ms = []
        for r in range(reps + 2):  # two warm-up runs
            if corrupt:
                inject_bytes(image, n, pos, val, xor=True)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= 2:
                ms.append(a.elapsed_time(b))
        spread[name + "_minmax_us"] = [min(ms) * 1e3, max(ms) * 1e3]
        return statistics.median(ms) * 1e3  # us

    res = {
        "list_identity_us": timed("list_identity", lambda: eng.decode_list(image, ident, out, st, write_back=True)),
        "list_permuted_us": timed("list_permuted", lambda: eng.decode_list(image, perm, out, st, write_back=True)),
    }
    assert int(st.max()) <= 1 and torch.equal(out.view(blocks, k), data.view(blocks, k)[perm.long()]), "list results differ"
    res["contiguous_us"] = timed("contiguous", lambda: eng.decode(image, out, st, write_back=True))
    res["copy_us"] = timed("copy", lambda: device_copy(dst, image), corrupt=False)
    assert int(st.max()) <= 1 and torch.equal(out, data), "decode results differ from the payloads"
    res.update(spread)
    res["identity_over_contiguous"] = res["list_identity_us"] / res["contiguous_us"]
    res["permuted_over_contiguous"] = res["list_permuted_us"] / res["contiguous_us"]
    res.update(blocks=blocks, raw_block_size=n, data_size=k, reps=reps, image_bytes=blocks * n,
               piece_blocks=eng.host_chunk_blocks() & ~1023, kernel=eng.kernel_name, list_kernel=eng.list_kernel_name(),
               device=torch.cuda.get_device_name(0))
    return res


def worker_extents(bs: int, t: int, blocks: int, reps: int) -> dict:
    import numpy as np
    import torch

    from paritypartyfs_amd import ECC_REED_SOLOMON, EccEngine, device_copy, inject_bytes
    from paritypartyfs_amd._native import EXTENT_DTYPE
    from paritypartyfs_amd.block_device import file_extents

    torch.cuda.set_device(0)
    eng = EccEngine(ECC_REED_SOLOMON, bs, t)
    n, k = eng.raw_block_size, eng.data_size
    g = torch.Generator(device="cuda").manual_seed(20240611)
    data = torch.randint(0, 256, (blocks * k,), dtype=torch.uint8, device="cuda", generator=g)
    image = torch.empty(blocks * n, dtype=torch.uint8, device="cuda")
    eng.encode(data, image)
    pos = torch.randint(0, n, (blocks,), dtype=torch.uint8, device="cuda", generator=g)
    val = torch.randint(1, 256, (blocks,), dtype=torch.uint8, device="cuda", generator=g)
    st = torch.empty(blocks, dtype=torch.uint8, device="cuda")
    perm_np = np.random.default_rng(7).permutation(blocks).astype(np.uint32)
    perm = torch.from_numpy(perm_np.view(np.int32)).cuda()

    spread = {}

    def timed(name, fn, corrupt=True):
        ms = []
        for r in range(reps + 2):  # two warm-up runs
            if corrupt:
                inject_bytes(image, n, pos, val, xor=True)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= 2:
                ms.append(a.elapsed_time(b))
        spread[name + "_minmax_us"] = [min(ms) * 1e3, max(ms) * 1e3]
        return statistics.median(ms) * 1e3  # us

    # the read: a file over every block of the list, from byte 100 of its first block to the middle of its last
    off0 = 100
    nbytes = (k - off0) + (blocks - 2) * k + k // 2
    r_ext = file_extents(perm_np, off0, nbytes, k)
    assert len(r_ext) == blocks
    r_ext_d = torch.from_numpy(r_ext.view(np.uint8)).cuda()
    packed = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    payloads = torch.empty_like(data)
    copy_dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    res = {
        "read_extents_us": timed("read_extents", lambda: eng.read_extents(image, r_ext_d, packed, st, write_back=True)),
        "decode_list_us": timed("decode_list", lambda: eng.decode_list(image, perm, payloads, st, write_back=True)),
        "pack_copy_us": timed("pack_copy", lambda: device_copy(copy_dst, payloads, nbytes), corrupt=False),
    }
    want = data.view(blocks, k)[perm.long()].reshape(-1)
    assert int(st.max()) <= 1 and torch.equal(payloads, want), "decode_list results differ from the payloads"
    assert torch.equal(packed, want[off0:off0 + nbytes]), "read_extents results differ from the file range"
    # the write: 64 bytes at offset 32 of every block of the list
    seg, at = 64, 32
    w_ext = np.zeros(blocks, EXTENT_DTYPE)
    w_ext["pos"], w_ext["block"], w_ext["offset"], w_ext["length"] = np.arange(blocks, dtype=np.uint64) * seg, perm_np, at, seg
    w_ext_d = torch.from_numpy(w_ext.view(np.uint8)).cuda()
    fresh = torch.randint(0, 256, (blocks * seg,), dtype=torch.uint8, device="cuda", generator=g)
    res["write_extents_us"] = timed("write_extents", lambda: eng.write_extents(fresh, image, w_ext_d, st))
    assert int(st.max()) <= 1
    eng.decode_list(image, perm, payloads, st, write_back=False)
    got = payloads.view(blocks, k)
    assert int(st.max()) == 0 and torch.equal(got[:, at:at + seg].reshape(-1), fresh), "write_extents: segments differ"
    keep = torch.ones(k, dtype=torch.bool, device="cuda")
    keep[at:at + seg] = False
    assert torch.equal(got[:, keep], want.view(blocks, k)[:, keep]), "write_extents: bytes outside the segments changed"
    res["write_list_us"] = timed("write_list", lambda: eng.write_list(want, image, perm, st))
    assert int(st.max()) <= 1
    res["read_over_list"] = res["read_extents_us"] / res["decode_list_us"]
    res["write_over_list"] = res["write_extents_us"] / res["write_list_us"]
    # the issue's budget of the read: the list decode, the pack's traffic as a copy, 20 % for the launches
    res["read_budget_us"] = 1.2 * (res["decode_list_us"] + res["pack_copy_us"])
    res["read_within_budget"] = res["read_extents_us"] <= res["read_budget_us"]
    res.update(spread)
    res.update(entries=blocks, raw_block_size=n, data_size=k, reps=reps, image_bytes=blocks * n, read_bytes=nbytes,
               read_offset_in_first_block=off0, write_segment_bytes=seg, write_segment_offset=at,
               piece_blocks=eng.host_chunk_blocks() & ~1023, kernel=eng.kernel_name, list_kernel=eng.list_kernel_name(),
               device=torch.cuda.get_device_name(0))
    return res


def worker_writes(bs: int, t: int, blocks: int, reps: int) -> dict:
    import numpy as np
    import torch

    from paritypartyfs_amd import ECC_REED_SOLOMON, EccEngine, device_copy, inject_bytes

    torch.cuda.set_device(0)
    eng = EccEngine(ECC_REED_SOLOMON, bs, t)
    n, k = eng.raw_block_size, eng.data_size
    g = torch.Generator(device="cuda").manual_seed(20240611)
    old = torch.randint(0, 256, (blocks * k,), dtype=torch.uint8, device="cuda", generator=g)
    data = torch.randint(0, 256, (blocks * k,), dtype=torch.uint8, device="cuda", generator=g)  # the payloads written
    image = torch.empty(blocks * n, dtype=torch.uint8, device="cuda")
    want = torch.empty_like(image)  # the new codewords in list order
    eng.encode(data, want)
    pos = torch.randint(0, n, (blocks,), dtype=torch.uint8, device="cuda", generator=g)
    val = torch.randint(1, 256, (blocks,), dtype=torch.uint8, device="cuda", generator=g)
    st = torch.empty(blocks, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(image)
    ident = torch.arange(blocks, dtype=torch.int32, device="cuda")
    perm = torch.from_numpy(np.random.default_rng(7).permutation(blocks).astype(np.int32)).cuda()

    spread = {}

    def timed(name, fn, before=None):
        ms = []
        for r in range(reps + 2):  # two warm-up runs
            if before:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= 2:
                ms.append(a.elapsed_time(b))
        spread[name + "_minmax_us"] = [min(ms) * 1e3, max(ms) * 1e3]
        return statistics.median(ms) * 1e3  # us

    def old_blocks():  # valid old codewords with one byte error each, untimed
        eng.encode(old, image)
        inject_bytes(image, n, pos, val, xor=True)

    def landed(ix, what):
        assert torch.equal(image.view(blocks, n)[ix.long()], want.view(blocks, n)), what + ": codewords differ"

    res = {}
    image.zero_()
    res["encode_list_identity_us"] = timed("encode_list_identity", lambda: eng.encode_list(data, image, ident))
    landed(ident, "encode_list identity")
    image.zero_()
    res["encode_list_permuted_us"] = timed("encode_list_permuted", lambda: eng.encode_list(data, image, perm))
    landed(perm, "encode_list permuted")
    res["encode_us"] = timed("encode", lambda: eng.encode(data, image))
    res["write_list_identity_us"] = timed("write_list_identity", lambda: eng.write_list(data, image, ident, st), old_blocks)
    assert int(st.min()) == 1 and int(st.max()) == 1, "write_list identity: every old block had one error"
    landed(ident, "write_list identity")
    res["write_list_permuted_us"] = timed("write_list_permuted", lambda: eng.write_list(data, image, perm, st), old_blocks)
    assert int(st.min()) == 1 and int(st.max()) == 1, "write_list permuted: every old block had one error"
    landed(perm, "write_list permuted")
    res["write_us"] = timed("write", lambda: eng.write(data, image, st), old_blocks)
    assert int(st.min()) == 1 and int(st.max()) == 1
    res["copy_us"] = timed("copy", lambda: device_copy(dst, image))
    res.update(spread)
    for leg, yard in (("encode_list_identity", "encode"), ("encode_list_permuted", "encode"),
                      ("write_list_identity", "write"), ("write_list_permuted", "write")):
        res[leg + "_over_contiguous"] = res[leg + "_us"] / res[yard + "_us"]
    res.update(blocks=blocks, raw_block_size=n, data_size=k, reps=reps, image_bytes=blocks * n,
               piece_blocks=eng.host_chunk_blocks() & ~1023, kernel=eng.kernel_name, list_kernel=eng.list_kernel_name(),
               list_encode_kernel=eng.list_encode_kernel_name(), device=torch.cuda.get_device_name(0))
    return res


def run_worker(bs: int, t: int, blocks: int, reps: int, mode: str, staged: bool):
    """One measurement in a child process under a time limit; mode: "", "--extents" or "--writes"; staged:
    with PPFS_ECC_LIST_DIRECT=0 in its environment.  None when the child failed."""
    cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--blocks", str(blocks),
           "--reps", str(reps), "--worker", str(bs), str(t)] + ([mode] if mode else [])
    env = {k: v for k, v in os.environ.items() if k != "PPFS_ECC_LIST_DIRECT"}
    if staged:
        env["PPFS_ECC_LIST_DIRECT"] = "0"
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(f"bs {bs} t {t} blocks {blocks}: child ended with status {r.returncode}; stopping", file=sys.stderr)
        return None
    return json.loads(r.stdout.strip().splitlines()[-1])


# the legs a staged worker repeats, by mode
STAGED_LEGS = {"": ("list_identity", "list_permuted"),
               "--extents": ("read_extents", "decode_list", "write_extents", "write_list"),
               "--writes": ("encode_list_identity", "encode_list_permuted", "write_list_identity", "write_list_permuted")}
WORKERS = {"": worker, "--extents": worker_extents, "--writes": worker_writes}
WHAT = {"": "block-list decode (direct and staged) vs contiguous decode, one byte error per block (tools/bench_list.py)",
        "--extents": "byte-extent read / write vs the list decode / list write of the same build, direct and staged, one byte "
                     "error per block (tools/bench_list.py --extents)",
        "--writes": "block-list encode / write (direct and staged) vs contiguous encode / write, old blocks of the writes with "
                    "one byte error each (tools/bench_list.py --writes)"}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default=None, help=f"comma-separated block counts (default {SIZES}; --extents: 1048576)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="write the records here as one JSON document")
    ap.add_argument("--extents", action="store_true", help="the byte-extent legs (RS(255,249)) instead of the list legs")
    ap.add_argument("--writes", action="store_true", help="the list encode / write legs instead of the list decode legs")
    ap.add_argument("--worker", nargs=2, type=int, metavar=("BLOCK_SIZE", "T"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.extents and a.writes:
        ap.error("--extents and --writes are two modes")
    mode = "--extents" if a.extents else "--writes" if a.writes else ""
    sizes = [int(x) for x in (a.blocks or ("1048576" if a.extents else SIZES)).split(",")]
    if a.worker:
        print(json.dumps(WORKERS[mode](a.worker[0], a.worker[1], sizes[0], a.reps)))
        return 0
    records = []
    for name, bs, t in (CODECS[:1] if a.extents else CODECS):
        for blocks in sizes:
            if a.writes and t == 16 and blocks != max(sizes):
                continue  # the staged-only codec: its largest size alone
            rec = run_worker(bs, t, blocks, a.reps, mode, False)
            if rec is None:
                return 1
            rec = {"codec": name, **rec}
            if rec["list_kernel"] != "gather-stage-scatter":
                st = run_worker(bs, t, blocks, a.reps, mode, True)
                if st is None:
                    return 1
                assert st["list_kernel"] == "gather-stage-scatter"
                for leg in STAGED_LEGS[mode]:
                    rec["staged_" + leg + "_us"] = st[leg + "_us"]
                    rec["staged_" + leg + "_minmax_us"] = st[leg + "_minmax_us"]
                    rec["direct_over_staged_" + leg] = rec[leg + "_us"] / st[leg + "_us"]
                    if a.writes:  # the routing rule: the direct median below the staged runs' minimum
                        rec["direct_below_staged_min_" + leg] = rec[leg + "_us"] < st[leg + "_minmax_us"][0]
                if not mode:  # how far the two workers' runs of the unchanged contiguous decode lie apart
                    rec["staged_worker_contiguous_us"] = st["contiguous_us"]
                if a.writes:
                    rec["staged_worker_encode_us"], rec["staged_worker_write_us"] = st["encode_us"], st["write_us"]
            records.append(rec)
            print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": WHAT[mode], "records": records}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
