"""bench_list.py -- what a block-list decode costs next to the contiguous call it wraps.

For RS(255,249) and RS(255,223) at 2^20 blocks with one injected byte error per block, device-resident:
  decode_list, identity index        gather + decode + scatter of the rows in image order
  decode_list, seeded permutation    the same with 255-byte rows fetched from random places
  decode (contiguous)                ppfs_ecc_decode_device on the same image: the yardstick
  device copy                        ppfs_copy_device of the image's bytes: the HBM ceiling
and the two ratios list / contiguous.  Times are medians of --reps runs between stream events, the
image re-corrupted (untimed) before every run.  Recorded, not gating: DESIGN.md "Block lists".

Every codec is measured in a child process of its own under a time limit; the first child that
fails ends the run.

    python tools/bench_list.py [--blocks 1048576 --reps 7 --out profiles/list_io.json]
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

CODECS = [("RS(255,249)", 512, 3), ("RS(255,223)", 512, 16)]
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

    def timed(fn, corrupt=True):
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
        return statistics.median(ms) * 1e3  # us

    res = {
        "list_identity_us": timed(lambda: eng.decode_list(image, ident, out, st, write_back=True)),
        "list_permuted_us": timed(lambda: eng.decode_list(image, perm, out, st, write_back=True)),
        "contiguous_us": timed(lambda: eng.decode(image, out, st, write_back=True)),
        "copy_us": timed(lambda: device_copy(dst, image), corrupt=False),
    }
    assert int(st.max()) <= 1 and torch.equal(out, data), "decode results differ from the payloads"
    res["identity_over_contiguous"] = res["list_identity_us"] / res["contiguous_us"]
    res["permuted_over_contiguous"] = res["list_permuted_us"] / res["contiguous_us"]
    res.update(blocks=blocks, raw_block_size=n, data_size=k, reps=reps, image_bytes=blocks * n,
               piece_blocks=eng.host_chunk_blocks() & ~1023, kernel=eng.kernel_name,
               device=torch.cuda.get_device_name(0))
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="write the records here as one JSON document")
    ap.add_argument("--worker", nargs=2, type=int, metavar=("BLOCK_SIZE", "T"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        print(json.dumps(worker(a.worker[0], a.worker[1], a.blocks, a.reps)))
        return 0
    records = []
    for name, bs, t in CODECS:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--blocks",
               str(a.blocks), "--reps", str(a.reps), "--worker", str(bs), str(t)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(f"{name}: child ended with status {r.returncode}; stopping", file=sys.stderr)
            return 1
        rec = {"codec": name, **json.loads(r.stdout.strip().splitlines()[-1])}
        records.append(rec)
        print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "block-list decode vs contiguous decode, one byte error per block (tools/bench_list.py)",
                       "records": records}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
