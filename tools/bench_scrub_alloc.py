"""bench_scrub_alloc.py -- what the allocated-block scrub costs next to the two calls it can be compared with.

RS(255,249), block size 512, 2^20 data blocks, device-resident; the allocation bitmap (RS-encoded like any
block, 527 blocks) lies behind the data region.  For fills of 10 %, 50 % and 100 % (random allocation),
with one byte error in a tenth of the allocated blocks:
  scrub_allocated                    ppfs_ecc_scrub_allocated_device: bitmap decode, count / offsets / expand,
                                     the count read-back (one stream synchronisation per 1 Mi bits), the list
                                     decode with write-back, the tally (per-bit statuses and counts)
  (a) scrub, whole region            ppfs_ecc_scrub_device over all 2^20 data blocks
  (b) decode_list, same list         ppfs_ecc_decode_list_device(data=NULL, write_back=1) with the list of
                                     allocated blocks built on the host beforehand: the codec cost alone
and the overhead of scrub_allocated over (b).  Times are medians of --reps runs between stream events after
--warmup runs, each with the run's spread (*_minmax_us); the image is restored to its corrupted state
(untimed) before every run, and the three legs alternate within a repetition.  The first run checks the
counts against what was injected.  Recorded, not gating: DESIGN.md section 4.9.

    python tools/bench_scrub_alloc.py [--blocks 1048576 --reps 15 --warmup 3 --out profiles/scrub_alloc.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1 << 20)
    ap.add_argument("--fills", default="0.1,0.5,1.0")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scrub_alloc.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from paritypartyfs_amd import ECC_REED_SOLOMON, EccEngine, ScrubCounts

    if not torch.cuda.is_available():
        sys.exit("bench_scrub_alloc.py needs a GPU")
    eng = EccEngine(ECC_REED_SOLOMON, 512, 3)
    raw, ds, N = eng.raw_block_size, eng.data_size, args.blocks
    assert (N * raw) % 16 == 0, "the data region's end must keep the contiguous calls' 16-byte rule"
    B = eng.bitmap_blocks(N)
    rng = np.random.default_rng(20240917)
    payload = torch.from_numpy(rng.integers(0, 256, (N + B) * ds, dtype=np.uint8)).cuda()
    good = torch.zeros((N + B) * raw, dtype=torch.uint8, device="cuda")
    image = torch.empty_like(good)
    status = torch.zeros(N, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(8, dtype=torch.int64, device="cuda")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    rows = []
    for fill in [float(f) for f in args.fills.split(",")]:
        bits = rng.random(N) < fill if fill < 1.0 else np.ones(N, bool)
        alloc = np.nonzero(bits)[0]
        stream = np.zeros(B * ds, np.uint8)
        packed = np.packbits(bits)
        stream[:packed.size] = packed
        payload[N * ds:] = torch.from_numpy(stream).cuda()
        eng.encode(payload, good)
        hit = alloc[rng.random(alloc.size) < 0.1]  # one byte error in a tenth of the allocated blocks
        pos = torch.from_numpy(hit * raw + rng.integers(0, raw, hit.size)).cuda()
        val = torch.from_numpy(rng.integers(1, 256, hit.size, dtype=np.uint8)).cuda()
        bad = good.clone()
        bad[pos] ^= val
        index = torch.from_numpy(alloc.astype(np.uint32).view(np.int32)).cuda()
        list_status = torch.zeros(max(alloc.size, 16), dtype=torch.uint8, device="cuda")
        legs = {
            "scrub_allocated": lambda: eng.scrub_allocated(image, N, 0, N, status=status, counts=counts),
            "scrub_whole": lambda: eng.scrub(image[:N * raw], status, nblocks=N),
            "decode_list": lambda: eng.decode_list(image, index, None, list_status, write_back=True),
        }
        times = {k: [] for k in legs}
        for rep in range(args.warmup + args.reps):
            for name, fn in legs.items():
                image.copy_(bad)
                torch.cuda.synchronize()
                us = timed(fn)
                if rep >= args.warmup:
                    times[name].append(us)
                if rep == 0:  # the calls did what they are timed for
                    assert torch.equal(image[:N * raw], good[:N * raw]), name
                    if name == "scrub_allocated":
                        got = ScrubCounts(*counts.tolist())
                        want = ScrubCounts(alloc.size - hit.size, hit.size, 0, 0, N - alloc.size, B, 0, 0)
                        assert got == want, (got, want)
        row = {"codec": "RS(255,249)", "blocks": N, "fill": fill, "allocated": int(alloc.size), "corrupted": int(hit.size),
               "bitmap_blocks": B, "reps": args.reps, "list_kernel": eng.list_kernel_name()}
        for name, t in times.items():
            row[name + "_us"] = round(statistics.median(t), 1)
            row[name + "_minmax_us"] = [round(min(t), 1), round(max(t), 1)]
        row["overhead_over_decode_list_us"] = round(row["scrub_allocated_us"] - row["decode_list_us"], 1)
        row["overhead_over_decode_list"] = round(row["scrub_allocated_us"] / row["decode_list_us"] - 1, 3)
        row["scrub_allocated_over_scrub_whole"] = round(row["scrub_allocated_us"] / row["scrub_whole_us"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
