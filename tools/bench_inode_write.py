"""bench_inode_write.py -- what writing a batch of inodes in one call costs next to what was there before it.

An inode table of 2^20 random inodes and its bitmap (an eighth of the bits free) on a clean, device-resident image,
for RS(255,249) (block size 512, t = 3: the direct list path) and Hamming-512 (staged).  Workloads:
  consecutive   10,000 consecutive inode numbers
  random        10,000 random ones
  few           100 random ones
Timed as wall-clock time of the calling thread from the first call to the synchronised stream, median of --reps runs
after two warm-up runs, the runs of one leg back to back, with the spread (*_minmax_us):
  one_call     EccEngine.write_inodes with check_bitmap = 1: numbers, records and metadata in device memory, statuses
               left in device memory
  yardstick    what the engine offered before that call, from the same numbers and records in host memory: the batch
               grouped by table block with numpy, one EccEngine.read_extents of the per-block hulls, the hulls read
               back (a synchronisation), the inodes' bytes composed on the host and uploaded, one
               EccEngine.write_extents over the distinct blocks.  It is spared the bitmap read: it takes the free flags
               from host memory.
Each leg writes the same records onto its own copy of the image; after each leg the inodes are read back with
read_inodes and compared with what was written, and at the end the two raw images are compared with each other.
Recorded, not gating: DESIGN.md section 4.15.

Every (codec, workload) is measured in a child process of its own under a time limit; the first child that fails ends
the run.

    python tools/bench_inode_write.py [--reps 9 --out profiles/inode_write_io.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_inodes import CODECS, STEP_TIMEOUT_S, TOTAL, WORKLOADS, build, numbers_of  # noqa: E402


def worker(typ: int, bs: int, t: int, workload: str, n: int, reps: int) -> dict:
    import numpy as np
    import torch

    from paritypartyfs_amd import EccEngine
    from paritypartyfs_amd._native import EXTENT_DTYPE, INODE_META_DTYPE

    torch.cuda.set_device(0)
    eng = EccEngine(typ, bs, t)
    ds = eng.data_size
    table, image, _, free = build(eng)
    tb = int(table["table_block"][0])
    nums = numbers_of(workload, n)
    rng = np.random.default_rng(20250607)
    recs = rng.integers(0, 256, (n, 81), dtype=np.uint8)
    files = np.ascontiguousarray(recs[:, 16:80]).reshape(-1)
    meta = np.zeros(n, INODE_META_DTYPE)
    meta["time_creation"] = np.ascontiguousarray(recs[:, 0:8]).view("<u8").reshape(n)
    meta["time_modified"] = np.ascontiguousarray(recs[:, 8:16]).view("<u8").reshape(n)
    meta["type"] = recs[:, 80]
    live = ~free[nums]
    last = {int(i): j for j, i in enumerate(nums)}  # a number that repeats ends with its last record
    want = np.stack([recs[last[int(i)]] for i in nums])
    want_status = np.where(live, 0, 255).astype(np.uint8)

    images = {"one_call": image.clone(), "yardstick": image.clone()}
    d_nums = torch.from_numpy(nums.view(np.int32)).cuda()
    d_files = torch.from_numpy(files).cuda()
    d_meta = torch.from_numpy(meta.view(np.uint8).reshape(-1)).cuda()
    d_status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def one_call():
        eng.write_inodes(images["one_call"], table, d_nums, d_files, d_meta, status=d_status)

    yard = {}

    def yardstick():
        img = images["yardstick"]
        keep = np.zeros(n, bool)
        keep[list(last.values())] = True
        rows = np.flatnonzero(live & keep)
        at = 81 * nums[rows].astype(np.int64)
        first = np.minimum(81, ds - at % ds)
        two = first < 81  # ds >= 81: at most two pieces
        # the pieces: block, offset, length, the entry and where its bytes start in the 81
        block = np.concatenate([tb + at // ds, (tb + at // ds + 1)[two]])
        off = np.concatenate([at % ds, np.zeros(int(two.sum()), np.int64)])
        length = np.concatenate([first, (81 - first)[two]])
        src = np.concatenate([rows, rows[two]])
        pos = np.concatenate([np.zeros(rows.size, np.int64), first[two]])
        ublock, group = np.unique(block, return_inverse=True)
        lo, hi = np.full(ublock.size, ds, np.int64), np.zeros(ublock.size, np.int64)
        np.minimum.at(lo, group, off)
        np.maximum.at(hi, group, off + length)
        ext = np.zeros(ublock.size, EXTENT_DTYPE)
        hull = hi - lo
        ext["pos"], ext["block"], ext["offset"], ext["length"] = np.concatenate([[0], np.cumsum(hull)[:-1]]), ublock, lo, hull
        nbytes = int(hull.sum())
        d_buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        eng.read_extents(img, ext, d_buf, None, write_back=False)
        buf = d_buf.cpu().numpy()  # the synchronisation
        # every piece's bytes onto the old ones
        rep = np.repeat(np.arange(block.size), length)
        within = np.arange(rep.size) - np.repeat(np.cumsum(length) - length, length)
        dst = (ext["pos"].astype(np.int64)[group] + off - lo[group])[rep] + within
        buf[dst] = recs[src[rep], pos[rep] + within]
        st = torch.empty(ublock.size, dtype=torch.uint8, device="cuda")
        eng.write_extents(torch.from_numpy(buf).cuda(), img, ext, st)
        yard["status"], yard["blocks"] = st, int(ublock.size)

    spread = {}

    def timed(name, fn):
        us = []
        for k in range(reps + 2):  # two warm-up runs
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= 2:
                us.append((time.perf_counter() - t0) * 1e6)
        spread[name + "_minmax_us"] = [min(us), max(us)]
        return statistics.median(us)

    def read_back(img):
        f = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
        m = torch.zeros(24 * n, dtype=torch.uint8, device="cuda")
        s = torch.zeros(n, dtype=torch.uint8, device="cuda")
        eng.read_inodes(img, table, d_nums, files=f, meta=m, status=s)
        f, m, s = f.cpu().numpy().reshape(n, 64), m.cpu().numpy().reshape(n, 24), s.cpu().numpy()
        assert np.array_equal(s, want_status)
        assert np.array_equal(f[live], want[live, 16:80]) and np.array_equal(m[live, :16], want[live, :16])
        assert np.array_equal(m[live, 16], want[live, 80])

    res = {}
    res["one_call_us"] = timed("one_call", one_call)
    assert np.array_equal(d_status.cpu().numpy(), want_status)
    read_back(images["one_call"])
    res["yardstick_us"] = timed("yardstick", yardstick)
    assert not yard["status"].cpu().numpy().any()
    read_back(images["yardstick"])
    assert torch.equal(images["one_call"], images["yardstick"]), "the two paths' images differ"
    assert not torch.equal(images["one_call"], image)
    res.update(spread)
    res["yardstick_over_one_call"] = res["yardstick_us"] / res["one_call_us"]
    res.update(inodes=n, total_inodes=TOTAL, allocated=int(live.sum()), distinct_blocks=yard["blocks"], raw_block_size=eng.raw_block_size,
               data_size=ds, reps=reps, list_kernel=eng.list_kernel_name(), device=torch.cuda.get_device_name(0),
               rocm=str(torch.version.hip))
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", default="")
    a = ap.parse_args()
    if a.worker:
        typ, bs, t, workload = a.worker.split(",")
        print(json.dumps(worker(int(typ), int(bs), int(t), workload, WORKLOADS[workload], a.reps)))
        return 0
    results = {}
    for name, typ, bs, t in CODECS:
        for workload in WORKLOADS:
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", f"{typ},{bs},{t},{workload}", "--reps",
                                    str(a.reps)], capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
            except subprocess.TimeoutExpired:
                print(f"{name} {workload}: no result within {STEP_TIMEOUT_S} s; stopping", file=sys.stderr)
                return 1
            if p.returncode != 0:
                print(f"{name} {workload}: worker failed ({p.returncode}); stopping\n{p.stderr[-2000:]}", file=sys.stderr)
                return 1
            r = results[f"{name} {workload}"] = json.loads(p.stdout.strip().splitlines()[-1])
            print(f"{name} {workload}: {r['inodes']} inodes, {r['distinct_blocks']} blocks | one call {r['one_call_us'] / 1e3:.3f} ms "
                  f"vs yardstick {r['yardstick_us'] / 1e3:.3f} ms = x{r['yardstick_over_one_call']:.2f}", flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
