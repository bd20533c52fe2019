"""bench_inodes.py -- what reading a batch of inodes in one call costs next to what was there before it.

An inode table of 2^20 random inodes and its bitmap (an eighth of the bits free) on a clean, device-resident image,
for RS(255,249) (block size 512, t = 3: the direct list path) and Hamming-512 (staged).  Workloads:
  consecutive   10,000 consecutive inode numbers
  random        10,000 random ones
  few           100 random ones
Timed as wall-clock time of the calling thread from the first call to the synchronised stream, median of --reps runs
after two warm-up runs, the runs of one leg back to back, with the spread (*_minmax_us):
  one_call     EccEngine.read_inodes: records, metadata and statuses in device memory
  yardstick    the way before that call, from the same inode numbers in host memory: the bitmap extents built with
               numpy and uploaded, one EccEngine.read_extents, the bytes read back (a synchronisation), the table
               extents of the allocated inodes built with numpy, a second read_extents, the rows split on the host
               (the records end in host memory, where read_files wants them; the one call's 64-byte-per-inode copy to
               the host is timed as one_call_to_host_us beside it)
  python_loop  few only: the Python block device's per-inode loop (IBlockDevice.read_inodes, one engine call per
               readBlock) on a host copy of the image
Every leg's records are compared with the table that was written.  repeats: the fraction of the blocks the one call
decodes that another entry of the batch decodes as well -- what a single-decode pass would remove.  Recorded, not
gating: DESIGN.md section 4.13.

Every (codec, workload) is measured in a child process of its own under a time limit; the first child that fails ends
the run.

    python tools/bench_inodes.py [--reps 9 --out profiles/inodes_io.json]
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

CODECS = [("RS(255,249)", 4, 512, 3), ("Hamming-512", 2, 512, 0)]
WORKLOADS = {"consecutive": 10000, "random": 10000, "few": 100}
TOTAL = 1 << 20
STEP_TIMEOUT_S = 300


def build(eng):
    """(table record, device image, the 81-byte records, the free flags)"""
    import numpy as np
    import torch

    from paritypartyfs_amd import INODE_TABLE_DTYPE

    raw, ds = eng.raw_block_size, eng.data_size
    rng = np.random.default_rng(20250505)
    bm_blocks, t_blocks = -(-(TOTAL // 8) // ds), -(-81 * TOTAL // ds)
    table = np.zeros(1, INODE_TABLE_DTYPE)
    table["bitmap_block"], table["table_block"], table["total_inodes"], table["check_bitmap"] = 1, 1 + bm_blocks + 1, TOTAL, 1
    blocks = int(table["table_block"][0]) + t_blocks + 1
    payload = np.zeros((blocks, ds), np.uint8)
    free = rng.random(TOTAL) < 0.125
    payload[1:1 + bm_blocks].reshape(-1)[:TOTAL // 8] = np.packbits(free)
    records = rng.integers(0, 256, (TOTAL, 81), dtype=np.uint8)
    tb = int(table["table_block"][0])
    payload[tb:tb + t_blocks].reshape(-1)[:81 * TOTAL] = records.reshape(-1)
    image = torch.zeros(blocks * raw, dtype=torch.uint8, device="cuda")
    eng.encode(torch.from_numpy(payload.reshape(-1)).cuda(), image)
    return table, image, records, free


def numbers_of(workload: str, n: int):
    import numpy as np

    rng = np.random.default_rng(20250506)
    if workload == "consecutive":
        return np.arange(300000, 300000 + n, dtype=np.uint32)
    return rng.integers(0, TOTAL, n).astype(np.uint32)


def worker(typ: int, bs: int, t: int, workload: str, n: int, reps: int) -> dict:
    import numpy as np
    import torch

    from paritypartyfs_amd import EccEngine
    from paritypartyfs_amd._native import EXTENT_DTYPE, FILE_DTYPE

    torch.cuda.set_device(0)
    eng = EccEngine(typ, bs, t)
    ds = eng.data_size
    table, image, records, free = build(eng)
    tb, bb = int(table["table_block"][0]), int(table["bitmap_block"][0])
    nums = numbers_of(workload, n)
    want_files = np.where(free[nums][:, None], 0, records[nums, 16:80]).astype(np.uint8)
    want_status = np.where(free[nums], 255, 0).astype(np.uint8)

    d_nums = torch.from_numpy(nums.view(np.int32)).cuda()
    d_files = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    d_meta = torch.zeros(24 * n, dtype=torch.uint8, device="cuda")
    d_status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    h_files = torch.zeros(64 * n, dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize()

    def one_call():
        eng.read_inodes(image, table, d_nums, files=d_files, meta=d_meta, status=d_status)

    def one_call_to_host():
        one_call()
        h_files.copy_(d_files, non_blocking=True)

    yard = {}

    def yardstick():
        i = nums.astype(np.int64)
        ext = np.zeros(n, EXTENT_DTYPE)
        ext["pos"], ext["block"], ext["offset"], ext["length"] = np.arange(n), bb + (i // 8) // ds, (i // 8) % ds, 1
        bm = torch.empty(n, dtype=torch.uint8, device="cuda")
        bst = torch.empty(n, dtype=torch.uint8, device="cuda")
        eng.read_extents(image, ext, bm, bst)
        byte, st = bm.cpu().numpy(), bst.cpu().numpy()  # the synchronisation
        live = np.flatnonzero((st <= 1) & ((byte & (0x80 >> (i % 8)).astype(np.uint8)) == 0))
        at = 81 * i[live]
        first = np.minimum(81, ds - at % ds)
        two = first < 81  # ds >= 81: at most two pieces
        k = live.size + int(two.sum())
        ext = np.zeros(k, EXTENT_DTYPE)
        a, b = ext[:live.size], ext[live.size:]
        a["pos"], a["block"], a["offset"], a["length"] = 81 * np.arange(live.size), tb + at // ds, at % ds, first
        b["pos"], b["block"], b["offset"], b["length"] = (81 * np.arange(live.size) + first)[two], (tb + at // ds + 1)[two], 0, (81 - first)[two]
        rows = torch.empty(81 * live.size, dtype=torch.uint8, device="cuda")
        rst = torch.empty(k, dtype=torch.uint8, device="cuda")
        eng.read_extents(image, ext, rows, rst)
        r = rows.cpu().numpy().reshape(live.size, 81)
        files = np.zeros((n, 64), np.uint8)
        files[live] = r[:, 16:80]
        status = np.full(n, 255, np.uint8)
        status[live] = rst.cpu().numpy()[:live.size]
        yard["files"], yard["status"] = files.view(FILE_DTYPE).reshape(n), status

    spread = {}

    def timed(name, fn, sync=True):
        us = []
        for k in range(reps + 2):  # two warm-up runs
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if sync:
                torch.cuda.synchronize()
            if k >= 2:
                us.append((time.perf_counter() - t0) * 1e6)
        spread[name + "_minmax_us"] = [min(us), max(us)]
        return statistics.median(us)

    res = {}
    res["one_call_us"] = timed("one_call", one_call)
    assert np.array_equal(d_files.cpu().numpy().reshape(n, 64), want_files) and np.array_equal(d_status.cpu().numpy(), want_status)
    assert np.array_equal(d_meta.cpu().numpy().reshape(n, 24)[:, :16], np.where(free[nums][:, None], 0, records[nums, :16]))
    res["one_call_to_host_us"] = timed("one_call_to_host", one_call_to_host)
    assert np.array_equal(h_files.numpy().reshape(n, 64), want_files)
    res["yardstick_us"] = timed("yardstick", yardstick)
    assert np.array_equal(yard["files"].view(np.uint8).reshape(n, 64), want_files) and np.array_equal(yard["status"], want_status)
    if workload == "few":
        from paritypartyfs_amd.block_device import ECCType, HeapDisk, IBlockDevice, create_block_device

        disk = HeapDisk(int(image.numel()))
        disk.buf[:] = image.cpu().numpy()
        dev = create_block_device(disk, bs, ECCType(typ), rs_correctable_bytes=t)
        got = {}
        res["python_loop_us"] = timed("python_loop", lambda: got.update(r=IBlockDevice.read_inodes(dev, table, nums)), sync=False)
        for j, (rec, err) in enumerate(got["r"]):
            assert (rec is None) == bool(free[nums[j]]) and (rec is None or rec.tobytes() == records[nums[j]].tobytes())
    res.update(spread)
    res["yardstick_over_one_call"] = res["yardstick_us"] / res["one_call_us"]
    res["yardstick_over_one_call_to_host"] = res["yardstick_us"] / res["one_call_to_host_us"]
    # the blocks the one call decodes, entry by entry, and how many of them another entry decodes as well
    i = nums.astype(np.int64)
    live = ~free[nums]
    at = 81 * i[live]
    touched = np.concatenate([bb + (i // 8) // ds, tb + at // ds, (tb + at // ds + 1)[(at % ds) + 81 > ds]])
    res.update(decoded=int(touched.size), distinct=int(np.unique(touched).size),
               repeats=1.0 - np.unique(touched).size / touched.size)
    res.update(inodes=n, total_inodes=TOTAL, allocated=int(live.sum()), raw_block_size=eng.raw_block_size, data_size=ds, reps=reps,
               list_kernel=eng.list_kernel_name(), device=torch.cuda.get_device_name(0), rocm=str(torch.version.hip))
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
            loop = f", python loop {r['python_loop_us'] / 1e3:.2f} ms" if "python_loop_us" in r else ""
            print(f"{name} {workload}: {r['inodes']} inodes | one call {r['one_call_us'] / 1e3:.3f} ms (to host "
                  f"{r['one_call_to_host_us'] / 1e3:.3f} ms) vs yardstick {r['yardstick_us'] / 1e3:.3f} ms = "
                  f"x{r['yardstick_over_one_call']:.2f} (x{r['yardstick_over_one_call_to_host']:.2f}){loop}; repeats "
                  f"{100 * r['repeats']:.1f} %", flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
