"""bench_file_write.py -- what an in-place file write from the inode records costs next to the way before it.

Three workloads, each on a clean, device-resident image whose data and index blocks are placed by a seeded
permutation (so every file is fragmented), for RS(255,249) (block size 512, t = 3: the direct list path) and
Hamming-512 (staged); I = entries per index block:
  big      one file of 100,000 blocks, written whole
  small    10,000 files of 1 .. 12 blocks, seeded sizes, written whole: no tree at all, pure fixed cost
  records  10,000 writes of 128 bytes into distinct blocks of 2,000 files of 13 .. 12 + 4 I blocks (five per file)
Timed as wall-clock time of the calling thread from the call to the synchronised stream, median of --reps runs after
two warm-up runs, the runs of one leg back to back, with the spread (*_minmax_us):
  write_files  EccEngine.write_files of the whole batch: one call, nothing read back
  four_step    what there was before that call: EccEngine.files_blocks on the device, index and path status read back
               to the host, the extents built with numpy (from files_plan's slots) and uploaded, one
               EccEngine.write_extents
Each leg writes its own bytes; after each leg the image is read back with read_files and compared with what the leg
wrote, and both legs' final raw images are compared with each other after writing the same bytes.  Recorded, not
gating: DESIGN.md section 4.12.

--launches N runs one write_files call over N small files and nothing else, for a kernel trace of its own: the
number of launches must not depend on N.

Every (codec, workload) is measured in a child process of its own under a time limit; the first child that fails
ends the run.

    python tools/bench_file_write.py [--reps 9 --out profiles/file_write_io.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

CODECS = [("RS(255,249)", 4, 512, 3), ("Hamming-512", 2, 512, 0)]
WORKLOADS = ("big", "small", "records")
STEP_TIMEOUT_S = 400
NO_BLOCK = 0xFFFFFFFF


def build(eng, sizes):
    """(files, device image, blocks, index blocks) of fragmented files of sizes[f] blocks"""
    import numpy as np
    import torch
    from bench_file import leaf_of, tree_of

    from paritypartyfs_amd import FILE_DTYPE

    raw, ds = eng.raw_block_size, eng.data_size
    I = ds // 4
    rng = np.random.default_rng(20250404)
    trees = [tree_of(n, I) for n in sizes]
    index_blocks = sum(len(t) for t in trees)
    blocks = int(sum(sizes)) + index_blocks + 16
    perm = rng.permutation(blocks).astype(np.uint32)
    payload = rng.integers(0, 256, (blocks, ds), dtype=np.uint8)
    files = np.zeros(len(sizes), FILE_DTYPE)
    at = 0
    for f, (n, nodes) in enumerate(zip(sizes, trees)):
        data_blk = perm[at:at + n]
        node_blk = {nid: int(perm[at + n + k]) for k, (nid, _, _) in enumerate(nodes)}
        at += n + len(nodes)
        files["file_size"][f] = n * ds - 7
        files["direct"][f, :min(n, 12)] = data_blk[:12]
        entries = {nid: np.zeros(I, np.uint32) for nid, _, _ in nodes}
        for nid, parent, slot in nodes:
            if parent is None:
                files[("indirect", "doubly_indirect", "trebly_indirect")[slot - 12]][f] = node_blk[nid]
            else:
                entries[parent][slot] = node_blk[nid]
        for j in range(12, n):
            nid, slot = leaf_of(j, I)
            entries[nid][slot] = data_blk[j]
        for nid, _, _ in nodes:
            payload[node_blk[nid]] = 0
            payload[node_blk[nid], :4 * I] = entries[nid].view(np.uint8)
    image = torch.zeros(blocks * raw, dtype=torch.uint8, device="cuda")
    eng.encode(torch.from_numpy(payload.reshape(-1)).cuda(), image)
    return files, image, int(sum(sizes)), index_blocks


def batch_of(eng, workload: str, nfiles: int):
    """(the batch's file records, its (offset, nbytes) ranges, device image, file blocks in the image, index blocks)"""
    import numpy as np

    ds = eng.data_size
    I = ds // 4
    rng = np.random.default_rng(20250405)
    if workload == "big":
        sizes = [100000]
    elif workload == "small":
        sizes = rng.integers(1, 13, nfiles).tolist()
    else:
        sizes = rng.integers(13, 12 + 4 * I + 1, 2000).tolist()
    files, image, nblocks, index_blocks = build(eng, sizes)
    if workload != "records":
        ranges = np.stack([np.zeros(len(sizes), np.uint64), files["file_size"].astype(np.uint64)], axis=1)
        return files, np.ascontiguousarray(ranges), image, nblocks, index_blocks
    sel, ranges = [], []
    for f, n in enumerate(sizes):  # five records of 128 bytes in five distinct blocks of every file
        for j in sorted(rng.choice(n - 1, 5, replace=False).tolist()):
            sel.append(f)
            ranges.append((j * ds + int(rng.integers(0, ds - 128 + 1)), 128))
    return np.ascontiguousarray(files[sel]), np.array(ranges, np.uint64).reshape(-1, 2), image, nblocks, index_blocks


def worker(typ: int, bs: int, t: int, workload: str, nfiles: int, reps: int, launches: bool) -> dict:
    import numpy as np
    import torch

    from paritypartyfs_amd import EccEngine
    from paritypartyfs_amd._native import EXTENT_DTYPE

    torch.cuda.set_device(0)
    eng = EccEngine(typ, bs, t)
    ds = eng.data_size
    files, ranges, image, image_file_blocks, index_blocks = batch_of(eng, workload, nfiles)
    n = files.size
    slots, totals = eng.files_plan(files, ranges)
    nb, nbytes = int(totals["blocks"]), int(totals["bytes"])
    rng = np.random.default_rng(7)
    datas = [torch.from_numpy(rng.integers(0, 256, nbytes, dtype=np.uint8)).cuda() for _ in range(3)]
    st = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    ps = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    ix = torch.zeros(nb, dtype=torch.int32, device="cuda")
    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    written = torch.zeros(n, dtype=torch.int64, device="cuda")
    counts = torch.zeros(8, dtype=torch.int64, device="cuda")
    out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def write_files(data):
        eng.write_files(data, image, files, ranges, st, flags, written=written, counts=counts)

    if launches:
        write_files(datas[0])
        torch.cuda.synchronize()
        eng.read_files(image, files, ranges, out)
        assert torch.equal(out, datas[0])
        return dict(files=n, blocks=nb)

    def four_step(data):
        eng.files_blocks(image, files, ranges, ix, ps)
        torch.cuda.synchronize()
        index, path = ix.cpu().numpy().view(np.uint32), ps.cpu().numpy()
        s, _ = eng.files_plan(files, ranges)
        rep = np.repeat(np.arange(n), s["blocks"].astype(np.int64))
        k = np.arange(nb, dtype=np.uint64) - s["block_pos"][rep]
        off0 = (ranges[:, 0] % np.uint64(ds))[rep]
        first = k == 0
        ext = np.zeros(nb, EXTENT_DTYPE)
        pos = np.where(first, np.uint64(0), k * np.uint64(ds) - off0)
        offset = np.where(first, off0, np.uint64(0))
        ext["pos"] = s["out_pos"][rep] + pos
        ext["block"] = np.where(path != 0, np.uint32(NO_BLOCK), index)
        ext["offset"] = offset
        ext["length"] = np.minimum(np.uint64(ds) - offset, s["bytes"][rep] - pos)
        eng.write_extents(data, image, torch.from_numpy(ext.view(np.uint8)).cuda(), st)

    spread = {}

    def timed(name, fn, data):
        us = []
        for r in range(reps + 2):  # two warm-up runs
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(data)
            torch.cuda.synchronize()
            if r >= 2:
                us.append((time.perf_counter() - t0) * 1e6)
        spread[name + "_minmax_us"] = [min(us), max(us)]
        return statistics.median(us)

    def checked(name, data):
        assert int(st.max()) == 0, f"{name}: a block failed"
        eng.read_files(image, files, ranges, out)
        assert torch.equal(out, data), f"{name}: the image does not hold what was written"
        out.zero_()

    res = {}
    res["write_files_us"] = timed("write_files", write_files, datas[0])
    assert int(flags.abs().max()) == 0 and written.cpu().numpy().tolist() == ranges[:, 1].tolist()
    assert counts.cpu().numpy().tolist()[0] == nb
    checked("write_files", datas[0])
    res["four_step_us"] = timed("four_step", four_step, datas[1])
    checked("the four-step path", datas[1])
    # the same bytes through both: the raw images must be equal
    write_files(datas[2])
    torch.cuda.synchronize()
    a = image.clone()
    four_step(datas[0])
    four_step(datas[2])
    torch.cuda.synchronize()
    assert torch.equal(a, image), "the two paths leave different images"
    res.update(spread)
    res["four_step_over_write_files"] = res["four_step_us"] / res["write_files_us"]
    res.update(ranges=int(n), blocks=nb, bytes=nbytes, image_file_blocks=image_file_blocks, index_blocks=index_blocks,
               raw_block_size=eng.raw_block_size, data_size=ds, entries_per_index_block=ds // 4, reps=reps,
               list_kernel=eng.list_kernel_name(), device=torch.cuda.get_device_name(0), rocm=str(torch.version.hip))
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=0)
    ap.add_argument("--worker", default="")
    a = ap.parse_args()
    if a.launches:
        print(json.dumps(worker(4, 512, 3, "small", a.launches, 0, True)))
        return 0
    if a.worker:
        typ, bs, t, workload = a.worker.split(",")
        print(json.dumps(worker(int(typ), int(bs), int(t), workload, 10000, a.reps, False)))
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
            print(f"{name} {workload}: {r['ranges']} ranges, {r['blocks']} blocks | write_files "
                  f"{r['write_files_us'] / 1e3:.3f} ms vs four-step {r['four_step_us'] / 1e3:.3f} ms = "
                  f"x{r['four_step_over_write_files']:.2f}", flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
