"""bench_files.py -- what reading many files in one call costs next to one read_file call per file.

Two workloads, each on a clean, device-resident image whose data and index blocks are placed by a seeded
permutation (so every file is fragmented), for RS(255,249) (block size 512, t = 3: the direct list path) and
Hamming-512 (staged); I = entries per index block:
  small   10,000 files of 1 .. 12 blocks, seeded sizes: no tree at all, pure fixed cost
  tree    2,000 files of 13 .. 12 + I + 3 I blocks: every file has an indirect block, about half a doubly tree
Timed as wall-clock time of the calling thread from the first call to the synchronised stream, median of --reps
runs after two warm-up runs, the runs of one leg back to back, with the spread (*_minmax_us):
  batch        EccEngine.read_files of all the files, every file whole: one call
  loop         the way before that call: EccEngine.read_file per file on one stream, synchronised once at the end
Both sides' bytes are compared with what was written.  Recorded, not gating: DESIGN.md section 4.11.

--launches N runs one read_files call over N small files and nothing else, for a kernel trace of its own: the
number of launches must not depend on N.

Every (codec, workload) is measured in a child process of its own under a time limit; the first child that fails
ends the run.

    python tools/bench_files.py [--reps 9 --out profiles/files_io.json]
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
WORKLOADS = {"small": 10000, "tree": 2000}
STEP_TIMEOUT_S = 400


def build(eng, workload: str, nfiles: int):
    """(files, device image, the bytes written file after file, block counts)"""
    import numpy as np
    import torch

    from paritypartyfs_amd import FILE_DTYPE

    raw, ds = eng.raw_block_size, eng.data_size
    I = ds // 4
    S1 = 12 + I
    rng = np.random.default_rng(20250202)
    sizes = rng.integers(1, 13, nfiles) if workload == "small" else rng.integers(13, 12 + I + 3 * I + 1, nfiles)
    index_blocks = sum(0 if n <= 12 else 1 if n <= S1 else 2 + -(-(n - S1) // I) for n in sizes.tolist())
    blocks = int(sizes.sum()) + index_blocks + 16
    perm = rng.permutation(blocks).astype(np.uint32)
    payload = rng.integers(0, 256, (blocks, ds), dtype=np.uint8)
    files = np.zeros(nfiles, FILE_DTYPE)
    at, want = 0, []

    def node(entries):
        nonlocal at
        b = int(perm[at])
        at += 1
        payload[b] = 0
        payload[b, :4 * entries.size] = entries.astype("<u4").view(np.uint8)
        return b

    for f, n in enumerate(sizes.tolist()):
        data = perm[at:at + n]
        at += n
        size = n * ds - 7
        files["file_size"][f] = size
        files["direct"][f, :min(n, 12)] = data[:12]
        if n > 12:
            files["indirect"][f] = node(data[12:min(n, S1)])
        if n > S1:
            files["doubly_indirect"][f] = node(np.array([node(data[a:min(n, a + I)]) for a in range(S1, n, I)], np.uint32))
        want.append(payload[data].reshape(-1)[:size])
    image = torch.zeros(blocks * raw, dtype=torch.uint8, device="cuda")
    eng.encode(torch.from_numpy(payload.reshape(-1)).cuda(), image)
    return files, image, np.concatenate(want), int(sizes.sum()), index_blocks


def worker(typ: int, bs: int, t: int, workload: str, nfiles: int, reps: int, launches: bool) -> dict:
    import numpy as np
    import torch

    from paritypartyfs_amd import EccEngine

    torch.cuda.set_device(0)
    eng = EccEngine(typ, bs, t)
    files, image, want, nblocks, index_blocks = build(eng, workload, nfiles)
    slots, totals = eng.files_plan(files)
    assert int(totals["blocks"]) == nblocks and int(totals["bytes"]) == want.size and int(totals["tree_blocks"]) == index_blocks
    out = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
    st = torch.zeros(nblocks, dtype=torch.uint8, device="cuda")
    flags = torch.zeros(nfiles, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if launches:
        eng.read_files(image, files, None, out, st, flags)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)
        return dict(files=nfiles, blocks=nblocks)
    records = [files[f:f + 1] for f in range(nfiles)]
    sizes = files["file_size"].tolist()
    outs = [out[int(s["out_pos"]):int(s["out_pos"]) + int(s["bytes"])] for s in slots]
    sts = [st[int(s["block_pos"]):int(s["block_pos"]) + int(s["blocks"])] for s in slots]

    def loop():
        for f in range(nfiles):
            eng.read_file(image, records[f], 0, sizes[f], outs[f], sts[f])

    spread = {}

    def timed(name, fn):
        """median wall-clock microseconds of fn() from the call to the synchronised stream; the runs of one leg
        follow each other directly"""
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

    def checked(name):
        assert int(st.max()) == 0 and np.array_equal(out.cpu().numpy(), want), f"{name} differs from what was written"
        out.zero_()

    res = {}
    res["batch_us"] = timed("batch", lambda: eng.read_files(image, files, None, out, st, flags))
    assert int(flags.abs().max()) == 0
    checked("read_files")
    res["loop_us"] = timed("loop", loop)
    checked("the read_file loop")
    res.update(spread)
    res["loop_over_batch"] = res["loop_us"] / res["batch_us"]
    res.update(files=nfiles, blocks=nblocks, index_blocks=index_blocks, bytes=int(want.size), raw_block_size=eng.raw_block_size,
               data_size=eng.data_size, entries_per_index_block=eng.data_size // 4, reps=reps, list_kernel=eng.list_kernel_name(),
               device=torch.cuda.get_device_name(0), rocm=str(torch.version.hip))
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
        print(json.dumps(worker(int(typ), int(bs), int(t), workload, WORKLOADS[workload], a.reps, False)))
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
            print(f"{name} {workload}: {r['files']} files, {r['blocks']} blocks, {r['index_blocks']} index blocks | batch "
                  f"{r['batch_us'] / 1e3:.2f} ms vs loop {r['loop_us'] / 1e3:.2f} ms = "
                  f"x{r['loop_over_batch']:.1f}", flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
