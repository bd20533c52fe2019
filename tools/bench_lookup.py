"""bench_lookup.py -- what looking up a batch of names in one call costs next to what was there before it.

100 directories of 300 entries each (155 blocks at ds = 249: direct, indirect and doubly indirect blocks; 76 at ds = 508) on a clean,
device-resident image, for RS(255,249) (block size 255, t = 3: the direct list path) and Hamming-512 (staged).  The
queries are names drawn uniformly over the directories and their entries, one in ten a name that no entry has.
Timed as wall-clock time of the calling thread from the first call to the synchronised stream, median of --reps runs
after two warm-up runs, the runs of one leg back to back, with the spread (*_minmax_us):
  lookup        EccEngine.lookup: the hit records in device memory (lookup_to_host_us: and copied to the host)
  copy_match    the best the engine offered before: one EccEngine.read_files of the 100 directories, the payloads
                copied to page-locked host memory, and a numpy match there -- per directory the names cut at their NUL,
                sorted once, every query placed by binary search (the first of equal names wins)
  read_files    the read_files call alone: what both ways share
  loop          the reference's way, on --loop-queries of the queries and scaled to all of them: per query one
                EccEngine.read_file per 256-entry batch up to the match, copied to the host and matched there
for nq = 10,000 and, to see where the device match starts to pay, for the other sizes of --sweep.  Every leg's answers
are compared with the entries that were written.  Recorded, not gating: DESIGN.md section 4.16.

Every codec is measured in a child process of its own under a time limit; the first child that fails ends the run.

    python tools/bench_lookup.py [--reps 7 --out profiles/lookup.json]
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

CODECS = [("RS(255,249)", 4, 255, 3), ("Hamming-512", 2, 512, 0)]
NDIRS, NENTRIES, NQ = 100, 300, 10000
STEP_TIMEOUT_S = 400


def build(eng):
    """(directory records, device image, the entries as (NDIRS, NENTRIES, 128) bytes)"""
    import numpy as np
    import torch

    from paritypartyfs_amd import FILE_DTYPE

    raw, ds = eng.raw_block_size, eng.data_size
    ipb = ds // 4
    rng = np.random.default_rng(20250606)
    entries = np.full((NDIRS, NENTRIES, 128), 0xEE, np.uint8)  # garbage behind every NUL
    for d in range(NDIRS):
        for i in range(NENTRIES):
            name = b"file_%04d_in_directory_%03d.dat" % (i * 7919 % 10007, d) if i % 2 else b"n%d" % (i * 31 + d)
            entries[d, i, :4] = np.frombuffer(np.uint32(1 + d * NENTRIES + i).tobytes(), np.uint8)
            entries[d, i, 4:4 + len(name)] = np.frombuffer(name, np.uint8)
            entries[d, i, 4 + len(name)] = 0
    nb = -(-NENTRIES * 128 // ds)
    assert 12 < nb <= 12 + ipb + ipb * ipb
    leaves = -(-max(nb - 12 - ipb, 0) // ipb)  # none: the indirect block holds the rest (Hamming-512)
    per_dir = nb + 2 + leaves
    blocks = 1 + NDIRS * per_dir
    payload = np.zeros((blocks, ds), np.uint8)
    files = np.zeros(NDIRS, FILE_DTYPE)
    for d in range(NDIRS):
        base = 1 + d * per_dir
        data = base + np.arange(nb, dtype=np.uint32)
        payload[base:base + nb].reshape(-1)[:NENTRIES * 128] = entries[d].reshape(-1)
        files["direct"][d] = data[:12]
        at = base + nb
        files["indirect"][d] = at
        under = data[12:12 + ipb].astype("<u4")
        payload[at, :4 * under.size] = under.view(np.uint8)
        if not leaves:
            files["file_size"][d] = NENTRIES * 128 + int(rng.integers(0, 128))
            continue
        files["doubly_indirect"][d] = at + 1
        top = np.zeros(ipb, "<u4")
        for k in range(leaves):
            top[k] = at + 2 + k
            part = data[12 + ipb + k * ipb:12 + ipb + (k + 1) * ipb].astype("<u4")
            payload[at + 2 + k, :4 * part.size] = part.view(np.uint8)
        payload[at + 1, :4 * ipb] = top.view(np.uint8)
        files["file_size"][d] = NENTRIES * 128 + int(rng.integers(0, 128))
    image = torch.zeros(blocks * raw, dtype=torch.uint8, device="cuda")
    eng.encode(torch.from_numpy(payload.reshape(-1)).cuda(), image)
    return files, image, entries


def queries_of(entries, nq):
    """(LOOKUP_QUERY_DTYPE array, the name records, the entry each query must find or -1)"""
    import numpy as np

    from paritypartyfs_amd import LOOKUP_QUERY_DTYPE

    rng = np.random.default_rng(20250607 + nq)
    q = np.zeros(nq, LOOKUP_QUERY_DTYPE)
    q["dir"] = rng.integers(0, NDIRS, nq)
    pick = rng.integers(0, NENTRIES, nq)
    rec = entries[q["dir"], pick, 4:].copy()
    rec = np.concatenate([rec, np.zeros((nq, 4), np.uint8)], axis=1)
    miss = rng.random(nq) < 0.1
    rec[miss, 0] = ord("#")  # no entry's name starts like this
    return q, np.ascontiguousarray(rec), np.where(miss, -1, pick)


def cut_names(names):
    """Name bytes (..., 124) with everything from the first NUL on set to zero."""
    import numpy as np

    return np.where(np.logical_and.accumulate(names != 0, axis=-1), names, 0).astype(np.uint8)


def host_match(payload, q, rec):
    """The numpy match over the payloads of read_files: per directory the names cut at their NUL and sorted once, the
    queries placed by binary search; the entry found or -1, and the inode numbers."""
    import numpy as np

    ent = payload[:NDIRS * NENTRIES * 128].reshape(NDIRS, NENTRIES, 128)
    names = cut_names(ent[:, :, 4:])
    keys = np.ascontiguousarray(names).view("S124").reshape(NDIRS, NENTRIES)  # cut names hold no NUL before their end
    want = np.ascontiguousarray(cut_names(rec[:, :124])).view("S124").reshape(-1)
    usable = (rec[:, :124] == 0).any(axis=1)  # a query without a NUL in 124 bytes matches nothing
    found = np.full(q.size, -1, np.int64)
    order = np.argsort(q["dir"], kind="stable")
    bounds = np.searchsorted(q["dir"][order], np.arange(NDIRS + 1))
    for d in range(NDIRS):
        mine = order[bounds[d]:bounds[d + 1]]
        if not mine.size:
            continue
        by_name = np.argsort(keys[d], kind="stable")
        at = np.searchsorted(keys[d][by_name], want[mine])
        at = np.minimum(at, NENTRIES - 1)
        hit = keys[d][by_name][at] == want[mine]
        found[mine] = np.where(hit & usable[mine], by_name[at], -1)
    inode = np.where(found >= 0, ent[q["dir"], np.maximum(found, 0), :4].copy().view("<u4").reshape(-1), 0xFFFFFFFF)
    return found, inode


def worker(typ: int, bs: int, t: int, reps: int, sweep, loop_queries: int) -> dict:
    import numpy as np
    import torch

    from paritypartyfs_amd import LOOKUP_HIT_DTYPE, EccEngine

    torch.cuda.set_device(0)
    eng = EccEngine(typ, bs, t)
    files, image, entries = build(eng)
    slots, totals = eng.lookup_plan(files)
    nbytes, nb = int(totals["bytes"]), int(totals["blocks"])
    ranges = np.stack([np.zeros(NDIRS, np.uint64), np.full(NDIRS, NENTRIES * 128, np.uint64)], axis=1)
    d_entries = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    d_status = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    h_entries = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
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

    res = {"sizes": {}}
    res["read_files_us"] = timed("read_files", lambda: eng.read_files(image, files, ranges, d_entries, d_status))
    for nq in sweep:
        q, rec, want = queries_of(entries, nq)
        want_inode = np.where(want >= 0, 1 + q["dir"].astype(np.int64) * NENTRIES + want, 0xFFFFFFFF)
        d_names = torch.from_numpy(rec.reshape(-1)).cuda()
        d_hits = torch.zeros(4 * nq, dtype=torch.int32, device="cuda")
        h_hits = torch.zeros(4 * nq, dtype=torch.int32).pin_memory()
        host = {}

        def lookup():
            eng.lookup(image, files, q, d_names, 0, d_entries, d_status, d_hits)

        def lookup_to_host():
            lookup()
            h_hits.copy_(d_hits, non_blocking=True)

        def copy_match():
            eng.read_files(image, files, ranges, d_entries, d_status)
            h_entries.copy_(d_entries, non_blocking=True)
            torch.cuda.synchronize()
            host["found"], host["inode"] = host_match(h_entries.numpy(), q, rec)

        r = {}
        r["lookup_us"] = timed(f"lookup_{nq}", lookup)
        hits = d_hits.cpu().numpy().view(np.uint32).view(LOOKUP_HIT_DTYPE)
        assert np.array_equal(hits["status"], np.where(want >= 0, 0, 2)) and np.array_equal(hits["inode"], want_inode)
        assert np.array_equal(hits["entry"][want >= 0], want[want >= 0])
        r["lookup_to_host_us"] = timed(f"lookup_to_host_{nq}", lookup_to_host)
        r["copy_match_us"] = timed(f"copy_match_{nq}", copy_match, sync=False)
        assert np.array_equal(host["found"], want) and np.array_equal(host["inode"], want_inode)
        r["copy_match_over_lookup_to_host"] = r["copy_match_us"] / r["lookup_to_host_us"]
        r["match_and_finish_us"] = r["lookup_us"] - res["read_files_us"]
        if nq == NQ:
            m = min(loop_queries, nq)
            one = torch.zeros(256 * 128, dtype=torch.uint8, device="cuda")
            got = np.full(m, -1, np.int64)

            def loop():
                for k in range(m):
                    f, name = files[int(q["dir"][k]):int(q["dir"][k]) + 1], cut_names(rec[k, :124]).tobytes()
                    got[k] = -1
                    for checked in range(0, NENTRIES, 256):
                        size = min(256, NENTRIES - checked)
                        eng.read_file(image, f, checked * 128, size * 128, one)
                        batch = cut_names(one[:size * 128].cpu().numpy().reshape(size, 128)[:, 4:])
                        at = np.flatnonzero(np.ascontiguousarray(batch).view("S124").reshape(-1) == np.frombuffer(name, "S124")[0])
                        if at.size:
                            got[k] = checked + int(at[0])
                            break

            r["loop_queries"] = m
            r["loop_us_scaled"] = timed("loop", loop, sync=False) * nq / m
            assert np.array_equal(got, want[:m])
            r["loop_over_lookup_to_host"] = r["loop_us_scaled"] / r["lookup_to_host_us"]
        res["sizes"][str(nq)] = r
    res.update(spread)
    res.update(directories=NDIRS, entries=NENTRIES, blocks=nb, entry_bytes=nbytes, raw_block_size=eng.raw_block_size,
               data_size=eng.data_size, reps=reps, list_kernel=eng.list_kernel_name(), device=torch.cuda.get_device_name(0),
               rocm=str(torch.version.hip))
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweep", default="100,1000,10000,100000")
    ap.add_argument("--loop-queries", type=int, default=200)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", default="")
    a = ap.parse_args()
    sweep = [int(x) for x in a.sweep.split(",")]
    if a.worker:
        typ, bs, t = a.worker.split(",")
        print(json.dumps(worker(int(typ), int(bs), int(t), a.reps, sweep, a.loop_queries)))
        return 0
    results = {}
    for name, typ, bs, t in CODECS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", f"{typ},{bs},{t}", "--reps", str(a.reps), "--sweep",
                                a.sweep, "--loop-queries", str(a.loop_queries)], capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {STEP_TIMEOUT_S} s; stopping", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"{name}: worker failed ({p.returncode}); stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            return 1
        r = results[name] = json.loads(p.stdout.strip().splitlines()[-1])
        print(f"{name}: read_files alone {r['read_files_us'] / 1e3:.3f} ms", flush=True)
        for nq, s in r["sizes"].items():
            loop = f"; loop (scaled from {s['loop_queries']}) {s['loop_us_scaled'] / 1e3:.1f} ms" if "loop_us_scaled" in s else ""
            print(f"  nq {nq}: lookup {s['lookup_us'] / 1e3:.3f} ms (to host {s['lookup_to_host_us'] / 1e3:.3f} ms) vs copy and match "
                  f"{s['copy_match_us'] / 1e3:.3f} ms = x{s['copy_match_over_lookup_to_host']:.2f}{loop}", flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
