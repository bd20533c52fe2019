"""bench_file.py -- what reading a file from its inode costs next to the walk the integrator had to run before.

A fragmented file of --blocks blocks (default 100,000) in a device-resident image, for RS(255,249) (block size
512, t = 3) and Hamming-512: data and index blocks placed by a seeded permutation, the image clean.  Timed as
wall-clock time of the calling thread from the call to the synchronised stream, median of --reps runs after two
warm-up runs, the runs of one leg back to back, with the spread (*_minmax_us):
  read_file                 EccEngine.read_file of the whole file: one call from the 64-byte inode record
  file_blocks               EccEngine.file_blocks of the whole file: the block list and the tree's statuses
against what the build offered before these calls for the same job:
  host walk                 the BlockIndexIterator loop on the CPU: every index block read with a one-entry
                            decode_list (index uploaded, payload read back, each read waiting for the one before)
  extents on the host       the file_extents entries of the resolved list, built with numpy, and their upload
  read_extents              one call over them
baseline_read = host walk + extents on the host + read_extents; baseline_blocks = host walk.  Both sides' bytes
and block lists are compared with what was written.  Recorded, not gating: DESIGN.md section 4.10.

Every codec is measured in a child process of its own under a time limit; the first child that fails ends
the run.

    python tools/bench_file.py [--blocks 100000 --reps 9 --out profiles/file_io.json]
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
STEP_TIMEOUT_S = 240


def tree_of(n, I):
    """The index blocks of a file of n blocks in walk order: (id, parent id or None, slot in the parent); an id is
    the path from the inode, (segment,), (segment, a) or (3, a, b)."""
    S1, S2 = 12 + I, 12 + I + I * I
    nodes = []
    if n > 12:
        nodes.append(((1,), None, 12))
    if n > S1:
        nodes.append(((2,), None, 13))
        nodes += [((2, a), (2,), a) for a in range(-(-(min(n, S2) - S1) // I))]
    if n > S2:
        nodes.append(((3,), None, 14))
        leaves = -(-(n - S2) // I)
        nodes += [((3, a), (3,), a) for a in range(-(-leaves // I))]
        nodes += [((3, f // I, f % I), (3, f // I), f % I) for f in range(leaves)]
    return nodes


def leaf_of(j, I):
    """(id of the index block that holds file block j's pointer, slot), j >= 12"""
    s = j - 12
    if s < I:
        return (1,), s
    s -= I
    if s < I * I:
        return (2, s // I), s % I
    s -= I * I
    return (3, s // (I * I), (s // I) % I), s % I


def worker(typ: int, bs: int, t: int, n: int, reps: int) -> dict:
    import numpy as np
    import torch

    from paritypartyfs_amd import FILE_DTYPE, EccEngine
    from paritypartyfs_amd._native import EXTENT_DTYPE

    torch.cuda.set_device(0)
    eng = EccEngine(typ, bs, t)
    raw, ds = eng.raw_block_size, eng.data_size
    I = ds // 4
    rng = np.random.default_rng(20250101)
    nodes = tree_of(n, I)
    blocks = n + len(nodes) + 16
    perm = rng.permutation(blocks).astype(np.uint32)
    data_blk, node_blk = perm[:n], {nid: int(perm[n + k]) for k, (nid, _, _) in enumerate(nodes)}
    file = np.zeros(1, FILE_DTYPE)
    file["file_size"] = n * ds - 7
    file["direct"][0, :min(n, 12)] = data_blk[:12]
    payload = rng.integers(0, 256, (blocks, ds), dtype=np.uint8)
    entries = {nid: np.zeros(I, np.uint32) for nid, _, _ in nodes}
    for nid, parent, slot in nodes:
        if parent is None:
            file[("indirect", "doubly_indirect", "trebly_indirect")[slot - 12]] = node_blk[nid]
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
    size = int(file["file_size"][0])
    want = payload[data_blk].reshape(-1)[:size]
    first, count, clamped = eng.file_span(file, 0, size)
    assert (first, count, clamped) == (0, n, size)

    out = torch.zeros(size, dtype=torch.uint8, device="cuda")
    st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ix = torch.zeros(n, dtype=torch.int32, device="cuda")
    one_pay = torch.zeros(ds + 16, dtype=torch.uint8, device="cuda")
    one_st = torch.zeros(16, dtype=torch.uint8, device="cuda")

    def host_walk():
        """The BlockIndexIterator loop: the block list of the whole file, one index block at a time."""
        loaded = {}

        def load(nid, pointer):
            one = torch.tensor([pointer], dtype=torch.int64).to(torch.int32).cuda()
            eng.decode_list(image, one, one_pay[:ds], one_st[:1], write_back=True)
            torch.cuda.synchronize()
            assert int(one_st[0]) <= 1
            loaded[nid] = one_pay[:4 * I].cpu().numpy().view("<u4").copy()
            return loaded[nid]

        f = file[0]
        lst = [f["direct"][:min(n, 12)].astype(np.uint32)]
        S1, S2 = 12 + I, 12 + I + I * I
        if n > 12:
            lst.append(load((1,), int(f["indirect"]))[:min(n, S1) - 12])
        if n > S1:
            root = load((2,), int(f["doubly_indirect"]))
            left = min(n, S2) - S1
            for a in range(-(-left // I)):
                lst.append(load((2, a), int(root[a]))[:min(I, left - a * I)])
        if n > S2:
            root = load((3,), int(f["trebly_indirect"]))
            left = n - S2
            for a in range(-(-left // (I * I))):
                mid = load((3, a), int(root[a]))
                for b in range(min(I, -(-(left - a * I * I) // I))):
                    lst.append(load((3, a, b), int(mid[b]))[:min(I, left - (a * I + b) * I)])
        return np.concatenate(lst)

    def host_extents(index):
        ext = np.zeros(index.size, EXTENT_DTYPE)
        ext["block"] = index
        ext["pos"] = np.arange(index.size, dtype=np.uint64) * ds
        ext["length"] = np.minimum(ds, size - ext["pos"].astype(np.int64))
        return torch.from_numpy(ext.view(np.uint8).copy()).cuda()

    spread = {}

    def timed(name, fn):
        """median wall-clock microseconds of fn() from the call to the synchronised stream; the runs of one leg
        follow each other directly, so that none starts on a device another leg's checks left idle"""
        us, r = [], None
        for k in range(reps + 2):  # two warm-up runs
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            if k >= 2:
                us.append((time.perf_counter() - t0) * 1e6)
        spread[name + "_minmax_us"] = [min(us), max(us)]
        return statistics.median(us), r

    res = {}
    out.zero_()
    res["read_file_us"], _ = timed("read_file", lambda: eng.read_file(image, file, 0, size, out, st))
    assert int(st.max()) == 0 and np.array_equal(out.cpu().numpy(), want), "read_file differs from what was written"
    res["file_blocks_us"], _ = timed("file_blocks", lambda: eng.file_blocks(image, file, 0, n, ix))
    assert np.array_equal(ix.cpu().numpy().view(np.uint32), data_blk), "file_blocks differs from the file's blocks"
    res["host_walk_us"], index = timed("host_walk", host_walk)
    assert np.array_equal(index, data_blk), "the host walk differs from the file's blocks"
    res["host_extents_us"], d_ext = timed("host_extents", lambda: host_extents(index))
    out.zero_()
    res["read_extents_us"], _ = timed("read_extents", lambda: eng.read_extents(image, d_ext, out, st))
    assert int(st.max()) == 0 and np.array_equal(out.cpu().numpy(), want), "read_extents differs from what was written"
    res.update(spread)
    res["baseline_read_us"] = res["host_walk_us"] + res["host_extents_us"] + res["read_extents_us"]
    res["baseline_read_over_read_file"] = res["baseline_read_us"] / res["read_file_us"]
    res["host_walk_over_file_blocks"] = res["host_walk_us"] / res["file_blocks_us"]
    res.update(blocks=n, tree_blocks=len(nodes), raw_block_size=raw, data_size=ds, entries_per_index_block=I, reps=reps,
               file_bytes=size, image_blocks=blocks, list_kernel=eng.list_kernel_name(), device=torch.cuda.get_device_name(0),
               rocm=str(torch.version.hip))
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", default="")
    a = ap.parse_args()
    if a.worker:
        typ, bs, t = (int(x) for x in a.worker.split(","))
        print(json.dumps(worker(typ, bs, t, a.blocks, a.reps)))
        return 0
    results = {}
    for name, typ, bs, t in CODECS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", f"{typ},{bs},{t}", "--blocks", str(a.blocks),
                                "--reps", str(a.reps)], capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {STEP_TIMEOUT_S} s; stopping", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"{name}: worker failed ({p.returncode}); stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            return 1
        results[name] = json.loads(p.stdout.strip().splitlines()[-1])
        r = results[name]
        print(f"{name}: {r['blocks']} blocks, {r['tree_blocks']} index blocks | read_file {r['read_file_us'] / 1e3:.2f} ms vs "
              f"walk {r['host_walk_us'] / 1e3:.2f} + extents {r['host_extents_us'] / 1e3:.2f} + read_extents "
              f"{r['read_extents_us'] / 1e3:.2f} ms = x{r['baseline_read_over_read_file']:.1f} | file_blocks "
              f"{r['file_blocks_us'] / 1e3:.2f} ms vs walk = x{r['host_walk_over_file_blocks']:.1f}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
