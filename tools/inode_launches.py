"""inode_launches.py -- the launch record of the inode calls (profiles/inode_walk_refactor_launches.txt).

Run: one two-piece EccEngine.read_inodes and one two-piece EccEngine.write_inodes per context -- RS(255,249) direct,
RS(255,249) created under PPFS_ECC_LIST_DIRECT=0 (staged), Hamming-512 -- on an image of 4,096 inodes, a batch being
the call's piece plus 3 numbers (one past the table).  A one-element torch fill of a float tensor separates the calls
in a kernel trace.  Reduce: per call the dispatches in start order, kernel name, grid (threads) and workgroup size.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- python tools/inode_launches.py
    python tools/inode_launches.py --reduce DIR/.../trace_kernel_trace.csv > record.txt
(PPFS_ECC_LIB names another build of the library, as everywhere.)
"""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TOTAL = 4096
CONTEXTS = [("rs-direct", 4, 512, 3, None), ("rs-staged", 4, 512, 3, "0"), ("hamming-512", 2, 512, 0, None)]
LABELS = [f"{name} {call}" for name, *_ in CONTEXTS for call in ("setup", "read_inodes", "write_inodes")]


def run() -> None:
    import numpy as np
    import torch

    from paritypartyfs_amd import INODE_TABLE_DTYPE, EccEngine

    torch.cuda.set_device(0)
    mark = torch.empty(1, dtype=torch.float32, device="cuda")  # no fill of its own: every float fill is a separator
    rng = np.random.default_rng(20251021)
    for name, typ, bs, t, direct in CONTEXTS:
        if direct is not None:
            os.environ["PPFS_ECC_LIST_DIRECT"] = direct
        eng = EccEngine(typ, bs, t)
        os.environ.pop("PPFS_ECC_LIST_DIRECT", None)
        raw, ds = eng.raw_block_size, eng.data_size
        K = 2 + 79 // ds
        bm_blocks, t_blocks = -(-(TOTAL // 8) // ds), -(-81 * TOTAL // ds)
        table = np.zeros(1, INODE_TABLE_DTYPE)
        table["bitmap_block"], table["table_block"], table["total_inodes"], table["check_bitmap"] = 1, 2 + bm_blocks, TOTAL, 1
        blocks = 2 + bm_blocks + t_blocks + 1
        payload = rng.integers(0, 256, (blocks, ds), dtype=np.uint8)
        image = torch.zeros(blocks * raw, dtype=torch.uint8, device="cuda")
        eng.encode(torch.from_numpy(payload.reshape(-1)).cuda(), image)
        staged = max(1024, min(eng.host_chunk_blocks() & ~1023, max(1024, ((1 << 31) // raw) & ~1023)))  # list_plan.hpp piece_blocks
        piece = {"read": 32768 // K, "write": min(32768 // K, max(staged // K, 1))}
        bufs = {}
        for call in ("read", "write"):
            n = piece[call] + 3
            nums = rng.integers(0, TOTAL, n).astype(np.uint32)
            nums[n // 2] = TOTAL
            bufs[call] = (torch.from_numpy(nums.view(np.int32)).cuda(), torch.zeros(64 * n, dtype=torch.uint8, device="cuda"),
                          torch.zeros(24 * n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"),
                          torch.zeros(n * (1 + K), dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        mark.fill_(1.0)  # ends the context's setup
        d_nums, files, meta, status, pieces = bufs["read"]
        eng.read_inodes(image, table, d_nums, files=files, meta=meta, status=status, piece_status=pieces, counts=True)
        torch.cuda.synchronize()
        mark.fill_(2.0)
        d_nums, files, meta, status, pieces = bufs["write"]
        eng.write_inodes(image, table, d_nums, files, meta, status=status, piece_status=pieces, counts=True)
        torch.cuda.synchronize()
        mark.fill_(3.0)
        torch.cuda.synchronize()
        print(f"{name}: read_inodes {piece['read'] + 3} numbers, write_inodes {piece['write'] + 3}, K = {K}, list kernel "
              f"{eng.list_kernel_name()}", flush=True)


def short(name: str) -> str:
    n = re.sub(r"^void ", "", name)
    n = re.sub(r"\(.*$", "", n) if not n.startswith("(") else n
    return n.replace("ppfs::", "").replace("at::native::", "")


def reduce(path: str) -> None:
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), short(r["Kernel_Name"]),
                         "x".join(r[f"Grid_Size_{a}"] for a in "XYZ"), "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")))
    rows.sort()
    part, parts = [], []
    for _, name, grid, wg in rows:
        if "FillFunctor<float>" in name and grid.split("x")[0] == wg.split("x")[0]:  # the separator: one workgroup
            parts.append(part)
            part = []
        else:
            part.append(f"    {name} grid {grid} wg {wg}")
    assert len(parts) == len(LABELS), (len(parts), len(LABELS))
    for label, part in zip(LABELS, parts):
        if not label.endswith("setup"):
            print(label + f" ({len(part)} dispatches)")
            print("\n".join(part) + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--reduce":
        reduce(sys.argv[2])
    else:
        run()
