#!/usr/bin/env python3
"""Which kernels a similarity call launches: a fixed list of small shapes through every route of mdir_amd/csrc/mdx_index.hip,
to be run under `rocprofv3 --kernel-trace` once per library build (MDIR_AMD_LIB selects the build), and the comparison of
two such traces.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/scores_launches.py run
    python3 tools/scores_launches.py compare A_kernel_trace.csv B_kernel_trace.csv

`run` issues the calls in a fixed order and checks no value (tests/test_gpu_lattice.py pins the values): every storage, every
compute mode, the row-major call and a routed (mdx_scores_p2p) step, over shapes of tests/lattice.py on both sides of every
threshold.  MDX_NO_PASS_GRID, MDX_NO_QUERY_SPLIT, MDX_NO_LEFTOVER_MFMA and MDX_F16_RING are read once per process: one run
per setting.  MDX_SCORES_PIPE is read per launch: the R = 2 shapes are repeated with it set to 0 inside the one run.
`compare` holds the ordered lists of (kernel, grid, workgroup, LDS bytes) of the `mdx::` kernels against each other."""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def shapes():
    import lattice
    r1 = [(1, 1, 1), (17, 64, 16), (64, 100, 112), (65, 128, 113), (129, 256, 257), (17, 1, 257), (64, 8, 128), (8192, 64, 128),
          (8193, 64, 128), (16401, 65, 50)]
    assert all(t in lattice.TRIPLES for t in r1)
    chain = r1 + lattice.R2_TRIPLES
    split = r1[:6] + lattice.R2_TRIPLES[::3] + lattice.SPLIT_TRIPLES[-2:]
    f16 = lattice.F16_TRIPLES + lattice.R2_TRIPLES[::4]
    i8 = r1 + lattice.R2_TRIPLES[::2]
    return chain, split, f16, i8


def run():
    import numpy as np
    import torch
    from mdir_amd import ops
    from mdir_amd.sharded import shard_bounds
    dev = "cuda:0"
    chain, split, f16, i8 = shapes()
    made = {}

    def data(n, d, nq):
        if (n, d, nq) not in made:
            g = torch.Generator().manual_seed(n * 7 + d * 3 + nq)
            made.clear()
            made[(n, d, nq)] = (torch.randn(n, d, generator=g).to(dev), torch.randn(nq, d, generator=g).to(dev))
        return made[(n, d, nq)]

    def indexed(triples, storage, modes):
        for n, d, nq in triples:
            rows, q = data(n, d, nq)
            ix = ops.DescriptorIndex(rows, "ND", storage=storage)
            for mode in modes:
                ix.scores(q, "ND", compute=mode)
            if storage == "f32" and n > 32640:
                os.environ["MDX_SCORES_PIPE"] = "0"
                ix.scores(q, "ND")
                del os.environ["MDX_SCORES_PIPE"]
            torch.cuda.synchronize()
            ix.close()

    indexed(chain, "f32", ["chain"])
    indexed(split, "f32", ["split3", "split2"])
    indexed(f16, "f16", ["chain"])
    indexed(i8, "i8", ["chain"])
    for n, d, nq in chain:
        if d % 4 == 0:
            rows, q = data(n, d, nq)
            ops.scores_rowmajor(rows, q, "ND")
            torch.cuda.synchronize()
    # a routed step: two ranks in this process, each with a chunk below and one above the 128-row switch
    for n, nq, d, G in [(98400, 23, 64, 2), (98400, 32, 64, 2), (3000, 5, 64, 2), (20000, 70, 64, 2)]:
        rows, q = data(n, d, nq)
        peers = [ops.P2P(G, r, nq, n, dev) for r in range(G)]
        for p in peers:
            p.connect_local(peers)
        streams = [torch.cuda.Stream(device=dev) for _ in range(G)]
        parts = []
        for r in range(G):
            lo, hi = shard_bounds(n, G, r)
            cut = lo + (hi - lo) // 3
            parts.append([ops.DescriptorIndex(rows[lo:cut], "ND", lo), ops.DescriptorIndex(rows[cut:hi], "ND", cut)])
        torch.cuda.synchronize()
        for r in range(G):
            with torch.cuda.stream(streams[r]):
                for ix in parts[r]:
                    ix.scores_p2p(q, peers[r], "ND")
                peers[r].close_step()
        torch.cuda.synchronize()
        for r in range(G):
            for ix in parts[r]:
                ix.close()
            peers[r].close()
    print("scores_launches: done")


def launches(path):
    rows = [r for r in csv.DictReader(open(path)) if "mdx::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], tuple(int(r["Grid_Size_" + a]) for a in "XYZ"), tuple(int(r["Workgroup_Size_" + a]) for a in "XYZ"),
             int(r["LDS_Block_Size"])) for r in rows]


def compare(a, b):
    la, lb = launches(a), launches(b)
    diff = [i for i, (x, y) in enumerate(zip(la, lb)) if x != y]
    names = {x[0].split("(")[0] for x in la}
    print("launches: %d and %d, %d distinct kernels, differing positions: %d" % (len(la), len(lb), len(names), len(diff)))
    for i in diff[:10]:
        print("  #%d\n    %r\n    %r" % (i, la[i], lb[i]))
    return 0 if len(la) == len(lb) and not diff else 1


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
