#!/usr/bin/env python3
"""Where the shortcut convolutions sit in a traced step: two `rocprofv3 --kernel-trace` CSVs of the same bench command, the
parent's and the branch's, read launch by launch (profiles/conv1x1/README.md).

    python tools/conv1x1_launches.py parent_kernel_trace.csv branch_kernel_trace.csv > profiles/conv1x1/launches.txt

One steady step a side (between the last two launches of the fused forward kernel), per hardware queue in launch order.
The two name sequences of a queue are aligned (difflib); every stretch where the branch launches a `conv1x1s2_*` kernel is
one shortcut call, and the parent's launches of the same stretch are what MIOpen (and ATen, for the `add` behind a data
gradient) ran for it.  Printed: kernel time per step of the last five steady steps, the kernels whose count per step
differs, and the stretches with each side's launches and microseconds."""
import collections
import csv
import difflib
import statistics
import sys


def steps(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    idx = [i for i, r in enumerate(rows) if "warp_ssim_min_fwd" in r["Kernel_Name"]]
    out = []
    for a, b in zip(idx[:-1], idx[1:]):
        out.append([(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, r["Queue_Id"],
                     int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows[a:b]])
    return out


def short(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    if "vectorized_elementwise_kernel" in name or "elementwise_kernel_manual_unroll" in name:
        for functor in ("CUDAFunctor_add", "CUDAFunctorOnSelf_add", "FillFunctor", "MulFunctor", "BinaryFunctor", "BUnaryFunctor",
                        "AUnaryFunctor"):
            if functor in name:
                return "aten elementwise <%s>" % functor
        return "aten elementwise"
    return name.split("(")[0][:72]


def main():
    sides = {"parent": steps(sys.argv[1]), "branch": steps(sys.argv[2])}
    for side, st in sides.items():
        last = st[-5:]
        sums = [sum(k[1] for k in s) for s in last]
        print("%s: kernel time per step, last five steady steps: %s us (median %.0f); step %d launches, wall %.0f us"
              % (side, " ".join("%.0f" % v for v in sums), statistics.median(sums), len(st[-1]),
                 (max(k[4] for k in st[-1]) - min(k[3] for k in st[-1])) / 1e3))
    p, b = sides["parent"][-1], sides["branch"][-1]
    cp, cb = collections.Counter(short(k[0]) for k in p), collections.Counter(short(k[0]) for k in b)
    print("\nkernels whose launch count per step differs (parent -> branch), with each side's durations in us:")
    for name in sorted(set(cp) | set(cb)):
        if cp[name] != cb[name]:
            print("  %-74s %3d -> %3d   sum %8.1f -> %8.1f" % (name, cp[name], cb[name], sum(k[1] for k in p if short(k[0]) == name),
                                                              sum(k[1] for k in b if short(k[0]) == name)))
    print("\nstretches of the step where the branch launches a conv1x1s2 kernel, per queue in launch order:")
    total_p = total_b = 0.0
    queues = sorted({k[2] for k in b if "conv1x1s2" in k[0]})
    # a queue is numbered by the runtime: pair the sides' queues by their launch counts
    for q in queues:
        bq = [k for k in b if k[2] == q]
        pq = max(({qq: [k for k in p if k[2] == qq] for qq in {k[2] for k in p}}).values(),
                 key=lambda ks: difflib.SequenceMatcher(None, [short(k[0]) for k in ks], [short(k[0]) for k in bq],
                                                        autojunk=False).ratio())
        sm = difflib.SequenceMatcher(None, [short(k[0]) for k in pq], [short(k[0]) for k in bq], autojunk=False)
        for tag, i1, i2, j1, j2 in sm.get_opcodes():
            if tag == "equal":
                continue
            mine = bq[j1:j2]
            print("  queue %s, %s:" % (q, "a shortcut call" if any("conv1x1s2" in k[0] for k in mine) else "another difference"))
            for k in pq[i1:i2]:
                print("      parent  %7.1f us  %s" % (k[1], short(k[0])))
            for k in mine:
                print("      branch  %7.1f us  %s" % (k[1], short(k[0])))
            sp, sb = sum(k[1] for k in pq[i1:i2]), sum(k[1] for k in mine)
            total_p, total_b = total_p + sp, total_b + sb
            print("      %d launches, %.1f us -> %d launches, %.1f us" % (i2 - i1, sp, j2 - j1, sb))
    print("\nall stretches: parent %.1f us, branch %.1f us per step" % (total_p, total_b))


if __name__ == "__main__":
    main()
