"""Where the fused hash+assign call's small kernels sit around its FAST kernel:
reads a rocprofv3 --kernel-trace CSV (of tools/time_fused.py, say) and prints,
over the last CALLS calls, every kernel's and fill's start and end relative to
the FAST kernel (fused_hi_kernel) -- before it: to its start, after it: to its
end -- with the length of the chain before it, the tail after it, the gap to
the next call's first kernel and the launches per call. Medians (min-max), us.

    python tools/trace_tail.py kernel_trace.csv [CALLS]
"""
import csv
import re
import statistics
import sys

PRE = ("fillBuffer", "fused_centroid_prep", "exact_prep_kernel")      # what runs ahead of the FAST kernel


def short(name):
    name = re.sub(r"\(.*", "", name)
    name = re.sub(r"^(void )?(lshkm::)?", "", name)
    return name[:44]


def main():
    path, ncalls = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 10
    ev = []
    with open(path) as f:
        for r in csv.DictReader(f):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"],
                       r.get("Queue_Id", r.get("Stream_Id", "?"))))
    ev.sort()
    fast = [i for i, e in enumerate(ev) if "fused_hi_kernel" in e[2]]
    # a call: from the first chain kernel after the previous FAST kernel to the last kernel before the next call's
    first = []
    for n, i in enumerate(fast):
        lo = fast[n - 1] + 1 if n else 0
        pre = [j for j in range(lo, i) if any(p in ev[j][2] for p in PRE)]
        first.append(pre[0] if pre else i)
    calls = [(first[n], fast[n], (first[n + 1] if n + 1 < len(fast) else len(ev))) for n in range(len(fast))]
    calls = calls[-ncalls - 1:-1]          # the last call has no next one to measure the gap to
    rows, chain, tail, gap, launches = {}, [], [], [], []
    for b, i, e in calls:
        fs, fe = ev[i][0], ev[i][1]
        seen = {}
        for j in range(b, e):
            s, t, name, q = ev[j]
            k = (j > i, short(name), q)
            seen[k] = seen.get(k, 0) + 1
            ref = fe if j > i else fs
            rows.setdefault(k + (seen[k],), []).append(((s - ref) / 1e3, (t - ref) / 1e3))
        chain.append((fs - ev[b][0]) / 1e3)
        tail.append((max(ev[j][1] for j in range(i, e)) - fe) / 1e3)
        if e < len(ev):
            gap.append((ev[e][0] - max(ev[j][1] for j in range(i, e))) / 1e3)
        launches.append(e - b)

    def mm(v):
        return f"{statistics.median(v):8.1f} ({min(v):.1f}-{max(v):.1f})" if v else "       -"

    print(f"{len(calls)} calls; us relative to the FAST kernel's start (before it) / end (after it); median (min-max)")
    print(f"{'kernel':46s} {'queue':>5s} {'start':>26s} {'end':>26s} {'length':>8s}")
    for k in sorted(rows, key=lambda k: statistics.median(x[0] for x in rows[k]) + (1e9 if k[0] else 0)):
        v = rows[k]
        print(f"{k[1]:46s} {k[2]:>5s} {mm([x[0] for x in v]):>26s} {mm([x[1] for x in v]):>26s} "
              f"{statistics.median(x[1] - x[0] for x in v):8.1f}")
    print(f"chain before the FAST kernel (first start to FAST start): {mm(chain)}")
    print(f"tail (FAST end to the last kernel's end):                 {mm(tail)}")
    print(f"gap (last kernel's end to the next call's first start):   {mm(gap)}")
    print(f"launches per call (kernels and fills):                    {mm(launches)}")


if __name__ == "__main__":
    main()
