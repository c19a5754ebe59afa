"""Where a steady-state group launch's time goes, from one rocprofv3 kernel trace of bench.py.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python3 bench.py --steps 4000 --warmup 64
    python3 profiles/group_launch_trace.py DIR/**/t_kernel_trace.csv [label]

A group launch is a chain on one hardware queue: pileup (plain or with the Fisher epilogue), call_group_kernel (unfolded
form only), phase_group_run_kernel, phase_assign_group_kernel, done_group_kernel.  For the steady state (the last launches
of the trace, the closing ones left out) this prints, per kernel, the in-loop duration against the duration of the same
kernel in the set-up launches (one group alone on the device), the time between the end of its predecessor on the queue
and its own start, and the share of wall time during which 4 / 3 / 2 / 1 / 0 pileup kernels are resident.
"""
import csv
import statistics
import sys

KINDS = (("pileup", ("pileup_fold_group_kernel", "pileup_planes_group_kernel", "pileup_index_fold_group_kernel", "pileup_index_group_kernel")), ("call", ("call_group_kernel",)),
         ("phase", ("phase_group_run_kernel",)), ("assign", ("phase_assign_group_kernel",)), ("done", ("done_group_kernel",)))


def kind_of(name):
    for kind, subs in KINDS:
        if any(s in name for s in subs):
            return kind
    return None


def main():
    path = sys.argv[1]
    label = sys.argv[2] if len(sys.argv) > 2 else path
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            k = kind_of(r["Kernel_Name"])
            if k is None:
                continue
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "0"), k, r["Kernel_Name"].split("(")[0],
                         int(r.get("Grid_Size_Z", r.get("Grid_Size_z", "0")) or 0)))
    rows.sort()
    # a group launch = a pileup and what follows it on the same queue up to the done kernel
    launches, open_by_queue = [], {}
    for s, e, q, k, name, gz in rows:
        if k == "pileup":
            open_by_queue[q] = {"pileup": (s, e), "name": name, "z": gz, "order": ["pileup"]}
        elif q in open_by_queue:
            cur = open_by_queue[q]
            cur[k] = (s, e)
            cur["order"].append(k)
            if k == "done":
                launches.append(open_by_queue.pop(q))
    full = [l for l in launches if l["z"] == max(x["z"] for x in launches)]
    n_set_up = 4                       # bench.py runs every launch unit alone once before the warm-up
    alone = full[1:n_set_up]           # (the very first pays for the code upload)
    steady = full[len(full) // 2:-8]   # second half of the trace, the closing launches left out
    if len(steady) < 32:
        raise SystemExit(f"{path}: only {len(full)} full group launches in the trace")
    t0, t1 = steady[0]["pileup"][0], steady[-1]["done"][1]
    print(f"== {label}: {len(steady)} steady-state launches of {len(full)}, {1e-3 * (t1 - t0) / len(steady):.1f} us of wall time per launch, "
          f"pileup kernel {steady[0]['name']}")
    print(f"{'kernel':8s} {'in loop us (median, mean)':>26s} {'alone us (median)':>18s} {'queue gap us (median, mean)':>28s}")
    for kind, _ in KINDS:
        d = [1e-3 * (l[kind][1] - l[kind][0]) for l in steady if kind in l]
        if not d:
            continue
        a = [1e-3 * (l[kind][1] - l[kind][0]) for l in alone if kind in l]
        gaps = []
        for l in steady:
            if kind in l and kind != "pileup":
                prev = l["order"][l["order"].index(kind) - 1]
                gaps.append(1e-3 * (l[kind][0] - l[prev][1]))
        gap_txt = f"{statistics.median(gaps):9.2f} {statistics.mean(gaps):9.2f}" if gaps else f"{'-':>19s}"
        print(f"{kind:8s} {statistics.median(d):12.2f} {statistics.mean(d):13.2f} {statistics.median(a) if a else float('nan'):18.2f} {gap_txt:>28s}")
    span = [1e-3 * (l["done"][1] - l["pileup"][0]) for l in steady]
    tail = [1e-3 * (l["done"][1] - l["pileup"][1]) for l in steady]
    print(f"launch, first start to completion word: median {statistics.median(span):.1f} us; of it behind the pileup: {statistics.median(tail):.1f} us")
    # how many pileup kernels are resident, as a share of wall time
    ev = []
    for l in steady:
        ev.append((l["pileup"][0], 1))
        ev.append((l["pileup"][1], -1))
    ev.sort()
    share, depth, last = {}, 0, ev[0][0]
    for t, dlt in ev:
        share[depth] = share.get(depth, 0) + (t - last)
        depth += dlt
        last = t
    total = sum(share.values())
    print("pileup kernels resident, share of wall time: " + ", ".join(f"{k}: {100.0 * v / total:.1f} %" for k, v in sorted(share.items(), reverse=True)))
    # the device with no pileup AND no other kernel of a group launch running
    ev = []
    for l in steady:
        for kind, _ in KINDS:
            if kind in l:
                ev.append((l[kind][0], 1))
                ev.append((l[kind][1], -1))
    ev.sort()
    idle, depth, last = 0, 0, ev[0][0]
    for t, dlt in ev:
        if depth == 0:
            idle += t - last
        depth += dlt
        last = t
    print(f"no kernel of any group launch running: {100.0 * idle / total:.2f} % of wall time")


if __name__ == "__main__":
    main()
