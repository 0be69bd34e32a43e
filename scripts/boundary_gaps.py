#!/usr/bin/env python3
"""Time between kernels on the two decode queues, from one rocprofv3 per-dispatch kernel trace.

    rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- python3 bench.py --steps 5 --warmup 2
    python3 scripts/boundary_gaps.py DIR/.../run_kernel_trace.csv

(kernel trace only, the program after ``--``; never together with ``--pmc``.)

The overlapped decode step runs as two 512-row halves on two streams, each a serial chain of
kernels.  For each of the two queues that carry it this prints, per predecessor kernel family, the
number of kernel boundaries, the median and mean gap between that kernel's end and the next kernel's
start on the same queue, and the family's own median / mean run time (a shorter gap paid for by an
equally longer kernel is no gain: the table shows both).  It also prints the share of the decode
wall time that a queue spends in no kernel.

A boundary counts when both its kernels belong to the decode step and the gap is below ``--max-gap``
microseconds (default 50): longer gaps are graph-replay, join or host gaps, counted separately.

Caveat: the tracer itself perturbs the timeline (profiles/r2_timeline_b1024_profiled.txt measured the
traced step a third longer than the untraced one, with the two queues overlapping less), so the gaps
are compared between two traced runs, never with an untraced step time."""
import argparse
import csv
import re
import statistics
from collections import defaultdict

# decode-step kernel families, by what the predecessor leaves behind
_GEMM = re.compile(r"gemm_tn_kernel<(\d+), (\d+), \d+, \d+, \d+, (\d+)")
_EPI = {"6": "gemm slabs (EPI_PARTIAL)", "4": "gemm QKV", "1": "gemm ff (GELU)", "0": "gemm bf16"}


def family(name: str):
    """Family of a decode-step kernel, or None for a kernel that is not part of the decode step."""
    m = _GEMM.search(name)
    if m:
        if int(m.group(1)) > 64:  # 128-row tiles: prefill
            return None
        return _EPI.get(m.group(3))
    if "add_layernorm_kernel" in name:
        return "add+LN"
    if "attn_persist_kernel" in name or "attn_wave_kernel" in name:
        return "attention"
    if "gemm_ps_kernel" in name:
        return "LM head (gemm_ps)"
    if "decode_update_kernel" in name:
        return "decode_update"
    return None


def load(path):
    per_q = defaultdict(list)
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            per_q[r["Queue_Id"]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    for rows in per_q.values():
        rows.sort()
    return per_q


def queue_report(rows, max_gap_ns):
    """rows: (start, end, name) of one queue, sorted.  Returns (families, totals)."""
    fams = defaultdict(lambda: {"gaps": [], "dur": []})
    kern_ns = gap_ns = 0
    long_gaps = 0
    for (s0, e0, n0), (s1, _e1, n1) in zip(rows, rows[1:]):
        f0, f1 = family(n0), family(n1)
        if f0 is None:
            continue
        fams[f0]["dur"].append(e0 - s0)
        if f1 is None:
            continue
        gap = s1 - e0
        if gap >= max_gap_ns:
            long_gaps += 1
            continue
        fams[f0]["gaps"].append(gap)
        kern_ns += e0 - s0
        gap_ns += max(gap, 0)
    return fams, {"kernel_ns": kern_ns, "gap_ns": gap_ns, "long_gaps": long_gaps}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("trace", help="rocprofv3 *_kernel_trace.csv")
    ap.add_argument("--max-gap", type=float, default=50.0, help="us; longer gaps are replay / host gaps")
    args = ap.parse_args()
    per_q = load(args.trace)
    n_attn = {q: sum(1 for r in rows if family(r[2]) == "attention") for q, rows in per_q.items()}
    queues = [q for q in sorted(per_q, key=lambda q: -n_attn[q]) if n_attn[q] > 0][:2]
    if not queues:
        print("no decode attention kernels in the trace")
        return 1
    print(f"trace: {args.trace.rsplit('/', 1)[-1]}; decode queues: {', '.join(queues)}; "
          f"boundaries with a gap >= {args.max_gap:g} us are listed as long gaps, not as boundaries")
    us = 1e-3
    all_gaps = []
    for q in queues:
        fams, tot = queue_report(per_q[q], int(args.max_gap * 1000))
        wall = tot["kernel_ns"] + tot["gap_ns"]
        print(f"\nqueue {q}: {sum(len(v['gaps']) for v in fams.values())} boundaries, "
              f"{tot['long_gaps']} long gaps; decode wall time {wall * 1e-6:.1f} ms, "
              f"in no kernel {100.0 * tot['gap_ns'] / max(1, wall):.1f} %")
        print(f"  {'predecessor family':<26} {'bounds':>7} {'gap med':>8} {'gap mean':>9} {'kern med':>9} "
              f"{'kern mean':>10}   (us)")
        for fam in sorted(fams, key=lambda k: -sum(fams[k]["gaps"])):
            g, d = fams[fam]["gaps"], fams[fam]["dur"]
            if not g:
                continue
            all_gaps += g
            print(f"  {fam:<26} {len(g):>7} {statistics.median(g) * us:>8.2f} {statistics.fmean(g) * us:>9.2f} "
                  f"{statistics.median(d) * us:>9.2f} {statistics.fmean(d) * us:>10.2f}")
    if all_gaps:
        print(f"\nboth queues: {len(all_gaps)} boundaries, median gap {statistics.median(all_gaps) * us:.2f} us, "
              f"mean {statistics.fmean(all_gaps) * us:.2f} us")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
