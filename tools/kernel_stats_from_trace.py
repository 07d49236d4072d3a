"""Per-kernel statistics of a `rocprofv3 --kernel-trace` run from its result database (`*_results.db`, the rocpd format), as a
CSV in the column layout of rocprofv3's own `kernel_stats.csv`: Name, Calls, TotalDurationNs, AverageNs, Percentage, MinNs, MaxNs,
StdDev (population), sorted by total duration.  Names are taken as the trace recorded them.

    rocprofv3 --kernel-trace --stats -d <dir> -o native -- python tools/decode_step_bench.py --engines hip_native --warmup 1 --reps 2
    python tools/kernel_stats_from_trace.py <dir>/native_results.db profiles/r08/hip_prefill_kernel_stats.csv
"""
import csv
import math
import sqlite3
import sys


def main(db_path, out_path):
    con = sqlite3.connect(db_path)
    durations = {}
    for name, start, end in con.execute("select name, start, end from kernels"):     # the database's view over all kernel dispatches
        durations.setdefault(name, []).append(end - start)
    total = sum(sum(v) for v in durations.values())
    rows = []
    for name, v in durations.items():
        t, mean = sum(v), sum(v) / len(v)
        sd = math.sqrt(sum((x - mean) ** 2 for x in v) / len(v))
        rows.append((name, len(v), t, round(mean, 6), round(100.0 * t / total, 2), min(v), max(v), round(sd, 6)))
    rows.sort(key=lambda r: -r[2])
    with open(out_path, "w", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs", "StdDev"])
        w.writerows(rows)
    print(f"{len(rows)} kernels, {sum(r[1] for r in rows)} dispatches, {total / 1e6:.3f} ms -> {out_path}")


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2])
