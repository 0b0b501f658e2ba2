"""Kernel rates of tools/deltas_rate.py from its rocprofv3 kernel trace.

    python tools/deltas_rate_summary.py KERNEL_TRACE_CSV DELTAS_RATE_JSON_LINE_FILE

The dispatches of deltas_kernel and normalize_apply_kernel are grouped by grid size; the groups, in the order of their
first dispatch, are config 2 and config 5 (the order tools/deltas_rate.py runs them in).  Rate = algorithmic bytes
over the median kernel time: 4W + 4W(1 + K) per row for deltas_kernel (K = 2), 8W per row for the apply pass."""
import csv
import json
import statistics
import sys

KERNELS = {"deltas_kernel": lambda w: 4 * w + 4 * w * 3, "normalize_apply_kernel": lambda w: 8 * w}


def main(trace, line_file):
    line = json.loads(open(line_file).read().strip().splitlines()[-1])
    groups = {k: {} for k in KERNELS}
    with open(trace) as f:
        rows = list(csv.DictReader(f))
    grid_cols = [c for c in rows[0] if c.startswith("Grid_Size")]
    for i, r in enumerate(rows):
        name = r["Kernel_Name"]
        for k in KERNELS:
            if k + "(" in name or k + "<" in name or name.endswith(k):
                grid = tuple(r[c] for c in grid_cols)
                g = groups[k].setdefault(grid, {"first": i, "ns": []})
                g["ns"].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = {}
    for k, per_grid in groups.items():
        ordered = sorted(per_grid.items(), key=lambda kv: kv[1]["first"])
        if len(ordered) != 2:
            raise SystemExit("%s: %d grid sizes in the trace, expected 2 (config 2, config 5)" % (k, len(ordered)))
        for cfg, (grid, g) in zip(("config2", "config5"), ordered):
            R, W = line[cfg]["rows"], line[cfg]["width"]
            med = statistics.median(g["ns"])
            out.setdefault(cfg, {})[k] = dict(dispatches=len(g["ns"]), grid=list(grid), median_us=round(med / 1e3, 2),
                                              min_us=round(min(g["ns"]) / 1e3, 2),
                                              TBps=round(R * KERNELS[k](W) / (med * 1e-9) / 1e12, 3))
    for cfg in out:
        out[cfg]["deltas_over_apply_rate"] = round(out[cfg]["deltas_kernel"]["TBps"] /
                                                   out[cfg]["normalize_apply_kernel"]["TBps"], 3)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
