"""From a rocprofv3 --kernel-trace CSV of a bench.py run: how long the resolve kernel and the subpath launches take, and for
what share of the resolve kernel's wall time a k_trace_subpath launch is in flight (both have started and neither has ended).

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 bench.py --steps 64 --warmup 4
    python tools/resolve_coresidency.py DIR [label]
"""
import csv
import glob
import sys


def main(argv):
    path = glob.glob(f"{argv[1]}/**/*_kernel_trace.csv", recursive=True)[0]
    label = argv[2] if len(argv) > 2 else argv[1]
    res, sub = [], []
    for row in csv.DictReader(open(path)):
        name, a, b = row["Kernel_Name"], int(row["Start_Timestamp"]), int(row["End_Timestamp"])
        if "k_connect_resolve" in name:
            res.append((a, b))
        elif "k_trace_subpath" in name:
            sub.append((a, b))
    sub.sort()
    wall = over = 0
    for a, b in res:
        wall += b - a
        covered, at = 0, a                      # union of the subpath intervals inside [a, b]
        for c, d in sub:
            if d <= at or c >= b:
                continue
            c = max(c, at)
            covered += min(d, b) - c
            at = min(d, b)
        over += covered
    n_r, n_s = max(len(res), 1), max(len(sub), 1)
    print(f"{label}: resolve launches {len(res)}, avg {wall / n_r / 1e6:.4f} ms; subpath launches {len(sub)}, avg "
          f"{sum(d - c for c, d in sub) / n_s / 1e6:.4f} ms; subpath launch in flight for {100.0 * over / max(wall, 1):.1f} % of the "
          f"resolve kernel's wall time")
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv))
