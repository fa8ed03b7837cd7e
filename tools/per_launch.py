"""Per-launch statistics by kernel and grid from a rocprofv3 kernel-trace database, the layout of
profiles/*/per_launch_*.txt.

    python tools/per_launch.py run_results.db [kernel-name-part ...] > profiles/<name>/per_launch_<arm>.txt

Launches are grouped by (kernel, grid in threads); the inverse levels' launches of one grid alternate
phase 0, phase 1 in start order and are kept apart.  Default kernels: the column update, the diagonal
factor and the inverse levels."""
import sqlite3
import statistics
import sys
from collections import defaultdict

from db_stats import _demangle

DEFAULT = ("k_chol_diag", "k_chol_update_trsm", "k_inv_level", "k_inv_copydiag")


def main(db, parts):
    c = sqlite3.connect(db)
    cols = [r[1] for r in c.execute("pragma table_info(rocpd_kernel_dispatch)")]
    gx = "grid_size_x" if "grid_size_x" in cols else "0"
    rows = c.execute(f"select s.kernel_name, k.start, k.end - k.start, k.{gx} from rocpd_kernel_dispatch k "
                     "join rocpd_info_kernel_symbol s on k.kernel_id = s.id order by k.start").fetchall()
    dm = _demangle(sorted({r[0] for r in rows}))
    groups, seen = defaultdict(list), defaultdict(int)
    for name, _, dur, grid in rows:
        short = dm[name].split("(")[0].replace("void ", "")
        if not any(p in short for p in parts):
            continue
        key = (short, grid)
        if "k_inv_level" in short:
            key += (seen[(short, grid)] % 2,)
            seen[(short, grid)] += 1
        groups[key].append(dur / 1e3)
    # the alternation holds when every level has a grid of its own and no launch is missing from the
    # trace (the sequential schedule): the two phases of a grid then have equal calls
    for key in groups:
        if len(key) > 2 and len(groups[key]) != len(groups.get(key[:2] + (1 - key[2],), [])):
            sys.exit(f"{key[0]} grid={key[1]}: phases with unequal calls, the phase labels cannot be trusted")
    totals = defaultdict(list)
    for key in sorted(groups):
        v = groups[key]
        totals[key[0]] += v
        phase = f" phase={key[2]}" if len(key) > 2 else ""
        print(f"{key[0]} grid={key[1]}{phase} calls={len(v)} mean_us={statistics.mean(v):.1f} "
              f"median_us={statistics.median(v):.1f} min_us={min(v):.1f}")
    for name in sorted(totals):
        v = totals[name]
        print(f"TOTAL {name} calls={len(v)} mean_us={statistics.mean(v):.1f} sum_ms={sum(v) / 1e3:.1f}")


if __name__ == "__main__":
    main(sys.argv[1], tuple(sys.argv[2:]) or DEFAULT)
