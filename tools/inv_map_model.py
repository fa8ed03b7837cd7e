"""List-scheduling model of one inverse-level launch (k_inv_level) under a block -> job map: what a change
of the map is worth before a GPU is used.  Standard library only; runs in seconds.

    python tools/inv_map_model.py [--nt 16] [--counts 70 83 100] [--sub 1]

Assumptions (a model, not a measurement):
  * 8 XCDs of 32 CUs; block b runs on XCD b % 8, and an XCD starts its blocks in block order, each on
    the CU with the fewest resident workgroups, as soon as a slot is free (two slots per CU);
  * two resident workgroups share a CU's MFMA pipe at half rate each, a lone one runs at `lone` of the
    CU's rate (0.6 and 0.8 are both shown);
  * a job costs its K range in tiles plus 0.3 tile of fixed cost (over sub for sub-tiles).
It does not know how the dispatcher really refills slots, what the L2 loses when the order changes, or
how much of a lone workgroup's rate `lone` gets right.

Printed per level and phase: the makespan as a multiple of total work / 256 CUs, for xcd_map's equal-
count cut in the matrices' item order and for the work-balanced cut, longest K first (inv_map_job,
csrc/mk_types.hpp: rebuilt here by sorting, not by its closed form)."""
import argparse

FIXED = 0.3


def matrix_items(nt, sz, phase, sub, clipped):
    """(K, live) per item slot of one matrix in xcd_map's order: pair, then t = slow * sz + fast."""
    items = []
    for p in range((nt + 2 * sz - 1) // (2 * sz)):
        B0 = 2 * p * sz + sz
        for t in range(sz * sz):
            i = B0 + (t % sz if phase == 0 else t // sz)
            j = B0 - sz + (t // sz if phase == 0 else t % sz)
            K = B0 - j if phase == 0 else i - B0 + 1
            if i < nt or clipped:
                items += [(K, i < nt)] * sub
    return items


def xcd_map(count, nt, sz, phase, sub):
    """Per XCD, the K of its jobs in block order: eight contiguous chunks of equal item count."""
    seq = matrix_items(nt, sz, phase, sub, True) * count
    C = (len(seq) + 7) // 8
    return [[K for K, live in seq[x * C:(x + 1) * C] if live] for x in range(8)]


def work_map(count, nt, sz, phase, sub):
    """Per XCD, the K of its jobs in block order: the matrices' live items, class-major from the longest
    K down, cut where the work midpoint passes an eighth of the total; longest K first within an XCD."""
    mat = sorted((K for K, _ in matrix_items(nt, sz, phase, sub, False)), reverse=True)
    seq = mat * count
    total, c, out = sum(seq), 0, [[] for _ in range(8)]
    for K in seq:
        out[min(7, (8 * c + 4 * K) // total)].append(K)
        c += K
    return [sorted(v, reverse=True) for v in out]      # stable: entry, then tile, within a class


def xcd_makespan(jobs, sub, lone, cus=32):
    """Processor-sharing list schedule of one XCD's jobs, in order, on cus CUs of two slots."""
    left = [[] for _ in range(cus)]     # remaining cost of the resident jobs
    nxt, now = 0, 0.0
    while True:
        while nxt < len(jobs):
            cu = min(range(cus), key=lambda u: len(left[u]))
            if len(left[cu]) == 2:
                break
            left[cu].append((jobs[nxt] + FIXED) / sub)
            nxt += 1
        busy = [u for u in range(cus) if left[u]]
        if not busy:
            return now
        rate = {u: (lone if len(left[u]) == 1 else 0.5) for u in busy}
        dt = min(min(left[u]) / rate[u] for u in busy)
        now += dt
        for u in busy:
            left[u] = [r - dt * rate[u] for r in left[u] if r - dt * rate[u] > 1e-12]


def ratio(per_xcd, sub, lone):
    work = sum((K + FIXED) / sub for v in per_xcd for K in v)
    return max(xcd_makespan(v, sub, lone) for v in per_xcd) / (work / 256.0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--nt", type=int, default=16)
    ap.add_argument("--counts", type=int, nargs="+", default=[70, 83, 100])
    ap.add_argument("--sub", type=int, default=1, choices=(1, 4, 16))
    a = ap.parse_args()
    print(f"nt = {a.nt}, sub = {a.sub}: makespan / (work / 256 CUs), lone = 0.6 | 0.8")
    for count in a.counts:
        sz = 1
        while sz < a.nt:
            for phase in (0, 1):
                cells = []
                for build in (xcd_map, work_map):
                    per = build(count, a.nt, sz, phase, a.sub)
                    cells.append(" | ".join(f"{ratio(per, a.sub, lone):.3f}" for lone in (0.6, 0.8)))
                print(f"  count {count:4d}  level {128 * sz:5d}  phase {phase}   equal-count cut {cells[0]}   "
                      f"work-balanced, longest first {cells[1]}")
            sz *= 2


if __name__ == "__main__":
    main()
