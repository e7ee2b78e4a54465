#!/usr/bin/env python3
"""Concurrency of the LP kernels from a rocprofv3 `--kernel-trace --stats` run's rocpd database (DESIGN.md §6
"Slot groups"): do kernels of the two slot groups of a block (NEP_BLOCK_GROUPS=2) overlap on the device, and what
share of a block's span is the device idle.

  python3 tools/trace_overlap.py PROF_DIR [--functions F] [--min-slots 8] > overlap.json

From the start / end timestamps of every x_pass / node_pass / scalar_pass dispatch:
  * blocks: a block starts at a certificate x pass (x_pass<.., true, ..>) that begins more than --gap-ms after the
    previous one (the two groups' certificate passes start together) and lasts to the end of the last LP kernel that
    begins before the next block's first one; only blocks whose certificate passes carry at least --min-slots slots
    are reported (the ones the split rule divides at the bench's shape);
  * idle share: 1 - (union of the kernels' intervals) / (block span), summed over those blocks;
  * overlap share: time with two or more LP kernels running / block span;
  * node passes under an x pass: node_pass dispatches whose interval intersects an x_pass interval;
  * the hardware queues (and streams, where the database has them) the blocks' kernels ran on.
x_pass durations rise under overlap by construction: the benchmark's value is the yardstick, not these."""
import argparse
import glob
import json
import math
import os
import re
import sqlite3
import sys


def union_and_multi(iv):
    """(time covered by >= 1 interval, time covered by >= 2) of [(start, end)]."""
    ev = sorted([(s, 1) for s, _ in iv] + [(e, -1) for _, e in iv])
    one = two = 0
    depth, last = 0, None
    for t, d in ev:
        if last is not None and depth >= 1:
            one += t - last
            if depth >= 2:
                two += t - last
        depth += d
        last = t
    return one, two


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir", help="the directory rocprofv3 wrote (-d)")
    ap.add_argument("--functions", type=int, default=256)
    ap.add_argument("--min-slots", type=int, default=8)
    ap.add_argument("--gap-ms", type=float, default=3.0)
    a = ap.parse_args()
    dbs = sorted(glob.glob(os.path.join(a.dir, "**", "*.db"), recursive=True))
    if not dbs:
        sys.exit(f"no rocpd database under {a.dir}")
    rows = []
    for db in dbs:
        c = sqlite3.connect(db)
        cols = [d[0] for d in c.execute("select * from kernels limit 1").description]
        extra = [k for k in ("queue_id", "stream_id") if k in cols]
        q = "select name, start, end, grid_x, workgroup_x" + "".join(", " + k for k in extra) + " from kernels"
        for r in c.execute(q):
            name = r[0]
            if not re.search(r"nep::(fac_)?(x_pass|node_pass|scalar_pass)<", name):
                continue
            rows.append({"name": name, "s": r[1], "e": r[2], "wgs": r[3] // max(1, r[4]),
                         **{k: r[5 + i] for i, k in enumerate(extra)}})
    rows.sort(key=lambda r: r["s"])
    is_x = lambda r: "x_pass<" in r["name"]
    is_chk = lambda r: re.search(r"x_pass<\d+, true", r["name"]) is not None
    # block starts
    starts, last = [], -math.inf
    for i, r in enumerate(rows):
        if is_chk(r):
            if r["s"] - last > a.gap_ms * 1e6:
                starts.append(i)
            last = r["s"]
    out = {"databases": len(dbs), "lp_kernels": len(rows), "blocks_seen": len(starts)}
    span = busy = multi = 0
    nblocks = node_n = node_under = 0
    queues, streams = {}, {}
    for b, i0 in enumerate(starts):
        i1 = starts[b + 1] if b + 1 < len(starts) else len(rows)
        blk = rows[i0:i1]
        t_next = rows[i1]["s"] if i1 < len(rows) else math.inf
        slots = sum(r["wgs"] for r in blk if is_chk(r) and r["s"] - blk[0]["s"] <= a.gap_ms * 1e6) / a.functions
        if slots < a.min_slots or len(blk) < 8:
            continue
        # (a kernel of this block may end after the next block's first kernel begins only across a host gap: clip)
        iv = [(r["s"], min(r["e"], t_next)) for r in blk]
        one, two = union_and_multi(iv)
        span += max(e for _, e in iv) - blk[0]["s"]
        busy += one
        multi += two
        nblocks += 1
        xs = [(r["s"], r["e"]) for r in blk if is_x(r)]
        k = 0
        for r in blk:
            for key, d in (("queue_id", queues), ("stream_id", streams)):
                if key in r:
                    d[r[key]] = d.get(r[key], 0) + 1
            if "node_pass<" in r["name"]:
                node_n += 1
                while k < len(xs) and xs[k][1] <= r["s"]:
                    k += 1
                node_under += any(s < r["e"] and e > r["s"] for s, e in xs[max(0, k - 2):k + 3])
    out.update({"min_slots": a.min_slots, "blocks": nblocks, "span_ms": span / 1e6, "busy_ms": busy / 1e6,
                "idle_share": 1.0 - busy / span if span else None,
                "overlap_share": multi / span if span else None,
                "node_passes": node_n, "node_passes_under_an_x_pass": node_under,
                "kernels_by_queue": {str(k): v for k, v in sorted(queues.items(), key=lambda kv: str(kv[0]))},
                "kernels_by_stream": {str(k): v for k, v in sorted(streams.items(), key=lambda kv: str(kv[0]))}})
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
