#!/usr/bin/env python3
"""Summarise the rocprofv3 passes of tools/gpu_pmc.sh for a queue answered by several kernels
(a shared queue: k_frontier / k_expand / k_subtree / k_scan_* / k_reduce) into
profiles/pmc_<cfg>.json, in the manner of tools/pmc_kernels.py: every counter is summed over all
of the queue's kernels.

    python tools/pmc_queue.py DIR CFG QUERIES_PER_QUEUE RECORDS RECORD_BYTES [QUEUES_PER_RUN]

DIR is the directory tools/gpu_pmc.sh wrote its passes into.  Reads
DIR/pmc_<cfg>_*/run_counter_collection.csv (one --pmc pass each, never combined with tracing),
DIR/prof_<cfg>/run_kernel_stats.csv and DIR/pmc_<cfg>_lib_sha256.txt.
tools/gpu_pmc.sh runs W = K, so a run holds QUEUES_PER_RUN = 2 equal queues; "per launch" below
means per queue, as bench.py reads it.

HBM read bytes: gfx950's FETCH_SIZE counts half the bytes of 16-B-per-lane streaming reads and
is uncalibrated for other widths (MI355X_MICROARCH.md, HBM).  The scan kernels read the shard, a
known byte count, once per launch: their factor (1 or 2) is the one that brings FETCH_SIZE x
1024 x factor / launches nearest to the shard's bytes, and it is reported per kernel; the other
kernels' reads (tree nodes, shares) are taken at factor 2, an upper bound."""
import csv
import glob
import json
import os
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIP = ("k_keygen", "k_fill", "k_encode", "__amd_rocclr")


def short(name):
    return name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").strip()


def main():
    src, cfg = os.path.abspath(sys.argv[1]), sys.argv[2]
    K, records, efs = int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    nqueues = int(sys.argv[6]) if len(sys.argv) > 6 else 2
    shard = records * efs
    per = defaultdict(lambda: defaultdict(float))   # kernel -> counter -> sum over the run
    launches = defaultdict(lambda: defaultdict(int))
    for f in sorted(glob.glob(os.path.join(src, f"pmc_{cfg}_*", "run_counter_collection.csv"))):
        for r in csv.DictReader(open(f)):
            k = short(r["Kernel_Name"])
            if "pir::" not in k or any(s in k for s in SKIP):
                continue
            per[k][r["Counter_Name"]] += float(r["Counter_Value"])
            launches[k][r["Counter_Name"]] += 1
    total = defaultdict(float)
    kernels = {}
    rd = wr = 0.0
    for k, cs in sorted(per.items()):
        n = max(launches[k].values()) / nqueues
        d = {"launches_per_queue": n, "counters_per_queue": {c: v / nqueues for c, v in cs.items()}}
        for c, v in cs.items():
            total[c] += v / nqueues
        if "FETCH_SIZE" in cs:
            raw = cs["FETCH_SIZE"] * 1024 / nqueues
            factor = 2
            if "k_scan" in k or "k_query" in k:
                factor = min((1, 2), key=lambda f: abs(raw * f / n - shard))
                d["shard_reads_per_queue"] = round(raw * factor / shard, 3)
            d["fetch_factor"] = factor
            d["hbm_read_bytes_per_queue"] = raw * factor
            rd += raw * factor
        if "WRITE_SIZE" in cs:
            d["hbm_write_bytes_per_queue"] = cs["WRITE_SIZE"] * 1024 / nqueues
            wr += d["hbm_write_bytes_per_queue"]
        kernels[k] = d
    out = {"config": cfg, "kernel": "the queue's kernels: " + ", ".join(sorted(kernels)),
           "queries_per_launch": K, "queues_per_run": nqueues,
           "counters_per_launch": dict(total), "kernels": kernels,
           "correction": "read bytes = FETCH_SIZE x 1024 x fetch_factor per kernel (gfx950: 2 for "
                         "16-B-per-lane streams; the scan kernels' factor calibrated on the "
                         "shard's bytes per launch; others 2, an upper bound)",
           "algorithmic_bytes_per_launch": shard * K,
           "hbm_read_bytes_per_launch": int(rd), "hbm_write_bytes_per_launch": int(wr),
           "hbm_bytes_per_launch": int(rd + wr), "hbm_bytes_per_query": int((rd + wr) / K),
           "traffic_over_algorithmic": round((rd + wr) / (shard * K), 4)}
    shaf = os.path.join(src, f"pmc_{cfg}_lib_sha256.txt")
    if os.path.exists(shaf):
        out["lib_sha256"] = open(shaf).read().split()[0]
    stats = os.path.join(src, f"prof_{cfg}", "run_kernel_stats.csv")
    if os.path.exists(stats):
        ks = {}
        for r in csv.DictReader(open(stats)):
            k = short(r["Name"])
            if k in kernels:
                ks[k] = {"calls_per_queue": int(r["Calls"]) / nqueues,
                         "ms_per_queue": round(float(r["TotalDurationNs"]) / nqueues / 1e6, 4)}
        out["kernel_trace_ms"] = ks
    dst = os.path.join(ROOT, "profiles", f"pmc_{cfg}.json")
    json.dump(out, open(dst, "w"), indent=1)
    print(json.dumps({k: out[k] for k in ("hbm_bytes_per_query", "traffic_over_algorithmic",
                                          "lib_sha256") if k in out}))
    for k, d in kernels.items():
        print(k, d.get("shard_reads_per_queue"), d.get("fetch_factor"), d.get("hbm_read_bytes_per_queue"))


if __name__ == "__main__":
    main()
