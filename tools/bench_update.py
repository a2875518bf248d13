#!/usr/bin/env python3
"""Live record updates on one GPU: pir_engine_update_across_dev on a resident shard (default 2^24
records of 1 KiB, taken as an across-encoded database of k 2^n files) that holds a valid fold
image, for batches of random files, against the only route a build without the update calls has:
pir_engine_set_shard of as many rows (re-encoded by the caller; one call per row, since the rows
are scattered), then pir_engine_fold_image(BUILD).

  update     wall clock around update_across_dev + sync (the host's grouping of the batch, the
             table upload and k_update_rows), and the time between two HIP events recorded on
             the stream around the call; the image must still be whole afterwards
  baseline   --parent-lib LIB: that build's library (else this one); wall clock of the set_shard
             calls, and of the image rebuild alone (drop, then build: synchronous)

`--warmup` untimed rounds, then the median, min and max of `--iters` timed ones.  Prints ONE JSON
line; `rebuild_over_update` is the baseline's rebuild alone over the update's wall clock.

    python tools/bench_update.py [--log-records 24] [--record-bytes 1024] [--k 2]
        [--batches 1,64,4096] [--iters 20] [--warmup 3] [--parent-lib LIB]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import erasurecodedpir_amd as pir  # noqa: E402
from bench_shamir import Events, hip_runtime  # noqa: E402
from bench_woodruff import other_library_engine  # noqa: E402


def stats(v):
    return {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
            "ms_max": round(max(v), 4)}


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def bench_update(a, batches, out):
    n, efs, k = a.log_records, a.record_bytes, a.k
    num_files = k << n
    os.environ["PIR_FOLD_IMAGE"] = "1"
    ev = Events(hip_runtime())
    with pir.Engine(2, 1, n, efs, 1) as e:
        e.fill_shard_random(15)
        full = e.fold_image("build")
        assert full, "no room for the fold image"
        out["image_bytes"] = full
        d_delta = e.alloc_dev(max(batches) * efs)
        e.fill_random_dev(d_delta, max(batches) * efs, 3)
        e.sync()
        rng = np.random.default_rng(11)
        for B in batches:
            draws = iter([rng.integers(0, num_files, B).astype(np.uint64)
                          for _ in range(a.warmup + 2 * a.iters)])

            def go():
                e.update_across_dev(next(draws), d_delta, efs, num_files, k)

            def go_sync():
                go()
                e.sync()
            for _ in range(a.warmup):
                go_sync()
            wall = [wall_ms(go_sync) for _ in range(a.iters)]
            dev = [ev.time(e.stream, go) for _ in range(a.iters)]
            assert e.fold_image() == full, "the update lost the image"
            out["batches"][str(B)] = {"update_wall": stats(wall), "update_events": stats(dev)}


def bench_baseline(a, batches, out):
    n, efs = a.log_records, a.record_bytes
    os.environ["PIR_FOLD_IMAGE"] = "1"
    e = other_library_engine(a.parent_lib, 2, 1, n, efs, 1) if a.parent_lib \
        else pir.Engine(2, 1, n, efs, 1)
    with e:
        e.fill_shard_random(15)
        assert e.fold_image("build"), "no room for the fold image"
        rng = np.random.default_rng(12)
        rows = rng.integers(0, 256, (max(batches), efs), dtype=np.uint8)

        def rebuild():
            e.fold_image("drop")
            e.fold_image("build")
        for B in batches:
            def set_rows():
                for i, r in enumerate(rng.integers(0, 1 << n, B)):
                    e.set_shard(rows[i], int(r))
            for _ in range(a.warmup):
                set_rows()
                rebuild()
            sets, builds = [], []
            for _ in range(a.iters):
                sets.append(wall_ms(set_rows))
                builds.append(wall_ms(rebuild))
            q = out["batches"][str(B)]
            q["baseline_set_shard"] = stats(sets)
            q["baseline_rebuild"] = stats(builds)
            q["rebuild_over_update"] = round(q["baseline_rebuild"]["ms"] / q["update_wall"]["ms"], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-records", type=int, default=24)
    ap.add_argument("--record-bytes", type=int, default=1024)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    out = {"bench": "update", "log_records": a.log_records, "record_bytes": a.record_bytes,
           "k": a.k, "iters": a.iters, "warmup": a.warmup, "parent_lib": bool(a.parent_lib),
           "batches": {}}
    bench_update(a, batches, out)
    bench_baseline(a, batches, out)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
