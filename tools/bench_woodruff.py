#!/usr/bin/env python3
"""Woodruff answers against one shard-sized read, on one GPU.

One engine of 2^n records (default 2^24 x 1 KiB: 16 GiB), HIP events around the device forms
after warm-up, four legs alternated in the same process so that all see the same machine state:

  fused    pir_engine_answer_woodruff_dev with $PIR_WD_FUSED=2: k_query's Woodruff mode (the
           pair products built into the LDS ring beside the scan) + k_reduce
  two      the same with $PIR_WD_FUSED=0: k_woodruff_coefs, k_scan_uni, k_reduce
  coefs    pir_engine_answer_coefs_dev, one round over the same rows: the interleave kernel,
           k_scan_uni, k_reduce -- one shard-sized read of the explicit-coefficient scan
  deriv    pir_engine_answer_woodruff_deriv_dev: the rows pass, the totals kernel, the columns
           pass (two shard-sized reads)

Prints ONE JSON line: per leg the median, min and max ms, each leg's spread (max - min), the
fused leg against the other two, and the derivative answer as a multiple of the coefs leg.  The
fused path is worth being the default only if it is no slower than `two` and `coefs` by more than
the spread the run shows between repeats of one leg.

    python tools/bench_woodruff.py [--log-records 24] [--record-bytes 1024] [--iters 10]
                                   [--warmup 3] [--no-deriv]

--queue measures queues of Woodruff value queries instead (pir_engine_answer_woodruff_queue_dev;
the knobs are read at engine creation, so every leg has its own engine over the same shard
bytes), for each queue length of --queue-lengths (default 2,4,8,20):

  shared     $PIR_WD_SHARE=2: G keys per read of the shard (coefficient kernel, G-round scan)
  unshared   $PIR_WD_SHARE=0: the single answers back to back
  parent     --parent-lib PATH, the parent commit's library built into a second directory: K
             back-to-back pir_engine_answer_woodruff_dev calls on one stream

and prints ONE JSON line: per queue length and leg the median, min and max ms and ms per key,
the largest max - min spread of any leg, shared against parent, and `shared_equals_unshared`,
a byte comparison of the two legs' answers at full size.

    python tools/bench_woodruff.py --queue [--parent-lib DIR/libpir_engine.so] [--queue-lengths 2,4,8,20]

--deriv-queue measures queues of Woodruff derivative queries the same way
(pir_engine_answer_woodruff_deriv_queue_dev, M + 1 records per key): shared is $PIR_WDD_SHARE=2
(8 keys per read of the shard in each of the two passes), unshared $PIR_WDD_SHARE=0, and parent K
back-to-back pir_engine_answer_woodruff_deriv_dev calls of the parent commit's library.
--pair-legs adds shared_pair0 .. 3: the shared engine with $PIR_WDD_PAIR forced (which pass hands
a wave a long segment and then a short one; bit 0 the rows pass, bit 1 the columns pass).

    python tools/bench_woodruff.py --deriv-queue [--parent-lib DIR/libpir_engine.so] [--pair-legs]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import erasurecodedpir_amd as pir  # noqa: E402
from bench_shamir import Events, hip_runtime  # noqa: E402


def other_library_engine(path, *args):
    """An Engine that runs on another build of the library (one without the queue calls too)."""
    from erasurecodedpir_amd import _lib
    other = ctypes.CDLL(path)
    for name, (res, argtypes) in _lib.PROTOTYPES.items():
        fn = getattr(other, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, argtypes
    mine = _lib.load()
    _lib._lib = other
    try:
        return pir.Engine(*args)
    finally:
        _lib._lib = mine


def queue_bench(a):
    n, efs = a.log_records, a.record_bytes
    N, M = 1 << n, pir.woodruff_m(n)
    lengths = [int(x) for x in a.queue_lengths.split(",")]
    kmax = max(lengths)
    ev = Events(hip_runtime())
    keys = np.random.default_rng(5).integers(0, 256, (kmax, M), dtype=np.uint8)
    engines, bufs = {}, {}
    deriv = a.deriv_queue
    knob = "PIR_WDD_SHARE" if deriv else "PIR_WD_SHARE"
    rb = (M + 1) * efs if deriv else efs      # result bytes per key
    for leg, env in (("shared", {knob: "2"}), ("unshared", {knob: "0"})):
        os.environ.update(env)
        engines[leg] = pir.Engine(2, 1, n, efs, 1)
        for k in env:
            del os.environ[k]
    if a.parent_lib:
        engines["parent"] = other_library_engine(a.parent_lib, 2, 1, n, efs, 1)
    for leg, e in engines.items():
        e.fill_shard_random(15)
        bufs[leg] = (e.alloc_dev(kmax * M), e.alloc_dev(kmax * rb))
        e.h2d(bufs[leg][0], keys.reshape(-1))
        if leg != "parent":
            (e.reserve_woodruff_deriv_queue if deriv else e.reserve_woodruff_queue)(kmax)

    # --pair-legs: the shared engine again with the segment hand-out forced ($PIR_WDD_PAIR is read
    # per answer): shared_pair0 longest first in both passes, 1 / 2 / 3 a long segment and then a
    # short one per wave in the rows pass / the columns pass / both
    legs = {leg: leg for leg in engines}
    if deriv and a.pair_legs:
        legs.update({"shared_pair%d" % p: "shared" for p in range(4)})

    def run(leg, K):
        e, (d_k, d_r) = engines[legs[leg]], bufs[legs[leg]]
        if leg.startswith("shared_pair"):
            os.environ["PIR_WDD_PAIR"] = leg[-1]
            e.answer_woodruff_deriv_queue_dev(d_k, M, K, 0, N, d_r)
            del os.environ["PIR_WDD_PAIR"]
        elif leg == "parent":
            one = e.answer_woodruff_deriv_dev if deriv else e.answer_woodruff_dev
            for k in range(K):
                one(d_k + k * M, M, 0, N, d_r + k * rb)
        elif deriv:
            e.answer_woodruff_deriv_queue_dev(d_k, M, K, 0, N, d_r)
        else:
            e.answer_woodruff_queue_dev(d_k, M, K, 0, N, d_r)

    out = {"bench": "woodruff_deriv_queue" if deriv else "woodruff_queue", "log_records": n,
           "record_bytes": efs, "key_len": M,
           "iters": a.iters, "warmup": a.warmup, "shard_bytes": N * efs,
           "parent_lib": bool(a.parent_lib), "queues": {}}
    same, spread = True, 0.0
    for K in lengths:
        got = {}
        for leg in legs:
            run(leg, K)
            engines[legs[leg]].sync()
            got[leg] = engines[legs[leg]].d2h(bufs[legs[leg]][1], K * rb).copy()
        same = same and all(np.array_equal(got["shared"], g) for g in got.values())
        for _ in range(a.warmup):
            for leg in legs:
                run(leg, K)
        for e in engines.values():
            e.sync()
        ms = {leg: [] for leg in legs}
        for _ in range(a.iters):
            for leg in legs:
                ms[leg].append(ev.time(engines[legs[leg]].stream, lambda: run(leg, K)))
        q = {}
        for leg, v in ms.items():
            med = statistics.median(v)
            q[leg] = {"ms": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                      "spread": round(max(v) - min(v), 4), "ms_per_key": round(med / K, 4)}
            spread = max(spread, max(v) - min(v))
        out["queues"][str(K)] = q
    out["shared_equals_unshared"] = bool(same)
    out["largest_spread_ms"] = round(spread, 4)
    if a.parent_lib:
        for K in lengths:
            q = out["queues"][str(K)]
            q["parent_minus_shared_ms"] = round(q["parent"]["ms"] - q["shared"]["ms"], 4)
            q["shared_beats_parent"] = bool(q["parent"]["ms"] - q["shared"]["ms"] > spread)
            q["parent_over_shared"] = round(q["parent"]["ms"] / q["shared"]["ms"], 3)
    for e in engines.values():
        e.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-records", type=int, default=24)
    ap.add_argument("--record-bytes", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-deriv", action="store_true")
    ap.add_argument("--queue", action="store_true")
    ap.add_argument("--deriv-queue", action="store_true")
    ap.add_argument("--pair-legs", action="store_true")
    ap.add_argument("--queue-lengths", default="2,4,8,20")
    ap.add_argument("--parent-lib", default="")
    a = ap.parse_args()
    if a.queue or a.deriv_queue:
        return queue_bench(a)
    n, efs = a.log_records, a.record_bytes
    N, M = 1 << n, pir.woodruff_m(n)
    ev = Events(hip_runtime())
    rng = np.random.default_rng(5)
    with pir.Engine(2, 1, n, efs, 1) as e:
        e.fill_shard_random(15)
        tile = e.woodruff_fused_tile
        d_key, d_res = e.alloc_dev(M), e.alloc_dev((M + 1) * efs)
        d_coefs = e.alloc_dev(N)
        e.h2d(d_key, rng.integers(0, 256, M, dtype=np.uint8))
        e.h2d(d_coefs, rng.integers(0, 256, N, dtype=np.uint8))

        def forced(mode):
            def run():
                os.environ["PIR_WD_FUSED"] = mode   # read per answer
                e.answer_woodruff_dev(d_key, M, 0, N, d_res)
            return run

        legs = {"two": forced("0"),
                "coefs": lambda: e.answer_coefs_dev(d_coefs, N, 0, N, d_res)}
        if tile:
            legs["fused"] = forced("2")
        if not a.no_deriv:
            legs["deriv"] = lambda: e.answer_woodruff_deriv_dev(d_key, M, 0, N, d_res)
        # the two value paths give the same bytes
        same = None
        if tile:
            legs["fused"]()
            r_f = e.d2h(d_res, efs).copy()
            legs["two"]()
            same = bool(np.array_equal(r_f, e.d2h(d_res, efs)))
        for _ in range(a.warmup):
            for fn in legs.values():
                fn()
        e.sync()
        ms = {k: [] for k in legs}
        for _ in range(a.iters):
            for k, fn in legs.items():
                ms[k].append(ev.time(e.stream, fn))
        os.environ.pop("PIR_WD_FUSED", None)
    out = {"bench": "woodruff", "log_records": n, "record_bytes": efs, "key_len": M,
           "fused_tile": tile, "fused_equals_two_kernel": same, "iters": a.iters,
           "warmup": a.warmup, "shard_bytes": N * efs, "legs": {}}
    for k, v in ms.items():
        med = statistics.median(v)
        out["legs"][k] = {"ms": round(med, 4), "ms_min": round(min(v), 4),
                          "ms_max": round(max(v), 4), "spread": round(max(v) - min(v), 4),
                          "gbps_of_NEFS": round(N * efs / med / 1e6, 1)}
    L = out["legs"]
    if "fused" in L:
        spread = max(x["spread"] for x in L.values() if x is not L.get("deriv"))
        out["fused_minus_two_ms"] = round(L["fused"]["ms"] - L["two"]["ms"], 4)
        out["fused_minus_coefs_ms"] = round(L["fused"]["ms"] - L["coefs"]["ms"], 4)
        out["value_legs_spread_ms"] = spread
        out["fused_no_slower"] = bool(L["fused"]["ms"] <= min(L["two"]["ms"], L["coefs"]["ms"])
                                      + spread)
    if "deriv" in L:
        out["deriv_over_coefs"] = round(L["deriv"]["ms"] / L["coefs"]["ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
