#!/usr/bin/env python3
"""Queues of explicit-coefficient (Hollanti), multiparty and covering-design queries on one GPU:
pir_engine_answer_{coefs,mp,cd}_queue_dev, HIP events around the device forms, `--warmup`
untimed rounds then `--iters` timed ones, the legs alternated in one process:

  shared     $PIR_GQ_SHARE=2: 8 / nrp keys per read of the shard (share kernel, W-round scan)
  unshared   $PIR_GQ_SHARE=0: the single answers back to back
  parent     --parent-lib: the parent commit's library, which has no queue call: K
             back-to-back single _dev answers on one stream

and prints ONE JSON line per mode: per queue length and leg the median, min and max ms and ms
per key, the largest max - min spread of any leg, shared against parent, and
`shared_equals_unshared`, a byte comparison of the two legs' answers at full size.

    python tools/bench_group_queue.py [--modes hollanti1,hollanti2,mp3,cd842]
        [--log-records 24] [--record-bytes 1024] [--queue-lengths 2,4,8,20] [--parent-lib LIB]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import erasurecodedpir_amd as pir  # noqa: E402
from bench_shamir import Events, hip_runtime  # noqa: E402
from bench_woodruff import other_library_engine  # noqa: E402


def sqrt_key(eval_bytes, tog_lo, tog_hi, seed):
    """a synthetic sqrt(N) key: random bytes, toggle bytes in {0, 1, raw} (a third clear)"""
    key = np.random.default_rng(seed).integers(0, 256, max(eval_bytes, 16), dtype=np.uint8)
    tb = key[tog_lo:tog_hi]
    key[tog_lo:tog_hi] = np.where(tb % 3 == 0, 0, np.where(tb % 3 == 1, 1, tb))
    return key


def cd_sizes(n, q, nck):
    p2, mu = 1 << (q - 1), 1 << (n // 2 + 3)
    nu = (1 << n) // mu
    tog = nu * 16 * p2
    cw = tog + nck * nu * p2
    return nck, tog, cw, cw + p2 * mu


def mp3_sizes(n):
    """p = 3, t = 1: 2 shares, 4 seeds per row, mu = 2^ceil(n/2 + 1)"""
    eb = pir._lib.load().pir_engine_mp_eval_bytes(3, n, 1)
    mu = 1 << -(-(n + 2) // 2)
    nu = (1 << n) // mu
    tog = nu * 16 * 4
    cw = tog + 2 * nu * 4
    assert cw + 4 * mu == eb, (cw + 4 * mu, eb)
    return 2, tog, cw, eb


def mode_setup(mode, n, kmax):
    """rounds, the keys as one (kmax, key_bytes) array, and run(engine, d_keys, K, d_res, queue)"""
    N = 1 << n
    if mode.startswith("hollanti"):
        nr = int(mode[len("hollanti"):])
        keys = np.random.default_rng(7).integers(0, 256, (kmax, nr * N), dtype=np.uint8)

        def run(e, d_k, K, d_r, queue, out):
            if queue:
                e.answer_coefs_queue_dev(d_k, N, nr * N, K, 0, N, d_r)
            else:
                for k in range(K):
                    e.answer_coefs_dev(d_k + k * nr * N, N, 0, N, d_r + k * out)
        return nr, keys, run
    if mode == "mp3":
        nr, tog, cw, eb = mp3_sizes(n)

        def call_q(e, d_k, stride, K, d_r):
            e.answer_mp_queue_dev(d_k, stride, K, 3, 1, d_r)

        def call_1(e, d_k, d_r):
            e.answer_mp_dev(d_k, 3, 1, d_r)
    elif mode == "cd842":
        nr, tog, cw, eb = cd_sizes(n, 6, 3)

        def call_q(e, d_k, stride, K, d_r):
            e.answer_cd_queue_dev(d_k, stride, K, 6, 3, d_r)

        def call_1(e, d_k, d_r):
            e.answer_cd_dev(d_k, 6, 3, d_r)
    else:
        raise SystemExit("unknown mode " + mode)
    stride = (eb + 15) & ~15
    keys = np.zeros((kmax, stride), np.uint8)
    for k in range(kmax):
        keys[k, :eb] = sqrt_key(eb, tog, cw, 100 + k)[:eb]

    def run(e, d_k, K, d_r, queue, out):
        if queue:
            call_q(e, d_k, stride, K, d_r)
        else:
            for k in range(K):
                call_1(e, d_k + k * stride, d_r + k * out)
    return nr, keys, run


def bench_mode(a, mode, ev):
    n, efs = a.log_records, a.record_bytes
    lengths = [int(x) for x in a.queue_lengths.split(",")]
    kmax = max(lengths)
    nr, keys, run = mode_setup(mode, n, kmax)
    out_bytes = nr * efs
    engines, bufs = {}, {}
    for leg, env in (("shared", {"PIR_GQ_SHARE": "2"}), ("unshared", {"PIR_GQ_SHARE": "0"})):
        os.environ.update(env)
        engines[leg] = pir.Engine(2, 1, n, efs, nr)
        for k in env:
            del os.environ[k]
    if a.parent_lib:
        engines["parent"] = other_library_engine(a.parent_lib, 2, 1, n, efs, nr)
    for leg, e in engines.items():
        e.fill_shard_random(15)
        bufs[leg] = (e.alloc_dev(keys.size), e.alloc_dev(kmax * out_bytes))
        e.h2d(bufs[leg][0], keys.reshape(-1))
        if leg != "parent":
            e.reserve_group_queue(kmax)

    def go(leg, K):
        run(engines[leg], bufs[leg][0], K, bufs[leg][1], leg != "parent", out_bytes)

    out = {"bench": "group_queue", "mode": mode, "log_records": n, "record_bytes": efs,
           "rounds": nr, "iters": a.iters, "warmup": a.warmup, "shard_bytes": (1 << n) * efs,
           "parent_lib": bool(a.parent_lib), "queues": {}}
    same, spread = True, 0.0
    for K in lengths:
        got = {}
        for leg in engines:
            go(leg, K)
            engines[leg].sync()
            got[leg] = engines[leg].d2h(bufs[leg][1], K * out_bytes).copy()
        same = same and all(np.array_equal(got["shared"], g) for g in got.values())
        for _ in range(a.warmup):
            for leg in engines:
                go(leg, K)
        for e in engines.values():
            e.sync()
        ms = {leg: [] for leg in engines}
        for _ in range(a.iters):
            for leg, e in engines.items():
                ms[leg].append(ev.time(e.stream, lambda: go(leg, K)))
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
    for e in engines.values():
        e.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="hollanti1,hollanti2,mp3,cd842")
    ap.add_argument("--log-records", type=int, default=24)
    ap.add_argument("--record-bytes", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--queue-lengths", default="2,4,8,20")
    ap.add_argument("--parent-lib", default="")
    a = ap.parse_args()
    ev = Events(hip_runtime())
    for mode in a.modes.split(","):
        bench_mode(a, mode, ev)


if __name__ == "__main__":
    main()
