#!/usr/bin/env python3
"""Shamir sqrt(N) answers against one shard-sized read, on one GPU.

For NUM_ROUNDS in --rounds (default 1,2): a Shamir engine of 2^n value rows + 2^n Hermite rows
(default 2^24 x 1 KiB: 32 GiB), HIP events around pir_engine_answer_shamir_dev after warm-up,
alternated in the same process with a one-round pir_engine_answer_coefs_dev over the same N
value rows -- the cost of one shard-sized read of the explicit-coefficient scan.  Prints ONE
JSON line: per leg ms (median), ms_coefs_one_read, their ratio and the bytes of the value and
Hermite rows (2 N EFS) over the answer time.  The floor of the ratio is about 2 (both halves
read once); the answer's three passes (rows, strips, Hermite scan) are 3 reads of N EFS.

    python tools/bench_shamir.py [--log-records 24] [--record-bytes 1024] [--rounds 1,2]
                                 [--iters 10] [--warmup 3]

--queue measures queues of one-round Shamir queries instead (pir_engine_answer_shamir_queue_dev;
the knobs are read at engine creation, so every leg has its own engine over the same shard
bytes), for each queue length of --queue-lengths (default 2,4,8,20):

  shared       $PIR_SH_SHARE=2: 8 virtual keys per read of the value rows and of the Hermite rows
  shared_rx4   the same with the Rx pass / the Ry pass / both on k_shamir_rows / k_shamir_strips,
  shared_ry4   up to 4 virtual keys per launch ($PIR_SH_PASS = 2 / 1 / 0, read per answer): a
  shared_rxy4  transposed value pass against the four-round kernel in its place
  unshared     $PIR_SH_SHARE=0: the single answers back to back
  parent       --parent-lib PATH, the parent commit's library built into a second directory: K
               back-to-back pir_engine_answer_shamir_dev calls on one stream
  rounds4      a 4-round engine over the same bytes answering 4 keys per single call (the queued
               keys taken as rounds: what k_shamir_rows / k_shamir_strips<4> give)

and prints ONE JSON line: per queue length and leg the median, min and max ms and ms per key,
the largest max - min spread of any leg, shared against parent, the gain of each transposed
pass, and `shared_equals_unshared`, a byte comparison of every leg's answers at full size.

    python tools/bench_shamir.py --queue [--parent-lib DIR/libpir_engine.so] [--queue-lengths 2,4,8,20]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import erasurecodedpir_amd as pir  # noqa: E402


def hip_runtime():
    """The HIP runtime the engine library already loaded (for hipEvent*)."""
    pir.load()
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64.so" in line:
                return ctypes.CDLL(line.split()[-1])
    raise OSError("libamdhip64.so is not loaded")


class Events:
    def __init__(self, hip):
        self.hip = hip
        self.e = [ctypes.c_void_p(), ctypes.c_void_p()]
        for e in self.e:
            self._ck(hip.hipEventCreate(ctypes.byref(e)), "hipEventCreate")

    def _ck(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d)" % (what, rc))

    def time(self, stream, fn):
        """ms between two events around fn() on `stream`."""
        st = ctypes.c_void_p(stream)
        self._ck(self.hip.hipEventRecord(self.e[0], st), "hipEventRecord")
        fn()
        self._ck(self.hip.hipEventRecord(self.e[1], st), "hipEventRecord")
        self._ck(self.hip.hipEventSynchronize(self.e[1]), "hipEventSynchronize")
        ms = ctypes.c_float()
        self._ck(self.hip.hipEventElapsedTime(ctypes.byref(ms), self.e[0], self.e[1]),
                 "hipEventElapsedTime")
        return float(ms.value)


def queue_bench(a):
    from bench_woodruff import other_library_engine
    n, efs = a.log_records, a.record_bytes
    N = 1 << n
    x = (n + 1) // 2
    klen = (1 << x) + (1 << (n - x))
    rl = pir.shamir_response_len(n, efs)
    lengths = [int(v) for v in a.queue_lengths.split(",")]
    kmax = (max(lengths) + 3) // 4 * 4
    ev = Events(hip_runtime())
    keys = np.random.default_rng(6).integers(0, 256, (kmax, klen), dtype=np.uint8)
    engines, bufs = {}, {}
    for leg, env in (("shared", {"PIR_SH_SHARE": "2"}), ("unshared", {"PIR_SH_SHARE": "0"})):
        os.environ.update(env)
        engines[leg] = pir.Engine(2, 1, n + 1, efs, 1)
        for k in env:
            del os.environ[k]
    if a.parent_lib:
        engines["parent"] = other_library_engine(a.parent_lib, 2, 1, n + 1, efs, 1)
    engines["rounds4"] = pir.Engine(2, 1, n + 1, efs, 4)
    for leg, e in engines.items():
        e.fill_shard_random(16)
        bufs[leg] = (e.alloc_dev(kmax * klen), e.alloc_dev(kmax * rl))
        e.h2d(bufs[leg][0], keys.reshape(-1))
        if leg in ("shared", "unshared"):
            e.reserve_shamir_queue(kmax)
    # the shared engine also serves the legs with one value pass on the 4-round kernels
    # ($PIR_SH_PASS is read per answer)
    passes = {"shared": None, "shared_rx4": "2", "shared_ry4": "1", "shared_rxy4": "0"}
    legs = [l for l in ("shared", "shared_rx4", "shared_ry4", "shared_rxy4", "unshared", "parent",
                        "rounds4") if l in engines or l in passes]
    eng = {l: engines["shared" if l in passes else l] for l in legs}

    def run(leg, K):
        e = eng[leg]
        d_k, d_r = bufs["shared" if leg in passes else leg]
        if leg == "parent":
            for k in range(K):
                e.answer_shamir_dev(d_k + k * klen, klen, 0, N, d_r + k * rl)
        elif leg == "rounds4":   # the queued keys taken as rounds, 4 per single answer
            for k in range(0, K, 4):
                e.answer_shamir_dev(d_k + k * klen, klen, 0, N, d_r + k * rl)
        else:
            if passes.get(leg):
                os.environ["PIR_SH_PASS"] = passes[leg]
            try:
                e.answer_shamir_queue_dev(d_k, klen, klen, K, 0, N, d_r)
            finally:
                os.environ.pop("PIR_SH_PASS", None)

    out = {"bench": "shamir_queue", "log_records": n, "record_bytes": efs, "key_len": klen,
           "iters": a.iters, "warmup": a.warmup, "value_bytes": N * efs,
           "parent_lib": bool(a.parent_lib), "queues": {}}
    same, spread = True, 0.0
    for K in lengths:
        got = {}
        for leg in legs:
            run(leg, K)
            eng[leg].sync()
            got[leg] = eng[leg].d2h(bufs["shared" if leg in passes else leg][1], K * rl).copy()
        same = same and all(np.array_equal(got["shared"], g) for g in got.values())
        for _ in range(a.warmup):
            for leg in legs:
                run(leg, K)
        for e in engines.values():
            e.sync()
        ms = {leg: [] for leg in legs}
        for _ in range(a.iters):
            for leg in legs:
                ms[leg].append(ev.time(eng[leg].stream, lambda: run(leg, K)))
        q = {}
        for leg, v in ms.items():
            med = statistics.median(v)
            q[leg] = {"ms": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                      "spread": round(max(v) - min(v), 4), "ms_per_key": round(med / K, 4)}
            spread = max(spread, max(v) - min(v))
        out["queues"][str(K)] = q
    out["shared_equals_unshared"] = bool(same)
    out["largest_spread_ms"] = round(spread, 4)
    for K in lengths:
        q = out["queues"][str(K)]
        if a.parent_lib:
            q["parent_minus_shared_ms"] = round(q["parent"]["ms"] - q["shared"]["ms"], 4)
            q["shared_beats_parent"] = bool(q["parent"]["ms"] - q["shared"]["ms"] > spread)
        # a transposed value pass against the 4-round kernel in its place: the other passes of
        # the two legs are the same launches
        q["rx_transposed_gain_ms"] = round(q["shared_rx4"]["ms"] - q["shared"]["ms"], 4)
        q["ry_transposed_gain_ms"] = round(q["shared_ry4"]["ms"] - q["shared"]["ms"], 4)
    for e in engines.values():
        e.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-records", type=int, default=24)
    ap.add_argument("--record-bytes", type=int, default=1024)
    ap.add_argument("--rounds", default="1,2")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--queue", action="store_true")
    ap.add_argument("--queue-lengths", default="2,4,8,20")
    ap.add_argument("--parent-lib", default="")
    a = ap.parse_args()
    if a.queue:
        return queue_bench(a)
    n, efs = a.log_records, a.record_bytes
    N = 1 << n
    x = (n + 1) // 2
    klen = (1 << x) + (1 << (n - x))
    ev = Events(hip_runtime())
    rng = np.random.default_rng(2)
    legs = []
    # the one-round explicit-coefficient scan over N value rows: its own one-round engine
    with pir.Engine(2, 1, n, efs, 1) as ec:
        ec.fill_shard_random(11)
        d_coefs, d_cres = ec.alloc_dev(N), ec.alloc_dev(efs)
        ec.h2d(d_coefs, rng.integers(0, 256, N, dtype=np.uint8))
        for rounds in [int(r) for r in a.rounds.split(",")]:
            with pir.Engine(2, 1, n + 1, efs, rounds) as e:
                e.fill_shard_random(12)
                rl = e.shamir_response_len
                d_keys, d_res = e.alloc_dev(rounds * klen), e.alloc_dev(rounds * rl)
                e.h2d(d_keys, rng.integers(0, 256, rounds * klen, dtype=np.uint8))

                def shamir():
                    e.answer_shamir_dev(d_keys, klen, 0, N, d_res)

                def coefs():
                    ec.answer_coefs_dev(d_coefs, N, 0, N, d_cres)

                for _ in range(a.warmup):
                    shamir()
                    coefs()
                e.sync()
                ec.sync()
                ms_s, ms_c = [], []
                for _ in range(a.iters):  # alternated: both see the same machine state
                    ms_s.append(ev.time(e.stream, shamir))
                    ms_c.append(ev.time(ec.stream, coefs))
                ms, mc = statistics.median(ms_s), statistics.median(ms_c)
                legs.append({"rounds": rounds, "ms": round(ms, 4),
                             "ms_min": round(min(ms_s), 4), "ms_max": round(max(ms_s), 4),
                             "ms_coefs_one_read": round(mc, 4), "ratio": round(ms / mc, 3),
                             "shard_bytes": 2 * N * efs,
                             "gbps_of_2NEFS": round(2 * N * efs / ms / 1e6, 1),
                             "gbps_coefs_read": round(N * efs / mc / 1e6, 1)})
    print(json.dumps({"bench": "shamir", "log_records": n, "record_bytes": efs,
                      "iters": a.iters, "warmup": a.warmup, "legs": legs}))


if __name__ == "__main__":
    main()
