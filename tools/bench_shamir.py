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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-records", type=int, default=24)
    ap.add_argument("--record-bytes", type=int, default=1024)
    ap.add_argument("--rounds", default="1,2")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
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
