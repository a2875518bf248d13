#!/usr/bin/env python3
"""Hollanti key generation on one GPU: k_hollanti_keys against its store floor and the host loop.

2^n records (default 2^24), t = 1, p = 5; nq = 1 and 2, K = 1 and 8 keys.  Per (nq, K) the legs

  dev     pir_gen_hollanti_keys_dev into a device buffer (aligned pitches), HIP events on the
          stream around the call
  memset  hipMemsetAsync of the same p K nq N bytes: what storing that much costs
  host    pir_gen_hollanti_keys: the same kernel, its own stream and device buffer, the vectors
          copied back to pageable host memory (host clock around the synchronous call)

after warm-ups, the legs alternated in every repeat; median, min and max.  Then, once,

  shim    the shim's host generateHollantiQuery (one thread: OS random bytes + Horner) at the
          same parameters, timed at 2^20 records first; the whole 2^n is run if that predicts
          under a minute, else the 2^20 figure is scaled and labelled so

One JSON line per (nq, K) and one for the shim leg.

    python tools/bench_hollanti_keygen.py [--log-records 24] [--iters 10] [--warmup 3]
                                          [--host-iters 3] [--no-shim] [--shim-only]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T_, P_ = 1, 5


def stats(v):
    return {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
            "ms_max": round(max(v), 4), "n": len(v)}


def shim_leg(n, nq):
    """the shim's host generateHollantiQuery with NUM_PARTIES = 5 and NUM_ROUNDS = nq:
    T = 1, RHO = 1 and (K, R) = (1, 3) or (2, 2) (params.cpp:423-429, NUM_ROUNDS = K / RHO)"""
    from erasurecodedpir_amd import server as S
    k, r = {1: (1, 3), 2: (2, 2)}[nq]

    def run(L):
        S.setSystemParams(L, 64, T_, k, r, 0, 1, 0, 3)
        prm = S.params()
        assert (prm["NUM_PARTIES"], prm["NUM_ROUNDS"], prm["NUM_ENCODED_FILES"]) == (P_, nq, 1 << L)
        lib = S._lib.load()
        keys = np.ones((P_, nq, 1 << L), np.uint8)     # touched before the clock starts
        rows = [S._row_ptrs(keys[q]) for q in range(P_)]
        outer = (ctypes.POINTER(S.c_u8_p) * P_)(
            *[ctypes.cast(x, ctypes.POINTER(S.c_u8_p)) for x in rows])
        cl = S.CClient()
        t0 = time.perf_counter()
        lib.generateHollantiQuery(ctypes.byref(cl), 12345, outer)
        return (time.perf_counter() - t0) * 1e3

    S.hollanti_keygen_on_gpu(0)
    small = min(n, 20)
    run(small)
    ms_small = run(small)
    out = {"bench": "hollanti_keygen_shim_host", "t": T_, "p": P_, "nq": nq, "threads": 1,
           "log_records_measured": small, "ms_measured": round(ms_small, 2)}
    if ms_small * (1 << (n - small)) < 60e3:
        out.update(log_records_measured=n, ms_measured=round(run(n), 2), scaled_by=1)
        out["ms"] = out["ms_measured"]
    else:
        out.update(scaled_by=1 << (n - small), ms=round(ms_small * (1 << (n - small)), 1),
                   label="scaled from 2^%d records" % small)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-records", type=int, default=24)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--no-shim", action="store_true")
    ap.add_argument("--shim-only", action="store_true")
    a = ap.parse_args()
    n = a.log_records
    N = 1 << n
    shim = {} if a.no_shim else {nq: shim_leg(n, nq) for nq in (1, 2)}
    for o in shim.values():
        print(json.dumps(o), flush=True)
    if a.shim_only:
        return
    import erasurecodedpir_amd as pir
    from erasurecodedpir_amd import _lib
    from bench_shamir import Events, hip_runtime
    hip = hip_runtime()
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    ev = Events(hip)
    lib = _lib.load()
    rng = np.random.default_rng(24)
    with pir.Engine(2, 1, 6, 16, 1) as e:
        for nq in (1, 2):
            for K in (1, 8):
                nbytes = P_ * K * nq * N
                idx = rng.integers(0, N, K, dtype=np.uint64)
                seeds = rng.integers(0, 256, 16 * K, dtype=np.uint8).tobytes()
                d = e.alloc_dev(nbytes)
                host = np.ones(nbytes, np.uint8)
                sd = np.frombuffer(seeds, np.uint8).copy()

                def dev():
                    pir.gen_hollanti_keys_dev(N, idx, T_, P_, d, N, nq * N, K * nq * N, nq=nq,
                                              seeds=seeds, stream=e.stream)

                def memset():
                    rc = hip.hipMemsetAsync(d, 0, nbytes, e.stream)
                    assert rc == 0, rc

                def host_form():
                    t0 = time.perf_counter()
                    rc = lib.pir_gen_hollanti_keys(0, N, idx.ctypes.data_as(ctypes.c_void_p), K, T_,
                                                   P_, nq, 1, sd.ctypes.data_as(ctypes.c_void_p),
                                                   host.ctypes.data_as(ctypes.c_void_p))
                    assert rc == 0, rc
                    return (time.perf_counter() - t0) * 1e3

                for _ in range(a.warmup):
                    dev()
                    memset()
                e.sync()
                host_form()
                dev()
                e.sync()
                same = bool(np.array_equal(e.d2h(d, nbytes), host))   # both forms, one stream
                ms = {"dev": [], "memset": [], "host": []}
                for it in range(a.iters):
                    ms["dev"].append(ev.time(e.stream, dev))
                    ms["memset"].append(ev.time(e.stream, memset))
                    if it < a.host_iters:
                        ms["host"].append(host_form())
                out = {"bench": "hollanti_keygen", "log_records": n, "t": T_, "p": P_, "nq": nq,
                       "keys": K, "bytes": nbytes, "aes_blocks": K * nq * T_ * (N // 16),
                       "host_form_equals_device_form": same,
                       "legs": {k: stats(v) for k, v in ms.items()}}
                t_dev = out["legs"]["dev"]["ms"]
                out["dev_ms_per_key"] = round(t_dev / K, 4)
                out["dev_gbps_stored"] = round(nbytes / t_dev / 1e6, 1)
                out["dev_over_memset"] = round(t_dev / out["legs"]["memset"]["ms"], 2)
                if nq in shim:
                    out["shim_host_over_dev_per_key"] = round(shim[nq]["ms"] / (t_dev / K), 1)
                print(json.dumps(out), flush=True)
                e.free_dev(d)


if __name__ == "__main__":
    main()
