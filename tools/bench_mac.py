#!/usr/bin/env python3
"""CheckMAC record tags on one GPU: k_hmac_sha256_files over a device-resident database.

2^n files (default 2^24) of payload + 32 bytes (default 992 + 32: 16 GiB), random payloads from
the engine's generator, tagged in place by pir_mac_files_dev.  HIP events around the call after
warm-up; median and max - min over the repeats.  Two comparisons in the same process:

  floor   one one-round pir_engine_answer_coefs_dev pass over an engine shard of the same
          2^n x (payload + 32) bytes: what one read of the database costs
  host    the library's own host mac() (what initialize_client would pay per file without the
          kernel) over the first 2^m of the same files (default 2^20) on 16 host threads --
          8 worker processes of 2 threads each, so the interpreter lock is not what is timed;
          the workers' rates are summed and the time is SCALED by 2^(n-m) to the whole database

Prints ONE JSON line.

    python tools/bench_mac.py [--log-files 24] [--payload 992] [--iters 10] [--warmup 3]
                              [--host-log-files 20] [--no-host] [--no-floor]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEY = b"1234567812345678"  # client.cpp:19
WORKERS, THREADS = 8, 2


def host_worker(path, pitch, payload, start, count):
    """mac() over files [start, start + count) of the file at `path`, on THREADS threads."""
    from erasurecodedpir_amd import _lib
    lib = _lib.load()
    files = np.fromfile(path, np.uint8, count * pitch, offset=start * pitch)
    base = files.ctypes.data
    key = (ctypes.c_uint8 * 16)(*KEY)

    def run(a, b):
        out = (ctypes.c_uint8 * 32)()
        for i in range(a, b):
            lib.mac(key, base + i * pitch, payload, out, 32)

    run(0, min(count, 256))  # warm
    th = [threading.Thread(target=run, args=(count * t // THREADS, count * (t + 1) // THREADS))
          for t in range(THREADS)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    print(json.dumps({"files": count, "s": time.perf_counter() - t0}))


def host_leg(e, d_files, pitch, payload, m):
    n = 1 << m
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "files.bin")
        e.d2h(d_files, n * pitch).tofile(path)
        per = n // WORKERS
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--host-worker", path,
                                   str(pitch), str(payload), str(w * per), str(per)],
                                  stdout=subprocess.PIPE) for w in range(WORKERS)]
        res = [json.loads(p.communicate()[0]) for p in procs]
        if any(p.returncode for p in procs):
            raise RuntimeError("a host worker failed")
    rate = sum(r["files"] / r["s"] for r in res)
    return n, rate


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--host-worker":
        return host_worker(sys.argv[2], *[int(x) for x in sys.argv[3:7]])
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-files", type=int, default=24)
    ap.add_argument("--payload", type=int, default=992)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-log-files", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-floor", action="store_true")
    a = ap.parse_args()
    import erasurecodedpir_amd as pir
    from bench_shamir import Events, hip_runtime
    n, payload = a.log_files, a.payload
    N, pitch = 1 << n, a.payload + 32
    ev = Events(hip_runtime())
    blocks = (payload + 9 + 63) // 64 + 1  # per file: the inner message's blocks + the outer hash
    out = {"bench": "mac", "log_files": n, "payload_bytes": payload, "file_pitch": pitch,
           "database_bytes": N * pitch, "sha256_blocks_per_file": blocks, "iters": a.iters,
           "warmup": a.warmup}
    with pir.Engine(2, 1, n, pitch, 1) as e:
        d_files = e.alloc_dev(N * pitch)
        e.fill_random_dev(d_files, N * pitch, 21)
        legs = {"tag": lambda: pir.mac_files_dev(d_files, pitch, N, payload, KEY, stream=e.stream)}
        if not a.no_floor:
            e.fill_shard_random(15)
            d_coefs, d_res = e.alloc_dev(N), e.alloc_dev(pitch)
            e.fill_random_dev(d_coefs, N, 22)
            legs["floor"] = lambda: e.answer_coefs_dev(d_coefs, N, 0, N, d_res)
        # the kernel's tags are right at this size too: a sample against the host mac()
        legs["tag"]()
        e.sync()
        from erasurecodedpir_amd import server as S
        ok = True
        for i in (0, 1, N // 3, N - 1):
            rec = e.d2h(d_files + i * pitch, pitch).tobytes()
            ok = ok and rec[payload:] == S.mac(KEY, rec[:payload])
        out["sample_tags_match_host_mac"] = bool(ok)
        for _ in range(a.warmup):
            for fn in legs.values():
                fn()
        e.sync()
        ms = {k: [] for k in legs}
        for _ in range(a.iters):
            for k, fn in legs.items():
                ms[k].append(ev.time(e.stream, fn))
        out["legs"] = {}
        for k, v in ms.items():
            med = statistics.median(v)
            out["legs"][k] = {"ms": round(med, 4), "ms_min": round(min(v), 4),
                              "ms_max": round(max(v), 4), "spread": round(max(v) - min(v), 4),
                              "gbps_of_database": round(N * pitch / med / 1e6, 1)}
        t = out["legs"]["tag"]["ms"]
        out["sha256_blocks_per_s"] = round(N * blocks / (t * 1e-3), 0)
        if "floor" in out["legs"]:
            out["tag_over_floor"] = round(t / out["legs"]["floor"]["ms"], 2)
        if not a.no_host:
            nh, rate = host_leg(e, d_files, pitch, payload, min(a.host_log_files, n))
            host_ms = N / rate * 1e3
            out["host"] = {"files_measured": nh, "threads": WORKERS * THREADS,
                           "files_per_s": round(rate, 0), "ms_scaled_to_database": round(host_ms, 1),
                           "scaled_by": N // nh}
            out["host_scaled_over_tag"] = round(host_ms / t, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
