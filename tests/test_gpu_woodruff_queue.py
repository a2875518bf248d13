"""Queued Woodruff value queries (pir_engine_answer_woodruff_queue[_dev]): K keys, G per read of
the shard.  One coefficient kernel writes a group's pair products (the keys interleaved, the
group's products one packed GF(2^8) multiply), one G-round scan answers the group.

Every queue answer must equal, byte for byte, the single answer of the same key and range, the
unshared queue ($PIR_WD_SHARE=0) and the numpy restatement woodruff_ref of test_woodruff.py
(which the CPU tests there pin to the reference's own answers).  The arithmetic is exact: no
tolerance anywhere.  The knobs are read at engine creation, so they are set before it."""
import ctypes
import os

import numpy as np
import pytest

import _oracle as O
from test_shamir import MUL
from test_woodruff import _ranges, wd_m, wd_pairs, wd_rank, wd_start, woodruff_deriv_ref, woodruff_ref

gpu = pytest.mark.gpu
NAMES = ["pir_engine_answer_woodruff_queue", "pir_engine_answer_woodruff_queue_dev",
         "pir_engine_reserve_woodruff_queue"]


# -------------------------------------------------------------------------------- CPU test
def test_names_and_loud_errors():
    import erasurecodedpir_amd as pir
    from erasurecodedpir_amd import _lib
    with open(os.path.join(O.ROOT, "include", "pir_engine.h")) as f:
        header = f.read()
    for name in NAMES:
        assert "int %s(pir_engine_t *e" % name in header, name
        assert name in _lib.PROTOTYPES, name
    for m in ("answer_woodruff_queue", "answer_woodruff_queue_dev", "reserve_woodruff_queue"):
        assert callable(getattr(pir.Engine, m)), m
    # no engine: every call refuses, none answers
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    calls = [lambda: lib.pir_engine_answer_woodruff_queue(None, buf, 5, 1, 0, 1, buf),
             lambda: lib.pir_engine_answer_woodruff_queue_dev(None, buf, 5, 1, 0, 1, buf, None),
             lambda: lib.pir_engine_reserve_woodruff_queue(None, 4)]
    for name, call in zip(NAMES, calls):
        rc = call()
        assert rc != 0, name
        with pytest.raises(pir.PirError, match="null|bad argument"):
            _lib.check(rc, name)
    # ... and without a usable device there is no engine to call them on (no CPU path)
    try:
        e = pir.Engine(2, 1, 10, 16, 1)
    except pir.PirError as err:
        assert "pir_engine_create failed" in str(err)
    else:
        e.close()


# -------------------------------------------------------------------------------- GPU tests
@pytest.fixture(scope="module")
def pir():
    import erasurecodedpir_amd as pir
    pir.load()
    return pir


def _engine(pir, monkeypatch, n, efs, share=2, G=None, lds=None, **kw):
    for name, v in (("PIR_WD_SHARE", share), ("PIR_WD_G", G), ("PIR_WD_LDS", lds)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    return pir.Engine(2, 1, n, efs, 1, **kw)


_CASES = {}


def _case(n, efs, nkeys):
    """rows, keys and the restatement's answers of a shape: computed once, shared, never changed"""
    k = (n, efs, nkeys)
    if k not in _CASES:
        rng = np.random.default_rng(4000 + 97 * n + efs)
        rows = rng.integers(0, 256, (1 << n, efs), dtype=np.uint8)
        keys = rng.integers(0, 256, (nkeys, wd_m(n)), dtype=np.uint8)
        keys[:, 1] = 0      # a zero factor in every key
        want = np.stack([woodruff_ref(rows, key) for key in keys])
        for a in (rows, keys, want):
            a.setflags(write=False)
        _CASES[k] = (rows, keys, want)
    return _CASES[k]


def _free_device_bytes():
    """hipMemGetInfo of the HIP runtime the engine library runs on, after a device sync (what
    torch.cuda.mem_get_info wraps; torch's bundled runtime is a second one in the process and
    finds no device once the engine's is up, so the call goes to the engine's)."""
    with open("/proc/self/maps") as f:
        paths = [line.split()[-1] for line in f if "libamdhip64.so" in line]
    own = [p for p in paths if "/torch/" not in p] or paths
    hip = ctypes.CDLL(own[0])
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def _path(e, fn):
    e.set_profiling(1)
    got = fn()
    t = e.last_timings()
    e.set_profiling(0)
    assert {"launch", "scan", "reduce", "total"} <= set(t), t
    assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
    return got, t["fused"]


@gpu
@pytest.mark.parametrize("G", [None, 2, 4])
def test_group_boundaries(pir, monkeypatch, G):
    n, efs = 11, 1024   # M = 65: 2 080 pairs, the last triangle row cut by 32
    M, Gv = wd_m(n), G or 8
    assert M == 65 and M * (M - 1) // 2 - (1 << n) == 32
    rows, keys, want = _case(n, efs, 2 * 8 + 3)
    with _engine(pir, monkeypatch, n, efs, 2, G) as es, \
            _engine(pir, monkeypatch, n, efs, 0, G) as eu:
        es.set_shard(rows)
        eu.set_shard(rows)
        singles = np.stack([es.answer_woodruff(key) for key in keys])
        assert np.array_equal(singles, want)
        _, single_path = _path(es, lambda: es.answer_woodruff(keys[0]))
        assert single_path in (5.0, 6.0)
        for K in (0, 1, 2, Gv - 1, Gv, Gv + 1, 2 * Gv + 3):
            if K == 0:
                for e in (es, eu):
                    assert e.answer_woodruff_queue(keys[:0]).shape == (0, efs)
                continue
            got, path = _path(es, lambda: es.answer_woodruff_queue(keys[:K]))
            ungot, unpath = _path(eu, lambda: eu.answer_woodruff_queue(list(keys[:K])))
            print("G", Gv, "K", K, "path", path, unpath)
            assert got.shape == (K, efs)
            assert np.array_equal(got, want[:K]), K
            assert np.array_equal(got, singles[:K]), K
            assert np.array_equal(got, ungot), K
            assert path == (8.0 if K >= 2 else single_path), K
            assert unpath == single_path, K


@gpu
@pytest.mark.parametrize("n,efs", [(11, 1056), (12, 256), (10, 2048), (12, 96), (12, 64), (9, 24)])
def test_every_group_scan(pir, monkeypatch, n, efs):
    rows, keys, want = _case(n, efs, 2 * 8 + 3)
    with _engine(pir, monkeypatch, n, efs) as e:
        e.set_shard(rows)
        got = e.answer_woodruff_queue(keys)
        assert np.array_equal(got, want)
        for k in (0, 7, 18):
            assert np.array_equal(e.answer_woodruff(keys[k]), got[k]), k


@gpu
def test_product_table(pir, monkeypatch):
    """Keys that put (nearly) every unordered pair of byte values into every slot's multiply."""
    n, efs, K = 17, 64, 8
    N, M = 1 << n, wd_m(n)
    assert M == 513
    a, b = wd_pairs(M, N)
    keys = []
    for g in range(K):
        rng = np.random.default_rng(1700 + g)
        extra = rng.integers(0, 256, 1, dtype=np.uint8)
        key = rng.permutation(np.concatenate([np.arange(256, dtype=np.uint8),
                                              np.arange(256, dtype=np.uint8), extra]))
        x, y = key[a].astype(np.int64), key[b].astype(np.int64)
        seen = np.unique(np.minimum(x, y) * 256 + np.maximum(x, y)).size
        print("slot", g, "covers", seen / 32896)
        assert seen >= 0.999 * 32896, (g, seen)
        keys.append(key)
    rows = np.random.default_rng(17).integers(0, 256, (N, efs), dtype=np.uint8)
    with _engine(pir, monkeypatch, n, efs) as e:
        e.set_shard(rows)
        got = e.answer_woodruff_queue(keys)
    for g in range(K):
        assert np.array_equal(got[g], woodruff_ref(rows, keys[g])), g


@gpu
def test_byte_lane_isolation(pir, monkeypatch):
    n, efs, K = 11, 256, 8
    N, M = 1 << n, wd_m(n)
    rows, _, _ = _case(n, efs, 1)
    a, b = wd_pairs(M, N)
    a_last = int(a[-1])
    recs = [0, N - 1, wd_start(M, 7) - 1, wd_start(M, 7), wd_start(M, a_last) + 1,
            wd_start(M, 20) + 5, 77, 1000]
    assert len(set(recs)) == K and wd_start(M, a_last) + 1 < N - 1
    keys = np.zeros((K, M), np.uint8)
    for g, r in enumerate(recs):
        keys[g, a[r]], keys[g, b[r]] = 0xff, 0x80 + g
    ff = np.zeros((K, M), np.uint8)
    ff[0::2] = 0xff
    with _engine(pir, monkeypatch, n, efs) as e:
        e.set_shard(rows)
        got = e.answer_woodruff_queue(keys)
        for g, r in enumerate(recs):
            assert np.array_equal(got[g], MUL[int(MUL[0xff, 0x80 + g]), rows[r]]), (g, r)
        got = e.answer_woodruff_queue(ff)
        want = woodruff_ref(rows, ff[0])
        assert want.any()
        for g in range(K):
            assert np.array_equal(got[g], want if g % 2 == 0 else np.zeros(efs, np.uint8)), g


@gpu
def test_ranges(pir, monkeypatch):
    n, efs, K = 9, 24, 5
    N, M = 1 << n, wd_m(n)
    rows, keys, want = _case(n, efs, K)
    with _engine(pir, monkeypatch, n, efs) as e:
        e.set_shard(rows)
        for lo, hi in _ranges(M, N):
            got = e.answer_woodruff_queue(keys, lo, hi - lo)
            for k in range(K):
                assert np.array_equal(got[k], woodruff_ref(rows, keys[k], lo, hi)), (lo, hi, k)
        acc = np.zeros((K, efs), np.uint8)
        for lo, hi in [(0, 13), (13, 90), (90, N)]:
            acc ^= e.answer_woodruff_queue(keys, lo, hi - lo)
        assert np.array_equal(acc, e.answer_woodruff_queue(keys))
        assert np.array_equal(acc, want)


@gpu
def test_refusals(pir, monkeypatch):
    n, efs = 8, 16
    N, M = 1 << n, wd_m(n)
    keys = np.ones((3, M), np.uint8)
    with _engine(pir, monkeypatch, n, efs) as e:
        with pytest.raises(pir.PirError, match="M = %d" % M):
            e.answer_woodruff_queue(keys[:, :-1])
        with pytest.raises(pir.PirError, match="M = %d" % M):
            e.answer_woodruff_queue(np.ones((3, M + 1), np.uint8))
        with pytest.raises(pir.PirError, match="beyond"):
            e.answer_woodruff_queue(keys, 1, N)
        with pytest.raises(pir.PirError, match="beyond"):
            e.answer_woodruff_queue(keys, N + 1, 0)
        d_k, d_r = e.alloc_dev(3 * M), e.alloc_dev(3 * efs)
        with pytest.raises(pir.PirError, match="-1 keys"):
            e.answer_woodruff_queue_dev(d_k, M, -1, 0, N, d_r)
        with pytest.raises(pir.PirError, match="null"):
            e.answer_woodruff_queue_dev(None, M, 3, 0, N, d_r)
        with pytest.raises(pir.PirError, match="null"):
            e.answer_woodruff_queue_dev(d_k, M, 3, 0, N, None)
        e.answer_woodruff_queue_dev(None, M, 0, 0, N, None)   # an empty queue touches nothing
        e.attach_comm(pir.comm_unique_id(), 1, 0)
        with pytest.raises(pir.PirError, match="communicator"):
            e.answer_woodruff_queue(keys)
        with pytest.raises(pir.PirError, match="communicator"):
            e.reserve_woodruff_queue(3)
    with pir.Engine(2, 1, n, efs, 2) as e:
        with pytest.raises(pir.PirError, match="one round"):
            e.answer_woodruff_queue(keys)
    with pir.Engine(2, 1, n + 1, efs, 1, log_num_partitions=1, partition_index=0) as e:
        with pytest.raises(pir.PirError, match="split shard"):
            e.answer_woodruff_queue(np.ones((3, wd_m(n + 1)), np.uint8))


@gpu
def test_stale_state_and_streams(pir, monkeypatch):
    n, efs = 12, 256
    N, M = 1 << n, wd_m(n)
    rows, keys, want = _case(n, efs, 19)
    tree_keys = [pir.gen_keys(n, 100 + 37 * i, 2, 1)[0] for i in range(10)]
    steps = [lambda e: e.answer_stream(tree_keys),
             lambda e: e.answer_woodruff_queue(keys[:11]),
             lambda e: e.answer_woodruff(keys[3]),
             lambda e: e.answer_woodruff_queue(keys[11:14], 100, 3000),
             lambda e: e.answer_woodruff_deriv(keys[2]),
             lambda e: e.answer_woodruff_queue(keys[:11])]

    def fresh(step):
        with _engine(pir, monkeypatch, n, efs) as f:
            f.set_shard(rows)
            return step(f)

    with _engine(pir, monkeypatch, n, efs) as e, pir.Engine(2, 1, 6, 16, 1) as caller:
        e.set_shard(rows)
        for i, step in enumerate(steps):
            assert np.array_equal(step(e), fresh(step)), i
        assert np.array_equal(steps[1](e), want[:11])
        assert np.array_equal(steps[4](e), woodruff_deriv_ref(rows, keys[2]))
        # a queue on a caller's stream, then a single answer on the engine's, no host sync
        _, single_path = _path(e, lambda: e.answer_woodruff(keys[0]))
        d_k, d_r = e.alloc_dev(11 * M), e.alloc_dev(11 * efs)
        e.h2d(d_k, keys[:11].reshape(-1))
        e.set_profiling(4)
        e.answer_woodruff_queue_dev(d_k, M, 11, 0, N, d_r, stream=caller.stream)
        single = e.answer_woodruff(keys[5])
        caller.sync()
        t = e.last_timings()
        assert t["fused"] == (8.0 + single_path) / 2, t   # each slot read with its own path
        assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
        assert np.array_equal(single, want[5])
        assert np.array_equal(e.d2h(d_r, 11 * efs).reshape(11, efs), want[:11])
        e.set_profiling(0)
        e.free_dev(d_k)
        e.free_dev(d_r)
    # a reserved queue allocates nothing: shared, and under the default policy
    for share in (2, None):
        with _engine(pir, monkeypatch, n, efs, share) as e:
            e.set_shard(rows)
            d_k, d_r = e.alloc_dev(19 * M), e.alloc_dev(19 * efs)
            e.h2d(d_k, keys.reshape(-1))
            e.answer_woodruff_queue_dev(d_k, M, 2, 0, 1, d_r)   # a tiny queue: tiny buffers
            e.sync()
            e.reserve_woodruff_queue(19)
            free0 = _free_device_bytes()
            e.answer_woodruff_queue_dev(d_k, M, 19, 0, N, d_r)
            e.sync()
            free1 = _free_device_bytes()
            print("share", share, "free before", free0, "after", free1)
            assert free1 >= free0, (share, free0, free1)
            assert np.array_equal(e.d2h(d_r, 19 * efs).reshape(19, efs), want)


@gpu
def test_unaligned_device_keys(pir, monkeypatch):
    n, efs, K = 11, 1024, 8
    N, M = 1 << n, wd_m(n)
    assert M % 2 == 1
    rows, keys, want = _case(n, efs, 2 * 8 + 3)
    with _engine(pir, monkeypatch, n, efs) as e:
        e.set_shard(rows)
        d_k, d_r = e.alloc_dev(K * M + 3), e.alloc_dev(K * efs)
        e.h2d(d_k + 3, keys[:K].reshape(-1))
        e.answer_woodruff_queue_dev(d_k + 3, M, K, 0, N, d_r)
        e.sync()
        assert np.array_equal(e.d2h(d_r, K * efs).reshape(K, efs), want[:K])


@gpu
@pytest.mark.parametrize("G", [None, 2, 4])
def test_key_table_in_global_memory(pir, monkeypatch, G):
    """$PIR_WD_LDS=0: the interleaved key table of the large domains (W M past the LDS budget,
    n >= 25 at 8 keys per pass), built by the transposing kernel, at a size a test can hold."""
    n, efs = 11, 1024
    N, M, Gv = 1 << n, wd_m(n), G or 8
    rows, keys, want = _case(n, efs, 2 * 8 + 3)
    K = 2 * Gv + 1
    with _engine(pir, monkeypatch, n, efs, 2, G, lds=0) as e:
        e.set_shard(rows)
        d_k, d_r = e.alloc_dev(K * M + 1), e.alloc_dev(K * efs)
        e.h2d(d_k + 1, keys[:K].reshape(-1))
        e.answer_woodruff_queue_dev(d_k + 1, M, K, 0, N, d_r)
        e.sync()
        assert np.array_equal(e.d2h(d_r, K * efs).reshape(K, efs), want[:K])
        lo, hi = wd_start(M, 3) - 1, N - 7
        got = e.answer_woodruff_queue(keys[:K], lo, hi - lo)
        assert np.array_equal(got[K - 1], woodruff_ref(rows, keys[K - 1], lo, hi))


@gpu
def test_default_policy_at_a_measured_shape(pir, monkeypatch):
    """No knob set, 2^20 x 1 KiB: queues of 4 keys and more share passes (the measured policy),
    shorter ones do not; the answers are the single answers either way."""
    n, efs = 20, 1024
    M = wd_m(n)
    keys = np.random.default_rng(20).integers(0, 256, (5, M), dtype=np.uint8)
    with _engine(pir, monkeypatch, n, efs, None) as e:
        e.fill_shard_random(2024)
        singles = np.stack([e.answer_woodruff(key) for key in keys])
        _, single_path = _path(e, lambda: e.answer_woodruff(keys[0]))
        assert singles.any(axis=1).all()
        for K, want_path in ((3, single_path), (4, 8.0), (5, 8.0)):
            got, path = _path(e, lambda: e.answer_woodruff_queue(keys[:K]))
            assert path == want_path, (K, path)
            assert np.array_equal(got, singles[:K]), K
