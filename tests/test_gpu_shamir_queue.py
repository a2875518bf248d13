"""Queued Shamir sqrt(N) queries (pir_engine_answer_shamir_queue[_dev]): the K x num_rounds
rounds of a queue are independent virtual keys, 8 per read of the shard.  Per group one key
table, two segmented transposed passes over the value rows (Rx, Ry straight into the responses)
and one 8-round scan of the Hermite rows.

Every check compares four things byte for byte: the queue with $PIR_SH_SHARE=2, the queue with
$PIR_SH_SHARE=0, the single answers, and the numpy restatement shamir_ref of test_shamir.py (which
the CPU tests there pin to the reference's own answers).  The arithmetic is exact: no tolerance
anywhere.  The knobs are read at engine creation, so they are set before it."""
import ctypes
import os

import numpy as np
import pytest

import _oracle as O
from test_shamir import CASES, IDS, _hex, _host_rows, _setup, dims, shamir_ref
from test_shamir import shamir_mode  # noqa: F401  (fixture)

gpu = pytest.mark.gpu
NAMES = ["pir_engine_answer_shamir_queue", "pir_engine_answer_shamir_queue_dev",
         "pir_engine_reserve_shamir_queue"]


# -------------------------------------------------------------------------------- CPU test
def test_names_and_loud_errors():
    import erasurecodedpir_amd as pir
    from erasurecodedpir_amd import _lib
    with open(os.path.join(O.ROOT, "include", "pir_engine.h")) as f:
        header = f.read()
    for name in NAMES:
        assert "int %s(pir_engine_t *e" % name in header, name
        assert name in _lib.PROTOTYPES, name
    for m in ("answer_shamir_queue", "answer_shamir_queue_dev", "reserve_shamir_queue"):
        assert callable(getattr(pir.Engine, m)), m
    # no engine: every call refuses, none answers
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    ptrs = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    calls = [lambda: lib.pir_engine_answer_shamir_queue(None, ptrs, 1, 0, 1, buf),
             lambda: lib.pir_engine_answer_shamir_queue_dev(None, buf, 8, 8, 1, 0, 1, buf, None),
             lambda: lib.pir_engine_reserve_shamir_queue(None, 4)]
    for name, call in zip(NAMES, calls):
        rc = call()
        assert rc != 0, name
        with pytest.raises(pir.PirError, match="null|bad argument"):
            _lib.check(rc, name)


# -------------------------------------------------------------------------------- GPU tests
@pytest.fixture(scope="module")
def pir():
    import erasurecodedpir_amd as pir
    pir.load()
    return pir


def _engine(pir, monkeypatch, n, efs, nq=1, share=2, G=None, **kw):
    """A Shamir engine: value rows [0, N), Hermite rows [N, 2N)."""
    monkeypatch.delenv("PIR_SH_PASS", raising=False)
    for name, v in (("PIR_SH_SHARE", share), ("PIR_SH_G", G)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    return pir.Engine(2, 1, n + 1, efs, nq, **kw)


_CASES = {}


def _case(n, efs, nq, K):
    """rows, keys and the restatement's answers of a shape: computed once, shared, never changed"""
    k = (n, efs, nq, K)
    if k not in _CASES:
        x, y, X, Y = dims(n)
        rng = np.random.default_rng(5000 + 97 * n + efs + 7 * nq)
        rows = rng.integers(0, 256, (2 << n, efs), dtype=np.uint8)
        keys = rng.integers(0, 256, (K, nq, X + Y), dtype=np.uint8)
        keys[:, :, 0] = 0      # a zero factor in every key
        want = shamir_ref(rows, keys.reshape(K * nq, X + Y), n).reshape(K, nq, X + Y + 2, efs)
        for a in (rows, keys, want):
            a.setflags(write=False)
        _CASES[k] = (rows, keys, want)
    return _CASES[k]


def _ref(rows, keys, n, lo, hi):
    K, nq, kl = keys.shape
    return shamir_ref(rows, keys.reshape(K * nq, kl), n, lo, hi).reshape(K, nq, kl + 2, -1)


def _singles(e, keys, lo=0, nrec=None):
    return np.stack([e.answer_shamir(k, lo, nrec) for k in keys])


def _free_device_bytes():
    """hipMemGetInfo of the HIP runtime the engine library runs on, after a device sync."""
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


def _four_way(pir, monkeypatch, n, efs, nq, K, G=None, ranges=None, shared_path=10.0):
    """shared queue == unshared queue == single answers == shamir_ref over every range"""
    rows, keys, want = _case(n, efs, nq, K)
    N = 1 << n
    with _engine(pir, monkeypatch, n, efs, nq, 2, G) as es, \
            _engine(pir, monkeypatch, n, efs, nq, 0, G) as eu:
        es.set_shard(rows)
        eu.set_shard(rows)
        for lo, hi in ranges or [(0, N)]:
            ref = want if (lo, hi) == (0, N) else _ref(rows, keys, n, lo, hi)
            got, path = _path(es, lambda: es.answer_shamir_queue(keys, lo, hi - lo))
            ungot, unpath = _path(eu, lambda: eu.answer_shamir_queue(keys, lo, hi - lo))
            print("n", n, "efs", efs, "nq", nq, "K", K, "range", lo, hi, "path", path, unpath)
            assert got.shape == ref.shape
            assert np.array_equal(got, ref), (lo, hi)
            assert np.array_equal(ungot, ref), (lo, hi)
            assert np.array_equal(_singles(es, keys, lo, hi - lo), ref), (lo, hi)
            assert path == (shared_path if hi > lo and K * nq >= 2 else 4.0), (lo, hi, path)
            assert unpath == 4.0, (lo, hi, unpath)


# (6, 256): segments shorter than 16 rows; (11, 512): Y = 32, less than a chunk; (12, 256): one
# chunk, one column group; (13, 1024): odd n, two chunks in the strided walk, 4 column groups;
# (13, 1030): pitch 1040, a ragged fifth column group and a bytewise tail store; the two smallest
# domains
@gpu
@pytest.mark.parametrize("n,efs", [(6, 256), (11, 512), (12, 256), (13, 1024), (13, 1030),
                                   (0, 256), (1, 256)])
def test_shapes(pir, monkeypatch, n, efs):
    _four_way(pir, monkeypatch, n, efs, 1, 9)


@gpu
def test_narrow_records_run_unshared(pir, monkeypatch):
    _four_way(pir, monkeypatch, 9, 100, 1, 9, shared_path=4.0)   # pitch 112 < 256


@gpu
@pytest.mark.parametrize("G", [None, 2, 4])
def test_group_boundaries(pir, monkeypatch, G):
    n, efs = 12, 256
    x, y, X, Y = dims(n)
    rows, keys, want = _case(n, efs, 1, 19)
    with _engine(pir, monkeypatch, n, efs, 1, 2, G) as es, \
            _engine(pir, monkeypatch, n, efs, 1, 0, G) as eu:
        es.set_shard(rows)
        eu.set_shard(rows)
        singles = _singles(es, keys)
        assert np.array_equal(singles, want)
        for K in (0, 1, 2, 7, 8, 9, 19):
            if K == 0:
                for e in (es, eu):
                    assert e.answer_shamir_queue(keys[:0]).shape == (0, 1, X + Y + 2, efs)
                continue
            got, path = _path(es, lambda: es.answer_shamir_queue(keys[:K]))
            ungot, unpath = _path(eu, lambda: eu.answer_shamir_queue(keys[:K]))
            print("G", G, "K", K, "path", path, unpath)
            assert np.array_equal(got, want[:K]), K
            assert np.array_equal(ungot, want[:K]), K
            assert path == (10.0 if K >= 2 else 4.0), K
            assert unpath == 4.0, K


@gpu
@pytest.mark.parametrize("nq", [2, 3])
def test_multi_round_engines(pir, monkeypatch, nq):
    n, efs, K = 12, 256, 5
    _four_way(pir, monkeypatch, n, efs, nq, K)
    # the device form: key_stride larger than nq * key_pitch, an odd key address
    x, y, X, Y = dims(n)
    kl, N = X + Y, 1 << n
    rows, keys, want = _case(n, efs, nq, K)
    pitch, stride = kl + 5, nq * (kl + 5) + 11
    host = np.zeros(1 + K * stride, np.uint8)
    for k in range(K):
        for a in range(nq):
            host[1 + k * stride + a * pitch:][:kl] = keys[k, a]
    for share in (2, 0):
        with _engine(pir, monkeypatch, n, efs, nq, share) as e:
            e.set_shard(rows)
            rl = e.shamir_response_len
            d_k, d_r = e.alloc_dev(host.size), e.alloc_dev(K * nq * rl)
            e.h2d(d_k, host)
            e.answer_shamir_queue_dev(d_k + 1, pitch, stride, K, 0, N, d_r)
            e.sync()
            assert np.array_equal(e.d2h(d_r, K * nq * rl).reshape(want.shape), want), share


@gpu
@pytest.mark.parametrize("passes", [0, 1, 2])
def test_value_passes_on_the_four_round_kernels(pir, monkeypatch, passes):
    """$PIR_SH_PASS: either value pass of a shared queue on k_shamir_rows / k_shamir_strips, up
    to 4 virtual keys per launch (what the policy picks where the transposed pass measured no
    faster), one round per key and three."""
    for nq, K in ((1, 9), (3, 5)):
        n, efs = 12, 256
        rows, keys, want = _case(n, efs, nq, K)
        with _engine(pir, monkeypatch, n, efs, nq) as e:
            e.set_shard(rows)
            monkeypatch.setenv("PIR_SH_PASS", str(passes))
            got, path = _path(e, lambda: e.answer_shamir_queue(keys))
            assert path == 10.0
            assert np.array_equal(got, want), (nq, passes)
            lo, hi = 5, 35 * 64 + 7
            assert np.array_equal(e.answer_shamir_queue(keys, lo, hi - lo),
                                  _ref(rows, keys, n, lo, hi)), (nq, passes)


@gpu
def test_ranges(pir, monkeypatch):
    n, efs, K = 12, 256, 9
    x, y, X, Y = dims(n)
    N = 1 << n
    _four_way(pir, monkeypatch, n, efs, 1, K,
              ranges=[(5, 35 * Y + 7),   # cuts its first and last matrix row
                      (3 * Y + 3, 3 * Y + 9),   # inside one matrix row
                      (77, 78), (N - 1, N), (0, 1),   # one record
                      (0, 0), (10, 10), (N, N)])   # empty
    rows, keys, want = _case(n, efs, 1, K)
    with _engine(pir, monkeypatch, n, efs) as e:
        e.set_shard(rows)
        acc = np.zeros_like(want)
        for lo, hi in [(0, 13), (13, 1990), (1990, N)]:
            acc ^= e.answer_shamir_queue(keys, lo, hi - lo)
        assert np.array_equal(acc, e.answer_shamir_queue(keys))
        assert np.array_equal(acc, want)
        with pytest.raises(pir.PirError, match="beyond"):
            e.answer_shamir_queue(keys, 1, N)


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_goldens_queued(pir, shamir_mode, case, monkeypatch):  # noqa: F811
    """The reference's rows and keys, queued three times over with the keys in a different order
    each time, against the reference's own answers."""
    _setup(shamir_mode, case)
    prm = case["params"]
    n, efs, nq = prm["LOG_NUM_ENCODED_FILES"], prm["ENCODED_FILE_SIZE_BYTES"], prm["NUM_ROUNDS"]
    rows = _host_rows(shamir_mode, case, case["party"], monkeypatch)
    keys = _hex(case["keys"], (nq, case["key_len"]))
    want = _hex(case["answer"], (nq, case["key_len"] + 2, efs))
    orders = [np.arange(nq), np.arange(nq)[::-1], np.roll(np.arange(nq), 1)]
    queue = np.stack([keys[o] for o in orders])
    for share in (2, 0):
        with _engine(pir, monkeypatch, n, efs, nq, share) as e:
            e.set_shard(rows)
            got = e.answer_shamir_queue(queue)
            for i, o in enumerate(orders):
                assert np.array_equal(got[i], want[o]), (share, i)
            assert np.array_equal(e.answer_shamir(keys), want)


@gpu
def test_byzantine(pir, monkeypatch):
    n, efs, K = 12, 256, 3
    N = 1 << n
    rows, keys, want = _case(n, efs, 1, 9)
    keys, want = keys[:K], want[:K]
    for share in (2, 0):
        with _engine(pir, monkeypatch, n, efs, 1, share, is_byzantine=True) as e:
            e.set_shard(rows)
            a, b = e.answer_shamir_queue(keys), e.answer_shamir_queue(keys)
            assert not np.array_equal(a, b)
            for k in range(K):      # random, and fresh for each key
                assert not np.array_equal(a[k], want[k])
                assert not np.array_equal(a[k], a[(k + 1) % K])
            got = e.answer_shamir_queue(keys, 0, N - 1) ^ e.answer_shamir_queue(keys, N - 1, 1)
            assert np.array_equal(got, want), share


@gpu
def test_refusals(pir, monkeypatch):
    n, efs = 8, 256
    x, y, X, Y = dims(n)
    N, kl = 1 << n, X + Y
    keys = np.ones((3, 1, kl), np.uint8)
    with pir.Engine(2, 1, n + 1, efs, 1, log_num_partitions=1, partition_index=0) as e:
        with pytest.raises(pir.PirError, match="split shard"):
            e.answer_shamir_queue(np.ones((3, 1, e.shamir_key_len), np.uint8), 0, 1)
        with pytest.raises(pir.PirError, match="split shard"):
            e.reserve_shamir_queue(3)
    with _engine(pir, monkeypatch, n, efs, 2) as e:
        rl = e.shamir_response_len
        d_k, d_r = e.alloc_dev(6 * kl), e.alloc_dev(6 * rl)
        with pytest.raises(pir.PirError, match="key_pitch"):
            e.answer_shamir_queue_dev(d_k, kl - 1, 2 * kl, 3, 0, N, d_r)
        with pytest.raises(pir.PirError, match="key_stride"):
            e.answer_shamir_queue_dev(d_k, kl, kl - 1, 3, 0, N, d_r)
        with pytest.raises(pir.PirError, match="-1 keys"):
            e.answer_shamir_queue_dev(d_k, kl, 2 * kl, -1, 0, N, d_r)
        with pytest.raises(pir.PirError, match="null"):
            e.answer_shamir_queue_dev(None, kl, 2 * kl, 3, 0, N, d_r)
        with pytest.raises(pir.PirError, match="null"):
            e.answer_shamir_queue_dev(d_k, kl, 2 * kl, 3, 0, N, None)
        with pytest.raises(pir.PirError, match="beyond"):
            e.answer_shamir_queue_dev(d_k, kl, 2 * kl, 3, N + 1, 0, d_r)
        e.answer_shamir_queue_dev(None, kl, 2 * kl, 0, 0, N, None)   # an empty queue touches nothing
    with _engine(pir, monkeypatch, n, efs) as e:
        e.attach_comm(pir.comm_unique_id(), 1, 0)
        with pytest.raises(pir.PirError, match="communicator"):
            e.answer_shamir_queue(keys)
        with pytest.raises(pir.PirError, match="communicator"):
            e.reserve_shamir_queue(3)


@gpu
def test_stale_state(pir, monkeypatch):
    """Two different shards and key sets back to back on one engine, a range call, a single
    answer and a tree queue between them."""
    n, efs, nq, K = 12, 256, 1, 9
    sets = [_case(n, efs, nq, K), _case(n, efs + 4, nq, K)]
    tree_keys = [pir.gen_keys(n + 1, 100 + 37 * i, 2, 1)[0] for i in range(10)]
    with _engine(pir, monkeypatch, n, efs) as e:
        for rows, keys, want in sets:
            rows = np.ascontiguousarray(rows[:, :efs])
            ref = _ref(rows, keys, n, 0, 1 << n)
            e.set_shard(rows)
            assert np.array_equal(e.answer_shamir_queue(keys), ref)
            assert np.array_equal(e.answer_shamir_queue(keys[:3], 100, 1700),
                                  _ref(rows, keys[:3], n, 100, 1800))
            e.answer_stream(tree_keys)
            assert np.array_equal(e.answer_shamir(keys[4]), ref[4])
            assert np.array_equal(e.answer_shamir_queue(keys[::-1]), ref[::-1])


@gpu
def test_caller_stream_profiling_and_reserve(pir, monkeypatch):
    n, efs, K = 12, 256, 9
    x, y, X, Y = dims(n)
    N, kl = 1 << n, X + Y
    rows, keys, want = _case(n, efs, 1, K)
    tree_key = pir.gen_keys(n + 1, 1234, 2, 1)[0]
    with _engine(pir, monkeypatch, n, efs) as e, pir.Engine(2, 1, 6, 16, 1) as caller:
        e.set_shard(rows)
        rl = e.shamir_response_len
        e.set_profiling(1)
        want_tree = e.answer(tree_key)
        tree_path = e.last_timings()["fused"]
        e.set_profiling(0)
        d_k, d_r = e.alloc_dev(K * kl), e.alloc_dev(K * rl)
        e.h2d(d_k, keys.reshape(-1))
        # alone, on a caller's stream
        e.set_profiling(4)
        e.answer_shamir_queue_dev(d_k, kl, kl, K, 0, N, d_r, stream=caller.stream)
        caller.sync()
        t = e.last_timings()
        assert t["fused"] == 10.0 and {"launch", "scan", "reduce", "total"} <= set(t), t
        assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
        assert t["scan"] <= t["total"]
        assert np.array_equal(e.d2h(d_r, K * rl).reshape(want.shape), want)
        # the queue on the caller's stream, then a tree answer on the engine's, no host sync:
        # each profiling slot is read with its own path
        e.answer_shamir_queue_dev(d_k, kl, kl, K, 0, N, d_r, stream=caller.stream)
        got_tree = e.answer(tree_key)
        caller.sync()
        t = e.last_timings()
        assert t["fused"] == (10.0 + tree_path) / 2, t
        assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
        assert np.array_equal(got_tree, want_tree)
        assert np.array_equal(e.d2h(d_r, K * rl).reshape(want.shape), want)
        e.set_profiling(0)
    # a reserved queue allocates nothing: shared, unshared, and under the default policy
    for share in (2, 0, None):
        with _engine(pir, monkeypatch, n, efs, 1, share) as e:
            e.set_shard(rows)
            rl = e.shamir_response_len
            d_k, d_r = e.alloc_dev(K * kl), e.alloc_dev(K * rl)
            e.h2d(d_k, keys.reshape(-1))
            e.answer_shamir_queue_dev(d_k, kl, kl, 2, 0, 1, d_r)   # a tiny queue: tiny buffers
            e.sync()
            e.reserve_shamir_queue(K)
            free0 = _free_device_bytes()
            e.answer_shamir_queue_dev(d_k, kl, kl, K, 0, N, d_r)
            e.sync()
            got = e.answer_shamir_queue(keys)
            free1 = _free_device_bytes()
            print("share", share, "free before", free0, "after", free1)
            assert free1 >= free0, (share, free0, free1)
            assert np.array_equal(e.d2h(d_r, K * rl).reshape(want.shape), want)
            assert np.array_equal(got, want)


@gpu
def test_default_policy(pir, monkeypatch):
    """No knob set: 2^20 x 1 KiB is a measured shape, so queues of two and more virtual keys
    share passes; 2^12 x 256 B is not, so they do not.  The answers are the single answers."""
    for n, efs, want_path in ((20, 1024, 10.0), (12, 256, 4.0)):
        x, y, X, Y = dims(n)
        keys = np.random.default_rng(n).integers(0, 256, (3, 1, X + Y), dtype=np.uint8)
        with _engine(pir, monkeypatch, n, efs, 1, None) as e:
            e.fill_shard_random(2026)
            singles = _singles(e, keys)
            assert singles.any(axis=(1, 2, 3)).all()
            for K in (1, 2, 3):
                got, path = _path(e, lambda: e.answer_shamir_queue(keys[:K]))
                assert path == (want_path if K >= 2 else 4.0), (n, K, path)
                assert np.array_equal(got, singles[:K]), (n, K)


@gpu
def test_row_addresses_past_32_bits(pir, monkeypatch):
    """n = 22 x 2 KiB: the value rows take 2^33 bytes, the strided pass spans them all, and a
    32-bit row offset wraps.  No restatement at this size: a shared queue of 8 one-round keys
    against the 8 single answers on the same engine."""
    n, efs, K = 22, 2048, 8
    x, y, X, Y = dims(n)
    assert (1 << n) * efs == 1 << 33
    keys = np.random.default_rng(22).integers(0, 256, (K, 1, X + Y), dtype=np.uint8)
    with _engine(pir, monkeypatch, n, efs) as e:
        e.fill_shard_random(2222)
        got, path = _path(e, lambda: e.answer_shamir_queue(keys))
        assert path == 10.0
        singles = _singles(e, keys)
        assert singles.any(axis=(1, 2, 3)).all()
        assert np.array_equal(got, singles)
        # the last matrix rows alone: every row address of the range is past 2^32
        lo = (X - 3) * Y + 5
        got = e.answer_shamir_queue(keys[:3], lo, (1 << n) - lo)
        assert np.array_equal(got, _singles(e, keys[:3], lo, (1 << n) - lo))
