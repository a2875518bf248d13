"""Queued Woodruff derivative queries (pir_engine_answer_woodruff_deriv_queue[_dev]): 8 keys per
read of the shard.  Per group one key table, the rows pass (a transposed four-Russians fold per
triangle row, stored into every key's response), the totals kernel per key, and the columns pass
(the same fold per column, XORed into what the rows pass stored).

Every check compares four things byte for byte: the queue with $PIR_WDD_SHARE=2, the queue with
$PIR_WDD_SHARE=0, the single answers, and the numpy restatement woodruff_deriv_ref of
test_woodruff.py (which the CPU tests there pin to the reference's own answers).  The arithmetic
is exact: no tolerance anywhere.  The knobs are read at engine creation, so they are set before
it."""
import ctypes
import os

import numpy as np
import pytest

import _oracle as O
from test_woodruff import CASES, IDS, _hex, _rows, wd_m, wd_pairs, wd_start, woodruff_deriv_ref

gpu = pytest.mark.gpu
NAMES = ["pir_engine_answer_woodruff_deriv_queue", "pir_engine_answer_woodruff_deriv_queue_dev",
         "pir_engine_reserve_woodruff_deriv_queue"]


# -------------------------------------------------------------------------------- CPU test
def test_names_and_loud_errors():
    import erasurecodedpir_amd as pir
    from erasurecodedpir_amd import _lib
    with open(os.path.join(O.ROOT, "include", "pir_engine.h")) as f:
        header = f.read()
    for name in NAMES:
        assert "int %s(pir_engine_t *e" % name in header, name
        assert name in _lib.PROTOTYPES, name
    for m in ("answer_woodruff_deriv_queue", "answer_woodruff_deriv_queue_dev",
              "reserve_woodruff_deriv_queue"):
        assert callable(getattr(pir.Engine, m)), m
    # no engine: every call refuses, none answers
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    calls = [lambda: lib.pir_engine_answer_woodruff_deriv_queue(None, buf, 3, 1, 0, 1, buf),
             lambda: lib.pir_engine_answer_woodruff_deriv_queue_dev(None, buf, 3, 1, 0, 1, buf, None),
             lambda: lib.pir_engine_reserve_woodruff_deriv_queue(None, 4)]
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


def _engine(pir, monkeypatch, n, efs, share=2, G=None, nq=1, **kw):
    monkeypatch.delenv("PIR_WDD_PAIR", raising=False)
    for name, v in (("PIR_WDD_SHARE", share), ("PIR_WDD_G", G)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    return pir.Engine(2, 1, n, efs, nq, **kw)


_CASES = {}


def _case(n, efs, K, seed=0):
    """rows, keys and the restatement's answers of a shape: computed once, shared, never changed"""
    k = (n, efs, K, seed)
    if k not in _CASES:
        M = wd_m(n)
        rng = np.random.default_rng(6000 + 97 * n + efs + 1000 * seed)
        rows = rng.integers(0, 256, (1 << n, efs), dtype=np.uint8)
        keys = rng.integers(0, 256, (K, M), dtype=np.uint8)
        keys[np.arange(K), rng.integers(0, M, K)] = 0      # a zero byte in every key
        want = np.stack([woodruff_deriv_ref(rows, key) for key in keys])
        for a in (rows, keys, want):
            a.setflags(write=False)
        _CASES[k] = (rows, keys, want)
    return _CASES[k]


def _ref(rows, keys, lo, hi):
    return np.stack([woodruff_deriv_ref(rows, key, lo, hi) for key in keys])


def _singles(e, keys, lo=0, nrec=None):
    return np.stack([e.answer_woodruff_deriv(k, lo, nrec) for k in keys])


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


def _four_way(pir, monkeypatch, n, efs, K, G=None, ranges=None, shared_path=11.0):
    """shared queue == unshared queue == single answers == woodruff_deriv_ref over every range"""
    rows, keys, want = _case(n, efs, K)
    N = 1 << n
    with _engine(pir, monkeypatch, n, efs, 2, G) as es, \
            _engine(pir, monkeypatch, n, efs, 0, G) as eu:
        es.set_shard(rows)
        eu.set_shard(rows)
        for lo, hi in ranges or [(0, N)]:
            ref = want if (lo, hi) == (0, N) else _ref(rows, keys, lo, hi)
            got, path = _path(es, lambda: es.answer_woodruff_deriv_queue(keys, lo, hi - lo))
            ungot, unpath = _path(eu, lambda: eu.answer_woodruff_deriv_queue(keys, lo, hi - lo))
            print("n", n, "efs", efs, "K", K, "range", lo, hi, "path", path, unpath)
            assert got.shape == ref.shape
            assert np.array_equal(got, ref), (lo, hi)
            assert np.array_equal(ungot, ref), (lo, hi)
            assert np.array_equal(_singles(es, keys, lo, hi - lo), ref), (lo, hi)
            assert path == (shared_path if hi > lo and K >= 2 else 7.0), (lo, hi, path)
            assert unpath == 7.0, (lo, hi, unpath)


# (0 .. 2, 256): the smallest domains (M = 3, N = 1 leaves triangle rows 1 and 2 empty);
# (6, 256): every segment shorter than the 16 rows loaded ahead; (11, 512): M = 65, triangle row 0
# is exactly one 64-row chunk and rows 57 .. 63 lie wholly past N; (12, 256): 91 rows, one chunk
# and a ragged second, one column group; (13, 1024): M = 129, exactly two chunks, 4 column groups,
# the last 64 ranks unused (row 117 cut, rows >= 118 empty); (14, 1030): M = 182, two chunks and
# a ragged third, pitch 1040: a ragged fifth column group and the bytewise tail store
@gpu
@pytest.mark.parametrize("n,efs,M", [(0, 256, 3), (1, 256, 3), (2, 256, 4), (6, 256, 12),
                                     (11, 512, 65), (12, 256, 92), (13, 1024, 129),
                                     (14, 1030, 182)])
def test_shapes(pir, monkeypatch, n, efs, M):
    assert wd_m(n) == M
    _four_way(pir, monkeypatch, n, efs, 9)


@gpu
def test_narrow_records_run_unshared(pir, monkeypatch):
    _four_way(pir, monkeypatch, 9, 100, 9, shared_path=7.0)   # pitch 112 < 256


@gpu
@pytest.mark.parametrize("G", [None, 2, 4])
def test_group_boundaries(pir, monkeypatch, G):
    n, efs = 12, 256
    M = wd_m(n)
    rows, keys, want = _case(n, efs, 19)
    with _engine(pir, monkeypatch, n, efs, 2, G) as es, \
            _engine(pir, monkeypatch, n, efs, 0, G) as eu:
        es.set_shard(rows)
        eu.set_shard(rows)
        assert np.array_equal(_singles(es, keys), want)
        for K in (0, 1, 2, 7, 8, 9, 19):
            if K == 0:
                for e in (es, eu):
                    assert e.answer_woodruff_deriv_queue(keys[:0]).shape == (0, M + 1, efs)
                continue
            got, path = _path(es, lambda: es.answer_woodruff_deriv_queue(keys[:K]))
            ungot, unpath = _path(eu, lambda: eu.answer_woodruff_deriv_queue(keys[:K]))
            print("G", G, "K", K, "path", path, unpath)
            assert np.array_equal(got, want[:K]), K
            assert np.array_equal(ungot, want[:K]), K
            assert path == (11.0 if K >= 2 else 7.0), K
            assert unpath == 7.0, K


@gpu
def test_ranges(pir, monkeypatch):
    n, efs, K = 12, 256, 9
    N, M = 1 << n, wd_m(n)
    s = lambda a: wd_start(M, a)  # noqa: E731
    _four_way(pir, monkeypatch, n, efs, K,
              ranges=[(s(3) + 5, s(40) + 7),      # cuts its first and last triangle row
                      (s(7) + 3, s(7) + 9),       # inside one triangle row
                      (0, 1), (N - 1, N), (1777, 1778),      # one record
                      (0, 0), (1000, 1000), (N, N)])      # empty
    rows, keys, want = _case(n, efs, K)
    with _engine(pir, monkeypatch, n, efs) as e:
        e.set_shard(rows)
        acc = np.zeros_like(want)
        for lo, hi in [(0, 13), (13, 1990), (1990, N)]:
            acc ^= e.answer_woodruff_deriv_queue(keys, lo, hi - lo)
        assert np.array_equal(acc, e.answer_woodruff_deriv_queue(keys))
        assert np.array_equal(acc, want)
        with pytest.raises(pir.PirError, match="beyond"):
            e.answer_woodruff_deriv_queue(keys, 1, N)


@gpu
def test_device_form_caller_stream_and_profiling(pir, monkeypatch):
    n, efs, K = 12, 256, 9
    N, M = 1 << n, wd_m(n)
    rl = (M + 1) * efs
    rows, keys, want = _case(n, efs, K)
    tree_key = pir.gen_keys(n, 1234, 2, 1)[0]
    with _engine(pir, monkeypatch, n, efs) as e, pir.Engine(2, 1, 6, 16, 1) as caller:
        e.set_shard(rows)
        e.set_profiling(1)
        want_tree = e.answer(tree_key)
        tree_path = e.last_timings()["fused"]
        e.set_profiling(0)
        d_k, d_r = e.alloc_dev(K * M + 3), e.alloc_dev(K * rl)
        e.h2d(d_k + 3, keys.reshape(-1))   # the keys at an odd address
        # alone, on a caller's stream
        e.set_profiling(4)
        e.answer_woodruff_deriv_queue_dev(d_k + 3, M, K, 0, N, d_r, stream=caller.stream)
        caller.sync()
        t = e.last_timings()
        assert t["fused"] == 11.0 and {"launch", "scan", "reduce", "total"} <= set(t), t
        assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
        assert t["scan"] <= t["total"]
        assert np.array_equal(e.d2h(d_r, K * rl).reshape(want.shape), want)
        # the queue on the caller's stream, then a tree answer on the engine's, no host sync:
        # each profiling slot is read with its own path
        e.answer_woodruff_deriv_queue_dev(d_k + 3, M, K, 0, N, d_r, stream=caller.stream)
        got_tree = e.answer(tree_key)
        caller.sync()
        t = e.last_timings()
        assert t["fused"] == (11.0 + tree_path) / 2, t
        assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
        assert np.array_equal(got_tree, want_tree)
        assert np.array_equal(e.d2h(d_r, K * rl).reshape(want.shape), want)
        e.set_profiling(0)


@gpu
@pytest.mark.parametrize("share", [2, 0, None])
def test_reserved_queue_allocates_nothing(pir, monkeypatch, share):
    n, efs, K = 12, 256, 9
    N, M = 1 << n, wd_m(n)
    rl = (M + 1) * efs
    rows, keys, want = _case(n, efs, K)
    with _engine(pir, monkeypatch, n, efs, share) as e:
        e.set_shard(rows)
        d_k, d_r = e.alloc_dev(K * M), e.alloc_dev(K * rl)
        e.h2d(d_k, keys.reshape(-1))
        e.reserve_woodruff_deriv_queue(K)
        free0 = _free_device_bytes()
        e.answer_woodruff_deriv_queue_dev(d_k, M, K, 0, N, d_r)
        e.sync()
        got = e.answer_woodruff_deriv_queue(keys)
        free1 = _free_device_bytes()
        print("share", share, "free before", free0, "after", free1)
        assert free1 >= free0, (share, free0, free1)
        assert np.array_equal(e.d2h(d_r, K * rl).reshape(want.shape), want)
        assert np.array_equal(got, want)


@gpu
def test_stale_state(pir, monkeypatch):
    """Two different shards and key sets back to back on one engine; a range call, a single
    derivative answer, a Woodruff value queue and a tree queue between the queues."""
    n, efs, K = 12, 256, 9
    tree_keys = [pir.gen_keys(n, 100 + 37 * i, 2, 1)[0] for i in range(10)]
    with _engine(pir, monkeypatch, n, efs) as e:
        for rows, keys, want in (_case(n, efs, K), _case(n, efs, K, seed=1)):
            e.set_shard(rows)
            assert np.array_equal(e.answer_woodruff_deriv_queue(keys), want)
            assert np.array_equal(e.answer_woodruff_deriv_queue(keys[:3], 100, 1700),
                                  _ref(rows, keys[:3], 100, 1800))
            assert np.array_equal(e.answer_woodruff_deriv_queue(keys[::-1]), want[::-1])
            assert np.array_equal(e.answer_woodruff_deriv(keys[4]), want[4])
            assert np.array_equal(e.answer_woodruff_deriv_queue(keys), want)
            values = e.answer_woodruff_queue(keys)
            assert np.array_equal(values, want[:, 0])
            assert np.array_equal(e.answer_woodruff_deriv_queue(keys[1:]), want[1:])
            e.answer_stream(tree_keys)
            assert np.array_equal(e.answer_woodruff_deriv_queue(keys), want)


@gpu
def test_refusals(pir, monkeypatch):
    n, efs = 8, 256
    N, M = 1 << n, wd_m(n)
    rl = (M + 1) * efs
    keys = np.ones((3, M), np.uint8)
    with _engine(pir, monkeypatch, n, efs) as e:
        with pytest.raises(pir.PirError, match="M = %d" % M):
            e.answer_woodruff_deriv_queue(keys[:, :-1])
        d_k, d_r = e.alloc_dev(3 * (M + 1)), e.alloc_dev(3 * rl)
        with pytest.raises(pir.PirError, match="M = %d" % M):
            e.answer_woodruff_deriv_queue_dev(d_k, M + 1, 3, 0, N, d_r)
        with pytest.raises(pir.PirError, match="-1 keys"):
            e.answer_woodruff_deriv_queue_dev(d_k, M, -1, 0, N, d_r)
        with pytest.raises(pir.PirError, match="null"):
            e.answer_woodruff_deriv_queue_dev(None, M, 3, 0, N, d_r)
        with pytest.raises(pir.PirError, match="null"):
            e.answer_woodruff_deriv_queue_dev(d_k, M, 3, 0, N, None)
        with pytest.raises(pir.PirError, match="beyond"):
            e.answer_woodruff_deriv_queue_dev(d_k, M, 3, N + 1, 0, d_r)
        with pytest.raises(pir.PirError, match="bad argument"):
            e.reserve_woodruff_deriv_queue(0)
        e.answer_woodruff_deriv_queue_dev(None, M, 0, 0, N, None)   # an empty queue touches nothing
        e.attach_comm(pir.comm_unique_id(), 1, 0)
        with pytest.raises(pir.PirError, match="communicator"):
            e.answer_woodruff_deriv_queue(keys)
        with pytest.raises(pir.PirError, match="communicator"):
            e.reserve_woodruff_deriv_queue(3)
    with _engine(pir, monkeypatch, n, efs, nq=2) as e:
        with pytest.raises(pir.PirError, match="one round"):
            e.answer_woodruff_deriv_queue(keys)
        with pytest.raises(pir.PirError, match="one round"):
            e.reserve_woodruff_deriv_queue(3)
    with _engine(pir, monkeypatch, n + 1, efs, log_num_partitions=1, partition_index=0) as e:
        with pytest.raises(pir.PirError, match="split shard"):
            e.answer_woodruff_deriv_queue(np.ones((3, wd_m(n + 1)), np.uint8))
        with pytest.raises(pir.PirError, match="split shard"):
            e.reserve_woodruff_deriv_queue(3)


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_goldens_queued(pir, case, monkeypatch):
    """The reference's rows and key, queued three times among random keys at different positions,
    against the reference's own derivative answer."""
    prm = case["params"]
    n, efs, M = prm["LOG_NUM_ENCODED_FILES"], prm["ENCODED_FILE_SIZE_BYTES"], prm["WOODRUFF_M"]
    rows = _rows(case)
    key = _hex(case["key"], (M,))
    want = _hex(case["deriv"], (M + 1, efs))
    queue = np.random.default_rng(M).integers(0, 256, (10, M), dtype=np.uint8)
    at = (0, 4, 9)
    queue[list(at)] = key
    for share in (2, 0):
        with _engine(pir, monkeypatch, n, efs, share) as e:
            e.set_shard(rows)
            got = e.answer_woodruff_deriv_queue(queue)
            for i in at:
                assert np.array_equal(got[i], want), (share, i)
            assert np.array_equal(got, _singles(e, queue)), share
            assert np.array_equal(e.answer_woodruff_deriv(key), want)


@gpu
def test_row_addresses_past_32_bits(pir, monkeypatch):
    """n = 22 x 2 KiB: the rows take 2^33 bytes, both passes span them all, and a 32-bit row
    offset wraps.  No restatement at this size: a shared queue of 8 keys against the 8 single
    answers on the same engine."""
    n, efs, K = 22, 2048, 8
    N, M = 1 << n, wd_m(n)
    assert N * efs == 1 << 33 and M == 2897
    keys = np.random.default_rng(22).integers(0, 256, (K, M), dtype=np.uint8)
    with _engine(pir, monkeypatch, n, efs) as e:
        e.fill_shard_random(2222)
        got, path = _path(e, lambda: e.answer_woodruff_deriv_queue(keys))
        assert path == 11.0
        singles = _singles(e, keys)
        assert singles.any(axis=(1, 2)).all()
        assert np.array_equal(got, singles)
        # the last triangle rows alone: every record of the range lies past 2^32 bytes, and so
        # does every row base of the columns pass
        a = next(a for a in range(M) if wd_start(M, a) * efs >= 1 << 32)
        lo = wd_start(M, a) + 5
        assert int(wd_pairs(M, N)[0][-1]) > a + 100
        got = e.answer_woodruff_deriv_queue(keys[:3], lo, N - lo)
        part = _singles(e, keys[:3], lo, N - lo)
        assert part.any(axis=(1, 2)).all()
        assert np.array_equal(got, part)


@gpu
def test_default_policy(pir, monkeypatch):
    """No knob set: 2^20 x 1 KiB is a measured shape, so queues of two and more keys share
    passes; 2^12 x 256 B is not, so they do not.  The answers are the single answers."""
    for n, efs, want_path in ((20, 1024, 11.0), (12, 256, 7.0)):
        M = wd_m(n)
        keys = np.random.default_rng(n).integers(0, 256, (3, M), dtype=np.uint8)
        with _engine(pir, monkeypatch, n, efs, None) as e:
            e.fill_shard_random(2026)
            singles = _singles(e, keys)
            assert singles.any(axis=(1, 2)).all()
            for K in (1, 2, 3):
                got, path = _path(e, lambda: e.answer_woodruff_deriv_queue(keys[:K]))
                assert path == (want_path if K >= 2 else 7.0), (n, K, path)
                assert np.array_equal(got, singles[:K]), (n, K)
