"""Queued explicit-coefficient (Hollanti), multiparty and covering-design queries
(pir_engine_answer_{coefs,mp,cd}_queue[_dev]): K keys, G = 8 / nrp key slots per read of the
shard.  One kernel writes a group's W-byte share rows (k_interleave_coefs_g from the vectors,
k_mp_shares_g from the sqrt(N) keys), one W-round scan answers the group.

Every queue answer must equal, byte for byte, the single answer of the same key and range, the
unshared queue ($PIR_GQ_SHARE=0) and the oracle (O.scan, O.mp_answer, O.cd_answer).  The
arithmetic is exact: no tolerance anywhere.  The knobs are read at engine creation, so they are
set before it.  A single explicit-coefficient or sqrt(N) answer records no profiling slot, so its
"path" reads as None; a shared queue's is 9."""
import ctypes
import os

import numpy as np
import pytest

import _oracle as O

gpu = pytest.mark.gpu
NAMES = ["pir_engine_answer_coefs_queue_dev", "pir_engine_answer_coefs_queue",
         "pir_engine_answer_mp_queue_dev", "pir_engine_answer_mp_queue",
         "pir_engine_answer_cd_queue_dev", "pir_engine_answer_cd_queue",
         "pir_engine_reserve_group_queue"]
METHODS = ["answer_coefs_queue_dev", "answer_coefs_queue", "answer_mp_queue_dev",
           "answer_mp_queue", "answer_cd_queue_dev", "answer_cd_queue", "reserve_group_queue"]


# -------------------------------------------------------------------------------- CPU test
def test_names_and_loud_errors():
    import erasurecodedpir_amd as pir
    from erasurecodedpir_amd import _lib
    with open(os.path.join(O.ROOT, "include", "pir_engine.h")) as f:
        header = f.read()
    for name in NAMES:
        assert "int %s(pir_engine_t *e" % name in header, name
        assert name in _lib.PROTOTYPES, name
    for m in METHODS:
        assert callable(getattr(pir.Engine, m)), m
    # no engine: every call refuses, none answers
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    ptrs = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    calls = [lambda: lib.pir_engine_answer_coefs_queue_dev(None, buf, 16, 16, 1, 0, 1, buf, None),
             lambda: lib.pir_engine_answer_coefs_queue(None, ptrs, 1, 0, 1, buf),
             lambda: lib.pir_engine_answer_mp_queue_dev(None, buf, 64, 1, 3, 1, 0, 1, buf, None),
             lambda: lib.pir_engine_answer_mp_queue(None, buf, 64, 1, 3, 1, 0, 1, buf),
             lambda: lib.pir_engine_answer_cd_queue_dev(None, buf, 64, 1, 6, 3, 0, 1, buf, None),
             lambda: lib.pir_engine_answer_cd_queue(None, buf, 64, 1, 6, 3, 0, 1, buf),
             lambda: lib.pir_engine_reserve_group_queue(None, 4)]
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


def _engine(pir, monkeypatch, n, efs, nr, share=2, G=None, **kw):
    for name, v in (("PIR_GQ_SHARE", share), ("PIR_GQ_G", G)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    return pir.Engine(2, 1, n, efs, nr, **kw)


def _path(e, fn):
    """fn's answer and the path code of the profiling slot it recorded (None: no slot)"""
    e.set_profiling(1)
    got = fn()
    t = e.last_timings()
    e.set_profiling(0)
    if t:
        if t["fused"] == 9.0:
            assert {"launch", "scan", "reduce", "total"} <= set(t), t
        assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
    return got, t.get("fused")


class Mode:
    """One mode's keys, calls and oracle over a shape: computed once, shared, never changed."""
    _cache = {}

    def __init__(self, kind, n, efs, par, nkeys):
        self.kind, self.n, self.efs, self.par, self.N = kind, n, efs, par, 1 << n
        seed = 1000 * n + efs + 7 * sum(par)
        self.shard = O.xorshift(seed, self.N * efs)
        if kind == "coefs":
            (self.nr,) = par
            self.keys = np.random.default_rng(seed).integers(
                0, 256, (nkeys, self.nr, self.N), dtype=np.uint8)
        elif kind == "mp":
            p, t = par
            self.nr = O.mp_sizes(p, n, t)["nrk"]
            self.keys = np.stack([O.mp_key(p, n, t, seed + 31 * k) for k in range(nkeys)])
        else:
            q, nck = par
            self.nr = nck
            self.keys = np.stack([O.cd_key(n, q, nck, seed + 31 * k) for k in range(nkeys)])
        for a in (self.shard, self.keys):
            a.setflags(write=False)
        self._want = {}

    @classmethod
    def get(cls, kind, n, efs, par, nkeys):
        k = (kind, n, efs, tuple(par), nkeys)
        if k not in cls._cache:
            cls._cache[k] = cls(*k)
        return cls._cache[k]

    @property
    def slots(self):
        nrp = 1
        while nrp < self.nr:
            nrp *= 2
        return 8 // nrp if nrp <= 4 else 1

    def want(self, k, th=0, T=1):
        """the oracle's answer of key k (sqrt(N) modes: thread slice th of T)"""
        if (k, th, T) not in self._want:
            key = self.keys[k]
            if self.kind == "coefs":
                w = O.scan(key, self.shard, self.efs)
            elif self.kind == "mp":
                w = O.mp_answer(self.par[0], self.par[1], self.n, self.efs, key, self.shard, th, T)
            else:
                w = O.cd_answer(self.n, self.par[0], self.par[1], self.efs, key, self.shard, th, T)
            self._want[(k, th, T)] = w
        return self._want[(k, th, T)]

    def wants(self, K, th=0, T=1):
        return np.stack([self.want(k, th, T) for k in range(K)]) if K else \
            np.zeros((0, self.nr, self.efs), np.uint8)

    def single(self, e, key, th=0, T=1):
        if self.kind == "coefs":
            return e.answer_coefs(key)
        if self.kind == "mp":
            return e.answer_mp(key, self.par[0], self.par[1], th, T)
        return e.answer_cd(key, self.par[0], self.par[1], th, T)

    def queue(self, e, keys, th=0, T=1):
        if self.kind == "coefs":
            return e.answer_coefs_queue(keys)
        if self.kind == "mp":
            return e.answer_mp_queue(keys, self.par[0], self.par[1], th, T)
        return e.answer_cd_queue(keys, self.par[0], self.par[1], th, T)

    def queue_dev(self, e, d_keys, stride, K, d_r, th=0, T=1, stream=None):
        if self.kind == "coefs":
            return e.answer_coefs_queue_dev(d_keys, self.N, stride, K, 0, self.N, d_r, stream)
        if self.kind == "mp":
            return e.answer_mp_queue_dev(d_keys, stride, K, self.par[0], self.par[1], d_r, th, T,
                                         stream)
        return e.answer_cd_queue_dev(d_keys, stride, K, self.par[0], self.par[1], d_r, th, T,
                                     stream)

    def engine(self, pir, monkeypatch, share=2, G=None, **kw):
        e = _engine(pir, monkeypatch, self.n, self.efs, self.nr, share, G, **kw)
        if not kw:
            e.set_shard(self.shard)
        return e


BOUNDARY = [("coefs", 11, 1024, (1,), 8), ("mp", 12, 256, (3, 1), 4), ("cd", 12, 256, (6, 3), 2)]


@gpu
@pytest.mark.parametrize("kind,n,efs,par,G", BOUNDARY)
def test_group_boundaries(pir, monkeypatch, kind, n, efs, par, G):
    m = Mode.get(kind, n, efs, par, 2 * G + 3)
    assert m.slots == G
    with m.engine(pir, monkeypatch, 2) as es, m.engine(pir, monkeypatch, 0) as eu:
        singles = np.stack([m.single(es, key) for key in m.keys])
        assert np.array_equal(singles, m.wants(2 * G + 3))
        _, single_path = _path(es, lambda: m.single(es, m.keys[0]))
        for K in sorted({0, 1, 2, G - 1, G, G + 1, 2 * G + 3}):
            got, path = _path(es, lambda: m.queue(es, m.keys[:K]))
            ungot, unpath = _path(eu, lambda: m.queue(eu, list(m.keys[:K])))
            print(kind, "G", G, "K", K, "path", path, unpath)
            assert got.shape == (K, m.nr, efs)
            assert np.array_equal(got, singles[:K]), K
            assert np.array_equal(got, m.wants(K)), K
            assert np.array_equal(got, ungot), K
            assert path == (9.0 if K >= 2 else single_path), K
            assert unpath == single_path, K


SCANS = [("coefs", 12, 256, (2,)), ("coefs", 11, 1056, (3,)), ("coefs", 12, 96, (1,)),
         ("coefs", 9, 24, (1,)), ("coefs", 10, 2048, (1,)), ("coefs", 10, 1024, (5,)),
         ("mp", 10, 64, (3, 2)), ("mp", 12, 1056, (4, 1)), ("mp", 10, 32, (5, 1)),
         ("mp", 8, 16, (6, 1)), ("mp", 11, 48, (3, 1)), ("cd", 13, 40, (12, 8))]


@gpu
@pytest.mark.parametrize("kind,n,efs,par", SCANS)
def test_every_group_scan_and_slot_width(pir, monkeypatch, kind, n, efs, par):
    nr = {"coefs": lambda: par[0], "mp": lambda: O.mp_sizes(par[0], n, par[1])["nrk"],
          "cd": lambda: par[1]}[kind]()
    K = {1: 17, 2: 9, 3: 5, 4: 5}.get(nr, 3)   # 2 G + 1 keys; 3 where there is one slot
    m = Mode.get(kind, n, efs, par, K)
    assert K == (2 * m.slots + 1 if m.slots > 1 else 3)
    with m.engine(pir, monkeypatch) as e:
        got, path = _path(e, lambda: m.queue(e, m.keys))
        _, single_path = _path(e, lambda: m.single(e, m.keys[0]))
        assert path == (9.0 if m.slots > 1 else single_path), (m.slots, path)
        assert np.array_equal(got, m.wants(K))
        for k in (0, K - 1):
            assert np.array_equal(m.single(e, m.keys[k]), got[k]), k
    if m.slots >= 4:   # narrower share rows ($PIR_GQ_G): W = 2 and 4 bytes per record
        for G in (2, 4):
            if G < m.slots:
                with m.engine(pir, monkeypatch, 2, G) as e:
                    got, path = _path(e, lambda: m.queue(e, m.keys))
                    assert path == 9.0 and np.array_equal(got, m.wants(K)), G


@gpu
def test_cd_thread_slices_of_a_large_domain(pir, monkeypatch):
    m = Mode.get("cd", 18, 256, (6, 3), 3)
    T = 8
    with m.engine(pir, monkeypatch) as e:
        acc = np.zeros((3, m.nr, m.efs), np.uint8)
        for th in range(T):
            got, path = _path(e, lambda: m.queue(e, m.keys, th, T))
            assert path == 9.0
            if th in (0, 5):
                assert np.array_equal(got, m.wants(3, th, T)), th
            acc ^= got
        whole = m.queue(e, m.keys)
        assert np.array_equal(acc, whole)
        assert np.array_equal(whole[2], m.single(e, m.keys[2]))
        assert np.array_equal(whole[1], m.want(1))


@gpu
@pytest.mark.parametrize("kind,n,efs,par", [("mp", 4, 16, (3, 1)), ("mp", 3, 8, (3, 1)),
                                            ("cd", 6, 16, (4, 2)), ("cd", 4, 16, (6, 3))])
def test_short_rows(pir, monkeypatch, kind, n, efs, par):
    m = Mode.get(kind, n, efs, par, 5)
    z = O.mp_sizes(par[0], n, par[1]) if kind == "mp" else O.cd_sizes(n, par[0], par[1])
    print(kind, n, z)
    if (kind, n) == ("mp", 4):
        assert z["mu"] == 8
    if (kind, n) == ("mp", 3):
        assert z["nu"] == 1 and z["eval_bytes"] == 104
    if (kind, n) == ("cd", 6):
        assert z["nu"] == 1
    if (kind, n) == ("cd", 4):
        assert z["nu"] == 0
    with m.engine(pir, monkeypatch) as e:
        got = m.queue(e, m.keys)
        assert np.array_equal(got, m.wants(5))
        if z["nu"] == 0:
            assert not got.any()
        else:
            assert got.any(axis=(1, 2)).all()
        assert np.array_equal(got[3], m.single(e, m.keys[3]))
        # the keys back to back in device memory at eval_bytes apart (104: unaligned)
        eb, out = z["eval_bytes"], m.nr * efs
        d_k, d_r = e.alloc_dev(5 * eb), e.alloc_dev(5 * out)
        e.h2d(d_k, np.concatenate([key[:eb] for key in m.keys]))
        m.queue_dev(e, d_k, eb, 5, d_r)
        e.sync()
        assert np.array_equal(e.d2h(d_r, 5 * out).reshape(5, m.nr, efs), got)
        e.free_dev(d_k)
        e.free_dev(d_r)


@gpu
@pytest.mark.parametrize("par,G", [((3, 1), 2), ((3, 2), 2), ((3, 2), 4)])
def test_short_rows_in_narrow_share_rows(pir, monkeypatch, par, G):
    """rows of 8 records (one counter block, byte stores) at W = 4 and 2 bytes per record"""
    m = Mode.get("mp", 4, 16, par, 2 * G + 1)
    assert O.mp_sizes(par[0], 4, par[1])["mu"] == 8 and m.slots > G
    with m.engine(pir, monkeypatch, 2, G) as e:
        got, path = _path(e, lambda: m.queue(e, m.keys))
        assert path == 9.0
        assert np.array_equal(got, m.wants(2 * G + 1))
        assert np.array_equal(got[G], m.single(e, m.keys[G]))


@gpu
def test_hollanti_ranges(pir, monkeypatch):
    n, efs, K = 11, 1024, 5
    m = Mode.get("coefs", n, efs, (1,), 19)
    N = m.N
    with m.engine(pir, monkeypatch) as e:
        for lo, hi in [(N // 3, N - 7), (77, 78), (100, 100), (0, 17), (N - 33, N)]:
            got, path = _path(e, lambda: e.answer_coefs_queue(m.keys[:K], lo, hi - lo))
            assert path == (9.0 if hi > lo else None), (lo, hi, path)
            for k in range(K):
                assert np.array_equal(got[k], O.scan(m.keys[k], m.shard, efs, lo, hi)), (lo, hi, k)
                assert np.array_equal(got[k], e.answer_coefs(m.keys[k], lo, hi - lo)), (lo, hi, k)
            if hi == lo:
                assert not got.any()


@gpu
@pytest.mark.parametrize("T", [2, 4])
def test_thread_slices_xor_to_the_whole(pir, monkeypatch, T):
    for kind, n, efs, par, G in BOUNDARY[1:]:
        m = Mode.get(kind, n, efs, par, 2 * G + 3)
        K = m.slots + 1
        with m.engine(pir, monkeypatch) as e:
            acc = np.zeros((K, m.nr, efs), np.uint8)
            for th in range(T):
                got, path = _path(e, lambda: m.queue(e, m.keys[:K], th, T))
                assert path == 9.0
                assert np.array_equal(got, m.wants(K, th, T)), (kind, th)
                assert np.array_equal(got[K - 1], m.single(e, m.keys[K - 1], th, T))
                acc ^= got
            assert np.array_equal(acc, m.wants(K)), kind


@gpu
def test_partition_engine(pir, monkeypatch):
    for kind, n, efs, par, G in BOUNDARY:
        m = Mode.get(kind, n, efs, par, 2 * G + 3)
        K, half = G + 1, m.N // 2
        acc = np.zeros((K, m.nr, efs), np.uint8)
        for part in range(2):
            with m.engine(pir, monkeypatch, log_num_partitions=1, partition_index=part) as e:
                e.set_shard(m.shard[part * half * efs:(part + 1) * half * efs])
                keys = m.keys[:K, :, part * half:(part + 1) * half] if kind == "coefs" \
                    else m.keys[:K]
                got, path = _path(e, lambda: m.queue(e, keys))
                assert path == 9.0, (kind, part)
                assert np.array_equal(got[1], m.single(e, keys[1])), (kind, part)
                acc ^= got
        assert np.array_equal(acc, m.wants(K)), kind


@gpu
def test_slot_isolation(pir, monkeypatch):
    # every even key all zero, every odd key random: even results zero, odd ones their singles
    for kind, n, efs, par, G in BOUNDARY:
        m = Mode.get(kind, n, efs, par, 2 * G + 3)
        K = 2 * G + 1
        keys = m.keys[:K].copy()
        if kind == "coefs":
            keys[0::2] = 0
        else:
            z = O.mp_sizes(par[0], n, par[1]) if kind == "mp" else O.cd_sizes(n, par[0], par[1])
            lo = z["nu"] * 16 * z["p2"]
            keys[0::2, lo:lo + z["nrk"] * z["nu"] * z["p2"]] = 0
        with m.engine(pir, monkeypatch) as e:
            got = m.queue(e, keys)
            for k in range(K):
                if k % 2 == 0:
                    assert not got[k].any(), (kind, k)
                else:
                    assert got[k].any() and np.array_equal(got[k], m.want(k)), (kind, k)
    # one-hot vectors that pick a different record in each slot
    m = Mode.get("coefs", 11, 1024, (1,), 19)
    recs = [0, m.N - 1, 15, 16, 17, 1000, 77, 1031]
    keys = np.zeros((8, 1, m.N), np.uint8)
    for g, r in enumerate(recs):
        keys[g, 0, r] = 1
    rows = m.shard.reshape(m.N, m.efs)
    with m.engine(pir, monkeypatch) as e:
        got = e.answer_coefs_queue(keys)
        for g, r in enumerate(recs):
            assert np.array_equal(got[g, 0], rows[r]), (g, r)


@gpu
def test_device_forms(pir, monkeypatch):
    # Hollanti: vectors at d_coefs + 3, a key stride larger than the key's vectors
    m = Mode.get("coefs", 12, 256, (2,), 9)
    K, N, efs, out = 9, m.N, m.efs, 2 * m.efs
    stride = 2 * N + 48 + 5
    with m.engine(pir, monkeypatch) as e, pir.Engine(2, 1, 6, 16, 1) as caller:
        host = np.zeros(K * stride + 3, np.uint8)
        for k in range(K):
            host[3 + k * stride:3 + k * stride + 2 * N] = m.keys[k].reshape(-1)
        d_k, d_r = e.alloc_dev(host.size), e.alloc_dev(K * out)
        e.h2d(d_k, host)
        e.answer_coefs_queue_dev(d_k + 3, N, stride, K, 0, N, d_r)
        e.sync()
        assert np.array_equal(e.d2h(d_r, K * out).reshape(K, 2, efs), m.wants(K))
        e.answer_coefs_queue_dev(d_k + 3, N, stride, K, 100, N - 333, d_r)
        e.sync()
        got = e.d2h(d_r, K * out).reshape(K, 2, efs)
        for k in (0, 8):
            assert np.array_equal(got[k], O.scan(m.keys[k], m.shard, efs, 100, N - 233)), k
        # a queue on a caller's stream, then a single tree answer on the engine's, no host sync:
        # each profiling slot is read with its own path
        tree_key = pir.gen_keys(m.n, 1234, 2, 2)[0]
        want_tree, tree_path = _path(e, lambda: e.answer(tree_key))
        e.set_profiling(4)
        e.answer_coefs_queue_dev(d_k + 3, N, stride, K, 0, N, d_r, stream=caller.stream)
        single = e.answer(tree_key)
        caller.sync()
        t = e.last_timings()
        assert t["fused"] == (9.0 + tree_path) / 2, t
        assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
        assert np.array_equal(single, want_tree)
        assert np.array_equal(e.d2h(d_r, K * out).reshape(K, 2, efs), m.wants(K))
        e.set_profiling(0)
        e.free_dev(d_k)
        e.free_dev(d_r)
    # sqrt(N) keys at d_keys + 1, a stride larger than the key and no multiple of 16
    for kind, n, efs, par, G in BOUNDARY[1:]:
        m = Mode.get(kind, n, efs, par, 2 * G + 3)
        K, ksz, out = G + 1, m.keys.shape[1], m.nr * efs
        for stride in (ksz + 24, ksz + 48 - ksz % 16):
            with m.engine(pir, monkeypatch) as e:
                host = np.zeros(K * stride + 1, np.uint8)
                for k in range(K):
                    host[1 + k * stride:1 + k * stride + ksz] = m.keys[k]
                d_k, d_r = e.alloc_dev(host.size), e.alloc_dev(K * out)
                e.h2d(d_k, host)
                m.queue_dev(e, d_k + 1, stride, K, d_r)
                e.sync()
                assert np.array_equal(e.d2h(d_r, K * out).reshape(K, m.nr, efs), m.wants(K)), kind
                e.free_dev(d_k)
                e.free_dev(d_r)


@gpu
def test_stale_state(pir, monkeypatch):
    from test_woodruff import wd_m
    n, efs = 11, 1024
    m = Mode.get("coefs", n, efs, (1,), 19)
    wkeys = np.random.default_rng(5).integers(0, 256, (11, wd_m(n)), dtype=np.uint8)
    tree_keys = [pir.gen_keys(n, 100 + 37 * i, 2, 1)[0] for i in range(10)]
    steps = [lambda e: e.answer_stream(tree_keys),
             lambda e: e.answer_coefs_queue(m.keys[:11]),
             lambda e: e.answer_woodruff_queue(wkeys),
             lambda e: e.answer_coefs(m.keys[3]),
             lambda e: e.answer_coefs_queue(m.keys[11:14], 100, 1500),
             lambda e: e.answer_woodruff(wkeys[2]),
             lambda e: e.answer_coefs_queue(m.keys[:11])]

    def make():
        monkeypatch.setenv("PIR_WD_SHARE", "2")
        return m.engine(pir, monkeypatch)

    def fresh(step):
        with make() as f:
            return step(f)

    with make() as e:
        for i, step in enumerate(steps):
            assert np.array_equal(step(e), fresh(step)), i
        assert np.array_equal(steps[1](e), m.wants(11))
    # the sqrt(N) queues between single answers and another slice
    m = Mode.get("mp", 12, 256, (3, 1), 11)
    steps = [lambda e: m.queue(e, m.keys[:7]),
             lambda e: m.single(e, m.keys[2]),
             lambda e: m.queue(e, m.keys[4:9], 1, 4),
             lambda e: e.answer_coefs_queue(np.ones((3, 2, m.N), np.uint8)),
             lambda e: m.queue(e, m.keys[:7])]

    def fresh_mp(step):
        with m.engine(pir, monkeypatch) as f:
            return step(f)

    with m.engine(pir, monkeypatch) as e:
        for i, step in enumerate(steps):
            assert np.array_equal(step(e), fresh_mp(step)), i
        assert np.array_equal(steps[0](e), m.wants(7))


def _free_device_bytes():
    """hipMemGetInfo of the HIP runtime the engine library runs on, after a device sync (torch's
    bundled runtime is a second one in the process; the call goes to the engine's)."""
    with open("/proc/self/maps") as f:
        paths = [line.split()[-1] for line in f if "libamdhip64.so" in line]
    own = [p for p in paths if "/torch/" not in p] or paths
    hip = ctypes.CDLL(own[0])
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


@gpu
def test_reserved_queue_allocates_nothing(pir, monkeypatch):
    m = Mode.get("coefs", 11, 1024, (1,), 19)
    K, N, efs = 19, m.N, m.efs
    for share in (2, 0):
        with m.engine(pir, monkeypatch, share) as e:
            d_k, d_r = e.alloc_dev(K * N), e.alloc_dev(K * efs)
            e.h2d(d_k, m.keys.reshape(-1))
            e.answer_coefs_queue_dev(d_k, N, N, 2, 0, 1, d_r)   # a tiny queue: tiny buffers
            e.sync()
            e.reserve_group_queue(K)
            free0 = _free_device_bytes()
            e.answer_coefs_queue_dev(d_k, N, N, K, 0, N, d_r)
            e.sync()
            free1 = _free_device_bytes()
            print("share", share, "free before", free0, "after", free1)
            assert free1 >= free0, (share, free0, free1)
            assert np.array_equal(e.d2h(d_r, K * efs).reshape(K, 1, efs), m.wants(K))
    # unaligned sqrt(N) keys: the staging is reserved for the longest key seen so far
    m = Mode.get("mp", 12, 256, (3, 1), 11)
    K, ksz, out = 11, m.keys.shape[1], m.nr * m.efs
    with m.engine(pir, monkeypatch) as e:
        d_k, d_r = e.alloc_dev(K * ksz + 1), e.alloc_dev(K * out)
        e.h2d(d_k + 1, m.keys.reshape(-1))
        m.queue_dev(e, d_k + 1, ksz, 2, d_r, 0, 64)
        e.sync()
        e.reserve_group_queue(K)
        free0 = _free_device_bytes()
        m.queue_dev(e, d_k + 1, ksz, K, d_r)
        e.sync()
        free1 = _free_device_bytes()
        assert free1 >= free0, (free0, free1)
        assert np.array_equal(e.d2h(d_r, K * out).reshape(K, m.nr, m.efs), m.wants(K))


@gpu
def test_refusals(pir, monkeypatch):
    n, efs = 10, 64
    N = 1 << n
    key = O.mp_key(3, n, 1, 1)
    keys = [key] * 3
    with _engine(pir, monkeypatch, n, efs, 2) as e:
        with pytest.raises(pir.PirError, match="shares"):
            e.answer_mp_queue(keys, 4, 1)          # 3 shares, the engine has 2 rounds
        with pytest.raises(pir.PirError, match="shares"):
            e.answer_cd_queue(keys, 6, 3)
        with pytest.raises(pir.PirError, match="evaluation reads"):
            e.answer_mp_queue([key[:100]] * 3, 3, 1)
        with pytest.raises(pir.PirError, match="evaluation reads"):
            e.answer_cd_queue([key[:100]] * 3, 6, 2)
        with pytest.raises(pir.PirError, match="thread_num"):
            e.answer_mp_queue(keys, 3, 1, 4, 4)
        with pytest.raises(pir.PirError, match="thread_num"):
            e.answer_cd_queue(keys, 6, 2, 2, 2)
        coefs = np.ones((3, 2, N), np.uint8)
        with pytest.raises(pir.PirError, match="beyond"):
            e.answer_coefs_queue(coefs, 1, N)
        with pytest.raises(pir.PirError, match="beyond"):
            e.answer_coefs_queue(coefs, N + 1, 0)
        d_k, d_r = e.alloc_dev(3 * 2 * N), e.alloc_dev(3 * 2 * efs)
        with pytest.raises(pir.PirError, match="-1 keys"):
            e.answer_coefs_queue_dev(d_k, N, 2 * N, -1, 0, N, d_r)
        with pytest.raises(pir.PirError, match="-1 keys"):
            e.answer_mp_queue_dev(d_k, 2 * N, -1, 3, 1, d_r)
        with pytest.raises(pir.PirError, match="-1 keys"):
            e.answer_cd_queue_dev(d_k, 2 * N, -1, 6, 2, d_r)
        with pytest.raises(pir.PirError, match="null"):
            e.answer_coefs_queue_dev(None, N, 2 * N, 3, 0, N, d_r)
        with pytest.raises(pir.PirError, match="null"):
            e.answer_coefs_queue_dev(d_k, N, 2 * N, 3, 0, N, None)
        with pytest.raises(pir.PirError, match="null"):
            e.answer_mp_queue_dev(None, 2 * N, 3, 3, 1, d_r)
        with pytest.raises(pir.PirError, match="null"):
            e.answer_cd_queue_dev(d_k, 2 * N, 3, 6, 2, None)
        with pytest.raises(pir.PirError, match="coef_pitch"):
            e.answer_coefs_queue_dev(d_k, N - 1, 2 * N, 3, 0, N, d_r)
        with pytest.raises(pir.PirError, match="key_stride"):
            e.answer_coefs_queue_dev(d_k, N, N, 3, 0, N, d_r)
        with pytest.raises(pir.PirError, match="key_stride"):
            e.answer_mp_queue_dev(d_k, 64, 3, 3, 1, d_r)
        # an empty queue touches nothing
        e.answer_coefs_queue_dev(None, N, 2 * N, 0, 0, N, None)
        e.answer_mp_queue_dev(None, 0, 0, 3, 1, None)
        e.answer_cd_queue_dev(None, 0, 0, 6, 2, None)
        with pytest.raises(pir.PirError, match="bad argument"):
            e.reserve_group_queue(0)
    # with a communicator (1 rank) the queue runs the single answers, each with its own exchange
    m = Mode.get("mp", 12, 256, (3, 1), 11)
    c = Mode.get("coefs", 12, 256, (2,), 9)
    with m.engine(pir, monkeypatch) as e:
        e.attach_comm(pir.comm_unique_id(), 1, 0)
        got, path = _path(e, lambda: m.queue(e, m.keys[:5]))
        assert path is None
        assert np.array_equal(got, m.wants(5))
        assert np.array_equal(got[4], m.single(e, m.keys[4]))
        got, path = _path(e, lambda: e.answer_coefs_queue(c.keys[:3]))
        assert path is None
        for k in range(3):
            assert np.array_equal(got[k], O.scan(c.keys[k], m.shard, m.efs)), k


@gpu
def test_default_policy_at_a_measured_shape(pir, monkeypatch):
    """No knob set, 2^20 x 1 KiB, one-round vectors: queues of 4 keys and more share passes (the
    measured policy), shorter ones do not; the answers are the single answers either way."""
    n, efs = 20, 1024
    keys = np.random.default_rng(20).integers(0, 256, (5, 1, 1 << n), dtype=np.uint8)
    with _engine(pir, monkeypatch, n, efs, 1, None) as e:
        e.fill_shard_random(2024)
        singles = np.stack([e.answer_coefs(key) for key in keys])
        _, single_path = _path(e, lambda: e.answer_coefs(keys[0]))
        assert singles.any(axis=(1, 2)).all()
        for K, want_path in ((3, single_path), (4, 9.0), (5, 9.0)):
            got, path = _path(e, lambda: e.answer_coefs_queue(keys[:K]))
            assert path == want_path, (K, path)
            assert np.array_equal(got, singles[:K]), K
