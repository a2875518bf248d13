"""Queued queries that share shard passes (answer_stream with G keys per read of the shard,
$PIR_STREAM_SHARE / $PIR_STREAM_G): every answer of a shared queue must equal, byte for byte,
the answer of the unshared queue ($PIR_STREAM_SHARE=0: k_query, a pass per query), of the same
key alone, and (small shards) of the oracle -- over group boundaries and ragged tails, every
scan a group can take, stale engine state, caller streams, split shards, the communicator
path, the byzantine flag and the profiling slots.  The arithmetic is exact GF(2^8): no
tolerance anywhere."""
import numpy as np
import pytest

import _oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pir():
    import erasurecodedpir_amd as pir
    pir.load()
    return pir


def _knobs(mp, share, g=0):
    """The knobs are read when an engine is made: set them before."""
    if share is None:
        mp.delenv("PIR_STREAM_SHARE", raising=False)
    else:
        mp.setenv("PIR_STREAM_SHARE", str(share))
    if g:
        mp.setenv("PIR_STREAM_G", str(g))
    else:
        mp.delenv("PIR_STREAM_G", raising=False)


def _keys(p, n, nq, nk, rng, party):
    fcw = O.final_cw(p, nq, 1)
    idxs = rng.choice(1 << n, nk, replace=False)
    return [bytes(O.gen_keys(n, int(i), fcw, p, nq,
                             rng.integers(0, 256, 16 * p, dtype=np.uint8).tobytes())[party])
            for i in idxs]


def _default_g(nq):  # the group size of $PIR_STREAM_SHARE=2 without $PIR_STREAM_G
    nrp = 1 if nq == 1 else 2 if nq == 2 else 4 if nq <= 4 else 8
    return max(2, 8 // nrp)


def _same(a, b):
    return np.array_equal(np.asarray(a).reshape(-1), np.asarray(b).reshape(-1))


def _check_oracle(shape, party, keys, shard, got):
    p, n, efs, nq = shape
    for k, key in enumerate(keys):
        assert _same(got[k], O.answer(p, party + 1, n, efs, nq, key, shard)), k


# ------------------------------------------------------------------------- group boundaries
@pytest.mark.parametrize("g", [0, 2, 4], ids=lambda g: "g%d" % g)
def test_group_boundaries(pir, monkeypatch, g):
    """nk = 0, 1, 2, G - 1, G, G + 1, 2G + 3 (three groups or more: share buffer j & 1 reused, and
    a ragged tail), one queue after another on the same engine."""
    shape = p, n, efs, nq = 2, 11, 1024, 1
    G = g or _default_g(nq)
    rng = np.random.default_rng(100 + g)
    shard = rng.integers(0, 256, (1 << n) * efs, dtype=np.uint8)
    keys = _keys(p, n, nq, 2 * G + 3, rng, 0)
    want = np.stack([O.answer(p, 1, n, efs, nq, k, shard).reshape(nq, efs) for k in keys])
    lens = sorted({0, 1, 2, G - 1, G, G + 1, 2 * G + 3})
    got = {}
    for share in (2, 0):
        _knobs(monkeypatch, share, g)
        with pir.Engine(p, 1, n, efs, nq) as e:
            e.set_shard(shard)
            got[share] = [e.answer_stream(keys[:nk]) for nk in lens]
            singles = np.stack([e.answer(k) for k in keys])
    assert _same(singles, want)
    for nk, a, b in zip(lens, got[2], got[0]):
        assert a.shape == (nk, nq, efs) and b.shape == (nk, nq, efs)
        assert _same(a, want[:nk]), nk
        assert _same(b, want[:nk]), nk


# ----------------------------------------------------------------------------- record widths
WIDTH_SHAPES = [  # (p, n, efs, nq): every scan a group can take
    (2, 11, 1024, 1),  # k_scan_t, four column groups
    (2, 11, 1056, 1),  # pitch padding
    (2, 12, 256, 1),
    (2, 10, 2048, 1),
    (2, 12, 96, 1),    # several records per wave row
    (3, 11, 1024, 2),  # two rounds: nrp = 2
    (8, 10, 1024, 5),  # five rounds: nrp = 8, two keys per pass
]


@pytest.mark.parametrize("shape", WIDTH_SHAPES, ids=lambda s: "p%d_n%d_efs%d_nq%d" % s)
def test_record_widths(pir, monkeypatch, shape):
    p, n, efs, nq = shape
    nk = 2 * _default_g(nq) + 3
    rng = np.random.default_rng(sum(shape))
    party = p - 1
    shard = rng.integers(0, 256, (1 << n) * efs, dtype=np.uint8)
    keys = _keys(p, n, nq, nk, rng, party)
    got = {}
    for share in (2, 0):
        _knobs(monkeypatch, share)
        with pir.Engine(p, party + 1, n, efs, nq) as e:
            e.set_shard(shard)
            got[share] = e.answer_stream(keys)
            singles = np.stack([e.answer(k) for k in keys])
    assert _same(got[2], got[0])
    assert _same(got[2], singles)
    _check_oracle(shape, party, keys, shard, got[2])


# -------------------------------------------------------------------------------- stale state
def test_stale_state(pir, monkeypatch):
    """A long shared queue then a shorter one with other keys; a lone answer right after a shared
    queue and a shared queue right after a lone answer (the slabs are shared); set_party between
    two queues."""
    shape = p, n, efs, nq = 2, 12, 1024, 1
    rng = np.random.default_rng(7)
    shard = rng.integers(0, 256, (1 << n) * efs, dtype=np.uint8)
    k1 = _keys(p, n, nq, 19, rng, 0)
    k1b = _keys(p, n, nq, 5, rng, 0)
    k2 = _keys(p, n, nq, 6, rng, 1)
    _knobs(monkeypatch, 2)
    with pir.Engine(p, 1, n, efs, nq) as e:
        e.set_shard(shard)
        long_q = e.answer_stream(k1)
        short_q = e.answer_stream(k1b)
        lone = e.answer(k1[3])
        again = e.answer_stream(k1b[:3])
        e.set_party(2)
        other = e.answer_stream(k2)
        e.set_party(1)
        back = e.answer_stream(k1[:9])
    _check_oracle(shape, 0, k1, shard, long_q)
    _check_oracle(shape, 0, k1b, shard, short_q)
    assert _same(lone, long_q[3])
    assert _same(again, short_q[:3])
    _check_oracle(shape, 1, k2, shard, other)
    assert _same(back, long_q[:9])


# ------------------------------------------------------------------------------------ streams
def test_caller_stream_then_engine_stream(pir, monkeypatch):
    """A shared queue on a caller's stream, then an answer on the engine's stream with no host
    synchronisation between them (the work buffers are ordered across the aux-stream join).  The
    caller's stream is another engine's."""
    shape = p, n, efs, nq = 2, 14, 1024, 1
    rng = np.random.default_rng(21)
    shard = rng.integers(0, 256, (1 << n) * efs, dtype=np.uint8)
    keys = _keys(p, n, nq, 11, rng, 0)
    _knobs(monkeypatch, 2)
    with pir.Engine(p, 1, n, efs, nq) as e, pir.Engine(2, 1, 6, 16, 1) as caller:
        e.set_shard(shard)
        st = caller.stream
        kl, ab = e.key_len, e.answer_bytes
        d_k, d_r, d_r1 = e.alloc_dev(kl * len(keys)), e.alloc_dev(ab * len(keys)), e.alloc_dev(ab)
        e.h2d(d_k, b"".join(keys))
        e.answer_stream_dev(d_k, len(keys), d_r, stream=st)
        e.answer_dev(d_k + 4 * kl, d_r1)
        e.answer_stream_dev(d_k, 5, d_r, stream=st)  # the same answers again
        caller.sync()
        e.sync()
        queue = e.d2h(d_r, ab * len(keys)).reshape(len(keys), nq, efs)
        lone = e.d2h(d_r1, ab)
        for d in (d_k, d_r, d_r1):
            e.free_dev(d)
    _check_oracle(shape, 0, keys, shard, queue)
    assert _same(lone, queue[4])


# ------------------------------------------------------------- split shard and communicator
def test_partitions_xor_to_full(pir, monkeypatch):
    p, n, efs, nq, nk = 2, 13, 512, 1, 11
    rng = np.random.default_rng(33)
    shard = rng.integers(0, 256, ((1 << n), efs), dtype=np.uint8)
    keys = _keys(p, n, nq, nk, rng, 0)
    _knobs(monkeypatch, 2)
    acc = np.zeros((nk, nq, efs), np.uint8)
    rows = (1 << n) >> 2
    for part in range(4):
        with pir.Engine(p, 1, n, efs, nq, log_num_partitions=2, partition_index=part) as e:
            e.set_shard(shard[part * rows:(part + 1) * rows])
            acc ^= e.answer_stream(keys)
    _check_oracle((p, n, efs, nq), 0, keys, shard.reshape(-1), acc)


def test_comm_single_rank(pir, monkeypatch):
    """The 1-rank communicator path (batch partition buffer, all-gather, XOR fold) equals the
    no-communicator answers."""
    shape = p, n, efs, nq = 2, 12, 1024, 1
    rng = np.random.default_rng(44)
    shard = rng.integers(0, 256, (1 << n) * efs, dtype=np.uint8)
    keys = _keys(p, n, nq, 11, rng, 0)
    _knobs(monkeypatch, 2)
    with pir.Engine(p, 1, n, efs, nq) as e:
        e.set_shard(shard)
        e.attach_comm(pir.comm_unique_id(), 1, 0)
        e.reserve_queue(len(keys))
        with_comm = e.answer_stream(keys)
        e.detach_comm()
        without = e.answer_stream(keys)
    assert _same(with_comm, without)
    _check_oracle(shape, 0, keys, shard, with_comm)


def test_byzantine(pir, monkeypatch):
    p, n, efs, nq = 2, 10, 64, 1
    keys = [pir.gen_keys(n, 3, p, nq)[0]] * 5
    _knobs(monkeypatch, 2)
    with pir.Engine(p, 1, n, efs, nq, is_byzantine=True) as e:
        a = e.answer_stream(keys)
    assert a.shape == (5, nq, efs)


# ------------------------------------------------- a shape both k_query and the groups take
def test_query_sized_shape_all_policies(pir, monkeypatch):
    """p = 2, n = 19, 1 KiB, 11 keys: the default policy, never (=0) and always (=2) against the
    single answers; a queue of one stays on k_query (fused == 2.0) under every setting."""
    p, n, efs, nq, nk = 2, 19, 1024, 1, 11
    rng = np.random.default_rng(55)
    keys = _keys(p, n, nq, nk, rng, 0)
    got = {}
    for share in (None, 0, 2):
        _knobs(monkeypatch, share)
        with pir.Engine(p, 1, n, efs, nq) as e:
            e.fill_shard_random(1234)
            e.reserve_queue(nk)
            got[share] = e.answer_stream(keys)
            if share == 0:
                singles = np.stack([e.answer(k) for k in keys])
            e.set_profiling(2)
            one = e.answer_stream(keys[:1])
            assert e.last_timings()["fused"] == 2.0
            assert _same(one, got[share][:1])
    for share in (None, 0, 2):
        assert _same(got[share], singles), share


# ---------------------------------------------------------------------------------- profiling
def test_profiling_slots(pir, monkeypatch):
    p, n, efs, nq = 2, 19, 1024, 1
    rng = np.random.default_rng(66)
    keys = _keys(p, n, nq, 9, rng, 0)
    _knobs(monkeypatch, 2)
    with pir.Engine(p, 1, n, efs, nq) as e:
        e.fill_shard_random(99)
        e.set_profiling(2)
        want = e.answer_stream(keys)
        t = e.last_timings()
        assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
        assert t["scan"] <= t["total"] and t["fused"] == 0.0
        assert {"scan", "reduce", "comm_fold", "total"} <= set(t)
        # a lone k_query answer and a shared queue in one window: each slot read with its own
        # layout (the queue's slot holds no leaf / scan chunk events)
        lone = e.answer(keys[2])
        again = e.answer_stream(keys)
        t = e.last_timings()
        assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
        assert t["scan"] <= t["total"] and t["fused"] == 1.0  # the mean of 2.0 and 0.0
        # and the other order, the lone answer the newest
        e.answer_stream(keys[:3])
        e.answer(keys[2])
        t = e.last_timings()
        assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
        assert e.last_timings() == {}
    assert _same(lone, want[2]) and _same(again, want)


# ------------------------------------------------- k_query's queue keeps its own coverage
# Shapes of the existing k_query queue tests (test_stream_equals_single_answers' STREAM_SHAPES,
# test_fused_reduce_equals_k_reduce, test_query_m4r_equals_plane_masks, the steal test) that the
# default policy routes to the shared path: their queues on k_query ($PIR_STREAM_SHARE=0)
# against the single answers.
UNSHARED_SHAPES = [  # (p, n, efs, nq, queued keys)
    (2, 20, 1024, 1, 4),  # test_stream_full_size_pir_property's queue
]


@pytest.mark.parametrize("shape", UNSHARED_SHAPES, ids=lambda s: "p%d_n%d_efs%d_nq%d_k%d" % s)
def test_unshared_queue_equals_singles(pir, monkeypatch, shape):
    p, n, efs, nq, nk = shape
    rng = np.random.default_rng(sum(shape) * 17)
    keys = _keys(p, n, nq, nk, rng, 0)
    _knobs(monkeypatch, 0)
    with pir.Engine(p, 1, n, efs, nq) as e:
        e.fill_shard_random(4242)
        e.set_profiling(1)
        got = e.answer_stream(keys)
        assert e.last_timings()["fused"] == 2.0
        e.set_profiling(0)
        singles = np.stack([e.answer(k) for k in keys])
    assert _same(got, singles)
