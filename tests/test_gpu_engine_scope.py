"""Buffer regrow and workspace ordering across streams, together: on one engine, with no host
synchronisation between the calls, a queue of 2 keys on one caller's stream, a queue of 9 keys
(more than one group: the staging, share and key buffers grow) on a second caller's stream, a
reserve for 32 keys, and the first 2 keys again on the engine's own stream; then the first step
once more on a re-created engine.  Every answer must equal the oracle's (the neighbouring
modules' references, computed once there), and the repeated answers the first ones bit for bit.
Once for the DPF-tree queue (shared passes, and k_query / single answers), once for the Woodruff
queue, once for the multiparty queue from a key pointer 8 bytes off a 16-byte boundary (the
d_mpkey staging copy on the caller's stream).  Exact GF(2^8): no tolerance."""
import numpy as np
import pytest

import _oracle as O
from test_gpu_group_queue import Mode
from test_gpu_stream_shared import _keys, _knobs
from test_gpu_woodruff_queue import _case, _engine as _wd_engine

pytestmark = pytest.mark.gpu

SMALL, LARGE, RESERVE = 2, 9, 32


@pytest.fixture(scope="module")
def pir():
    import erasurecodedpir_amd as pir
    pir.load()
    return pir


def _run(pir, make, keys, key_off, stride, out, call, reserve):
    """The sequence above.  make(): a loaded engine; keys: LARGE host keys (rows of a uint8
    array), laid out `stride` apart from `key_off` in a device buffer; call(e, d_keys, nk, d_res,
    stream) enqueues a queue; out: bytes per answer.  Returns the four answers."""
    host = np.zeros(key_off + LARGE * stride, np.uint8)
    for k, key in enumerate(keys):
        host[key_off + k * stride:key_off + k * stride + len(key)] = np.frombuffer(bytes(key), np.uint8)
    got = []
    with pir.Engine(2, 1, 6, 16, 1) as a, pir.Engine(2, 1, 6, 16, 1) as b:
        for streams in ((a.stream, b.stream, None), (a.stream,)):
            with make() as e:
                d_k = e.alloc_dev(host.size)
                d_r = [e.alloc_dev(LARGE * out) for _ in streams]
                e.h2d(d_k, host)
                for i, (st, nk) in enumerate(zip(streams, (SMALL, LARGE, SMALL))):
                    if i == 2:
                        reserve(e, RESERVE)
                    call(e, d_k + key_off, nk, d_r[i], st)
                a.sync()
                b.sync()
                e.sync()
                for d, nk in zip(d_r, (SMALL, LARGE, SMALL)):
                    got.append(e.d2h(d, nk * out).copy())
                    e.free_dev(d)
                e.free_dev(d_k)
    return got


def _check(got, want):
    """want: the LARGE reference answers"""
    first, large, again, recreated = [g.reshape(-1) for g in got]
    want = np.asarray(want).reshape(LARGE, -1)
    assert np.array_equal(large, want.reshape(-1))
    assert np.array_equal(first, want[:SMALL].reshape(-1))
    assert np.array_equal(again, first)
    assert np.array_equal(recreated, first)


_TREE = {}


def _tree_case(p, n, efs, nq):
    """shard, keys and the oracle's answers: computed once, shared, never changed"""
    if not _TREE:
        rng = np.random.default_rng(812)
        shard = rng.integers(0, 256, (1 << n) * efs, dtype=np.uint8)
        keys = _keys(p, n, nq, LARGE, rng, 0)
        want = np.stack([O.answer(p, 1, n, efs, nq, k, shard) for k in keys])
        shard.setflags(write=False)
        want.setflags(write=False)
        _TREE["case"] = (shard, keys, want)
    return _TREE["case"]


@pytest.mark.parametrize("share", [2, 0], ids=["shared", "unshared"])
def test_tree_queue(pir, monkeypatch, share):
    p, n, efs, nq = 2, 12, 256, 1
    shard, keys, want = _tree_case(p, n, efs, nq)
    _knobs(monkeypatch, share)

    def make():
        e = pir.Engine(p, 1, n, efs, nq)
        e.set_shard(shard)
        return e

    got = _run(pir, make, keys, 0, len(keys[0]), nq * efs,
               lambda e, d_k, nk, d_r, st: e.answer_stream_dev(d_k, nk, d_r, stream=st),
               lambda e, nk: e.reserve_queue(nk))
    _check(got, want)


def test_woodruff_queue(pir, monkeypatch):
    n, efs = 12, 256
    rows, keys, want = _case(n, efs, 19)
    M = keys.shape[1]

    def make():
        e = _wd_engine(pir, monkeypatch, n, efs)
        e.set_shard(rows)
        return e

    got = _run(pir, make, keys[:LARGE], 0, M, efs,
               lambda e, d_k, nk, d_r, st: e.answer_woodruff_queue_dev(d_k, M, nk, 0, 1 << n, d_r,
                                                                       stream=st),
               lambda e, nk: e.reserve_woodruff_queue(nk))
    _check(got, want[:LARGE])


def test_multiparty_queue_misaligned_keys(pir, monkeypatch):
    m = Mode.get("mp", 12, 256, (3, 1), 11)
    ksz = m.keys.shape[1]
    stride = (ksz + 15) // 16 * 16  # a multiple of 16: the pointer alone sends the keys to staging
    got = _run(pir, lambda: m.engine(pir, monkeypatch), m.keys[:LARGE], 8, stride, m.nr * m.efs,
               lambda e, d_k, nk, d_r, st: m.queue_dev(e, d_k, stride, nk, d_r, stream=st),
               lambda e, nk: e.reserve_group_queue(nk))
    _check(got, m.wants(LARGE))
