"""The fold image ($PIR_FOLD_IMAGE, include/pir_engine.h): a bit-transposed second copy of the
shard that the shared-queue scan (k_scan_t) reads in place of the rows.  Every answer with the
image must equal, byte for byte, the answer without it, the single answers and (small shards) the
oracle; a write to the shard drops the image and it comes back only by the rule; an image that
does not fit is left out (mode 1) or refused (mode 2); the group queues use it on block
boundaries only; partitions have images of their own.  Exact GF(2^8) arithmetic: no tolerance."""
import numpy as np
import pytest

import _oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pir():
    import erasurecodedpir_amd as pir
    pir.load()
    return pir


def _knobs(mp, image, share=2, max_bytes=None, gq=None):
    """The knobs are read when an engine is made: set them before."""
    mp.setenv("PIR_STREAM_SHARE", str(share))
    mp.delenv("PIR_STREAM_G", raising=False)
    mp.setenv("PIR_FOLD_IMAGE", str(image))
    if max_bytes is None:
        mp.delenv("PIR_FOLD_IMAGE_MAX_BYTES", raising=False)
    else:
        mp.setenv("PIR_FOLD_IMAGE_MAX_BYTES", str(max_bytes))
    if gq is None:
        mp.delenv("PIR_GQ_SHARE", raising=False)
    else:
        mp.setenv("PIR_GQ_SHARE", str(gq))


def _keys(p, n, nq, nk, rng, party):
    fcw = O.final_cw(p, nq, 1)
    idxs = rng.choice(1 << n, nk, replace=False)
    return [bytes(O.gen_keys(n, int(i), fcw, p, nq,
                             rng.integers(0, 256, 16 * p, dtype=np.uint8).tobytes())[party])
            for i in idxs]


def _same(a, b):
    return np.array_equal(np.asarray(a).reshape(-1), np.asarray(b).reshape(-1))


def _image_bytes(e):
    pitch = (e.record_bytes + 15) // 16 * 16
    return (e.num_rows + 3) // 4 * 4 * pitch


# ------------------------------------------------------------------------------------ answers
SHAPES = [  # (p, n, efs, nq): workgroups of fewer than 64 rows, ragged chunks
    (2, 11, 1024, 1),
    (2, 11, 1056, 1),  # padded pitch, a partial last column group
    (2, 12, 256, 1),
    (2, 10, 2048, 1),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "p%d_n%d_efs%d_nq%d" % s)
def test_answers(pir, monkeypatch, shape):
    p, n, efs, nq = shape
    G = 8
    nk = 2 * G + 3
    rng = np.random.default_rng(sum(shape) + 1)
    shard = rng.integers(0, 256, (1 << n) * efs, dtype=np.uint8)
    keys = _keys(p, n, nq, nk, rng, 1)
    got = {}
    for image in (2, 0):
        _knobs(monkeypatch, image)
        with pir.Engine(p, 2, n, efs, nq) as e:
            e.set_shard(shard)
            e.reserve_queue(nk)
            assert e.fold_image() == (_image_bytes(e) if image else 0)
            got[image] = e.answer_stream(keys)
            singles = np.stack([e.answer(k) for k in keys])
    assert _same(got[2], got[0])
    assert _same(got[2], singles)
    for k, key in enumerate(keys):
        assert _same(got[2][k], O.answer(p, 2, n, efs, nq, key, shard)), k


# ---------------------------------------------------------------------------------- staleness
MUTATORS = {
    "set_shard": lambda e, rng: e.set_shard(
        rng.integers(0, 256, (e.num_rows, e.record_bytes), dtype=np.uint8)),
    "set_shard_part": lambda e, rng: e.set_shard(
        rng.integers(0, 256, (7, e.record_bytes), dtype=np.uint8), row0=5),
    "fill_shard_random": lambda e, rng: e.fill_shard_random(77),
    "encode_across": lambda e, rng: e.encode_across(1000, 2),
    "encode_across_files": lambda e, rng: e.encode_across(
        900, 2, rng.integers(0, 256, (900, e.record_bytes), dtype=np.uint8)),
    "encode_across_synthetic_mac": lambda e, rng: e.encode_across_synthetic_mac(
        1000, 2, bytes(range(16))),
    "encode_within": lambda e, rng: e.encode_within(1000, 2 * e.record_bytes, 2),
    "encode_hermite": lambda e, rng: e.encode_hermite(1000, 2 * e.record_bytes, 2),
}


def test_staleness(pir, monkeypatch):
    """Reserve, a queue, then every mutator in turn: the next two queues equal the single answers
    on the new shard, the first without the image, the second after its rebuild."""
    p, n, efs, nq, nk = 2, 11, 1024, 1, 11
    rng = np.random.default_rng(5)
    keys = _keys(p, n, nq, nk, rng, 0)
    _knobs(monkeypatch, 1)
    with pir.Engine(p, 1, n, efs, nq) as e:
        full = _image_bytes(e)
        e.fill_shard_random(1)
        assert e.fold_image() == 0
        e.reserve_queue(nk)
        assert e.fold_image() == full
        before = e.answer_stream(keys)
        assert _same(before, np.stack([e.answer(k) for k in keys]))
        for name, mutate in MUTATORS.items():
            old = e.get_shard()
            mutate(e, rng)
            assert not np.array_equal(old, e.get_shard()), name
            assert e.fold_image() == 0, name
            singles = np.stack([e.answer(k) for k in keys])
            first = e.answer_stream(keys)
            assert e.fold_image() == 0, name      # wanted once: run without
            second = e.answer_stream(keys)
            assert e.fold_image() == full, name   # the shard stayed: rebuilt
            third = e.answer_stream(keys)
            assert _same(first, singles), name
            assert _same(second, singles), name
            assert _same(third, singles), name
        # the explicit call: drop, build now
        assert e.fold_image("drop") == 0
        assert e.fold_image("build") == full
        assert _same(e.answer_stream(keys), singles)


# ------------------------------------------------------------------------------------ no room
def test_no_room(pir, monkeypatch):
    p, n, efs, nq, nk = 2, 11, 1024, 1, 11
    rng = np.random.default_rng(6)
    shard = rng.integers(0, 256, (1 << n) * efs, dtype=np.uint8)
    keys = _keys(p, n, nq, nk, rng, 0)
    _knobs(monkeypatch, 1, max_bytes=4096)
    with pir.Engine(p, 1, n, efs, nq) as e:
        e.set_shard(shard)
        e.reserve_queue(nk)
        assert e.fold_image() == 0
        got = [e.answer_stream(keys) for _ in range(3)]
        assert e.fold_image() == 0
        singles = np.stack([e.answer(k) for k in keys])
    for g in got:
        assert _same(g, singles)
    _knobs(monkeypatch, 2, max_bytes=4096)
    with pir.Engine(p, 1, n, efs, nq) as e:
        e.set_shard(shard)
        with pytest.raises(pir.PirError, match="fold image"):
            e.reserve_queue(nk)
        with pytest.raises(pir.PirError, match="fold image"):
            e.answer_stream(keys)
        assert e.fold_image() == 0
        assert _same(np.stack([e.answer(k) for k in keys]), singles)


# -------------------------------------------------------------------------------- group queue
def test_group_queue(pir, monkeypatch):
    """An explicit-coefficient (Hollanti) queue over the whole shard uses the image; one over a
    row range starting at 1 (mod 4) reads the rows; both equal the unqueued answers."""
    p, n, efs, nq, nk = 2, 11, 1024, 1, 19
    rng = np.random.default_rng(8)
    shard = rng.integers(0, 256, (1 << n) * efs, dtype=np.uint8)
    coefs = rng.integers(0, 256, (nk, nq, 1 << n), dtype=np.uint8)
    for row0, nrows in ((0, 1 << n), (5, (1 << n) - 9), (8, (1 << n) - 21)):
        _knobs(monkeypatch, 2, gq=2)
        with pir.Engine(p, 1, n, efs, nq) as e:
            e.set_shard(shard)
            got = e.answer_coefs_queue(coefs, row0, nrows)
            assert e.fold_image() == (0 if row0 % 4 else _image_bytes(e)), row0
            want = np.stack([e.answer_coefs(coefs[k], row0, nrows) for k in range(nk)])
        assert _same(got, want), row0


# --------------------------------------------------------------------------------- partitions
def test_partitions_xor_to_full(pir, monkeypatch):
    p, n, efs, nq, nk = 2, 12, 1024, 1, 11
    rng = np.random.default_rng(9)
    shard = rng.integers(0, 256, ((1 << n), efs), dtype=np.uint8)
    keys = _keys(p, n, nq, nk, rng, 0)
    _knobs(monkeypatch, 2)
    acc = np.zeros((nk, nq, efs), np.uint8)
    rows = (1 << n) >> 1
    for part in range(2):
        with pir.Engine(p, 1, n, efs, nq, log_num_partitions=1, partition_index=part) as e:
            e.set_shard(shard[part * rows:(part + 1) * rows])
            acc ^= e.answer_stream(keys)
            assert e.fold_image() == _image_bytes(e)
    for k, key in enumerate(keys):
        assert _same(acc[k], O.answer(p, 1, n, efs, nq, key, shard.reshape(-1))), k
