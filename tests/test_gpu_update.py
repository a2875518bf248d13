"""Live record updates (pir_engine_update_*, k_update_rows; include/pir_engine.h): changed
records patched into the resident shard and into the fold image in place.  After an update the
shard must equal, byte for byte, what the matching encode call gives from the new files; a valid
image must stay valid and exact (a queue's answers through it equal the single answers, an engine
without an image, and the oracle: the DPF shares are dense, so a stale image block changes some
answer of a queue of 19 with probability 1 - 256^-19); an update is ordered between the answers
around it; bad arguments are refused with nothing touched.  Exact GF(2^8) arithmetic: no
tolerance anywhere.  The knobs are read when an engine is made: set them before."""
import ctypes
import hashlib
import hmac

import numpy as np
import pytest

import _oracle as O
from test_gpu_fold_image import _image_bytes, _knobs, _same

pytestmark = pytest.mark.gpu

P, PARTY, NK = 2, 2, 19


@pytest.fixture(scope="module")
def pir():
    import erasurecodedpir_amd as pir
    pir.load()
    return pir


def _keys(n, nk, rng, party1, p=P, nq=1):
    """nk keys of party `party1` (1-based) for random records (with repeats where 2^n < nk)"""
    fcw = O.final_cw(p, nq, 1)
    return [bytes(O.gen_keys(n, int(i), fcw, p, nq,
                             rng.integers(0, 256, 16 * p, dtype=np.uint8).tobytes())[party1 - 1])
            for i in rng.integers(0, 1 << n, nk)]


def _num_files(n, k):
    return k * (1 << n) - 5 if k * (1 << n) > 5 else k * (1 << n)


def _encdb(num_files, k):
    return (num_files + k - 1) // k


def _across_batch(num_files, k):
    """files f and f + encdb (one row); four files of one 4-row block; one file twice; file 0;
    the last file; a file in the last row"""
    encdb = _encdb(num_files, k)
    f = 5 % encdb
    batch = [f] + ([f + encdb] if f + encdb < num_files else [])
    b4 = encdb // 2 // 4 * 4
    batch += [x for x in range(b4, b4 + 4) if x < encdb]
    g = 9 % encdb
    batch += [g, g, 0, num_files - 1, encdb - 1]
    return batch


def _apply(files, batch, deltas):
    new = files.copy()
    for i, f in enumerate(batch):
        new[f] ^= deltas[i]
    return new


def _fresh_across(pir, n, efs, num_files, k, files, party=PARTY, **kw):
    with pir.Engine(P, party, n, efs, 1, **kw) as e:
        e.encode_across(num_files, k, files)
        return e.get_shard()


def _check_answers(pir, mp, e, n, efs, keys, shard, party=PARTY):
    """the queue through e's image == the single answers == an engine without an image == the
    oracle, all on `shard`"""
    got = e.answer_stream(keys)
    assert _same(got, np.stack([e.answer(k) for k in keys]))
    _knobs(mp, 0)
    with pir.Engine(P, party, n, efs, 1) as e0:
        e0.set_shard(shard)
        assert _same(got, e0.answer_stream(keys))
        assert e0.fold_image() == 0
    for i, key in enumerate(keys):
        assert _same(got[i], O.answer(P, party, n, efs, 1, key, shard.reshape(-1))), i


# ------------------------------------------------------------------- 1. across, image kept
ACROSS = [(11, 1024, 3), (11, 1000, 1), (12, 256, 2), (1, 64, 1)]


@pytest.mark.parametrize("shape", ACROSS, ids=lambda s: "n%d_efs%d_k%d" % s)
def test_across_updates_keep_the_image(pir, monkeypatch, shape):
    n, efs, k = shape
    rng = np.random.default_rng(100 + sum(shape))
    num_files = _num_files(n, k)
    files = rng.integers(0, 256, (num_files, efs), dtype=np.uint8)
    keys = _keys(n, NK, rng, PARTY)
    _knobs(monkeypatch, 1)
    with pir.Engine(P, PARTY, n, efs, 1) as e:
        full = _image_bytes(e)
        e.encode_across(num_files, k, files)
        e.reserve_queue(NK)
        if efs < 256:
            # k_scan_t takes no records under 256 B, so reserve_queue leaves their image out:
            # built by hand, the update must still keep and patch it
            e.fold_image("build")
        assert e.fold_image() == full
        for batch in (_across_batch(num_files, k), [num_files // 2]):
            deltas = rng.integers(0, 256, (len(batch), efs), dtype=np.uint8)
            files = _apply(files, batch, deltas)
            e.update_across(batch, deltas, num_files, k)
            assert e.fold_image() == full          # no queue in between
            shard = e.get_shard()
            _knobs(monkeypatch, 1)
            assert np.array_equal(shard, _fresh_across(pir, n, efs, num_files, k, files))
            _check_answers(pir, monkeypatch, e, n, efs, keys, shard)
            assert e.fold_image() == full


# -------------------------------------------------------------------------------- 2. rows
@pytest.mark.parametrize("shape", [(11, 1000), (1, 64)], ids=lambda s: "n%d_efs%d" % s)
def test_rows_form(pir, monkeypatch, shape):
    n, efs = shape
    rng = np.random.default_rng(200 + sum(shape))
    rows = 1 << n
    shard = rng.integers(0, 256, (rows, efs), dtype=np.uint8)
    keys = _keys(n, NK, rng, PARTY)
    _knobs(monkeypatch, 1)
    with pir.Engine(P, PARTY, n, efs, 1) as e:
        full = _image_bytes(e)
        e.set_shard(shard)
        e.reserve_queue(NK)
        if efs < 256:
            e.fold_image("build")
        assert e.fold_image() == full
        b4 = rows // 2 // 4 * 4
        for batch in ([3 % rows] + [r for r in range(b4, b4 + 4) if r < rows] +
                      [7 % rows, 7 % rows, 0, rows - 1], [rows // 3]):
            deltas = rng.integers(0, 256, (len(batch), efs), dtype=np.uint8)
            for i, r in enumerate(batch):
                shard[r] ^= deltas[i]
            e.update_rows(batch, deltas)
            assert e.fold_image() == full
            assert np.array_equal(e.get_shard(), shard)
            _check_answers(pir, monkeypatch, e, n, efs, keys, shard)
            assert e.fold_image() == full


# ------------------------------------------------------------------- 3. within and Hermite
def test_within_hermite_shamir_engine(pir, monkeypatch):
    n, efs, k = 10, 256, 3
    N, file_bytes = 1 << n, 3 * 256 - 7
    num_files = N - 3
    rng = np.random.default_rng(31)
    files = rng.integers(0, 256, (num_files, file_bytes), dtype=np.uint8)
    batch = [16, 18, 5, 5, 0, num_files - 1]            # 16 and 18: one block
    deltas = rng.integers(0, 256, (len(batch), file_bytes), dtype=np.uint8)
    new = _apply(files, batch, deltas)
    x = (n + 1) // 2
    keys = rng.integers(0, 256, (8, 1, (1 << x) + (1 << (n - x))), dtype=np.uint8)
    monkeypatch.setenv("PIR_SH_SHARE", "2")
    monkeypatch.delenv("PIR_SH_G", raising=False)
    monkeypatch.delenv("PIR_SH_PASS", raising=False)
    _knobs(monkeypatch, 2)

    def encode(e, f):
        e.encode_within(num_files, file_bytes, k, f)
        e.encode_hermite(num_files, file_bytes, k, f)

    with pir.Engine(2, 1, n + 1, efs, 1) as e, pir.Engine(2, 1, n + 1, efs, 1) as fresh:
        encode(e, files)
        encode(fresh, new)
        before = e.answer_shamir_queue(keys)
        e.update_within(batch, deltas, num_files, file_bytes, k, hermite=True)
        assert np.array_equal(e.get_shard(), fresh.get_shard())      # all 2N rows
        after = e.answer_shamir_queue(keys)
        assert np.array_equal(after, fresh.answer_shamir_queue(keys))
        assert not np.array_equal(after, before)


def test_within_hollanti_engine(pir, monkeypatch):
    n, efs, k, party = 10, 256, 3, 3
    file_bytes = 3 * 256 - 7
    num_files = (1 << n) - 3
    rng = np.random.default_rng(32)
    files = rng.integers(0, 256, (num_files, file_bytes), dtype=np.uint8)
    batch = [16, 18, 5, 5, 0, num_files - 1]
    deltas = rng.integers(0, 256, (len(batch), file_bytes), dtype=np.uint8)
    new = _apply(files, batch, deltas)
    coefs = rng.integers(0, 256, (8, 1, 1 << n), dtype=np.uint8)
    _knobs(monkeypatch, 2, gq=2)
    with pir.Engine(2, 1, n, efs, 1) as e, pir.Engine(2, 1, n, efs, 1) as fresh:
        e.encode_within(num_files, file_bytes, k, files, party=party)
        fresh.encode_within(num_files, file_bytes, k, new, party=party)
        before = e.answer_coefs_queue(coefs)
        full = _image_bytes(e)
        assert e.fold_image() == full
        e.update_within(batch, deltas, num_files, file_bytes, k, party=party, hermite=False)
        assert e.fold_image() == full
        assert np.array_equal(e.get_shard(), fresh.get_shard())
        after = e.answer_coefs_queue(coefs)
        assert np.array_equal(after, fresh.answer_coefs_queue(coefs))
        assert np.array_equal(after, np.stack([e.answer_coefs(c) for c in coefs]))
        assert not np.array_equal(after, before)


def test_image_block_with_absent_rows(pir, monkeypatch):
    """Two rows of 256 B: the one image block has two absent rows, and the explicit-coefficient
    queue reads it (the tree-DPF queue does not take records this few)."""
    n, efs = 1, 256
    rng = np.random.default_rng(33)
    shard = rng.integers(0, 256, (2, efs), dtype=np.uint8)
    coefs = rng.integers(1, 256, (8, 1, 2), dtype=np.uint8)
    _knobs(monkeypatch, 2, gq=2)
    with pir.Engine(2, 1, n, efs, 1) as e:
        e.set_shard(shard)
        e.answer_coefs_queue(coefs)
        assert e.fold_image() == _image_bytes(e) == 4 * efs
        for batch in ([1, 0, 1], [0]):
            deltas = rng.integers(0, 256, (len(batch), efs), dtype=np.uint8)
            for i, r in enumerate(batch):
                shard[r] ^= deltas[i]
            e.update_rows(batch, deltas)
            assert e.fold_image() == 4 * efs
            assert np.array_equal(e.get_shard(), shard)
            got = e.answer_coefs_queue(coefs)
            assert np.array_equal(got, np.stack([e.answer_coefs(c) for c in coefs]))
            for i in range(len(coefs)):
                assert _same(got[i], O.scan(coefs[i], shard.reshape(-1), efs)), i


# ------------------------------------------------------------------------------ 4. CheckMAC
def _tag(key, payload):
    return np.frombuffer(hmac.new(key, bytes(payload), hashlib.sha256).digest(), np.uint8)


def test_across_mac(pir, monkeypatch):
    from erasurecodedpir_amd import client
    n, payload, k = 8, 70, 2
    efs = payload + 32
    key = bytes(range(40, 56))
    rng = np.random.default_rng(41)
    num_files = _num_files(n, k)
    encdb = _encdb(num_files, k)
    pay = rng.integers(0, 256, (num_files, payload), dtype=np.uint8)
    files = np.concatenate([pay, np.stack([_tag(key, p) for p in pay])], axis=1)
    batch = [3, 3 + encdb, 100, 100, num_files - 1]
    new_pay = rng.integers(0, 256, (len(batch), payload), dtype=np.uint8)
    old_pay = np.empty_like(new_pay)
    cur = pay.copy()
    for i, f in enumerate(batch):       # the second change of a file starts from the first
        old_pay[i] = cur[f]
        cur[f] = new_pay[i]
    new = np.concatenate([cur, np.stack([_tag(key, p) for p in cur])], axis=1)
    _knobs(monkeypatch, 1)
    shards = {}
    for party in (1, 2):
        with pir.Engine(P, party, n, efs, 1) as e:
            e.encode_across(num_files, k, files)
            e.update_across_mac(batch, old_pay, new_pay, num_files, k, key)
            shards[party] = e.get_shard()
        assert np.array_equal(shards[party],
                              _fresh_across(pir, n, efs, num_files, k, new, party=party))
    # decode: row_q = f0 ^ q f1 for parties q = 1, 2, so f1 = (row_1 ^ row_2) / 3, f0 = row_1 ^ f1
    inv3 = next(v for v in range(256) if O.gf_mul(3, v) == 1)
    div3 = np.array([O.gf_mul(inv3, v) for v in range(256)], np.uint8)
    for f in (3, 3 + encdb, 100):
        r = f % encdb
        f1 = div3[shards[1][r] ^ shards[2][r]]
        rec = f1 if f >= encdb else shards[1][r] ^ f1
        assert np.array_equal(rec, new[f])
        assert client.mac_check(rec, payload, key)
        assert not np.array_equal(rec, files[f])


# ---------------------------------------------------------------------------- 5. partitions
def test_partitions_take_one_global_batch(pir, monkeypatch):
    n, efs, k = 12, 1024, 2
    rng = np.random.default_rng(51)
    num_files = _num_files(n, k)
    files = rng.integers(0, 256, (num_files, efs), dtype=np.uint8)
    batch = _across_batch(num_files, k) + [int(v) for v in rng.integers(0, num_files, 40)]
    deltas = rng.integers(0, 256, (len(batch), efs), dtype=np.uint8)
    new = _apply(files, batch, deltas)
    keys = _keys(n, 11, rng, PARTY)
    _knobs(monkeypatch, 2)
    acc = np.zeros((len(keys), 1, efs), np.uint8)
    rows = (1 << n) >> 1
    whole = _fresh_across(pir, n, efs, num_files, k, new)
    for part in range(2):
        with pir.Engine(P, PARTY, n, efs, 1, log_num_partitions=1, partition_index=part) as e:
            e.encode_across(num_files, k, files)
            e.answer_stream(keys)
            assert e.fold_image() == _image_bytes(e)
            e.update_across(batch, deltas, num_files, k)
            assert e.fold_image() == _image_bytes(e)
            assert np.array_equal(e.get_shard(), whole[part * rows:(part + 1) * rows])
            acc ^= e.answer_stream(keys)
            assert e.fold_image() == _image_bytes(e)
    for i, key in enumerate(keys):
        assert _same(acc[i], O.answer(P, PARTY, n, efs, 1, key, whole.reshape(-1))), i


# ---------------------------------------------------------------------------- 6. epoch rule
def test_epoch_rule(pir, monkeypatch):
    n, efs, k = 11, 1024, 2
    rng = np.random.default_rng(61)
    num_files = _num_files(n, k)
    files = rng.integers(0, 256, (num_files, efs), dtype=np.uint8)
    batch = _across_batch(num_files, k)
    deltas = rng.integers(0, 256, (len(batch), efs), dtype=np.uint8)
    new = _apply(files, batch, deltas)
    keys = _keys(n, 11, rng, PARTY)
    want = _fresh_across(pir, n, efs, num_files, k, new)
    # no image: queue (wanted once), update (not a rewrite), queue (builds)
    _knobs(monkeypatch, 1)
    with pir.Engine(P, PARTY, n, efs, 1) as e:
        e.encode_across(num_files, k, files)
        assert e.fold_image() == 0
        e.answer_stream(keys)
        assert e.fold_image() == 0
        e.update_across(batch, deltas, num_files, k)
        assert e.fold_image() == 0
        got = e.answer_stream(keys)
        assert e.fold_image() == _image_bytes(e)
        assert np.array_equal(e.get_shard(), want)
        assert _same(got, np.stack([e.answer(key) for key in keys]))
        assert _same(got, e.answer_stream(keys))
    # switched off: the rows alone
    _knobs(monkeypatch, 0)
    with pir.Engine(P, PARTY, n, efs, 1) as e:
        e.encode_across(num_files, k, files)
        e.answer_stream(keys)
        e.update_across(batch, deltas, num_files, k)
        assert e.fold_image() == 0
        assert np.array_equal(e.get_shard(), want)
        assert _same(e.answer_stream(keys), got)
        assert e.fold_image() == 0


# ------------------------------------------------------------------------------ 7. ordering
def test_update_is_ordered_between_answers(pir, monkeypatch):
    n, efs, k = 11, 1024, 2
    rng = np.random.default_rng(71)
    num_files = _num_files(n, k)
    files = rng.integers(0, 256, (num_files, efs), dtype=np.uint8)
    batch = _across_batch(num_files, k) + [int(v) for v in rng.integers(0, num_files, 300)]
    deltas = rng.integers(0, 256, (len(batch), efs), dtype=np.uint8)
    keys = _keys(n, NK, rng, PARTY)
    _knobs(monkeypatch, 1)
    with pir.Engine(P, PARTY, n, efs, 1) as e:
        e.encode_across(num_files, k, files)
        e.reserve_queue(NK)
        assert e.fold_image() == _image_bytes(e)
        old = np.stack([e.answer(key) for key in keys])
        d_k = e.alloc_dev(NK * e.key_len)
        d_r = [e.alloc_dev(NK * e.answer_bytes) for _ in range(2)]
        d_d = e.alloc_dev(deltas.size)
        e.h2d(d_k, b"".join(keys))
        e.h2d(d_d, deltas.reshape(-1))
        e.sync()
        e.answer_stream_dev(d_k, NK, d_r[0])       # one stream, no sync in between
        e.update_across_dev(batch, d_d, efs, num_files, k)
        e.answer_stream_dev(d_k, NK, d_r[1])
        e.sync()
        first, second = (e.d2h(d, NK * e.answer_bytes) for d in d_r)
        assert e.fold_image() == _image_bytes(e)
        new = np.stack([e.answer(key) for key in keys])
        assert np.array_equal(e.get_shard(),
                              _fresh_across(pir, n, efs, num_files, k, _apply(files, batch, deltas)))
    assert _same(first, old)
    assert _same(second, new)
    assert not _same(old, new)


# ------------------------------------------------------------------------------ 8. refusals
def test_refusals_touch_nothing(pir, monkeypatch):
    from erasurecodedpir_amd import _lib
    lib = _lib.load()
    n, efs, k = 8, 64, 2
    rng = np.random.default_rng(81)
    num_files = _num_files(n, k)
    files = rng.integers(0, 256, (num_files, efs), dtype=np.uint8)
    _knobs(monkeypatch, 1)
    d = rng.integers(0, 256, (2, efs), dtype=np.uint8)
    dw = rng.integers(0, 256, (2, 100), dtype=np.uint8)
    idx = (ctypes.c_uint64 * 2)(1, 2)
    buf = (ctypes.c_uint8 * (2 * efs))()
    with pir.Engine(P, PARTY, n, efs, 1) as e:
        e.encode_across(num_files, k, files)
        full = e.fold_image("build")
        assert full == _image_bytes(e)
        shard = e.get_shard()
        h = e._h
        key = (ctypes.c_uint8 * 16)()
        raw = [  # straight at the C ABI: null pointers, negative counts
            lambda: lib.pir_engine_update_rows(None, idx, 2, buf, efs),
            lambda: lib.pir_engine_update_rows(h, None, 2, buf, efs),
            lambda: lib.pir_engine_update_rows(h, idx, 2, None, efs),
            lambda: lib.pir_engine_update_rows(h, idx, -1, buf, efs),
            lambda: lib.pir_engine_update_rows_dev(h, idx, 2, None, efs, None),
            lambda: lib.pir_engine_update_across(h, None, 2, buf, efs, num_files, k),
            lambda: lib.pir_engine_update_across(h, idx, 2, None, efs, num_files, k),
            lambda: lib.pir_engine_update_across(h, idx, -2, buf, efs, num_files, k),
            lambda: lib.pir_engine_update_across_dev(h, idx, 2, None, efs, num_files, k, None),
            lambda: lib.pir_engine_update_within(h, None, 2, buf, efs, 256, efs, 1, 0, 0),
            lambda: lib.pir_engine_update_within(h, idx, 2, None, efs, 256, efs, 1, 0, 0),
            lambda: lib.pir_engine_update_within(h, idx, -1, buf, efs, 256, efs, 1, 0, 0),
            lambda: lib.pir_engine_update_within_dev(h, idx, 2, None, efs, 256, efs, 1, 0, 0, None),
            lambda: lib.pir_engine_update_across_mac_dev(h, idx, 2, None, buf, efs, num_files, k,
                                                         key, None),
            lambda: lib.pir_engine_update_across_mac_dev(h, idx, 2, buf, None, efs, num_files, k,
                                                         key, None),
            lambda: lib.pir_engine_update_across_mac_dev(h, idx, 2, buf, buf, efs, num_files, k,
                                                         None, None),
        ]
        for i, call in enumerate(raw):
            assert call() == -1, i                                     # PIR_EINVAL
        wrapped = [
            lambda: e.update_rows([0, 1 << n], d),                     # a row beyond the shard
            lambda: e.update_rows([0, 1], d[:, :efs - 1]),             # pitch below the bytes read
            lambda: e.update_across([0, num_files], d, num_files, k),  # growing the database
            lambda: e.update_across([0, 1], d, num_files, 0),
            lambda: e.update_across([0, 1], d, num_files, 17),
            lambda: e.update_across([0, 1], d, k * (1 << n) + 1, k),   # encdb beyond the domain
            lambda: e.update_across([0, 1], d[:, :efs - 1], num_files, k),
            lambda: e.update_within([0, 256], dw, 256, 100, 2),
            lambda: e.update_within([0, 1], dw, 256, 100, 0),
            lambda: e.update_within([0, 1], dw, 256, 100, 17),
            lambda: e.update_within([0, 1], dw, (1 << n) + 1, 100, 2),
            lambda: e.update_within([0, 1], dw[:, :99], 256, 100, 2),
            lambda: e.update_within([0, 1], dw, 256, 100, 1),          # file_bytes > k record_bytes
            lambda: e.update_within([0, 1], dw, 256, 100, 2, party=256),
            lambda: e.update_within([0, 200], dw, 256, 100, 2, hermite=True),   # 200 >= N = 128
        ]
        for i, call in enumerate(wrapped):
            with pytest.raises(pir.PirError, match=r"\(-1\)"):
                call()
        # an empty batch: PIR_OK, nothing done
        e.update_rows([], np.zeros((0, efs), np.uint8))
        e.update_across([], np.zeros((0, efs), np.uint8), num_files, k)
        e.update_within([], np.zeros((0, 100), np.uint8), 256, 100, 2)
        assert lib.pir_engine_update_across_dev(h, None, 0, None, 0, num_files, k, None) == 0
        assert lib.pir_engine_update_across_mac_dev(h, None, 0, None, None, 0, num_files, k, key,
                                                    None) == 0
        assert e.fold_image() == full
        assert np.array_equal(e.get_shard(), shard)
    # Hermite rows on an engine with partitions; the CheckMAC form on records with no payload
    with pir.Engine(P, PARTY, n, efs, 1, log_num_partitions=1, partition_index=1) as e:
        before = e.get_shard()
        with pytest.raises(pir.PirError, match=r"\(-1\)"):
            e.update_within([0, 1], dw, 64, 100, 2, hermite=True)
        assert np.array_equal(e.get_shard(), before)
    with pir.Engine(P, PARTY, 0, efs, 1) as e:        # one row: no Hermite row beside it
        with pytest.raises(pir.PirError, match=r"\(-1\)"):
            e.update_within([0], dw[:1, :efs], 1, efs, 1, hermite=True)
        assert not e.get_shard().any()
    with pir.Engine(P, PARTY, n, 32, 1) as e:
        with pytest.raises(pir.PirError, match=r"\(-1\)"):
            e.update_across_mac([0], np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.uint8), 16, 1,
                                bytes(16))
        assert not e.get_shard().any()
