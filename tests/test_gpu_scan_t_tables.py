"""k_scan_t's nibble tables (csrc/pir_scan_t.hip): per 64-row chunk a wave keeps 16 tables of
the 16 XOR combinations of 4 rows' coefficient words, and every bit position of 8 rows takes two
lookups (rows 0-3, rows 4-7), the indices coming from the shard's bits.  Checked against the
oracle's scan / answer (exact GF(2^8): no tolerance) over both entry widths (4 and 8 coefficient
bytes per record), pitch padding with inactive lanes, four column groups, waves that hold fewer
than 4 rows, row counts that are no multiple of 4 or 8, unaligned starts, two chunks per wave
with a ragged last one at full occupancy (fixed ranges and claimed chunks), shards that steer
every lookup to one entry or to one row's bit, and the key-major shares of a shared queue.
$PIR_SCAN_T=2 sends the 4- and 5-round shapes to the kernel as well."""
import numpy as np
import pytest

import _oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pir():
    import erasurecodedpir_amd as pir
    pir.load()
    return pir


@pytest.fixture(autouse=True)
def _scan_t_everywhere(monkeypatch):
    monkeypatch.setenv("PIR_SCAN_T", "2")  # read when an engine plans its scan


# ------------------------------------------------------------------ interleaved coefficients
SHAPES = [(256, 8), (260, 7), (1024, 6), (256, 5), (256, 4)]  # (record bytes, rounds)
RANGES = [(0, 4096), (3, 1), (5, 7), (0, 8), (1, 9), (61, 67), (7, 1000)]  # (row0, nrows)


@pytest.mark.parametrize("efs,nq", SHAPES, ids=lambda v: str(v))
def test_row_ranges(pir, efs, nq):
    n = 12
    rng = np.random.default_rng(efs * 10 + nq)
    shard = rng.integers(0, 256, (1 << n) * efs, dtype=np.uint8)
    coefs = rng.integers(0, 256, (nq, 1 << n), dtype=np.uint8)
    with pir.Engine(2, 1, n, efs, nq) as e:
        e.set_shard(shard)
        got = [e.answer_coefs(coefs, row0, nrows) for row0, nrows in RANGES]
    for (row0, nrows), g in zip(RANGES, got):
        assert np.array_equal(g, O.scan(coefs, shard, efs, row0, row0 + nrows)), (row0, nrows)


FULL = [(17, 1024, 8), (19, 256, 8)]  # (log rows, record bytes, rounds): every CU full
_full_cache = {}


def _full_case(n, efs, nq):
    """Inputs and the oracle's answer, computed once and shared by the two forms."""
    if (n, efs, nq) not in _full_cache:
        rng = np.random.default_rng(n * 1000 + efs + nq)
        shard = rng.integers(0, 256, (1 << n) * efs, dtype=np.uint8)
        coefs = rng.integers(0, 256, (nq, 1 << n), dtype=np.uint8)
        nrows = (1 << n) - 37
        want = O.scan(coefs, shard, efs, 0, nrows)
        for a in (shard, coefs, want):
            a.setflags(write=False)
        _full_cache[(n, efs, nq)] = shard, coefs, nrows, want
    return _full_cache[(n, efs, nq)]


@pytest.mark.parametrize("dyn", ["0", "1"], ids=["fixed_ranges", "claimed_chunks"])
@pytest.mark.parametrize("n,efs,nq", FULL, ids=lambda v: str(v))
def test_full_occupancy(pir, monkeypatch, n, efs, nq, dyn):
    """2^n - 37 rows: at the grid the engine picks a wave holds two chunks, the last ragged."""
    monkeypatch.setenv("PIR_SCAN_DYN", dyn)
    shard, coefs, nrows, want = _full_case(n, efs, nq)
    with pir.Engine(2, 1, n, efs, nq) as e:
        e.set_shard(shard)
        got = [e.answer_coefs(coefs, 0, nrows) for _ in range(2)]
    for g in got:
        assert np.array_equal(g, want)


# ----------------------------------------------------------------------------- shard patterns
def _pattern_shards(n, efs, rng):
    rnd = rng.integers(0, 256, ((1 << n), efs), dtype=np.uint8)
    yield "random", rnd
    yield "all_ff", np.full(((1 << n), efs), 0xFF, np.uint8)  # entry 15 of both tables, always
    for k in range(8):  # only row k of every 8 sets index bits: a row-to-bit or table mix-up
        s = np.zeros_like(rnd)
        s[k::8] = rnd[k::8] | 1
        yield "row_%d_of_8" % k, s


@pytest.mark.parametrize("kind", ["random", "all_ff", "one_row_in_eight"])
def test_shard_patterns(pir, kind):
    n, efs, nq = 12, 256, 8
    rng = np.random.default_rng(77)
    coefs = rng.integers(0, 256, (nq, 1 << n), dtype=np.uint8)
    shards = [(name, s) for name, s in _pattern_shards(n, efs, rng)
              if name == kind or (kind == "one_row_in_eight" and name.startswith("row_"))]
    assert shards
    with pir.Engine(2, 1, n, efs, nq) as e:
        for name, s in shards:
            e.set_shard(s)
            for row0, nrows in ((0, 1 << n), (5, 999)):
                got = e.answer_coefs(coefs, row0, nrows)
                want = O.scan(coefs, s.reshape(-1), efs, row0, row0 + nrows)
                assert np.array_equal(got, want), (name, row0, nrows)


# -------------------------------------------------------------------------- key-major shares
@pytest.mark.parametrize("nk", [20, 9], ids=lambda k: "keys%d" % k)
def test_shared_queue_key_major(pir, monkeypatch, nk):
    """A shared queue's groups (20 = 7 + 7 + 6 keys) read their shares key-major."""
    monkeypatch.setenv("PIR_STREAM_SHARE", "2")
    monkeypatch.delenv("PIR_STREAM_G", raising=False)
    p, n, efs, nq = 2, 12, 1024, 1
    rng = np.random.default_rng(500 + nk)
    shard = rng.integers(0, 256, (1 << n) * efs, dtype=np.uint8)
    fcw = O.final_cw(p, nq, 1)
    keys = [bytes(O.gen_keys(n, int(i), fcw, p, nq,
                             rng.integers(0, 256, 16 * p, dtype=np.uint8).tobytes())[0])
            for i in rng.choice(1 << n, nk, replace=False)]
    with pir.Engine(p, 1, n, efs, nq) as e:
        e.set_shard(shard)
        got = e.answer_stream(keys)
    assert got.shape == (nk, nq, efs)
    for k, key in enumerate(keys):
        assert np.array_equal(got[k], O.answer(p, 1, n, efs, nq, key, shard)), k
