"""The Woodruff mode (mode 5): runWoodruffQueryThread (src/c/server.cpp:564-645) served from the
device-resident shard, with genWoodruffVs / genWoodruffQuery / assembleWoodruffResponses.

Record i of the N = 2^n belongs to the i-th 2-subset (a, b) of [0, M) in lexicographic order, M
the smallest integer >= 3 with M (M - 1) / 2 >= N.  The checker is a vectorised numpy
restatement of the two formulas of the mode over GF(2^8)/0x11d,
    value:       out    = XOR_i key[a_i] * key[b_i] * row_i
    derivative:  out[0] = the value, out[1 + j] = XOR_{i : j in {a_i, b_i}} key[other] * row_i;
the CPU tests pin it against the reference's own answers (tests/golden/woodruff.json, from
tests/golden/make_golden_woodruff.py) and the GPU tests compare the engine, the shim and both
answer paths against it byte for byte.  The arithmetic is exact: no tolerance anywhere."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle as O
from test_shamir import MUL, gf_pow, synth_files, xor_reduce

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------- the checker
def wd_m(n):
    m = 3
    while m * (m - 1) // 2 < (1 << n):
        m += 1
    return m


def wd_start(M, a):
    return a * (2 * M - a - 1) // 2


def wd_rank(M, a, b):
    return wd_start(M, a) + b - a - 1


def wd_pairs(M, N):
    """(a, b) of the records 0 .. N - 1: the 2-subsets of [0, M) in lexicographic order."""
    a, b = np.triu_indices(M, 1)
    return a[:N], b[:N]


def woodruff_ref(rows, key, lo=0, hi=None, chunk=1 << 15):
    rows = np.asarray(rows, np.uint8)
    N, efs = rows.shape
    hi = N if hi is None else hi
    key = np.asarray(key, np.uint8)
    a, b = wd_pairs(key.size, N)
    coef = MUL[key[a], key[b]]
    out = np.zeros(efs, np.uint8)
    for c0 in range(lo, hi, chunk):
        c1 = min(hi, c0 + chunk)
        out ^= xor_reduce(MUL[coef[c0:c1, None], rows[c0:c1]], 0)
    return out


def woodruff_deriv_ref(rows, key, lo=0, hi=None):
    rows = np.asarray(rows, np.uint8)
    N, efs = rows.shape
    hi = N if hi is None else hi
    key = np.asarray(key, np.uint8)
    M = key.size
    a, b = wd_pairs(M, N)
    a, b, r = a[lo:hi], b[lo:hi], rows[lo:hi]
    out = np.zeros((M + 1, efs), np.uint8)
    out[0] = woodruff_ref(rows, key, lo, hi)
    np.bitwise_xor.at(out[1:], a, MUL[key[b][:, None], r])
    np.bitwise_xor.at(out[1:], b, MUL[key[a][:, None], r])
    return out


# -------------------------------------------------------------------------------- CPU tests
CASES = O.golden("woodruff.json")["cases"]
IDS = ["L%d_f%d_t%d_r%d" % (c["L"], c["f"], c["t"], c["r"]) for c in CASES]


@pytest.fixture
def S():
    from erasurecodedpir_amd import server as S
    S.set_woodruff_derivative(False)
    yield S
    S.set_woodruff_derivative(False)


def _setup(S, case, deriv=False):
    S.set_woodruff_derivative(deriv)
    S.setSystemParams(case["L"], case["f"], case["t"], 1, case["r"], 0, 1, 0, 5)


def _hex(h, shape):
    return np.frombuffer(bytes.fromhex(h), np.uint8).reshape(shape)


def _rows(case):
    """k = 1: every party's shard is the synthetic database."""
    rows = synth_files(case["params"]["NUM_FILES"], case["f"])
    for q, sha in case["shard_sha256"].items():
        assert hashlib.sha256(rows.tobytes()).hexdigest() == sha, q
    return rows


def test_key_length():
    import erasurecodedpir_amd as pir
    kat = O.golden("client_kat.json")["woodruff_key_len"]
    assert kat
    for args, want in kat.items():   # "p,r,t,logDomainSize,fileSizeBytes" -> M
        n = int(args.split(",")[3])
        assert pir.woodruff_m(n) == want == wd_m(n), args
    for n in range(4, 32):
        M = pir.woodruff_m(n)
        assert M == wd_m(n)
        assert M * (M - 1) // 2 >= 1 << n and (M - 1) * (M - 2) // 2 < 1 << n
    assert pir.woodruff_m(32) == 0 and pir.woodruff_m(-1) == 0


def test_pair_is_exact_for_every_domain():
    import erasurecodedpir_amd as pir
    for n in range(4, 32):
        M, N = wd_m(n), 1 << n
        rows_a = range(M - 1) if M < (1 << 12) else \
            sorted(set(int(x) for x in np.linspace(0, M - 2, 4096)))
        ranks = {N - 1, 0}
        for a in rows_a:
            ranks.update((wd_start(M, a) - 1, wd_start(M, a), wd_start(M, a) + 1))
        for i in ranks:
            if i < 0 or i >= M * (M - 1) // 2:
                continue
            a, b = pir.woodruff_pair(M, i)
            assert wd_start(M, a) <= i < wd_start(M, a + 1), (n, i, a, b)
            assert b == a + 1 + i - wd_start(M, a) and a < b < M, (n, i, a, b)
    with pytest.raises(pir.PirError):
        pir.woodruff_pair(7, 21)
    with pytest.raises(pir.PirError):
        pir.woodruff_pair(2, 0)


def test_pairs_restatement_matches_the_engine_map():
    import erasurecodedpir_amd as pir
    for n in (4, 7, 10):
        M = wd_m(n)
        a, b = wd_pairs(M, 1 << n)
        for i in range(1 << n):
            assert pir.woodruff_pair(M, i) == (a[i], b[i])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_globals_match_reference(S, case):
    _setup(S, case)
    got = S.params()
    assert {k: got[k] for k in case["params"]} == case["params"]
    assert got["NUM_RESPONSES"] == got["NUM_PARTIES"] - case["r"]
    _setup(S, case, deriv=True)
    assert S.params()["NUM_PARTIES"] == case["num_parties_derivative"]
    assert S.params()["WOODRUFF_M"] == case["params"]["WOODRUFF_M"]


def test_setup_refusals():
    for args, word in [("6, 16, 1, 2, 0, 0, 1, 0, 5", "k == 1"),
                       ("6, 16, 1, 1, 0, 0, 1, 1, 5", "CheckMAC"),
                       ("6, 16, 1, 1, 0, 1, 1, 0, 5", "B > 0"),
                       ("6, 16, 1, 1, 0, 0, 1, 0, 6", "outside the engine's scope")]:
        code = "from erasurecodedpir_amd import server as S; S.setSystemParams(%s)" % args
        r = subprocess.run([sys.executable, "-c", code], cwd=O.ROOT, capture_output=True, text=True)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr)
    # the other modes keep their Woodruff globals as they were
    code = ("from erasurecodedpir_amd import server as S; S.setSystemParams(6, 16, 1, 1, 0, 0, 1, 0, 0); "
            "print(S.params()['WOODRUFF_M'])")
    r = subprocess.run([sys.executable, "-c", code], cwd=O.ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split()[-1] == "0", r.stderr


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_reproduces_reference_answers(case):
    prm = case["params"]
    N, efs, M, T = prm["NUM_ENCODED_FILES"], prm["ENCODED_FILE_SIZE_BYTES"], prm["WOODRUFF_M"], \
        case["T"]
    assert M == wd_m(case["L"])
    rows = _rows(case)
    key = _hex(case["key"], (M,))
    assert (key == 0).any()
    want, dwant = _hex(case["value"], (efs,)), _hex(case["deriv"], (M + 1, efs))
    assert np.array_equal(woodruff_ref(rows, key), want)
    assert np.array_equal(woodruff_deriv_ref(rows, key), dwant)
    assert case["value_slices"] == case["value"] and case["deriv_slices"] == case["deriv"]
    acc, dacc = np.zeros_like(want), np.zeros_like(dwant)
    for t in range(T):
        acc ^= woodruff_ref(rows, key, t * N // T, (t + 1) * N // T)
        dacc ^= woodruff_deriv_ref(rows, key, t * N // T, (t + 1) * N // T)
    assert np.array_equal(acc, want) and np.array_equal(dacc, dwant)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_client_query_and_decode_match_reference(S, case):
    _setup(S, case)
    prm, e2e = case["params"], case["e2e"]
    M, p, t, efs = prm["WOODRUFF_M"], prm["NUM_PARTIES"], case["t"], prm["ENCODED_FILE_SIZE_BYTES"]
    v = _hex(e2e["v"], (t, M))
    keys = S.genWoodruffQuery(e2e["index"], t, p, M, v)
    assert np.array_equal(keys, _hex(e2e["keys"], (p, M)))
    a, b = wd_pairs(M, prm["NUM_FILES"])
    ind = np.zeros(M, np.uint8)
    ind[[a[e2e["index"]], b[e2e["index"]]]] = 1
    for i in range(p):   # key i = E + sum_k (i + 1)^(k + 1) v[k]
        want = ind.copy()
        for k in range(t):
            want ^= MUL[gf_pow(i + 1, k + 1), v[k]]
        assert np.array_equal(keys[i], want), i
    vs = S.genWoodruffVs(t, M)
    assert vs.shape == (t, M) and all((vs[i] == i).all() for i in range(t))
    resp = np.stack([_hex(h, (1, efs)) for h in e2e["responses"]])
    got = S.assembleWoodruffResponses(e2e["erasure"], resp, v)
    assert np.array_equal(got, _hex(e2e["decoded"], (prm["FILE_SIZE_BYTES"],)))
    assert np.array_equal(got, _rows(case)[e2e["index"]])
    # the stored responses are the restatement's answers to the stored keys
    alive = [q for q in range(1, p + 1) if e2e["erasure"][q - 1]]
    assert len(alive) == p - case["r"]
    for j, q in enumerate(alive):
        assert np.array_equal(woodruff_ref(_rows(case), keys[q - 1]), resp[j, 0]), q


def test_tsan_harness_still_links(tmp_path):
    """pir_server.cpp alone against the stub engine (its own pir_engine_* names only): the
    Woodruff unit must stay out of it."""
    r = subprocess.run(["make", "-C", os.path.join(O.ROOT, "tests", "tsan"),
                        "OUT=%s" % (tmp_path / "build")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "build" / "shim_threads").exists()


# -------------------------------------------------------------------------------- GPU tests
@pytest.fixture(scope="module")
def pir():
    import erasurecodedpir_amd as pir
    pir.load()
    return pir


def _engine(pir, n, efs, **kw):
    return pir.Engine(2, 1, n, efs, 1, **kw)


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_goldens_through_the_shim(S, case):
    """GPU setup -> runWoodruffQueryThread over the whole domain == the reference; T Thread slices
    + assemble == the same; both answer kinds."""
    prm = case["params"]
    N, efs, M, T = prm["NUM_ENCODED_FILES"], prm["ENCODED_FILE_SIZE_BYTES"], prm["WOODRUFF_M"], \
        case["T"]
    key = _hex(case["key"], (M,))
    for deriv, want in ((False, _hex(case["value"], (1, efs))),
                        (True, _hex(case["deriv"], (M + 1, efs)))):
        _setup(S, case, deriv)
        cl = S.Client(case["L"], case["f"])
        # fewer parties with derivatives; k = 1, so every party holds the same rows
        party = min(case["party"], S.params()["NUM_PARTIES"])
        sv = S.Server(party, case["L"], efs, 0, T)
        try:
            cl.encode_within_files_server(sv)
            assert np.array_equal(sv.runWoodruffQueryThread(key, 0, 0, N), want)
            parts = np.stack([sv.runWoodruffQueryThread(key, t, t * (N // T), (t + 1) * (N // T))
                              for t in range(T)])
            assert np.array_equal(S.assembleWoodruffQueryThreadResults(sv, parts), want)
            rows = np.stack([sv.read_row(i) for i in range(N)])
            assert hashlib.sha256(rows.tobytes()).hexdigest() == case["shard_sha256"][str(party)]
        finally:
            sv.freeServer()
            cl.free_client()


@gpu
@pytest.mark.parametrize("efs", [8, 30, 256, 1024])
@pytest.mark.parametrize("n", [4, 7, 10, 13])
def test_engine_matches_restatement(pir, n, efs):
    rng = np.random.default_rng(500 + 31 * n + efs)
    rows = rng.integers(0, 256, (1 << n, efs), dtype=np.uint8)
    M = wd_m(n)
    key = rng.integers(0, 256, M, dtype=np.uint8)
    key[rng.choice(M, 2, replace=False)] = 0
    with _engine(pir, n, efs) as e:
        e.set_shard(rows)
        assert e.woodruff_m == M
        assert np.array_equal(e.answer_woodruff(key), woodruff_ref(rows, key))
        assert np.array_equal(e.answer_woodruff_deriv(key), woodruff_deriv_ref(rows, key))


# lo / hi of the Thread form: empty, one record, odd offsets straddling triangle rows, inside the
# truncated last row, whole rows, the ends
def _ranges(M, N):
    a_last = int(wd_pairs(M, N)[0][-1])
    s = lambda a: wd_start(M, a)  # noqa: E731
    return [(0, 0), (5, 5), (N, N), (0, 1), (N - 1, N), (77, 78), (s(3) - 1, s(3) + 1),
            (s(2) + 3, s(7) - 2), (s(4), s(6)), (s(a_last) + 1, N - 1), (s(a_last), N),
            (s(a_last) - 5, s(a_last) + 2), (1, N - 1)]


@gpu
def test_ranges(pir):
    n, efs = 9, 24
    N, M = 1 << n, wd_m(n)   # M = 33: 528 pairs, triangle row 26 cut to 5 of its 6 records
    assert M * (M - 1) // 2 > N and N - wd_start(M, int(wd_pairs(M, N)[0][-1])) == 5
    rng = np.random.default_rng(8)
    rows = rng.integers(0, 256, (N, efs), dtype=np.uint8)
    key = rng.integers(1, 256, M, dtype=np.uint8)
    with _engine(pir, n, efs) as e:
        e.set_shard(rows)
        for lo, hi in _ranges(M, N):
            assert np.array_equal(e.answer_woodruff(key, lo, hi - lo),
                                  woodruff_ref(rows, key, lo, hi)), (lo, hi)
            assert np.array_equal(e.answer_woodruff_deriv(key, lo, hi - lo),
                                  woodruff_deriv_ref(rows, key, lo, hi)), (lo, hi)
        acc, dacc = np.zeros(efs, np.uint8), np.zeros((M + 1, efs), np.uint8)
        for lo, hi in [(0, 13), (13, 90), (90, N)]:
            acc ^= e.answer_woodruff(key, lo, hi - lo)
            dacc ^= e.answer_woodruff_deriv(key, lo, hi - lo)
        assert np.array_equal(acc, woodruff_ref(rows, key))
        assert np.array_equal(dacc, woodruff_deriv_ref(rows, key))


@gpu
def test_refusals(pir):
    n, efs = 8, 16
    M = wd_m(n)
    key = np.ones(M, np.uint8)
    with _engine(pir, n, efs) as e:
        for fn in (e.answer_woodruff, e.answer_woodruff_deriv):
            with pytest.raises(pir.PirError, match="M = %d" % M):
                fn(key[:-1])
            with pytest.raises(pir.PirError, match="M = %d" % M):
                fn(np.ones(M + 1, np.uint8))
            with pytest.raises(pir.PirError, match="beyond"):
                fn(key, 1, 1 << n)
            with pytest.raises(pir.PirError, match="beyond"):
                fn(key, (1 << n) + 1, 0)
        e.attach_comm(pir.comm_unique_id(), 1, 0)
        for fn in (e.answer_woodruff, e.answer_woodruff_deriv):
            with pytest.raises(pir.PirError, match="communicator"):
                fn(key)
    with pir.Engine(2, 1, n, efs, 2) as e:
        for fn in (e.answer_woodruff, e.answer_woodruff_deriv):
            with pytest.raises(pir.PirError, match="one round"):
                fn(key)
    with pir.Engine(2, 1, n + 1, efs, 1, log_num_partitions=1, partition_index=0) as e:
        assert e.woodruff_fused_tile == 0
        for fn in (e.answer_woodruff, e.answer_woodruff_deriv):
            with pytest.raises(pir.PirError, match="split shard"):
                fn(np.ones(wd_m(n + 1), np.uint8))


def _fused_n(pir, efs):
    """The smallest n whose whole domain k_query's Woodruff mode tiles on this GPU."""
    for n in range(12, 24):
        with _engine(pir, n, efs) as e:
            tile = e.woodruff_fused_tile
        if tile:
            return n, tile
    pytest.fail("no n <= 23 gets a tile for %d-byte records" % efs)


def _answer(e, monkeypatch, mode, key):
    monkeypatch.setenv("PIR_WD_FUSED", str(mode))
    e.set_profiling(1)
    got = e.answer_woodruff(key)
    path = e.last_timings()["fused"]
    e.set_profiling(0)
    monkeypatch.delenv("PIR_WD_FUSED")
    return got, path


@gpu
@pytest.mark.parametrize("efs", [256, 1024])
def test_fused_path(pir, monkeypatch, efs):
    """k_query's Woodruff mode (forced) against the coefficient kernel + scan (forced), byte for
    byte; both against the restatement at 256 B; sparse keys whose pairs sit on the first and
    last record, on both sides of a tile boundary and of a triangle-row boundary."""
    n, tile = _fused_n(pir, efs)
    N, M = 1 << n, wd_m(n)
    rng = np.random.default_rng(efs)
    dense = rng.integers(1, 256, M, dtype=np.uint8)
    a_all, b_all = wd_pairs(M, N)
    with _engine(pir, n, efs) as e:
        e.fill_shard_random(1900 + efs)
        fused, path = _answer(e, monkeypatch, 2, dense)
        assert path == 5.0
        plain, path = _answer(e, monkeypatch, 0, dense)
        assert path == 6.0
        assert fused.any() and np.array_equal(fused, plain)
        if efs == 256:
            assert np.array_equal(fused, woodruff_ref(e.get_shard(0, N), dense))
        a_mid = M // 3
        spots = [[0], [N - 1], [tile - 1, tile], [5 * tile - 1, 5 * tile],
                 [wd_start(M, a_mid) - 1, wd_start(M, a_mid)], [N - tile - 1, N - tile]]
        for recs in spots:
            idx = sorted({int(x) for r in recs for x in (a_all[r], b_all[r])})
            assert 2 <= len(idx) <= 6
            key = np.zeros(M, np.uint8)
            key[idx] = rng.integers(1, 256, len(idx), dtype=np.uint8)
            want = np.zeros(efs, np.uint8)
            hit = set()
            for x in idx:          # every pair inside the support that is a record
                for y in idx:
                    if x < y and wd_rank(M, x, y) < N:
                        i = wd_rank(M, x, y)
                        hit.add(i)
                        want ^= MUL[int(MUL[key[x], key[y]]), e.get_shard(i, 1)[0]]
            assert set(recs) <= hit
            for mode, code in ((2, 5.0), (0, 6.0)):
                got, path = _answer(e, monkeypatch, mode, key)
                assert path == code
                assert np.array_equal(got, want), (recs, mode)
        # the default policy answers too, and a slice never takes k_query
        assert np.array_equal(e.answer_woodruff(dense), plain)
        monkeypatch.setenv("PIR_WD_FUSED", "2")
        with pytest.raises(pir.PirError, match="PIR_WD_FUSED"):
            e.answer_woodruff(dense, 0, N // 2)
    with _engine(pir, 10, efs) as e:   # no tile at this size: forcing k_query fails
        assert e.woodruff_fused_tile == 0
        with pytest.raises(pir.PirError, match="PIR_WD_FUSED"):
            e.answer_woodruff(np.ones(wd_m(10), np.uint8))


@gpu
def test_derivative_n16(pir):
    n, efs = 16, 64
    rng = np.random.default_rng(16)
    rows = rng.integers(0, 256, (1 << n, efs), dtype=np.uint8)
    key = rng.integers(0, 256, wd_m(n), dtype=np.uint8)
    with _engine(pir, n, efs) as e:
        e.set_shard(rows)
        assert np.array_equal(e.answer_woodruff_deriv(key), woodruff_deriv_ref(rows, key))


@gpu
def test_derivative_at_size(pir):
    """n = 20 x 256 B, no full restatement: out[0] is the value answer, and 16 chosen j are
    recomputed on the host from the ~M rows each touches."""
    n, efs = 20, 256
    N, M = 1 << n, wd_m(n)
    rng = np.random.default_rng(20)
    key = rng.integers(1, 256, M, dtype=np.uint8)
    a_last = int(wd_pairs(M, N)[0][-1])
    cut = N - wd_start(M, a_last)            # records of the truncated last row
    assert 0 < cut < M - 1 - a_last
    zero_j = 777
    key[zero_j] = 0
    js = [0, 1, 2, M - 1, M - 2, a_last, a_last - 1, a_last + 1, a_last + cut, a_last + cut + 1,
          zero_j, zero_j + 1, M // 2, M // 3, 100, M - 100]
    assert len(set(js)) == 16
    with _engine(pir, n, efs) as e:
        e.fill_shard_random(2020)
        got = e.answer_woodruff_deriv(key)
        assert got.shape == (M + 1, efs)
        assert np.array_equal(got[0], e.answer_woodruff(key)) and got[0].any()
        for j in js:
            want = np.zeros(efs, np.uint8)
            recs = [(wd_rank(M, a, j), a) for a in range(j)] + \
                   [(wd_rank(M, j, b), b) for b in range(j + 1, M)]
            for i, other in recs:
                if i < N and key[other]:
                    want ^= MUL[int(key[other]), e.get_shard(i, 1)[0]]
            assert np.array_equal(got[1 + j], want), j


@gpu
def test_caller_stream_and_profiling_window(pir):
    """The device forms on a caller's stream, and a profiling window that holds a Woodruff answer
    and a k_query answer (each slot read by its own layout)."""
    n, efs = 19, 1024
    N, M = 1 << n, wd_m(n)
    rng = np.random.default_rng(19)
    key = rng.integers(0, 256, M, dtype=np.uint8)
    tree_key = pir.gen_keys(n, 12345, 2, 1)[0]
    with _engine(pir, n, efs) as e, pir.Engine(2, 1, 6, 16, 1) as caller:
        e.fill_shard_random(77)
        want, dwant = e.answer_woodruff(key), e.answer_woodruff_deriv(key)
        tree_want = e.answer(tree_key)
        d_k, d_r = e.alloc_dev(M + 3), e.alloc_dev((M + 1) * efs)
        e.h2d(d_k + 3, key)   # a key at an odd address
        e.set_profiling(4)
        e.answer_woodruff_dev(d_k + 3, M, 0, N, d_r, stream=caller.stream)
        caller.sync()
        t = e.last_timings()
        # the whole domain at this size: k_query's Woodruff mode (5); a slice: coefficients + scan (6)
        assert e.woodruff_fused_tile
        assert t["fused"] == 5.0 and {"launch", "scan", "reduce", "total"} <= set(t), t
        assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
        assert t["scan"] <= t["total"]
        assert np.array_equal(e.d2h(d_r, efs), want)
        e.answer_woodruff_dev(d_k + 3, M, 0, N // 2, d_r, stream=caller.stream)
        e.answer_woodruff_dev(d_k + 3, M, N // 2, N // 2, d_r + efs, stream=caller.stream)
        caller.sync()
        t = e.last_timings()
        assert t["fused"] == 6.0 and t["scan"] <= t["total"], t
        halves = e.d2h(d_r, 2 * efs).reshape(2, efs)
        assert np.array_equal(halves[0] ^ halves[1], want)
        # Woodruff on the caller's stream, then the tree answer on the engine's, no host sync
        e.answer_woodruff_dev(d_k + 3, M, 0, N, d_r, stream=caller.stream)
        tree_got = e.answer(tree_key)
        caller.sync()
        t = e.last_timings()
        assert t["fused"] == 3.5, t  # the mean of 5.0 (Woodruff) and 2.0 (k_query)
        assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
        assert np.array_equal(tree_got, tree_want)
        assert np.array_equal(e.d2h(d_r, efs), want)
        e.answer_woodruff_deriv_dev(d_k + 3, M, 0, N, d_r, stream=caller.stream)
        caller.sync()
        t = e.last_timings()
        assert t["fused"] == 7.0 and t["scan"] <= t["total"], t
        assert np.array_equal(e.d2h(d_r, (M + 1) * efs).reshape(M + 1, efs), dwant)
        e.free_dev(d_k)
        e.free_dev(d_r)


@gpu
def test_stale_state(pir, monkeypatch):
    """A tree answer, a Woodruff answer, a tree answer on one engine: small (two-kernel path) and
    at the fused size with k_query forced (its LDS ring and slabs after a tree's)."""
    for n, efs, mode in ((10, 48, None), (_fused_n(pir, 256)[0], 256, 2)):
        N, M = 1 << n, wd_m(n)
        rng = np.random.default_rng(n)
        key = rng.integers(0, 256, M, dtype=np.uint8)
        tree_key = pir.gen_keys(n, 321, 2, 1)[0]
        with _engine(pir, n, efs) as e:
            e.fill_shard_random(n)
            rows = e.get_shard(0, N)
            want = woodruff_ref(rows, key)
            if mode is not None:
                monkeypatch.setenv("PIR_WD_FUSED", str(mode))
            t0 = e.answer(tree_key)
            assert np.array_equal(e.answer_woodruff(key), want)
            assert np.array_equal(e.answer(tree_key), t0)
            assert np.array_equal(e.answer_woodruff(key), want)
            monkeypatch.delenv("PIR_WD_FUSED", raising=False)
            assert np.array_equal(e.answer_woodruff(key, 3, 100), woodruff_ref(rows, key, 3, 103))
            assert np.array_equal(e.answer(tree_key), t0) and t0.any()
