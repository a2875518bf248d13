"""The Shamir sqrt(N) mode (mode 2): runOptShamirDPFQuery[Thread] (src/c/server.cpp:203-302)
served from the device-resident value and Hermite rows.

The checker is a vectorised numpy restatement of the four formulas of the mode (row sums, column
sums, Hermite total, value total over GF(2^8)/0x11d); the CPU tests pin it against the
reference's own answers (tests/golden/shamir.json, from tests/golden/make_golden_shamir.py) and
the GPU tests compare the engine, the shim and the encode against it byte for byte.  The
arithmetic is exact: no tolerance anywhere."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle as O

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------- the checker
def _gf_tables():
    exp, log = np.zeros(512, np.int64), np.zeros(256, np.int64)
    x = 1
    for i in range(255):
        exp[i] = x
        log[x] = i
        x <<= 1
        if x & 0x100:
            x ^= 0x11d
    exp[255:510] = exp[:255]
    a = np.arange(256)
    mul = exp[(log[a][:, None] + log[a][None, :])].astype(np.uint8)
    mul[0, :] = 0
    mul[:, 0] = 0
    return mul


MUL = _gf_tables()


def gf_pow(a, e):
    r = 1
    for _ in range(e):
        r = int(MUL[r, a])
    return r


def dims(n):
    x = (n + 1) // 2
    return x, n - x, 1 << x, 1 << (n - x)


def xor_reduce(a, axis):
    return np.bitwise_xor.reduce(a, axis=axis)


def shamir_ref(rows, keys, n, lo=0, hi=None):
    """rows (2N, efs): values then Hermite rows; keys (nq, X + Y) -> (nq, X + Y + 2, efs) over
    the records [lo, hi)."""
    x, y, X, Y = dims(n)
    N = 1 << n
    hi = N if hi is None else hi
    rows = np.asarray(rows, np.uint8).reshape(2 * N, -1)
    efs = rows.shape[1]
    keep = np.zeros(N, bool)
    keep[lo:hi] = True
    A = np.where(keep[:, None], rows[:N], 0).astype(np.uint8).reshape(X, Y, efs)
    H = np.where(keep[:, None], rows[N:], 0).astype(np.uint8).reshape(X, Y, efs)
    keys = np.asarray(keys, np.uint8).reshape(-1, X + Y)
    out = np.zeros((keys.shape[0], X + Y + 2, efs), np.uint8)
    for a, key in enumerate(keys):
        ky, kx = key[:X], key[X:]
        out[a, :X] = xor_reduce(MUL[kx[None, :, None], A], 1)
        out[a, X:X + Y] = xor_reduce(MUL[ky[:, None, None], A], 0)
        c = MUL[ky[:, None], kx[None, :]]
        out[a, X + Y] = xor_reduce(MUL[c[:, :, None], H].reshape(N, efs), 0)
        out[a, X + Y + 1] = xor_reduce(MUL[c[:, :, None], A].reshape(N, efs), 0)
    return out


def synth_files(nf, fb):
    """client.cpp:16-33: file v = the byte v & 0xff, file 1 = 0, 1, 2, ..."""
    f = np.repeat((np.arange(nf) & 0xff).astype(np.uint8)[:, None], fb, 1)
    if nf > 1:
        f[1] = np.arange(fb) & 0xff
    return f


def encode_ref(files, fb, k, efs, party, N):
    """(value rows, Hermite rows), N x efs each (client.cpp:43-68)."""
    nf = files.shape[0]
    pad = np.zeros((N, k * efs), np.uint8)
    pad[:nf, :fb] = files[:, :fb]
    parts = pad.reshape(N, k, efs)
    val, her = np.zeros((N, efs), np.uint8), np.zeros((N, efs), np.uint8)
    for j in range(k):
        val ^= MUL[gf_pow(party, j), parts[:, j]]
        if j % 2 == 1:
            her ^= MUL[gf_pow(party, j - 1), parts[:, j]]
    return val, her


# -------------------------------------------------------------------------------- CPU tests
CASES = O.golden("shamir.json")["cases"]
IDS = ["L%d_f%d_k%d" % (c["L"], c["f"], c["k"]) for c in CASES]


@pytest.fixture
def shamir_mode():
    from erasurecodedpir_amd import server as S
    S.enable_shamir_mode(True)
    yield S
    S.enable_shamir_mode(False)


def _setup(S, case):
    S.setSystemParams(case["L"], case["f"], case["t"], case["k"], 0, 0, case["rho"], 0, 2)


def _hex(h, shape):
    return np.frombuffer(bytes.fromhex(h), np.uint8).reshape(shape)


def _host_rows(S, case, party, monkeypatch):
    """The 2N rows of `party` after the shim's host encode."""
    monkeypatch.setenv("PIR_SHIM_HOST_SETUP", "1")
    prm = case["params"]
    N, efs = prm["NUM_ENCODED_FILES"], prm["ENCODED_FILE_SIZE_BYTES"]
    cl = S.Client(case["L"], case["f"])
    sv = S.Server(party, case["L"], efs, 0, case["T"])
    try:
        assert sv.rows == 2 * N
        cl.encode_within_files_server(sv)
        return np.stack([sv.read_row(i) for i in range(2 * N)])
    finally:
        sv.freeServer()
        cl.free_client()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_globals_match_reference(shamir_mode, case):
    _setup(shamir_mode, case)
    got = shamir_mode.params()
    assert {k: got[k] for k in case["params"]} == case["params"]
    # and every other mode leaves the Hermite flag clear again
    shamir_mode.setSystemParams(case["L"], case["f"], case["t"], case["k"], 0, 0, case["rho"], 0, 3)
    assert shamir_mode.params()["IS_HERMITE"] == 0


def test_mode_is_opt_in_per_process():
    code = ("from erasurecodedpir_amd import server as S; "
            "S.setSystemParams(6, 16, 1, 2, 0, 0, 1, 0, 2)")
    r = subprocess.run([sys.executable, "-c", code], cwd=O.ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "outside the engine's scope" in r.stderr
    assert "pirEnableShamirMode" in r.stderr
    code = ("from erasurecodedpir_amd import server as S; S.enable_shamir_mode(); "
            "S.setSystemParams(6, 16, 1, 2, 0, 0, 1, 0, 2); print(S.params()['IS_HERMITE'])")
    r = subprocess.run([sys.executable, "-c", code], cwd=O.ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split()[-1] == "1", r.stderr
    code = ("from erasurecodedpir_amd import server as S; S.enable_shamir_mode(); "
            "S.setSystemParams(6, 16, 1, 2, 0, 0, 1, 1, 2)")  # CheckMAC keeps refusing
    r = subprocess.run([sys.executable, "-c", code], cwd=O.ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "CheckMAC" in r.stderr


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_encoded_rows_match_reference(shamir_mode, case, monkeypatch):
    _setup(shamir_mode, case)
    prm = case["params"]
    for q in range(1, prm["NUM_PARTIES"] + 1):
        rows = _host_rows(shamir_mode, case, q, monkeypatch)
        assert hashlib.sha256(rows.tobytes()).hexdigest() == case["shard_sha256"][str(q)], q
        val, her = encode_ref(synth_files(prm["NUM_FILES"], case["f"]), case["f"], case["k"],
                              prm["ENCODED_FILE_SIZE_BYTES"], q, prm["NUM_ENCODED_FILES"])
        assert np.array_equal(rows, np.concatenate([val, her])), q  # pins encode_ref too


def test_response_len_matches_shim():
    from erasurecodedpir_amd import engine as E, server as S
    for n in range(0, 25):
        x, y, X, Y = dims(n)
        for efs in (1, 5, 16, 30, 1024):
            assert E.shamir_response_len(n, efs) == S.calcShamirResponseLength(n, efs) \
                == (X + Y + 2) * efs
        assert S.calcShamirDPFKeyLength(n) == X + Y


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_reproduces_reference_answers(shamir_mode, case, monkeypatch):
    _setup(shamir_mode, case)
    prm = case["params"]
    n, N, efs, nq = prm["LOG_NUM_ENCODED_FILES"], prm["NUM_ENCODED_FILES"], \
        prm["ENCODED_FILE_SIZE_BYTES"], prm["NUM_ROUNDS"]
    rows = _host_rows(shamir_mode, case, case["party"], monkeypatch)
    keys = _hex(case["keys"], (nq, case["key_len"]))
    want = _hex(case["answer"], (nq, case["key_len"] + 2, efs))
    assert np.array_equal(shamir_ref(rows, keys, n), want)
    assert case["answer_slices"] == case["answer"]
    acc = np.zeros_like(want)
    T = case["T"]
    for t in range(T):
        acc ^= shamir_ref(rows, keys, n, t * N // T, (t + 1) * N // T)
    assert np.array_equal(acc, want)


def test_tsan_harness_still_links(tmp_path):
    """pir_server.cpp alone against the stub engine (today's pir_engine_* names only): the
    Shamir unit must stay out of it."""
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


def _engine(pir, n, efs, nq, **kw):
    """A Shamir engine: value rows [0, N), Hermite rows [N, 2N)."""
    return pir.Engine(2, 1, n + 1, efs, nq, **kw)


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_goldens_through_the_shim(shamir_mode, case):
    """GPU setup (rows still zero) -> runOptShamirDPFQuery == the reference; T Thread slices +
    assemble == the same."""
    S = shamir_mode
    _setup(S, case)
    prm = case["params"]
    N, efs, nq = prm["NUM_ENCODED_FILES"], prm["ENCODED_FILE_SIZE_BYTES"], prm["NUM_ROUNDS"]
    keys = _hex(case["keys"], (nq, case["key_len"]))
    want = _hex(case["answer"], (nq, case["response_len"]))
    cl = S.Client(case["L"], case["f"])
    sv = S.Server(case["party"], case["L"], efs, 0, case["T"])
    try:
        cl.encode_within_files_server(sv)
        assert np.array_equal(sv.runOptShamirDPFQuery(keys), want)
        T = case["T"]
        parts = np.stack([sv.runOptShamirDPFQueryThread(keys, t, t * N // T, (t + 1) * N // T)
                          for t in range(T)])
        assert np.array_equal(S.assembleShamirQueryThreadResults(sv, parts), want)
        # the device rows are the reference's
        rows = np.stack([sv.read_row(i) for i in range(2 * N)])
        assert hashlib.sha256(rows.tobytes()).hexdigest() == \
            case["shard_sha256"][str(case["party"])]
    finally:
        sv.freeServer()
        cl.free_client()


# (n, EFS, rounds): odd and even n, records below / at / above a wave row (1 KiB), padded pitch
# (8, 30, 100, 1040), one chunk per record and many, 1 / 2 / 3 / 4+1 / 4x4 rounds per pass
# group, more matrix rows than workgroups and fewer.  The answer has one path (rows pass, strips
# pass, Hermite scan) on every shape, so there is no switch-over shape to add; (3, 48, 4) adds
# the 3-round instance's neighbour (a full group of 4) and (7, 17, 7) a 4 + 3 split.
SHAPES = [(0, 16, 1), (1, 8, 1), (4, 8, 1), (5, 30, 3), (9, 100, 2), (10, 256, 1), (11, 1024, 2),
          (12, 1040, 1), (13, 64, 5), (13, 2048, 1), (14, 1024, 1), (10, 16, 16), (3, 48, 4),
          (7, 17, 7)]


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_efs%d_r%d" % s)
def test_engine_matches_restatement(pir, shape):
    n, efs, nq = shape
    x, y, X, Y = dims(n)
    rng = np.random.default_rng(1000 + 31 * n + efs + nq)
    rows = rng.integers(0, 256, (2 << n, efs), dtype=np.uint8)
    keys = rng.integers(0, 256, (nq, X + Y), dtype=np.uint8)
    with _engine(pir, n, efs, nq) as e:
        e.set_shard(rows)
        assert e.shamir_key_len == X + Y and e.shamir_response_len == (X + Y + 2) * efs
        got = e.answer_shamir(keys)
    assert np.array_equal(got, shamir_ref(rows, keys, n))


@gpu
def test_ranges(pir):
    n, efs, nq = 7, 24, 2
    x, y, X, Y = dims(n)  # 16 x 8
    N = 1 << n
    rng = np.random.default_rng(7)
    rows = rng.integers(0, 256, (2 * N, efs), dtype=np.uint8)
    keys = rng.integers(0, 256, (nq, X + Y), dtype=np.uint8)
    with _engine(pir, n, efs, nq) as e:
        e.set_shard(rows)
        for lo, hi in [(2 * Y, 6 * Y),   # whole matrix rows
                       (5, 35),          # cuts its first and last matrix row
                       (3, 6),           # inside one matrix row
                       (77, 78),         # one record
                       (N - 1, N), (0, 1)]:
            assert np.array_equal(e.answer_shamir(keys, lo, hi - lo),
                                  shamir_ref(rows, keys, n, lo, hi)), (lo, hi)
        for lo in (0, 10, N):            # empty
            assert not e.answer_shamir(keys, lo, 0).any()
        acc = np.zeros((nq, X + Y + 2, efs), np.uint8)
        for lo, hi in [(0, 13), (13, 90), (90, N)]:
            acc ^= e.answer_shamir(keys, lo, hi - lo)
        assert np.array_equal(acc, e.answer_shamir(keys))
        assert np.array_equal(acc, shamir_ref(rows, keys, n))
        with pytest.raises(pir.PirError):
            e.answer_shamir(keys, 1, N)


@gpu
@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_encode_hermite(pir, k):
    n, fb, party = 5, 37, 3  # 37 is no multiple of 2, 3, 5
    N = 1 << n
    efs = -(-fb // k)
    rng = np.random.default_rng(k)
    for nf, files in [(N, rng.integers(0, 256, (N, fb), dtype=np.uint8)),
                      (N - 3, rng.integers(0, 256, (N - 3, fb), dtype=np.uint8)),
                      (N, None)]:
        src = synth_files(nf, fb) if files is None else files
        val, her = encode_ref(src, fb, k, efs, party, N)
        with _engine(pir, n, efs, 1) as e:
            e.encode_within(nf, fb, k, files=files, party=party)
            before = e.get_shard(0, N)
            assert np.array_equal(before, val)
            e.encode_hermite(nf, fb, k, files=files, party=party)
            assert np.array_equal(e.get_shard(N, N), her)
            assert np.array_equal(e.get_shard(0, N), before)  # the value rows are untouched
        if k == 1:
            assert not her.any()


@gpu
def test_indicator_keys_at_size(pir):
    """n = 20, 256 B, no oracle: kx = c1 e_gamma, ky = c2 e_delta pick single records."""
    n, efs, nq = 20, 256, 2
    x, y, X, Y = dims(n)
    N = 1 << n
    picks = [(5, 1000, 0x53, 0xca), (X - 1, Y - 1, 0x02, 0x8e)]  # (delta, gamma, c1, c2)
    keys = np.zeros((nq, X + Y), np.uint8)
    for a, (d, g, c1, c2) in enumerate(picks):
        keys[a, d] = c2
        keys[a, X + g] = c1
    with _engine(pir, n, efs, nq) as e:
        e.fill_shard_random(2020)
        got = e.answer_shamir(keys)
        for a, (d, g, c1, c2) in enumerate(picks):
            col = np.stack([e.get_shard(dd * Y + g, 1)[0] for dd in range(X)])
            row = e.get_shard(d * Y, Y)
            h = e.get_shard(N + d * Y + g, 1)[0]
            c12 = int(MUL[c1, c2])
            assert np.array_equal(got[a, :X], MUL[c1, col]), a
            assert np.array_equal(got[a, X:X + Y], MUL[c2, row]), a
            assert np.array_equal(got[a, X + Y], MUL[c12, h]), a
            assert np.array_equal(got[a, X + Y + 1], MUL[c12, row[g]]), a
            assert col.any() and h.any()


@gpu
def test_byzantine(pir, shamir_mode):
    n, efs, nq = 6, 16, 2
    x, y, X, Y = dims(n)
    N = 1 << n
    rng = np.random.default_rng(3)
    rows = rng.integers(0, 256, (2 * N, efs), dtype=np.uint8)
    keys = rng.integers(0, 256, (nq, X + Y), dtype=np.uint8)
    want = shamir_ref(rows, keys, n)
    with _engine(pir, n, efs, nq, is_byzantine=True) as e:
        e.set_shard(rows)
        a, b = e.answer_shamir(keys), e.answer_shamir(keys)
        assert not np.array_equal(a, want) and not np.array_equal(a, b)
        assert np.array_equal(e.answer_shamir(keys, 0, N - 1) ^ e.answer_shamir(keys, N - 1, 1),
                              want)
    # the shim: the whole-domain call is random, the Thread form honest even over [0, N)
    S = shamir_mode
    S.setSystemParams(n, efs, 1, 1, 0, 0, 1, 0, 2)
    nq1 = S.params()["NUM_ROUNDS"]
    sv = S.Server(1, n, efs, 1, 1)
    try:
        assert sv.rows == 2 * N
        sv.write_rows(rows)
        k1 = keys[:nq1]
        honest = sv.runOptShamirDPFQueryThread(k1, 0, 0, N)
        assert np.array_equal(honest.reshape(nq1, -1, efs), want[:nq1])
        assert not np.array_equal(sv.runOptShamirDPFQuery(k1), honest)
    finally:
        sv.freeServer()


@gpu
def test_caller_stream_and_profiling_window(pir):
    """The device form on a caller's stream, and a profiling window that holds a Shamir answer
    and a k_query answer (each slot read by its own layout)."""
    n, efs, nq = 18, 1024, 1
    x, y, X, Y = dims(n)
    rng = np.random.default_rng(18)
    keys = rng.integers(0, 256, (nq, X + Y), dtype=np.uint8)
    tree_key = pir.gen_keys(n + 1, 12345, 2, nq)[0]
    with _engine(pir, n, efs, nq) as e, pir.Engine(2, 1, 6, 16, 1) as caller:
        e.fill_shard_random(77)
        want = e.answer_shamir(keys)
        tree_want = e.answer(tree_key)
        rl = e.shamir_response_len
        d_k, d_r = e.alloc_dev(keys.size), e.alloc_dev(nq * rl)
        e.h2d(d_k, keys.reshape(-1))
        e.set_profiling(4)
        e.answer_shamir_dev(d_k, X + Y, 0, 1 << n, d_r, stream=caller.stream)
        caller.sync()
        t = e.last_timings()
        assert t["fused"] == 4.0 and {"launch", "scan", "reduce", "total"} <= set(t), t
        assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
        assert t["scan"] <= t["total"]
        assert np.array_equal(e.d2h(d_r, nq * rl).reshape(want.shape), want)
        # Shamir on the caller's stream, then the tree answer on the engine's, no host sync between
        e.answer_shamir_dev(d_k, X + Y, 0, 1 << n, d_r, stream=caller.stream)
        tree_got = e.answer(tree_key)
        caller.sync()
        t = e.last_timings()
        assert t["fused"] == 3.0, t  # the mean of 4.0 (Shamir) and 2.0 (k_query)
        assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
        assert np.array_equal(tree_got, tree_want)
        assert np.array_equal(e.d2h(d_r, nq * rl).reshape(want.shape), want)
        e.free_dev(d_k)
        e.free_dev(d_r)


@gpu
def test_partition_engine_refuses(pir):
    with pir.Engine(2, 1, 8, 16, 1, log_num_partitions=1, partition_index=0) as e:
        with pytest.raises(pir.PirError, match="split shard"):
            e.answer_shamir(np.zeros((1, e.shamir_key_len), np.uint8), 0, 1)
        with pytest.raises(pir.PirError, match="split shard"):
            e.encode_hermite(4, 16, 1)


@gpu
def test_stale_state(pir):
    """Two different shards and keys back to back on one engine, a range call between them."""
    n, efs, nq = 9, 48, 3
    x, y, X, Y = dims(n)
    rng = np.random.default_rng(99)
    with _engine(pir, n, efs, nq) as e:
        for _ in range(2):
            rows = rng.integers(0, 256, (2 << n, efs), dtype=np.uint8)
            keys = rng.integers(0, 256, (nq, X + Y), dtype=np.uint8)
            e.set_shard(rows)
            assert np.array_equal(e.answer_shamir(keys), shamir_ref(rows, keys, n))
            assert np.array_equal(e.answer_shamir(keys, 100, 17),
                                  shamir_ref(rows, keys, n, 100, 117))
            assert np.array_equal(e.answer_shamir(keys), shamir_ref(rows, keys, n))
