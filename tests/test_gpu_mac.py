"""CheckMAC record tags on the GPU: k_hmac_sha256_files (pir_mac_files_dev / _rows) against
Python's hmac at the SHA-256 padding boundaries, odd pitches and alignments; the synthetic
CheckMAC encode of the engine against the oracle's encode of the tagged files; the shim's
CheckMAC setup end to end (tag every file, GPU setup, query, decode, verify the tag);
pirClientTagFiles; and a CheckMAC SETUP of pir_serve over the wire.  Every comparison is exact
bytes."""
import ctypes
import hashlib
import hmac

import numpy as np
import pytest

import _oracle as O

pytestmark = pytest.mark.gpu

REF_KEY = b"1234567812345678"  # client.cpp:19
KEYS = [REF_KEY, bytes(16), bytes(range(0x80, 0x90))]
NEW_SYMBOLS = ["pir_mac_files_dev", "pir_mac_files_rows", "pir_mac_check",
               "pir_engine_encode_across_synthetic_mac", "pirClientTagFiles"]
GUARD = 80
# the padding boundaries of the 64-byte-prefixed inner message (55/56, 119/120), block edges,
# lengths that are no dword multiple, and the workload's own 992
PAYLOADS = [1, 3, 31, 32, 55, 56, 63, 64, 65, 119, 120, 128, 992, 1001]
COUNTS = [1, 63, 64, 65, 1000]


def _tag(key, payload):
    return hmac.new(key, bytes(payload), hashlib.sha256).digest()


def test_new_symbols_exist():
    import erasurecodedpir_amd as pir
    lib = ctypes.CDLL(pir.LIB_PATH)
    missing = [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing


@pytest.fixture(scope="module")
def pir():
    test_new_symbols_exist()
    import erasurecodedpir_amd as pir
    pir.load()
    return pir


@pytest.fixture(scope="module")
def S(pir):
    from erasurecodedpir_amd import server
    return server


@pytest.fixture(scope="module")
def eng(pir):
    """A small engine: the owner of the device buffers and of the stream the tests tag on."""
    with pir.Engine(2, 1, 4, 16) as e:
        yield e


def _want_tags(host, off, n, pitch, payload, key):
    return [_tag(key, host[off + i * pitch: off + i * pitch + payload]) for i in range(n)]


def _run_case(pir, eng, rng, n, payload, pitch, off, key):
    """n rows `pitch` apart, `off` bytes into the allocation, tagged in place and into a packed
    buffer; everything but the tags must keep its (random) bytes."""
    total = off + n * pitch + GUARD
    host = rng.integers(0, 256, total, dtype=np.uint8)
    tags = _want_tags(host, off, n, pitch, payload, key)
    d = eng.alloc_dev(total)
    d_t = eng.alloc_dev(1 + n * 32 + GUARD)
    try:
        # separate packed tags (tag_pitch = 32), at an odd address when the rows are at one
        t_off = off & 1
        tag_host = rng.integers(0, 256, 1 + n * 32 + GUARD, dtype=np.uint8)
        eng.h2d(d, host)
        eng.h2d(d_t, tag_host)
        pir.mac_files_dev(d + off, pitch, n, payload, key, d_tags=d_t + t_off, tag_pitch=32,
                          stream=eng.stream)
        got_t = eng.d2h(d_t, tag_host.size)
        want_t = tag_host.copy()
        want_t[t_off:t_off + n * 32] = np.frombuffer(b"".join(tags), np.uint8)
        assert np.array_equal(got_t, want_t), "packed tags"
        assert np.array_equal(eng.d2h(d, total), host), "the rows changed under a packed tagging"
        # in place
        pir.mac_files_dev(d + off, pitch, n, payload, key, stream=eng.stream)
        got = eng.d2h(d, total)
        want = host.copy()
        for i in range(n):
            a = off + i * pitch + payload
            want[a:a + 32] = np.frombuffer(tags[i], np.uint8)
        assert np.array_equal(got, want), "in place"
    finally:
        eng.free_dev(d)
        eng.free_dev(d_t)


@pytest.mark.parametrize("payload", PAYLOADS)
def test_kernel_matches_hashlib(pir, eng, payload):
    rng = np.random.default_rng(payload)
    exact, rounded = payload + 32, (payload + 32 + 15) // 16 * 16
    for ci, n in enumerate(COUNTS):
        for pitch in (exact, rounded):
            _run_case(pir, eng, rng, n, payload, pitch, 0, KEYS[(ci + pitch) % 3])


@pytest.mark.parametrize("payload", [64, 65, 992])
def test_kernel_base_offset_one_byte(pir, eng, payload):
    """A base 1 byte into the allocation: byte loads, byte stores, whatever the pitch."""
    rng = np.random.default_rng(1000 + payload)
    _run_case(pir, eng, rng, 65, payload, (payload + 32 + 15) // 16 * 16, 1, REF_KEY)


def test_kernel_dword_rows_with_pitch_beyond_tag(pir, eng):
    """Rows on dword but not 16-byte boundaries, a pitch with guard bytes behind the tag."""
    rng = np.random.default_rng(7)
    _run_case(pir, eng, rng, 130, 100, 100 + 32 + 12, 4, KEYS[2])


def test_zero_files_touch_nothing(pir, eng):
    d = eng.alloc_dev(256)
    try:
        host = np.arange(256, dtype=np.uint8)
        eng.h2d(d, host)
        pir.mac_files_dev(d, 64, 0, 32, REF_KEY, stream=eng.stream)
        assert np.array_equal(eng.d2h(d, 256), host)
    finally:
        eng.free_dev(d)
    assert pir.mac_files(np.zeros((0, 64), np.uint8), 32, REF_KEY).shape == (0, 64)


def test_host_rows_cross_chunks(pir, eng, monkeypatch):
    """3 000 files of 100 + 32 bytes in chunks of 512 files: 5 full chunks and a short one."""
    n, payload = 3000, 100
    monkeypatch.setenv("PIR_MAC_CHUNK_FILES", "512")
    rng = np.random.default_rng(11)
    files = rng.integers(0, 256, (n, payload + 32), dtype=np.uint8)
    before = files.copy()
    pir.mac_files(files, payload, KEYS[2])
    assert np.array_equal(files[:, :payload], before[:, :payload])
    for i in range(n):
        assert files[i, payload:].tobytes() == _tag(KEYS[2], before[i, :payload]), i
    d = eng.alloc_dev(before.size)
    try:
        eng.h2d(d, before.reshape(-1))
        pir.mac_files_dev(d, payload + 32, n, payload, KEYS[2], stream=eng.stream)
        assert np.array_equal(eng.d2h(d, before.size).reshape(n, -1), files)
    finally:
        eng.free_dev(d)


def _tagged_synthetic(L, f, key):
    files = O.synthetic_db(L, f).reshape(1 << L, f)
    tags = {}
    out = np.zeros((1 << L, f + 32), np.uint8)
    out[:, :f] = files
    for i in range(1 << L):
        pb = files[i].tobytes()
        if pb not in tags:
            tags[pb] = np.frombuffer(_tag(key, pb), np.uint8)
        out[i, f:] = tags[pb]
    return out


@pytest.mark.parametrize("L,payload,k,r", [(12, 64, 1, 1), (13, 992, 4, 2), (12, 100, 5, 2)])
def test_encode_across_synthetic_mac(pir, S, L, payload, k, r):
    S.setSystemParams(L, payload, 1, k, r, 0, 1, 1, 0)
    prm = S.params()
    p, n, nq, efs = (prm["NUM_PARTIES"], prm["LOG_NUM_ENCODED_FILES"], prm["NUM_ROUNDS"],
                     prm["ENCODED_FILE_SIZE_BYTES"])
    assert efs == payload + 32
    key = KEYS[2] if k == 5 else REF_KEY
    files = _tagged_synthetic(L, payload, key)
    for party in (2, p):
        want = O.encode_across(L, efs, k, p, party, files.reshape(-1)).reshape(1 << n, efs)
        with pir.Engine(p, party, n, efs, nq) as e:
            e.encode_across_synthetic_mac(1 << L, k, key)
            got = e.get_shard()
            assert np.array_equal(got, want), party
            e.encode_across(1 << L, k, files=files)  # the same tagged files, given on the device
            assert np.array_equal(e.get_shard(), got), party


def test_encode_across_synthetic_mac_needs_a_payload(pir):
    with pir.Engine(2, 1, 4, 32) as e:
        with pytest.raises(pir.PirError):
            e.encode_across_synthetic_mac(16, 1, REF_KEY)


def test_shim_end_to_end(pir, S):
    """setSystemParams(checkMac = 1) -> Client (tagged files) -> GPU setup of every party ->
    queries answered by all but the first r servers -> decode -> the tag verifies."""
    L, payload, k, r = 12, 96, 2, 1
    S.setSystemParams(L, payload, 1, k, r, 0, 1, 1, 0)
    prm = S.params()
    p, n, nq, efs = (prm["NUM_PARTIES"], prm["LOG_NUM_ENCODED_FILES"], prm["NUM_ROUNDS"],
                     prm["ENCODED_FILE_SIZE_BYTES"])
    assert prm["FILE_SIZE_BYTES"] == payload + 32 == efs
    cl = S.Client(L, payload)
    want = _tagged_synthetic(L, payload, REF_KEY)
    for i in range(1 << L):
        assert cl.file(i) == want[i].tobytes(), i
    servers = []
    for q in range(p):
        sv = S.Server(q + 1, n, efs)
        cl.encode_across_files_server(sv)
        servers.append(sv)
    try:
        for idx in (1, 777):
            keys = cl.generate_opt_DPF_tree_query(idx)
            er = [0 if q < r else 1 for q in range(p)]
            ans = [servers[q].runOptimizedDPFTreeQuery(keys[q], nq) for q in range(p) if er[q]]
            rec = cl.assembleDPFTreeQueryResponses(er, np.stack(ans))
            assert rec.tobytes() == want[idx].tobytes(), idx
            assert pir.mac_check(rec, payload, REF_KEY)
            ans[1] = ans[1].copy()
            ans[1][0, 5] ^= 0x40  # one flipped response byte
            bad = cl.assembleDPFTreeQueryResponses(er, np.stack(ans))
            assert not pir.mac_check(bad, payload, REF_KEY)
    finally:
        for sv in servers:
            sv.freeServer()
        cl.free_client()


def test_client_tag_files(pir, S):
    """pirClientTagFiles: the caller's own payloads, retagged on the GPU under the client's key."""
    L, payload = 11, 70
    S.setSystemParams(L, payload, 1, 1, 0, 0, 1, 1, 0)
    fs = S.params()["FILE_SIZE_BYTES"]
    cl = S.Client(L, payload)
    try:
        rng = np.random.default_rng(3)
        mine = rng.integers(0, 256, (1 << L, payload), dtype=np.uint8)
        for i in range(1 << L):
            ctypes.memmove(cl.c.unencoded_files[i], mine[i].ctypes.data, payload)
        cl.tag_files()
        for i in range(1 << L):
            f = cl.file(i)
            assert len(f) == fs and f[:payload] == mine[i].tobytes(), i
            assert f[payload:] == _tag(REF_KEY, mine[i]), i
    finally:
        cl.free_client()


def test_pir_serve_checkmac_loopback(pir, S):
    """SETUP with CheckMAC = 1 (FileSizeBytes counts the tag) in mode 0; decoded records carry
    a tag that verifies; the same SETUP in mode 3 is refused and the server keeps answering."""
    from erasurecodedpir_amd import wire
    from test_wire import Servers, _synthetic
    L, payload, k, r = 12, 64, 1, 0
    f = payload + 32
    with Servers(2) as sv:
        for addr in sv.addrs:
            assert wire.setup(addr, L, f, k, r, check_mac=1)["ServerLatency"] >= 0
        for idx in (1, 5, (1 << L) - 1):
            rec, _, er = wire.tree_query(sv.addrs, idx, L, f, k, r, check_mac=1)
            assert er == [1, 1] and rec.size == f
            assert np.array_equal(rec[:payload], _synthetic(idx, payload)), idx
            assert pir.mac_check(rec, payload, REF_KEY), idx
            assert rec[payload:].tobytes() == _tag(REF_KEY, rec[:payload])
        with pytest.raises(wire.WireError):
            wire.setup(sv.addrs[0], L, f, 2, 1, mode=3, check_mac=1)
        with pytest.raises(wire.WireError):
            wire.setup(sv.addrs[0], L, 32, k, r, check_mac=1)  # no payload left
        rec, _, _ = wire.tree_query(sv.addrs, 9, L, f, k, r, check_mac=1)  # still serving
        assert pir.mac_check(rec, payload, REF_KEY)
        assert np.array_equal(rec[:payload], _synthetic(9, payload))
