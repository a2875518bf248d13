"""CheckMAC record tags, the host side (no GPU): pir_mac_check against Python's hmac, the sizing
of setSystemParams(checkMac = 1) for the served modes, the wire's CheckMAC field, and a pin to
the reference itself (tests/golden/checkmac.json, written by tests/golden/make_golden_checkmac.py
from the compiled reference: OpenSSL's HMAC and generate_encoded_across_file)."""
import hashlib
import hmac

import numpy as np
import pytest

import _oracle as O

REF_KEY = b"1234567812345678"  # client.cpp:19
NEW_SYMBOLS = ["pir_mac_files_dev", "pir_mac_files_rows", "pir_mac_check",
               "pir_engine_encode_across_synthetic_mac", "pirClientTagFiles"]


def _tag(key, payload):
    return hmac.new(key, bytes(payload), hashlib.sha256).digest()


def test_new_symbols_exist():
    import ctypes

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


@pytest.mark.parametrize("n", [1, 55, 56, 64, 1000])
def test_mac_check_accepts_hashlib_tag_and_rejects_flips(pir, n):
    rng = np.random.default_rng(n)
    for key in (REF_KEY, bytes(16), rng.integers(0, 256, 16, dtype=np.uint8).tobytes()):
        payload = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        rec = payload + _tag(key, payload)
        assert pir.mac_check(rec, n, key)
        for j in range(32):  # any single tag byte
            bad = bytearray(rec)
            bad[n + j] ^= 1 << (j % 8)
            assert not pir.mac_check(bytes(bad), n, key), j
        bad = bytearray(rec)  # one payload byte
        bad[n // 2] ^= 0x80
        assert not pir.mac_check(bytes(bad), n, key)


def test_mac_check_bad_arguments(pir):
    import ctypes
    lib = pir.load()
    rec = (ctypes.c_uint8 * 40)()
    key = (ctypes.c_uint8 * 16)()
    assert lib.pir_mac_check(None, 8, key) < 0
    assert lib.pir_mac_check(rec, 8, None) < 0
    assert lib.pir_mac_check(rec, 0, key) < 0
    # host-argument checks of the GPU forms come before any device call
    assert lib.pir_mac_files_rows(0, None, 4, 8, key) < 0
    assert lib.pir_mac_files_rows(0, None, 0, 0, key) < 0
    assert lib.pir_mac_files_dev(0, None, 40, 1, 8, key, None, 40, None) < 0
    one = ctypes.c_void_p(16)
    assert lib.pir_mac_files_dev(0, one, 40, 1, 0, key, one, 40, None) < 0   # payload_bytes == 0
    assert lib.pir_mac_files_dev(0, one, 7, 1, 8, key, one, 40, None) < 0    # pitch < payload
    assert lib.pir_mac_files_dev(0, one, 40, 1, 8, key, one, 31, None) < 0   # tag_pitch < 32


@pytest.mark.parametrize("mode,t,k,r,b", [(0, 1, 2, 1, 0), (1, 1, 2, 1, 0), (4, 1, 2, 1, 1)])
def test_checkmac_sizing(pir, mode, t, k, r, b):
    from erasurecodedpir_amd import server as S
    S.setSystemParams(10, 64, t, k, r, b, 1, 0, mode)
    off = S.params()
    S.setSystemParams(10, 64, t, k, r, b, 1, 1, mode)
    on = S.params()
    assert on["CHECK_MAC"] == 1 and off["CHECK_MAC"] == 0
    assert on["FILE_SIZE_BYTES"] == off["FILE_SIZE_BYTES"] + 32
    assert on["ENCODED_FILE_SIZE_BYTES"] == off["ENCODED_FILE_SIZE_BYTES"] + 32
    assert on["PAYLOAD_SIZE_BYTES"] == off["PAYLOAD_SIZE_BYTES"] == 64
    for name in ("NUM_PARTIES", "NUM_ENCODED_FILES", "NUM_ROUNDS"):
        assert on[name] == off[name], name


def test_wire_encodes_checkmac(pir, monkeypatch):
    from erasurecodedpir_amd import wire
    seen = {}

    class FakeConn:
        def __init__(self, host, port):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            pass

        def call(self, kind, req):
            seen[kind] = req
            return {"ServerLatency": 0}

    monkeypatch.setattr(wire, "Conn", FakeConn)
    wire.setup(("127.0.0.1", 1), 12, 96, 1, 0, check_mac=1)
    assert seen[wire.SETUP_REQUEST]["CheckMAC"] == 1
    assert seen[wire.SETUP_REQUEST]["FileSizeBytes"] == 96
    wire.setup(("127.0.0.1", 1), 12, 96, 1, 0)
    assert seen[wire.SETUP_REQUEST]["CheckMAC"] == 0


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


def test_reference_pin(pir):
    """The reference's own CheckMAC setup: its file 1 and file 300 (payload + OpenSSL tag) and
    every party's shard equal the synthetic database with hashlib tags, encoded by the oracle;
    the shim's initialize_client builds the same files."""
    from erasurecodedpir_amd import server as S
    g = O.golden("checkmac.json")
    a = g["params"]
    L, f, k = a["L"], a["f"], a["k"]
    key = g["mac_key"].encode()
    assert key == REF_KEY
    files = _tagged_synthetic(L, f, key)
    assert files[1].tobytes().hex() == g["file1"]
    assert files[300].tobytes().hex() == g["file300"]
    p = g["globals"]["NUM_PARTIES"]
    assert g["globals"]["ENCODED_FILE_SIZE_BYTES"] == f + 32
    for party in range(1, p + 1):
        shard = O.encode_across(L, f + 32, k, p, party, files.reshape(-1))
        assert O.sha(shard) == g["shard_sha256"][party - 1], party
    S.setSystemParams(L, f, a["t"], k, a["r"], a["b"], a["rho"], 1, a["mode"])
    prm = S.params()
    for name, val in g["globals"].items():
        assert prm[name] == val, name
    cl = S.Client(L, f)
    try:
        for i in (0, 1, 2, 255, 256, 257, 300, (1 << L) - 1):
            assert cl.file(i) == files[i].tobytes(), i
    finally:
        cl.free_client()


def test_initialize_client_tags_every_file(pir):
    from erasurecodedpir_amd import server as S
    L, f = 9, 100
    S.setSystemParams(L, f, 1, 1, 0, 0, 1, 1, 0)
    cl = S.Client(L, f)
    try:
        want = _tagged_synthetic(L, f, REF_KEY)
        for i in range(1 << L):
            assert cl.file(i) == want[i].tobytes(), i
    finally:
        cl.free_client()
