"""pir_gen_hollanti_keys[_dev] (include/pir_client.h) without a GPU: every refusal is PIR_EINVAL
before any device call, an empty call is PIR_OK and touches nothing, and a fresh shim process has
pirClientHollantiKeygenOnGpu off, so generateHollantiQuery is the host loop it always was."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle as O
from erasurecodedpir_amd import _lib

EINVAL = -1
HOOK = "_ZN8pir_shim17g_hollanti_keygenE"   # pir_shim::g_hollanti_keygen (pir_server_internal.h)


def test_names():
    import erasurecodedpir_amd as pir
    from erasurecodedpir_amd import client, server
    with open(os.path.join(O.ROOT, "include", "pir_client.h")) as f:
        header = f.read()
    for name in ("pir_gen_hollanti_keys_dev", "pir_gen_hollanti_keys"):
        assert "int %s(int device, uint64_t num_records" % name in header, name
        assert name in _lib.PROTOTYPES, name
    assert "OS CSPRNG" in header and "never a counter or a constant" in header
    with open(os.path.join(O.ROOT, "include", "pir_server.h")) as f:
        assert "void pirClientHollantiKeygenOnGpu(int on);" in f.read()
    assert "pirClientHollantiKeygenOnGpu" in _lib.PROTOTYPES
    assert callable(client.gen_hollanti_keys) and callable(client.gen_hollanti_keys_dev)
    assert pir.gen_hollanti_keys is client.gen_hollanti_keys
    assert callable(server.hollanti_keygen_on_gpu)


GOOD = dict(N=100, idx=(3, 99), K=2, t=2, p=3, nq=2, rho=1, pitch=100, kstride=200, pstride=400)
BAD = {
    "num_keys < 0": dict(K=-1),
    "t < 1": dict(t=0),
    "nq < 1": dict(nq=0),
    "nq > PIR_MAX_ROUNDS": dict(nq=17, kstride=1700, pstride=3400),
    "rho < 1": dict(rho=0),
    "p < 1": dict(p=0),
    "p > PIR_MAX_PARTIES": dict(p=18),
    "t + rho*nq > 255": dict(t=252, rho=2),
    "t + rho*nq > 255, large t": dict(t=2 ** 31 - 1),
    "t + rho*nq > 255, large rho": dict(rho=2 ** 30),
    "num_records == 0": dict(N=0, idx=(0, 0)),
    "num_records > 2^36": dict(N=2 ** 36 + 1, pitch=2 ** 36 + 1, kstride=2 ** 37 + 2,
                               pstride=2 ** 38 + 4),
    "index >= num_records": dict(idx=(3, 100)),
    "null indices": dict(idx=None),
    "null seeds": dict(seeds=None),
    "null keys": dict(out=None),
}
BAD_DEV = {
    "coef_pitch < num_records": dict(pitch=99),
    "key_stride < nq*coef_pitch": dict(kstride=199),
    "party_stride < num_keys*key_stride": dict(pstride=399),
    "key_stride*nq beyond 64 bits": dict(pitch=2 ** 63, kstride=2 ** 63, pstride=2 ** 63),
}


def _call(dev_form, **kw):
    a = dict(GOOD, seeds=b"\x01" * 64, out=True)
    a.update(kw)
    lib = _lib.load()
    idx = None if a["idx"] is None else (ctypes.c_uint64 * len(a["idx"]))(*a["idx"])
    seeds = None if a["seeds"] is None else (ctypes.c_uint8 * 64)(*a["seeds"])
    # a host buffer stands in for the keys: a refused or empty call touches nothing
    buf = np.full(4096, 0xA5, np.uint8)
    out = buf.ctypes.data_as(ctypes.c_void_p) if a["out"] else None
    if dev_form:
        rc = lib.pir_gen_hollanti_keys_dev(0, a["N"], idx, a["K"], a["t"], a["p"], a["nq"],
                                           a["rho"], seeds, out, a["pitch"], a["kstride"],
                                           a["pstride"], None)
    else:
        rc = lib.pir_gen_hollanti_keys(0, a["N"], idx, a["K"], a["t"], a["p"], a["nq"], a["rho"],
                                       seeds, out)
    assert (buf == 0xA5).all()
    return rc


@pytest.mark.parametrize("dev_form", [True, False])
@pytest.mark.parametrize("what", sorted(BAD))
def test_refusals(what, dev_form):
    assert _call(dev_form, **BAD[what]) == EINVAL, what


@pytest.mark.parametrize("what", sorted(BAD_DEV))
def test_stride_refusals(what):
    assert _call(True, **BAD_DEV[what]) == EINVAL, what


@pytest.mark.parametrize("dev_form", [True, False])
def test_no_keys_is_ok(dev_form):
    assert _call(dev_form, K=0) == 0
    assert _call(dev_form, K=0, idx=None, seeds=None, out=None) == 0
    assert _call(dev_form, K=0, t=0) == EINVAL   # the other checks still hold


def test_python_wrappers_refuse():
    from erasurecodedpir_amd import client
    with pytest.raises(_lib.PirError, match="pir_gen_hollanti_keys"):
        client.gen_hollanti_keys(100, [100], 1, 2)
    with pytest.raises(ValueError, match="16 bytes per key"):
        client.gen_hollanti_keys(100, [1, 2], 1, 2, seeds=b"\x00" * 16)
    with pytest.raises(_lib.PirError, match="pir_gen_hollanti_keys_dev"):
        client.gen_hollanti_keys_dev(100, [1], 1, 2, None, 100, 100, 100)
    assert client.gen_hollanti_keys(100, [], 1, 2).shape == (2, 0, 1, 100)


_FRESH = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
from erasurecodedpir_amd import _lib, server as S
hook = lambda: ctypes.c_void_p.in_dll(_lib.load(), sys.argv[2]).value
assert hook() is None, "a fresh process has the switch off"
import test_client_names as tcn
tcn.test_generateHollantiQuery_structure(8, 16, 1, 2, 1, 1)
tcn.test_generateHollantiQuery_structure(8, 20, 1, 4, 2, 2)
S.hollanti_keygen_on_gpu(1)
assert hook() is not None
S.hollanti_keygen_on_gpu(0)
assert hook() is None
tcn.test_generateHollantiQuery_structure(7, 30, 2, 3, 1, 1)
print("fresh shim OK")
"""


def test_fresh_shim_process_has_the_switch_off():
    r = subprocess.run([sys.executable, "-c", _FRESH, os.path.join(O.ROOT, "tests"), HOOK],
                       cwd=O.ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "fresh shim OK" in r.stdout, r.stderr
