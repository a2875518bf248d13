"""The Shamir sqrt(N) mode over the wire: two `pir_serve` parties on loopback, SETUP Mode 2
(synthetic database, value and Hermite rows encoded on the GPU), one SHAMIR_SEARCH per party.
The answers equal the engine's own for the same synthetic setup and the numpy restatement of
tests/test_shamir.py, byte for byte."""
import numpy as np
import pytest

from erasurecodedpir_amd import wire
from test_shamir import dims, encode_ref, shamir_ref, synth_files
from test_wire import Servers, serve_bin  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def test_shamir_over_the_wire(serve_bin):  # noqa: F811
    import erasurecodedpir_amd as pir
    L, f, t, k, rho = 10, 128, 1, 2, 1   # 2^10 records of 64 B, NUM_ROUNDS = 2
    N, efs, nq = 1 << L, f // k, k // rho
    x, y, X, Y = dims(L)
    keys = np.random.default_rng(10).integers(0, 256, (nq, X + Y), dtype=np.uint8)
    parties = (1, 2)
    with Servers(2, parties=parties) as sv:
        for addr in sv.addrs:
            wire.setup(addr, L, f, k, 0, rho, mode=2, t=t)
        resps = [wire.shamir_query(addr, keys) for addr in sv.addrs]
        with pytest.raises(wire.WireError, match="bad key"):
            wire.shamir_query(sv.addrs[0], keys[:, :-1])
        # a later tree setup on party 1: the Shamir request no longer matches the mode
        wire.setup(sv.addrs[0], L, f, 1, 0, 1, mode=0, t=1)
        with pytest.raises(wire.WireError, match="does not match the setup's mode"):
            wire.shamir_query(sv.addrs[0], keys)
    for q, resp in zip(parties, resps):
        got = np.stack([np.frombuffer(b, np.uint8) for b in resp["Results"]])
        assert got.shape == (nq, (X + Y + 2) * efs)
        assert "PartyIndex" not in resp and resp["ServerLatency"] >= 0
        with pir.Engine(2, 1, L + 1, efs, nq) as e:
            e.encode_within(N, f, k, party=q)
            e.encode_hermite(N, f, k, party=q)
            own = e.answer_shamir(keys)
        assert np.array_equal(got.reshape(own.shape), own), q
        val, her = encode_ref(synth_files(N, f), f, k, efs, q, N)
        assert np.array_equal(own, shamir_ref(np.concatenate([val, her]), keys, L)), q
