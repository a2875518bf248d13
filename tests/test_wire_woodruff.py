"""The Woodruff mode over the wire: `pir_serve` parties on loopback, SETUP Mode 5 (synthetic
database, k = 1: the shard is the database, encoded within files on the GPU), one
WOODRUFF_SEARCH per party with genWoodruffQuery's keys, one server left out (R = 1), and
assembleWoodruffResponses returns the record.  Every answer equals the numpy restatement of
tests/test_woodruff.py byte for byte; the M entries behind the answer are zero."""
import numpy as np
import pytest

from erasurecodedpir_amd import wire
from test_shamir import synth_files
from test_wire import Servers, serve_bin  # noqa: F401  (the fixture)
from test_woodruff import wd_m, woodruff_ref

pytestmark = pytest.mark.gpu


def test_woodruff_over_the_wire(serve_bin):  # noqa: F811
    from erasurecodedpir_amd import server as S
    L, f, t, r, index = 10, 48, 1, 1, 1   # 2^10 records of 48 B; record 1 is 0, 1, 2, ...
    N, M = 1 << L, wd_m(L)
    S.set_woodruff_derivative(False)
    S.setSystemParams(L, f, t, 1, r, 0, 1, 0, 5)
    p = S.params()["NUM_PARTIES"]
    assert p == 2 * t + 1 + r and S.params()["WOODRUFF_M"] == M
    v = np.random.default_rng(5).integers(0, 256, (t, M), dtype=np.uint8)
    keys = S.genWoodruffQuery(index, t, p, M, v)
    dropped = 2
    alive = [q for q in range(1, p + 1) if q != dropped]
    rows = synth_files(N, f)
    with Servers(len(alive), parties=alive) as sv:
        for addr in sv.addrs:
            wire.setup(addr, L, f, 1, r, 1, mode=5, t=t)
        resps = [wire.woodruff_query(addr, keys[q - 1]) for q, addr in zip(alive, sv.addrs)]
        with pytest.raises(wire.WireError, match="bad key"):
            wire.woodruff_query(sv.addrs[0], keys[0][:-1])
        with pytest.raises(wire.WireError, match="Woodruff mode needs K = 1"):
            wire.setup(sv.addrs[0], L, f, 2, r, 1, mode=5, t=t)
        # a later tree setup on the first party: the Woodruff request no longer matches the mode
        wire.setup(sv.addrs[0], L, f, 1, 0, 1, mode=0, t=1)
        with pytest.raises(wire.WireError, match="does not match the setup's mode"):
            wire.woodruff_query(sv.addrs[0], keys[0])
    answers = []
    for q, resp in zip(alive, resps):
        got = [np.frombuffer(b, np.uint8) for b in resp["Results"]]
        assert len(got) == M + 1 and all(g.size == f for g in got)
        assert "PartyIndex" not in resp and resp["ServerLatency"] >= 0
        assert np.array_equal(got[0], woodruff_ref(rows, keys[q - 1])), q
        assert not np.stack(got[1:]).any()
        answers.append(got[0])
    erasure = [0 if q == dropped else 1 for q in range(1, p + 1)]
    rec = S.assembleWoodruffResponses(erasure, np.stack(answers)[:, None, :], v)
    assert np.array_equal(rec, rows[index]) and rec.any()
