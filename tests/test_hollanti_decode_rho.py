"""assembleHollantiResponses with RHO parts recovered a round (RHO > 1), without a GPU: the
servers are emulated by the oracle's scan over numpy encode-within shards, the keys come from the
shim's host generateHollantiQuery.  Round i has to peel the i*RHO parts of the earlier rounds at
the exponents its own secret coefficient puts them at (the reference's decode, marked "FIX THIS"
at client.cpp:524, peels one part a round and is right for RHO == 1 only)."""
import numpy as np
import pytest

import _oracle as O


def _shards(L, f, k, efs, p):
    files = O.synthetic_db(L, f).reshape(1 << L, f)
    pad = np.zeros((1 << L, k * efs), np.uint8)
    pad[:, :f] = files
    out = []
    for q in range(1, p + 1):
        sh = np.zeros((1 << L, efs), np.uint8)
        for j in range(k):
            tab = np.array([O.gf_mul(x, O.gf_pow(q, j)) for x in range(256)], np.uint8)
            sh ^= tab[pad[:, j * efs:(j + 1) * efs]]
        out.append(sh.reshape(-1))
    return files, out


@pytest.mark.parametrize("L,f,t,k,r,rho", [(8, 20, 1, 4, 2, 2), (8, 30, 2, 6, 1, 3),
                                           (8, 33, 1, 4, 1, 2), (7, 30, 2, 3, 1, 1)])
def test_decode_with_rho_parts_a_round(L, f, t, k, r, rho):
    from erasurecodedpir_amd import server as S
    S.setSystemParams(L, f, t, k, r, 0, rho, 0, 3)
    prm = S.params()
    p, nq, N = prm["NUM_PARTIES"], prm["NUM_ROUNDS"], prm["NUM_ENCODED_FILES"]
    efs = prm["ENCODED_FILE_SIZE_BYTES"]
    assert nq == k // rho
    files, shards = _shards(L, f, k, efs, p)
    for idx in (1, N - 56):
        keys = S.generateHollantiQuery(idx)
        ans = [O.scan(keys[q], shards[q], efs) for q in range(p)]
        for first in (0, 1, p - 1):        # the R servers dropped: first, first + 1, ...
            er = [1] * p
            for i in range(r):
                er[(first + i) % p] = 0
            dec = S.assembleHollantiResponses(er, np.stack([ans[q] for q in range(p) if er[q]]))
            assert np.array_equal(dec, files[idx]), (idx, first)
