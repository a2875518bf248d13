"""GPU key generation for Hollanti queries (pir_gen_hollanti_keys[_dev], k_hollanti_keys).

The reference here is a numpy restatement of the key stream as include/pir_client.h defines it,
over the oracle's G (AES-128-CTR), gf_mul and gf_pow -- written from the definition, not from the
kernel:

    key[q][a][x] = (XOR_{m<t} rnd[a][m][x] * (q+1)^m) ^ ([x == index] * (q+1)^(t + (a+1) rho - 1))
    sk = G(seed, 16 nq t),  rnd[a][m] = G(sk[16 (a t + m) : +16], N)

Every comparison is exact (GF(2^8) arithmetic and a block cipher: no tolerance anywhere)."""
import ctypes

import numpy as np
import pytest

import _oracle as O
from test_client_names import _interp_coeffs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pir():
    import erasurecodedpir_amd as pir
    pir.load()
    return pir


@pytest.fixture(scope="module")
def dev(pir):
    """a small engine: device memory, copies and a stream for the device form"""
    with pir.Engine(2, 1, 6, 16, 1) as e:
        yield e


_MUL = {}


def _mul_table(c):
    """x -> c * x over GF(2^8)/0x11d"""
    if c not in _MUL:
        _MUL[c] = np.array([O.gf_mul(c, x) for x in range(256)], np.uint8)
    return _MUL[c]


def restate(N, index, t, p, nq, rho, seed):
    """(p, nq, N): the definition, term by term"""
    sk = O.G(seed, 16 * nq * t)
    out = np.zeros((p, nq, N), np.uint8)
    for a in range(nq):
        rnd = [O.G(sk[16 * (a * t + m):16 * (a * t + m) + 16], N) for m in range(t)]
        for q in range(p):
            v = np.zeros(N, np.uint8)
            for m in range(t):
                v ^= _mul_table(O.gf_pow(q + 1, m))[rnd[m]]
            v[index] ^= O.gf_pow(q + 1, t + (a + 1) * rho - 1)
            out[q, a] = v
    return out


def _seeds(K, salt):
    return np.random.default_rng(1000 + salt).integers(0, 256, 16 * K, dtype=np.uint8).tobytes()


def _indices(N):
    """0, N - 1 and one inside the (partial) last AES block"""
    last = 16 * ((N - 1) // 16)
    return [0, N - 1, last + (N - 1 - last) // 2]


SHAPES = [(5, 1, 2, 1, 1), (1000, 1, 3, 1, 1), (4097, 2, 5, 2, 1),
          (4096 + 64 * 3 + 7, 3, 8, 3, 2), (2 ** 20 + 17, 1, 2, 1, 1)]
_cache = {}


def case(i):
    """shape i: its seeds, indices and restatement, computed once, shared, never changed"""
    if i not in _cache:
        N, t, p, nq, rho = SHAPES[i]
        seeds, idx = _seeds(3, i), _indices(N)
        want = np.stack([restate(N, idx[k], t, p, nq, rho, seeds[16 * k:16 * k + 16])
                         for k in range(3)], axis=1)       # (p, K, nq, N)
        want.setflags(write=False)
        _cache[i] = (seeds, idx, want)
    return _cache[i]


def gen_dev(pir, dev, N, idx, t, p, nq, rho, seeds, pitch=None, kstride=None, pstride=None,
            fill=0xA5):
    """the device form into a buffer pre-filled with `fill`; the whole buffer copied back"""
    K = len(idx)
    pitch = N if pitch is None else pitch
    kstride = nq * pitch if kstride is None else kstride
    pstride = K * kstride if pstride is None else pstride
    total = p * pstride
    d = dev.alloc_dev(total)
    try:
        dev.h2d(d, np.full(total, fill, np.uint8))
        pir.gen_hollanti_keys_dev(N, idx, t, p, d, pitch, kstride, pstride, nq=nq, rho=rho,
                                  seeds=seeds, stream=dev.stream)
        dev.sync()
        return dev.d2h(d, total)
    finally:
        dev.free_dev(d)


def vectors(buf, N, p, K, nq, pitch, kstride, pstride):
    """(p, K, nq, N) view of the vectors in a strided buffer, and a mask of their bytes"""
    out = np.zeros((p, K, nq, N), np.uint8)
    mask = np.zeros(buf.size, bool)
    for q in range(p):
        for k in range(K):
            for a in range(nq):
                o = q * pstride + k * kstride + a * pitch
                out[q, k, a] = buf[o:o + N]
                mask[o:o + N] = True
    return out, mask


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_bit_exact_against_the_restatement(pir, dev, i):
    N, t, p, nq, rho = SHAPES[i]
    seeds, idx, want = case(i)
    got = gen_dev(pir, dev, N, idx, t, p, nq, rho, seeds).reshape(p, 3, nq, N)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (SHAPES[i], bad[:4], len(bad))


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_strides_and_untouched_bytes(pir, dev, i):
    N, t, p, nq, rho = SHAPES[i]
    seeds, idx, want = case(i)
    pitch = N + 3
    kstride = nq * pitch + 5
    kstride += kstride % 16 == 0            # padded, and no multiple of 16
    pstride = 3 * kstride + 7
    pstride += pstride % 16 == 0
    assert kstride % 16 and pstride % 16
    buf = gen_dev(pir, dev, N, idx, t, p, nq, rho, seeds, pitch, kstride, pstride)
    got, mask = vectors(buf, N, p, 3, nq, pitch, kstride, pstride)
    assert np.array_equal(got, want)
    assert (buf[~mask] == 0xA5).all()          # nothing at or past x = N of any vector
    # ... and with a second fill value, so that a stream byte equal to 0xA5 hides nothing
    buf = gen_dev(pir, dev, N, idx, t, p, nq, rho, seeds, pitch, kstride, pstride, fill=0x5A)
    assert (buf[~mask] == 0x5A).all()


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_host_form_is_the_device_form(pir, dev, i):
    N, t, p, nq, rho = SHAPES[i]
    seeds, idx, want = case(i)
    host = pir.gen_hollanti_keys(N, idx, t, p, nq, rho, seeds=seeds)
    assert host.shape == (p, 3, nq, N) and host.dtype == np.uint8
    assert np.array_equal(host, gen_dev(pir, dev, N, idx, t, p, nq, rho, seeds).reshape(host.shape))
    assert np.array_equal(host, want)


def test_more_keys_than_one_launch_holds(pir):
    """K = 19: the launches of 16 and 3 keys, each key its own seed and index"""
    N, t, p, nq, rho, K = 100, 2, 3, 2, 1, 19
    seeds = _seeds(K, 77)
    idx = [(37 * k) % N for k in range(K)]
    got = pir.gen_hollanti_keys(N, idx, t, p, nq, rho, seeds=seeds)
    for k in (0, 15, 16, 18):
        assert np.array_equal(got[:, k], restate(N, idx[k], t, p, nq, rho, seeds[16 * k:16 * k + 16])), k


def _check_structure(keys, idx, t, rho):
    """keys (p, nq, N): per round and record the parties' values lie on a polynomial of
    t + rho nq coefficients whose coefficient t + (a+1) rho - 1 is [x == idx], the other
    coefficients at or above t zero, the parties beyond the first t + rho nq on the same one"""
    p, nq, N = keys.shape
    m = t + rho * nq
    assert p >= m
    xs = list(range(1, m + 1))
    for a in range(nq):
        for x in (0, idx, N - 1):
            co = _interp_coeffs(xs, keys[:m, a, x])
            for c in range(t, m):
                want = 1 if (c == t + (a + 1) * rho - 1 and x == idx) else 0
                assert co[c] == want, (a, x, c)
            for q in range(m, p):
                val = 0
                for c in reversed(range(m)):
                    val = O.gf_mul(val, q + 1) ^ int(co[c])
                assert val == keys[q, a, x], (a, x, q)


@pytest.mark.parametrize("N,t,p,nq,rho", [(777, 1, 4, 2, 1), (300, 2, 6, 1, 3), (4099, 3, 8, 2, 2)])
def test_structure_by_interpolation(pir, N, t, p, nq, rho):
    idx = N // 3 + 1
    keys = pir.gen_hollanti_keys(N, [idx], t, p, nq, rho)[:, 0]
    _check_structure(keys, idx, t, rho)


def test_seed_behaviour(pir):
    N, t, p = 2 ** 12, 1, 2
    s1, s2 = _seeds(1, 501), _seeds(1, 502)
    a = pir.gen_hollanti_keys(N, [5], t, p, 2, 1, seeds=s1)
    assert np.array_equal(a, pir.gen_hollanti_keys(N, [5], t, p, 2, 1, seeds=s1))
    b = pir.gen_hollanti_keys(N, [5], t, p, 2, 1, seeds=s2)
    assert (a != b).mean() > 0.9
    # the random parts of two rounds of one key: the secret term taken out of record 5
    ra, rb = a[0, 0, 0].copy(), a[0, 0, 1].copy()
    ra[5] ^= O.gf_pow(1, 1)
    rb[5] ^= O.gf_pow(1, 2)
    assert (ra != rb).mean() > 0.9
    # one seed, two indices: the vectors differ at the two records and nowhere else
    i, j = 100, 3001
    ki = pir.gen_hollanti_keys(N, [i], t, p, 2, 1, seeds=s1)
    kj = pir.gen_hollanti_keys(N, [j], t, p, 2, 1, seeds=s1)
    d = ki ^ kj
    assert d[..., i].all() and d[..., j].all()
    d[..., i] = 0
    d[..., j] = 0
    assert not d.any()
    # 2^12 records of one vector take most byte values
    one = pir.gen_hollanti_keys(N, [5], t, p, seeds=s1)
    assert len(np.unique(one[0, 0, 0])) > 200 and len(np.unique(one[1, 0, 0])) > 200
    # a default seed is fresh each call
    assert (pir.gen_hollanti_keys(N, [5], t, p) != pir.gen_hollanti_keys(N, [5], t, p)).any()


@pytest.mark.parametrize("nq", [1, 2])
def test_feeds_the_queue(pir, dev, monkeypatch, nq):
    """K = 5 keys generated on the device straight into one buffer per party, answered from
    there by answer_coefs_queue_dev; each must be answer_coefs of the same vector from the host"""
    n, efs, k, t, rho, K = 11, 64, 2, 1, 1, 5
    N, p = 1 << n, t + rho * nq + 1   # one party more than the polynomial has coefficients
    monkeypatch.setenv("PIR_GQ_SHARE", "2")
    monkeypatch.delenv("PIR_GQ_G", raising=False)
    idx = [1, N - 1, 300, 16, 1031]
    pitch, kstride = N, nq * N
    pstride = K * kstride
    d = dev.alloc_dev(p * pstride)
    pir.gen_hollanti_keys_dev(N, idx, t, p, d, pitch, kstride, pstride, nq=nq, rho=rho,
                              seeds=_seeds(K, 900 + nq), stream=dev.stream)
    dev.sync()
    host = dev.d2h(d, p * pstride).reshape(p, K, nq, N)
    _check_structure(host[:, 0], idx[0], t, rho)
    for q in range(p):
        with pir.Engine(2, 1, n, efs, nq) as e:
            e.encode_within(N, k * efs, k, party=q + 1)
            d_r = e.alloc_dev(K * nq * efs)
            e.answer_coefs_queue_dev(d + q * pstride, pitch, kstride, K, 0, N, d_r)
            e.sync()
            got = e.d2h(d_r, K * nq * efs).reshape(K, nq, efs)
            for kk in range(K):
                assert np.array_equal(got[kk], e.answer_coefs(host[q, kk])), (q, kk)
            assert got.any()
            e.free_dev(d_r)
    dev.free_dev(d)


def _hollanti_servers(S, L, f, t, k, r, rho):
    S.setSystemParams(L, f, t, k, r, 0, rho, 0, 3)
    prm = S.params()
    c = S.Client(L, f)
    servers = []
    for q in range(prm["NUM_PARTIES"]):
        s = S.Server(q + 1, L, prm["ENCODED_FILE_SIZE_BYTES"])
        c.encode_within_files_server(s)
        servers.append(s)
    return prm, c, servers


def _decode(S, servers, keys, drop):
    """the servers' answers to keys (p, nq, N) decoded with server `drop` left out (and, as the
    decode takes exactly NUM_PARTIES - R answers, the R - 1 servers after it)"""
    p = len(servers)
    ans = [servers[q].runHollantiQuery(keys[q]) for q in range(p)]
    er = [1] * p
    for i in range(S.params()["R"]):
        er[(drop + i) % p] = 0
    return S.assembleHollantiResponses(er, np.stack([ans[q] for q in range(p) if er[q]]))


def _record(f, idx):
    return np.arange(f, dtype=np.uint8) if idx == 1 else np.full(f, idx & 0xFF, np.uint8)


E2E = [(10, 64, 1, 2, 1, 1), (8, 20, 1, 4, 2, 2)]


@pytest.mark.parametrize("L,f,t,k,r,rho", E2E)
def test_end_to_end(pir, L, f, t, k, r, rho):
    """GPU keys, the shim servers' runHollantiQuery, one server dropped, the client's decode"""
    from erasurecodedpir_amd import server as S
    prm, c, servers = _hollanti_servers(S, L, f, t, k, r, rho)
    try:
        p, nq, N = prm["NUM_PARTIES"], prm["NUM_ROUNDS"], prm["NUM_ENCODED_FILES"]
        for idx in (1, N - 56):
            keys = pir.gen_hollanti_keys(N, [idx], t, p, nq, rho)[:, 0]
            assert np.array_equal(_decode(S, servers, keys, 1), _record(f, idx)), idx
    finally:
        for s in servers:
            s.freeServer()
        c.free_client()


@pytest.mark.parametrize("L,f,t,k,r,rho", E2E)
def test_shim_switch(pir, L, f, t, k, r, rho):
    """pirClientHollantiKeygenOnGpu(1): generateHollantiQuery's vectors come from the GPU, have
    the structure and decode; switched back to 0 they still do"""
    from erasurecodedpir_amd import _lib, server as S
    hook = lambda: ctypes.c_void_p.in_dll(  # noqa: E731  pir_shim::g_hollanti_keygen
        _lib.load(), "_ZN8pir_shim17g_hollanti_keygenE").value
    prm, c, servers = _hollanti_servers(S, L, f, t, k, r, rho)
    try:
        p, nq, N = prm["NUM_PARTIES"], prm["NUM_ROUNDS"], prm["NUM_ENCODED_FILES"]
        for on in (1, 0):
            S.hollanti_keygen_on_gpu(on)
            assert (hook() is not None) == bool(on)
            for idx in (1, N // 3 + 1):
                keys = c.generateHollantiQuery(idx)
                assert keys.shape == (p, nq, N)
                _check_structure(keys, idx, t, rho)
                assert len(np.unique(keys[0, 0])) > 8
                assert np.array_equal(_decode(S, servers, keys, p - 1), _record(f, idx)), (on, idx)
            again = c.generateHollantiQuery(1)
            assert (again != c.generateHollantiQuery(1)).any()   # a fresh seed per query
    finally:
        S.hollanti_keygen_on_gpu(0)
        for s in servers:
            s.freeServer()
        c.free_client()
