#!/usr/bin/env python3
"""Generate tests/golden/woodruff.json from the REFERENCE itself (the Woodruff mode, mode 5).

Test infrastructure only; runs on the build machine.  Requires oracle/_ref/libref.so (`make -C
oracle ref`: the reference's own src/c compiled where it lies).  The reference's functions are
reached through ctypes by their C++ symbol names; nothing here restates what they compute.  Per
case the file holds the sizing globals after setSystemParams(mode 5) for both values of
WOODRUFF_DERIVATIVE, the SHA-256 of every party's rows after initialize_client +
encode_within_files_server (k = 1: the shard is the database), random key bytes with a few zero
bytes (stored: the server answer is pinned as a function of them), runWoodruffQueryThread's
value answer and its M + 1 derivative answers over the whole domain (taken with zeroed buffers:
the reference XORs into whatever out[1..M] held), the XOR of T Thread slices for both, and one
end-to-end vector: random v, an index, genWoodruffQuery's p keys, an erasure list with R servers
dropped and the record assembleWoodruffResponses decodes from the answers of the others.

    python tests/golden/make_golden_woodruff.py     # rewrites tests/golden/woodruff.json
"""
import ctypes
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref.so"))

u8p = ctypes.POINTER(ctypes.c_uint8)


class Server(ctypes.Structure):  # src/c/server.h:13-25
    _fields_ = [("ctx", ctypes.c_void_p), ("ctxThreads", ctypes.c_void_p),
                ("partyIndex", ctypes.c_int), ("indexList", ctypes.POINTER(u8p)),
                ("isByzantine", ctypes.c_int), ("numThreads", ctypes.c_int)]


class Client(ctypes.Structure):  # src/c/client.h:15-20
    _fields_ = [("ctx", ctypes.c_void_p), ("macCtx", ctypes.c_void_p),
                ("unencoded_files", ctypes.POINTER(u8p)), ("macKey", u8p)]


class U128(ctypes.Structure):  # uint128_t by value: two INTEGER eightbytes
    _fields_ = [("lo", ctypes.c_uint64), ("hi", ctypes.c_uint64)]


set_params = REF._Z15setSystemParamsiiiiiiiii
init_server = REF._Z16initializeServerP6serverijjii
init_server.argtypes = [ctypes.POINTER(Server), ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                        ctypes.c_int, ctypes.c_int]
init_client = REF._Z17initialize_clientP6clienthj
init_client.argtypes = [ctypes.POINTER(Client), ctypes.c_uint8, ctypes.c_uint32]
encode_within = REF._Z26encode_within_files_serverP6clientP6server
query_thread = REF._Z22runWoodruffQueryThreadP6serverPhiiiPS1_
query_thread.argtypes = [ctypes.POINTER(Server), ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                         ctypes.c_int, ctypes.c_void_p]
gen_query = REF._Z16genWoodruffQueryoiiiPPhS0_
gen_query.argtypes = [U128, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                      ctypes.c_void_p]
assemble = REF._Z25assembleWoodruffResponsesP6clientPhPPS1_S1_S2_
assemble.argtypes = [ctypes.POINTER(Client), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                     ctypes.c_void_p]

GLOBALS = ["NUM_PARTIES", "NUM_FILES", "NUM_ENCODED_FILES", "LOG_NUM_ENCODED_FILES",
           "ENCODED_PAYLOAD_SIZE_BYTES", "ENCODED_FILE_SIZE_BYTES", "ENCODE_ACROSS", "NUM_ROUNDS",
           "MODE", "FILE_SIZE_BYTES", "LOG_NUM_FILES", "K", "T", "R", "B", "RHO", "WOODRUFF_M",
           "WOODRUFF_D"]

#        L   f  t  r party T  index
CASES = [(4, 8, 1, 0, 1, 1, 5),
         (6, 16, 2, 1, 3, 2, 63),
         (7, 30, 1, 1, 2, 4, 0),
         (10, 64, 2, 0, 5, 8, 777),
         (5, 13, 1, 1, 1, 2, 17)]   # k = 1, an odd file size


def g(name):
    return ctypes.c_int.in_dll(REF, name).value


def set_deriv(on):
    ctypes.c_int.in_dll(REF, "WOODRUFF_DERIVATIVE").value = on


def row_ptrs(a):
    return (u8p * a.shape[0])(*[ctypes.cast(a.ctypes.data + i * a.strides[0], u8p)
                                for i in range(a.shape[0])])


def run(s, key, lo, hi, nout, efs):
    out = np.zeros((nout, efs), np.uint8)
    query_thread(ctypes.byref(s), key.ctypes.data_as(ctypes.c_void_p), 0, lo, hi,
                 ctypes.cast(row_ptrs(out), ctypes.c_void_p))
    return out


def main():
    rng = np.random.RandomState(50)
    cases = []
    for (L, f, t, r, party, T, index) in CASES:
        set_deriv(1)
        set_params(L, f, t, 1, r, 0, 1, 0, 5)
        parties_deriv = g("NUM_PARTIES")
        set_deriv(0)
        set_params(L, f, t, 1, r, 0, 1, 0, 5)
        prm = {n: g(n) for n in GLOBALS}
        N, efs, M, p = prm["NUM_ENCODED_FILES"], prm["ENCODED_FILE_SIZE_BYTES"], \
            prm["WOODRUFF_M"], prm["NUM_PARTIES"]
        cl = Client()
        init_client(ctypes.byref(cl), L, f)
        shards, srv = {}, {}
        for q in range(1, p + 1):
            s = Server()
            init_server(ctypes.byref(s), q, L, efs, 0, T)
            encode_within(ctypes.byref(cl), ctypes.byref(s))
            rows = np.stack([np.ctypeslib.as_array(s.indexList[i], (efs,)).copy()
                             for i in range(N)])
            shards[str(q)] = hashlib.sha256(rows.tobytes()).hexdigest()
            srv[q] = s
        key = rng.randint(0, 256, M).astype(np.uint8)
        key[rng.choice(M, max(1, M // 8), replace=False)] = 0
        s = srv[party]
        value = run(s, key, 0, N, 1, efs)
        value_sl = np.zeros_like(value)
        for th in range(T):
            value_sl ^= run(s, key, th * (N // T), (th + 1) * (N // T), 1, efs)
        set_deriv(1)
        deriv = run(s, key, 0, N, M + 1, efs)
        deriv_sl = np.zeros_like(deriv)
        for th in range(T):
            deriv_sl ^= run(s, key, th * (N // T), (th + 1) * (N // T), M + 1, efs)
        set_deriv(0)
        # end to end, value mode: R servers dropped
        v = rng.randint(0, 256, (t, M)).astype(np.uint8)
        keys = np.zeros((p, M), np.uint8)
        gen_query(U128(index, 0), t, p, M, ctypes.cast(row_ptrs(v), ctypes.c_void_p),
                  ctypes.cast(row_ptrs(keys), ctypes.c_void_p))
        erasure = np.ones(p, np.uint8)
        erasure[rng.choice(p, r, replace=False)] = 0
        alive = [q for q in range(1, p + 1) if erasure[q - 1]]
        resp = [run(srv[q], keys[q - 1], 0, N, 1, efs) for q in alive]
        rows = [row_ptrs(x) for x in resp]
        outer = (ctypes.POINTER(u8p) * len(alive))(*[ctypes.cast(x, ctypes.POINTER(u8p))
                                                      for x in rows])
        decoded = np.zeros(prm["FILE_SIZE_BYTES"], np.uint8)
        assemble(ctypes.byref(cl), erasure.ctypes.data_as(ctypes.c_void_p), outer,
                 decoded.ctypes.data_as(ctypes.c_void_p),
                 ctypes.cast(row_ptrs(v), ctypes.c_void_p))
        record = np.ctypeslib.as_array(cl.unencoded_files[index], (f,)).copy()
        assert np.array_equal(decoded, record), (L, f, t, r)
        cases.append({"L": L, "f": f, "t": t, "r": r, "party": party, "T": T,
                      "params": prm, "num_parties_derivative": parties_deriv,
                      "shard_sha256": shards, "key": key.tobytes().hex(),
                      "value": value.tobytes().hex(), "value_slices": value_sl.tobytes().hex(),
                      "deriv": deriv.tobytes().hex(), "deriv_slices": deriv_sl.tobytes().hex(),
                      "e2e": {"index": index, "v": v.tobytes().hex(),
                              "keys": keys.tobytes().hex(),
                              "erasure": [int(x) for x in erasure],
                              "responses": [x.tobytes().hex() for x in resp],
                              "decoded": decoded.tobytes().hex()}})
    with open(os.path.join(HERE, "woodruff.json"), "w") as fh:
        json.dump({"cases": cases}, fh, indent=1, sort_keys=True)
    print("wrote woodruff.json")


if __name__ == "__main__":
    main()
