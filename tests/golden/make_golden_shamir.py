#!/usr/bin/env python3
"""Generate tests/golden/shamir.json from the REFERENCE itself (the Shamir sqrt(N) mode, mode 2).

Test infrastructure only; runs on the build machine.  Requires oracle/_ref/libref.so (`make -C
oracle ref`: the reference's own src/c compiled where it lies).  The reference's functions are
reached through ctypes by their C++ symbol names; nothing here restates what they compute.  Per
case the file holds the sizing globals after setSystemParams(mode 2), the SHA-256 of every
party's 2N rows after initialize_client + encode_within_files_server, random key bytes (stored:
the server answer is pinned as a function of them), runOptShamirDPFQuery's answers for one
party, and the XOR of T runOptShamirDPFQueryThread slices.

    python tests/golden/make_golden_shamir.py     # rewrites tests/golden/shamir.json
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


set_params = REF._Z15setSystemParamsiiiiiiiii
init_server = REF._Z16initializeServerP6serverijjii
init_server.argtypes = [ctypes.POINTER(Server), ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                        ctypes.c_int, ctypes.c_int]
init_client = REF._Z17initialize_clientP6clienthj
init_client.argtypes = [ctypes.POINTER(Client), ctypes.c_uint8, ctypes.c_uint32]
encode_within = REF._Z26encode_within_files_serverP6clientP6server
query = REF._Z20runOptShamirDPFQueryP6serverPPhS2_
query_thread = REF._Z26runOptShamirDPFQueryThreadP6serverPPhiiiS2_
query_thread.argtypes = [ctypes.POINTER(Server), ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                         ctypes.c_int, ctypes.c_void_p]

GLOBALS = ["NUM_PARTIES", "NUM_FILES", "NUM_ENCODED_FILES", "LOG_NUM_ENCODED_FILES",
           "ENCODED_PAYLOAD_SIZE_BYTES", "ENCODED_FILE_SIZE_BYTES", "ENCODE_ACROSS", "NUM_ROUNDS",
           "IS_HERMITE", "D", "MODE", "FILE_SIZE_BYTES", "LOG_NUM_FILES", "K", "T", "R", "B", "RHO"]

#        L   f  t  k rho party T
CASES = [(6, 16, 1, 2, 1, 1, 4),
         (5, 30, 2, 3, 1, 3, 2),
         (7, 20, 1, 4, 2, 2, 8),
         (4, 8, 1, 1, 1, 1, 1),
         (8, 64, 1, 2, 1, 2, 4)]


def g(name):
    return ctypes.c_int.in_dll(REF, name).value


def row_ptrs(a):
    return (u8p * a.shape[0])(*[ctypes.cast(a.ctypes.data + i * a.strides[0], u8p)
                                for i in range(a.shape[0])])


def main():
    rng = np.random.RandomState(20)
    cases = []
    for (L, f, t, k, rho, party, T) in CASES:
        set_params(L, f, t, k, 0, 0, rho, 0, 2)
        prm = {n: g(n) for n in GLOBALS}
        N, efs, nq, n = prm["NUM_ENCODED_FILES"], prm["ENCODED_FILE_SIZE_BYTES"], prm["NUM_ROUNDS"], \
            prm["LOG_NUM_ENCODED_FILES"]
        x = (n + 1) // 2
        klen = (1 << x) + (1 << (n - x))
        rlen = (klen + 2) * efs
        cl = Client()
        init_client(ctypes.byref(cl), L, f)
        shards, srv = {}, {}
        for q in range(1, prm["NUM_PARTIES"] + 1):
            s = Server()
            init_server(ctypes.byref(s), q, L, efs, 0, T)
            encode_within(ctypes.byref(cl), ctypes.byref(s))
            rows = np.stack([np.ctypeslib.as_array(s.indexList[i], (efs,)).copy()
                             for i in range(2 * N)])
            shards[str(q)] = hashlib.sha256(rows.tobytes()).hexdigest()
            srv[q] = s
        keys = rng.randint(0, 256, (nq, klen)).astype(np.uint8)
        s = srv[party]
        whole = np.zeros((nq, rlen), np.uint8)
        query(ctypes.byref(s), row_ptrs(keys), row_ptrs(whole))
        sliced = np.zeros((nq, rlen), np.uint8)
        for th in range(T):
            part = np.zeros((nq, rlen), np.uint8)
            query_thread(ctypes.byref(s), ctypes.cast(row_ptrs(keys), ctypes.c_void_p), th,
                         th * N // T, (th + 1) * N // T,
                         ctypes.cast(row_ptrs(part), ctypes.c_void_p))
            sliced ^= part
        cases.append({"L": L, "f": f, "t": t, "k": k, "rho": rho, "party": party, "T": T,
                      "params": prm, "key_len": klen, "response_len": rlen,
                      "shard_sha256": shards, "keys": keys.tobytes().hex(),
                      "answer": whole.tobytes().hex(), "answer_slices": sliced.tobytes().hex()})
    with open(os.path.join(HERE, "shamir.json"), "w") as fh:
        json.dump({"cases": cases}, fh, indent=1, sort_keys=True)
    print("wrote shamir.json")


if __name__ == "__main__":
    main()
