#!/usr/bin/env python3
"""Generate tests/golden/checkmac.json from the REFERENCE itself (a CheckMAC setup).

Test infrastructure only; runs on the build machine.  Requires oracle/_ref/libref.so (`make -C
oracle ref`: the reference's own src/c compiled where it lies).  The reference's functions are
reached through ctypes by their C++ symbol names; nothing here restates what they compute.
After setSystemParams(10, 64, 1, 2, 1, 0, 1, checkMac = 1, mode 0) and initialize_client (which
tags every file with OpenSSL's HMAC, client.cpp:29-31) the file holds the sizing globals, file 1
(payload + tag) in hex, and per party the SHA-256 of the shard that generate_encoded_across_file
produces row by row into zeroed buffers.

    python tests/golden/make_golden_checkmac.py     # rewrites tests/golden/checkmac.json
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


class Client(ctypes.Structure):  # src/c/client.h:15-20
    _fields_ = [("ctx", ctypes.c_void_p), ("macCtx", ctypes.c_void_p),
                ("unencoded_files", ctypes.POINTER(u8p)), ("macKey", u8p)]


set_params = REF._Z15setSystemParamsiiiiiiiii
init_client = REF._Z17initialize_clientP6clienthj
init_client.argtypes = [ctypes.POINTER(Client), ctypes.c_uint8, ctypes.c_uint32]
encode_row = REF._Z28generate_encoded_across_fileP6clientiiPh
encode_row.argtypes = [ctypes.POINTER(Client), ctypes.c_int, ctypes.c_int, ctypes.c_void_p]

GLOBALS = ["NUM_PARTIES", "NUM_FILES", "NUM_ENCODED_FILES", "LOG_NUM_ENCODED_FILES",
           "ENCODED_PAYLOAD_SIZE_BYTES", "ENCODED_FILE_SIZE_BYTES", "NUM_ROUNDS", "CHECK_MAC",
           "MAC_SIZE_BYTES", "FILE_SIZE_BYTES", "PAYLOAD_SIZE_BYTES"]

PARAMS = dict(L=10, f=64, t=1, k=2, r=1, b=0, rho=1, mac=1, mode=0)


def glob(name):
    return ctypes.c_int.in_dll(REF, name).value


def main():
    a = PARAMS
    set_params(a["L"], a["f"], a["t"], a["k"], a["r"], a["b"], a["rho"], a["mac"], a["mode"])
    g = {n: glob(n) for n in GLOBALS}
    c = Client()
    init_client(ctypes.byref(c), a["L"], a["f"])
    fs, efs, rows = g["FILE_SIZE_BYTES"], g["ENCODED_FILE_SIZE_BYTES"], g["NUM_ENCODED_FILES"]
    shards = []
    for party in range(1, g["NUM_PARTIES"] + 1):
        shard = np.zeros((rows, efs), np.uint8)  # the reference XORs into the row
        for i in range(rows):
            encode_row(ctypes.byref(c), party, i, shard[i].ctypes.data)
        shards.append(hashlib.sha256(shard.tobytes()).hexdigest())
    out = {"params": a, "globals": g, "mac_key": ctypes.string_at(c.macKey, 16).decode(),
           "file1": ctypes.string_at(c.unencoded_files[1], fs).hex(),
           "file300": ctypes.string_at(c.unencoded_files[300], fs).hex(),
           "shard_sha256": shards}
    with open(os.path.join(HERE, "checkmac.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["globals"]))


if __name__ == "__main__":
    main()
