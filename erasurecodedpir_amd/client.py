"""Client-side helpers (include/pir_client.h): DPF key generation on the GPU, the finalCW
values of generate_opt_DPF_tree_query (src/c/client.cpp:144-153), the Hollanti coefficient
vectors (genHollantiDPF, shamir_dpf.cpp:190-237) and the CheckMAC record tags (HMAC-SHA256
under a 16-byte key, client.cpp:29-31) computed on the GPU."""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import check
from .engine import key_len


def final_cw(p, nq, rho=1):
    """nq*(p-1) bytes: out[a*(p-1) + j-2] = gf_pow(j, rho*(a+1)) ^ 1, j = 2..p."""
    out = np.zeros(nq * (p - 1), np.uint8)
    _lib.load().pir_final_cw(p, nq, rho, out.ctypes.data_as(ctypes.c_void_p))
    return out


def gen_keys(n, index, p, nq=1, fcw=None, rho=1, seeds=None, device=0):
    """genOptimizedDPF (src/c/dpf_tree.cpp:142-274) on the GPU.  Returns p keys (bytes).

    seeds: p*16 root-seed bytes (the reference draws them from RAND_bytes); default
    os.urandom."""
    if fcw is None:
        fcw = final_cw(p, nq, rho)
    fcw = np.ascontiguousarray(fcw, dtype=np.uint8)
    if seeds is None:
        seeds = os.urandom(16 * p)
    seeds = np.frombuffer(bytes(seeds), dtype=np.uint8).copy()
    kl = key_len(p, n, nq)
    out = np.zeros(p * kl, np.uint8)
    check(_lib.load().pir_gen_keys(device, n, index, fcw.ctypes.data_as(ctypes.c_void_p), p, nq,
                                   seeds.ctypes.data_as(ctypes.c_void_p),
                                   out.ctypes.data_as(ctypes.c_void_p)), "pir_gen_keys")
    return [out[j * kl:(j + 1) * kl].tobytes() for j in range(p)]


def _hollanti_args(indices, seeds):
    idx = np.ascontiguousarray(np.atleast_1d(indices), dtype=np.uint64)
    K = idx.size
    if seeds is None:
        seeds = os.urandom(16 * K)  # a fresh secret per query, from the OS CSPRNG
    sd = np.frombuffer(bytes(seeds), dtype=np.uint8).copy()
    if sd.size != 16 * K:
        raise ValueError("seeds holds 16 bytes per key")
    return idx, K, sd


def gen_hollanti_keys(num_records, indices, t, p, nq=1, rho=1, seeds=None, device=0):
    """The coefficient vectors of K Hollanti queries (genHollantiDPF with an AES-CTR key stream,
    include/pir_client.h), made on the GPU: a (p, K, nq, num_records) uint8 array, [q, k] what
    party q + 1 answers for record indices[k].

    seeds: 16 bytes per key, each the secret of one query; default os.urandom."""
    idx, K, sd = _hollanti_args(indices, seeds)
    out = np.zeros((p, K, nq, num_records), np.uint8)
    check(_lib.load().pir_gen_hollanti_keys(device, num_records, idx.ctypes.data_as(ctypes.c_void_p),
                                            K, t, p, nq, rho, sd.ctypes.data_as(ctypes.c_void_p),
                                            out.ctypes.data_as(ctypes.c_void_p)),
          "pir_gen_hollanti_keys")
    return out


def gen_hollanti_keys_dev(num_records, indices, t, p, d_keys, coef_pitch, key_stride, party_stride,
                          nq=1, rho=1, seeds=None, device=0, stream=None):
    """pir_gen_hollanti_keys_dev over device memory: party q, key k, round a, record x at
    d_keys + q*party_stride + k*key_stride + a*coef_pitch + x (d_keys a device address: an
    Engine.alloc_dev pointer or a torch tensor's data_ptr(), plus any offset); d_keys +
    q*party_stride is what Engine.answer_coefs_queue_dev(coef_pitch, key_stride) reads.
    Asynchronous on `stream` (a hipStream_t address; None: the null stream).  Returns the seeds
    used (16 bytes per key; default os.urandom)."""
    idx, K, sd = _hollanti_args(indices, seeds)
    check(_lib.load().pir_gen_hollanti_keys_dev(
        device, num_records, idx.ctypes.data_as(ctypes.c_void_p), K, t, p, nq, rho,
        sd.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(int(d_keys)) if d_keys else None,
        coef_pitch, key_stride, party_stride, ctypes.c_void_p(stream) if stream else None),
        "pir_gen_hollanti_keys_dev")
    return sd.tobytes()


MAC_BYTES = 32


def _key16(key):
    k = np.frombuffer(bytes(key), np.uint8).copy()
    if k.size != 16:
        raise ValueError("the tag key is 16 bytes")
    return k


def mac_files(files2d, payload_bytes, key, device=0):
    """Tag the rows of a C-contiguous uint8 (num_files, >= payload_bytes + 32) array in place on
    the GPU: row[payload_bytes : payload_bytes + 32] = HMAC-SHA256(key, row[:payload_bytes])
    (pir_mac_files_rows: only the payloads go to the device, only the tags come back)."""
    f = files2d
    if not (isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.ndim == 2 and
            f.flags.c_contiguous and f.flags.writeable):
        raise ValueError("files2d is a writeable C-contiguous 2-D uint8 array")
    if payload_bytes < 1 or f.shape[1] < payload_bytes + MAC_BYTES:
        raise ValueError("rows hold payload_bytes + 32 bytes")
    n, pitch = f.shape
    rows = (ctypes.c_void_p * max(1, n))(*[f.ctypes.data + i * pitch for i in range(n)])
    k = _key16(key)
    check(_lib.load().pir_mac_files_rows(device, rows, n, payload_bytes,
                                         k.ctypes.data_as(ctypes.c_void_p)), "pir_mac_files_rows")
    return f


def mac_files_dev(d_files, file_pitch, num_files, payload_bytes, key, d_tags=None, tag_pitch=None,
                  device=0, stream=None):
    """pir_mac_files_dev over device memory: d_files / d_tags are device addresses (an
    Engine.alloc_dev pointer or a torch tensor's data_ptr(), plus any offset).  d_tags=None tags
    in place (d_files + payload_bytes, the rows' own pitch).  Asynchronous on `stream` (a
    hipStream_t address; None: the null stream)."""
    if d_tags is None:
        d_tags, tag_pitch = int(d_files) + payload_bytes, file_pitch
    k = _key16(key)
    check(_lib.load().pir_mac_files_dev(device, ctypes.c_void_p(int(d_files)), file_pitch,
                                        num_files, payload_bytes,
                                        k.ctypes.data_as(ctypes.c_void_p),
                                        ctypes.c_void_p(int(d_tags)), tag_pitch,
                                        ctypes.c_void_p(stream) if stream else None),
          "pir_mac_files_dev")


def mac_check(record, payload_bytes, key):
    """True if record[payload_bytes : payload_bytes + 32] is the tag of record[:payload_bytes]
    (the client's check of a decoded record, benchmark.go:190-207).  Host only."""
    r = np.frombuffer(bytes(record), np.uint8).copy()
    if payload_bytes < 1 or r.size < payload_bytes + MAC_BYTES:
        raise ValueError("the record holds payload_bytes + 32 bytes")
    k = _key16(key)
    rc = _lib.load().pir_mac_check(r.ctypes.data_as(ctypes.c_void_p), payload_bytes,
                                   k.ctypes.data_as(ctypes.c_void_p))
    if rc < 0:
        check(rc, "pir_mac_check")
    return rc == 0
