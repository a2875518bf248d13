"""Python host mirror of the engine C ABI (include/pir_engine.h).

`Engine` is one PIR server's shard -- or one 2^-G partition of it -- resident in the HBM of one
MI355X, answering tree-DPF queries with the HIP kernels of csrc/pir_kernels.hip.  Method names
follow the reference's server operations (src/c/server.h:27-53):

    Engine.answer        runOptimizedDPFTreeQuery        (src/c/server.cpp:96-134)
    Engine.answer_slice  runOptimizedDPFTreeQueryThread  (src/c/server.cpp:505-549, intended)
    Engine.eval_all      evalAllOptimizedDPF             (src/c/dpf_tree.cpp:473-598)
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check


def _buf(b):
    if isinstance(b, (bytes, bytearray)):
        b = np.frombuffer(bytes(b), dtype=np.uint8)
    b = np.ascontiguousarray(b, dtype=np.uint8)
    return b, b.ctypes.data_as(ctypes.c_void_p)


def key_len(num_parties, log_num_records, num_rounds):
    """calcOptimizedDPFTreeKeyLength (src/c/utils.cpp:85-90)."""
    return _lib.load().pir_engine_key_len(num_parties, log_num_records, num_rounds)


class Engine:
    def __init__(self, num_parties, party_index, log_num_records, record_bytes, num_rounds=1,
                 device=0, log_num_partitions=0, partition_index=0, is_byzantine=False):
        lib = _lib.load()
        self._lib = lib
        cfg = _lib.PirConfig(device, num_parties, party_index, log_num_records, record_bytes,
                             num_rounds, log_num_partitions, partition_index, int(is_byzantine))
        h = ctypes.c_void_p()
        check(lib.pir_engine_create(ctypes.byref(cfg), ctypes.byref(h)), "pir_engine_create")
        self._h = h
        self.num_parties = num_parties
        self.party_index = party_index
        self.n = log_num_records
        self.record_bytes = record_bytes
        self.num_rounds = num_rounds
        self.log_num_partitions = log_num_partitions
        self.partition_index = partition_index
        self.key_len = key_len(num_parties, log_num_records, num_rounds)
        self.num_rows = int(lib.pir_engine_num_rows(h))
        self.answer_bytes = num_rounds * record_bytes

    # -- lifetime ------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.pir_engine_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- shard -----------------------------------------------------------------------------
    def set_shard(self, rows, row0=0):
        """rows: (nrows, record_bytes) uint8 array (or a flat buffer of whole rows)."""
        arr = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, self.record_bytes)
        check(self._lib.pir_engine_set_shard(self._h, arr.ctypes.data_as(ctypes.c_void_p), row0,
                                             arr.shape[0], self.record_bytes),
              "pir_engine_set_shard")

    def fill_shard_random(self, seed):
        check(self._lib.pir_engine_fill_shard_random(self._h, seed), "fill_shard_random")

    def encode_across(self, num_files, k, files=None):
        """The erasure-coded shard computed on the GPU (client.cpp:70-97): from `files`
        (num_files x record_bytes host array) or, files=None, the reference's synthetic
        database (client.cpp:16-33)."""
        d_f, pitch = None, 0
        if files is not None:
            f = np.ascontiguousarray(np.asarray(files, np.uint8).reshape(num_files, -1))
            pitch = f.shape[1]
            d_f = self.alloc_dev(f.size)
        try:
            if d_f is not None:
                self.h2d(d_f, f.reshape(-1))
            check(self._lib.pir_engine_encode_across_dev(self._h, d_f, pitch, num_files, k),
                  "encode_across")
        finally:
            if d_f is not None:
                self.free_dev(d_f)

    def encode_across_synthetic_mac(self, num_files, k, key):
        """encode_across(num_files, k) for a CheckMAC setup: the synthetic files are
        record_bytes - 32 payload bytes followed by their HMAC-SHA256 tag under the 16-byte
        `key` (client.cpp:29-31), the tags computed on the GPU."""
        key = np.frombuffer(bytes(key), np.uint8).copy()
        if key.size != 16:
            raise ValueError("the tag key is 16 bytes")
        check(self._lib.pir_engine_encode_across_synthetic_mac(
            self._h, num_files, k, key.ctypes.data_as(ctypes.c_void_p)),
            "encode_across_synthetic_mac")

    def encode_within(self, num_files, file_bytes, k, files=None, party=0):
        """The Hollanti-mode shard (encoded within files) computed on the GPU (client.cpp:43-56,
        99-103): from `files` (num_files x file_bytes host array) or, files=None, the
        reference's synthetic database (client.cpp:16-33).  party: the server's party index
        (0: the engine's)."""
        d_f, pitch = None, 0
        if files is not None:
            f = np.ascontiguousarray(np.asarray(files, np.uint8).reshape(num_files, -1))
            pitch = f.shape[1]
            d_f = self.alloc_dev(f.size)
        try:
            if d_f is not None:
                self.h2d(d_f, f.reshape(-1))
            check(self._lib.pir_engine_encode_within_dev(self._h, d_f, pitch, num_files,
                                                         file_bytes, k, party), "encode_within")
        finally:
            if d_f is not None:
                self.free_dev(d_f)

    def encode_hermite(self, num_files, file_bytes, k, files=None, party=0):
        """The Hermite rows [N, 2N) of a Shamir engine (log_num_records = n + 1) computed on the
        GPU (client.cpp:57-68, 103-107): the formal derivative of the within-file polynomial
        that encode_within evaluates.  files / party as for encode_within; the value rows
        [0, N) are left alone (call encode_within first: it zeroes the rows past num_files)."""
        d_f, pitch = None, 0
        if files is not None:
            f = np.ascontiguousarray(np.asarray(files, np.uint8).reshape(num_files, -1))
            pitch = f.shape[1]
            d_f = self.alloc_dev(max(1, f.size))
        try:
            if d_f is not None:
                self.h2d(d_f, f.reshape(-1))
            check(self._lib.pir_engine_encode_hermite_dev(self._h, d_f, pitch, num_files,
                                                          file_bytes, k, party), "encode_hermite")
        finally:
            if d_f is not None:
                self.free_dev(d_f)

    def shard_row(self, i):
        out = np.empty(self.record_bytes, np.uint8)
        check(self._lib.pir_engine_get_shard_row(self._h, i, out.ctypes.data_as(ctypes.c_void_p)),
              "get_shard_row")
        return out

    def get_shard(self, row0=0, nrows=None):
        nrows = self.num_rows - row0 if nrows is None else nrows
        out = np.empty((nrows, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_get_shard(self._h, row0, nrows,
                                             out.ctypes.data_as(ctypes.c_void_p)), "get_shard")
        return out

    # -- live updates ----------------------------------------------------------------------
    # Changed records patched into the resident shard, and into a valid fold image, in place
    # (include/pir_engine.h, "live record updates").  Every form takes DELTAS, old ^ new.
    @staticmethod
    def _index(index):
        idx = np.ascontiguousarray(np.asarray(index, np.uint64).reshape(-1))
        return idx, idx.ctypes.data_as(ctypes.c_void_p)

    @staticmethod
    def _deltas(deltas, num):
        d = np.ascontiguousarray(np.asarray(deltas, np.uint8).reshape(num, -1)) if num \
            else np.zeros((0, 1), np.uint8)
        return d, d.ctypes.data_as(ctypes.c_void_p), d.shape[1]

    def update_rows(self, rows, deltas):
        """Engine row rows[i] ^= deltas[i] ((num, record_bytes) uint8)."""
        idx, ip = self._index(rows)
        d, dp, pitch = self._deltas(deltas, idx.size)
        check(self._lib.pir_engine_update_rows(self._h, ip, idx.size, dp, pitch), "update_rows")

    def update_across(self, file_index, deltas, num_files, k):
        """Files file_index[i] of an across-encoded database (encode_across(num_files, k, files))
        changed by deltas[i] = old ^ new ((num, record_bytes) uint8): afterwards the shard is what
        encode_across gives from the new files."""
        idx, ip = self._index(file_index)
        d, dp, pitch = self._deltas(deltas, idx.size)
        check(self._lib.pir_engine_update_across(self._h, ip, idx.size, dp, pitch, num_files, k),
              "update_across")

    def update_within(self, file_index, deltas, num_files, file_bytes, k, party=0, hermite=False):
        """Files file_index[i] of a within-encoded database (encode_within) changed by deltas[i] =
        old ^ new ((num, file_bytes) uint8); hermite: a Shamir engine, whose Hermite rows
        (encode_hermite) follow too.  party as for encode_within."""
        idx, ip = self._index(file_index)
        d, dp, pitch = self._deltas(deltas, idx.size)
        check(self._lib.pir_engine_update_within(self._h, ip, idx.size, dp, pitch, num_files,
                                                 file_bytes, k, party, int(bool(hermite))),
              "update_within")

    def update_across_mac(self, file_index, old, new, num_files, k, key):
        """update_across for a CheckMAC setup: old / new are the files' PAYLOADS ((num,
        record_bytes - 32) uint8); the engine tags both under the 16-byte `key` on the GPU and
        applies payload-delta || tag-delta."""
        key = np.frombuffer(bytes(key), np.uint8).copy()
        if key.size != 16:
            raise ValueError("the tag key is 16 bytes")
        idx, ip = self._index(file_index)
        o, _, pitch = self._deltas(old, idx.size)
        n, _, npitch = self._deltas(new, idx.size)
        if pitch != npitch:
            raise ValueError("old and new payloads of different lengths")
        d_o = self.alloc_dev(max(1, o.size))
        try:
            d_n = self.alloc_dev(max(1, n.size))
            try:
                if idx.size:
                    self.h2d(d_o, o.reshape(-1))
                    self.h2d(d_n, n.reshape(-1))
                self.update_across_mac_dev(idx, d_o, d_n, pitch, num_files, k, key)
                self.sync()
            finally:
                self.free_dev(d_n)
        finally:
            self.free_dev(d_o)

    def update_rows_dev(self, rows, d_delta, delta_pitch, stream=None):
        idx, ip = self._index(rows)
        check(self._lib.pir_engine_update_rows_dev(self._h, ip, idx.size, d_delta, delta_pitch,
                                                   stream), "update_rows_dev")

    def update_across_dev(self, file_index, d_delta, delta_pitch, num_files, k, stream=None):
        """Asynchronous on `stream`: the indices (host) are read now, the deltas (device) on the
        stream, after every answer enqueued before and before every later one."""
        idx, ip = self._index(file_index)
        check(self._lib.pir_engine_update_across_dev(self._h, ip, idx.size, d_delta, delta_pitch,
                                                     num_files, k, stream), "update_across_dev")

    def update_within_dev(self, file_index, d_delta, delta_pitch, num_files, file_bytes, k,
                          party=0, hermite=False, stream=None):
        idx, ip = self._index(file_index)
        check(self._lib.pir_engine_update_within_dev(self._h, ip, idx.size, d_delta, delta_pitch,
                                                     num_files, file_bytes, k, party,
                                                     int(bool(hermite)), stream),
              "update_within_dev")

    def update_across_mac_dev(self, file_index, d_old, d_new, pitch, num_files, k, key,
                              stream=None):
        key = np.frombuffer(bytes(key), np.uint8).copy()
        idx, ip = self._index(file_index)
        check(self._lib.pir_engine_update_across_mac_dev(
            self._h, ip, idx.size, d_old, d_new, pitch, num_files, k,
            key.ctypes.data_as(ctypes.c_void_p), stream), "update_across_mac_dev")

    # -- answers ---------------------------------------------------------------------------
    def _check_key(self, key):
        k, kp = _buf(key)
        if k.size != self.key_len:
            raise ValueError(f"key has {k.size} bytes, expected {self.key_len}")
        return k, kp

    def answer(self, key):
        """(num_rounds, record_bytes) answer of this engine (XOR over ranks if a comm is
        attached)."""
        k, kp = self._check_key(key)
        out = np.empty((self.num_rounds, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_answer(self._h, kp, out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_answer")
        return out

    def answer_batch(self, keys):
        """(num_keys, num_rounds, record_bytes) answers of keys (a sequence of key_len-byte
        keys, or a (num_keys, key_len) uint8 array), batch_group keys per shard pass."""
        ks = [_buf(k)[0] for k in keys]
        for k in ks:
            if k.size != self.key_len:
                raise ValueError(f"key of {k.size} bytes, expected {self.key_len}")
        nk = len(ks)
        flat = np.ascontiguousarray(np.concatenate(ks) if nk else np.zeros(0, np.uint8),
                                    dtype=np.uint8)
        out = np.empty((nk, self.num_rounds, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_answer_batch(self._h, flat.ctypes.data_as(ctypes.c_void_p), nk,
                                                out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_answer_batch")
        return out

    @property
    def batch_group(self):
        """Keys answered per pass over the shard."""
        return self._lib.pir_engine_batch_group(self._h)

    @batch_group.setter
    def batch_group(self, g):
        check(self._lib.pir_engine_set_batch_group(self._h, int(g)), "set_batch_group")

    def answer_slice(self, key, thread_num, num_threads):
        k, kp = self._check_key(key)
        out = np.empty((self.num_rounds, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_answer_slice(self._h, kp, thread_num, num_threads,
                                                out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_answer_slice")
        return out

    def answer_slices(self, key, num_threads):
        """Every thread slice of one query at once, (num_threads, num_rounds, record_bytes):
        row t = answer_slice(key, t, num_threads) -- the T concurrent
        runOptimizedDPFTreeQueryThread calls of src/server_util/tree.go:60-76, from one tree and
        one pass over the shard where the shape allows."""
        k, kp = self._check_key(key)
        out = np.empty((num_threads, self.num_rounds, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_answer_slices(self._h, kp, num_threads,
                                                 out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_answer_slices")
        return out

    def answer_slices_dev(self, d_key, num_threads, d_results, stream=None):
        check(self._lib.pir_engine_answer_slices_dev(self._h, d_key, num_threads, d_results,
                                                     stream), "answer_slices_dev")

    def fold_gathered_dev(self, d_gathered, nranks, bytes_per_rank, d_result, stream=None):
        """The split-shard combine after the RCCL all-gather: d_result = XOR over r of the
        rank-r block of d_gathered (pir_engine_fold_gathered_dev)."""
        check(self._lib.pir_engine_fold_gathered_dev(self._h, d_gathered, nranks, bytes_per_rank,
                                                     d_result, stream), "fold_gathered_dev")

    def answer_coefs(self, coefs, row0=0, nrows=None):
        """Explicit-coefficient answer (runHollantiQuery[Thread], src/c/server.cpp:321-371):
        coefs is (num_rounds, rows) uint8 -- coefficient of engine row r in round a at
        coefs[a][r]; rows [row0, row0 + nrows) are answered.  (num_rounds, record_bytes)."""
        c = np.ascontiguousarray(np.asarray(coefs, np.uint8).reshape(self.num_rounds, -1))
        nrows = c.shape[1] - row0 if nrows is None else nrows
        ptrs = (ctypes.c_void_p * self.num_rounds)(*[c[a].ctypes.data for a in range(self.num_rounds)])
        out = np.empty((self.num_rounds, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_answer_coefs(self._h, ptrs, row0, nrows,
                                                out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_answer_coefs")
        return out

    def answer_coefs_dev(self, d_coefs, coef_pitch, row0, nrows, d_result, stream=None):
        check(self._lib.pir_engine_answer_coefs_dev(self._h, d_coefs, coef_pitch, row0, nrows,
                                                    d_result, stream), "answer_coefs_dev")

    @property
    def shamir_key_len(self):
        """calcShamirDPFKeyLength of a Shamir engine (log_num_records = n + 1): 2^x + 2^y."""
        n = self.n - 1
        x = (n + 1) // 2
        return (1 << x) + (1 << (n - x))

    @property
    def shamir_response_len(self):
        return shamir_response_len(self.n - 1, self.record_bytes)

    def answer_shamir(self, keys, rec0=0, nrec=None):
        """Shamir sqrt(N) answer (runOptShamirDPFQuery[Thread], src/c/server.cpp:203-319) of a
        Shamir engine (value rows [0, N), Hermite rows [N, 2N)): keys is (num_rounds, 2^x + 2^y)
        uint8; the records [rec0, rec0 + nrec) of the N-record domain are answered.
        -> (num_rounds, 2^x + 2^y + 2, record_bytes): row sums, column sums, the Hermite total
        and the value total."""
        kl = self.shamir_key_len
        k = np.ascontiguousarray(np.asarray(keys, np.uint8).reshape(self.num_rounds, kl))
        nrec = self.num_rows // 2 - rec0 if nrec is None else nrec
        ptrs = (ctypes.c_void_p * self.num_rounds)(*[k[a].ctypes.data
                                                     for a in range(self.num_rounds)])
        out = np.empty((self.num_rounds, kl + 2, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_answer_shamir(self._h, ptrs, rec0, nrec,
                                                 out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_answer_shamir")
        return out

    def answer_shamir_dev(self, d_keys, key_pitch, rec0, nrec, d_result, stream=None):
        check(self._lib.pir_engine_answer_shamir_dev(self._h, d_keys, key_pitch, rec0, nrec,
                                                     d_result, stream), "answer_shamir_dev")

    def answer_shamir_queue(self, keys, rec0=0, nrec=None):
        """A queue of independent Shamir queries over the records [rec0, rec0 + nrec): keys is
        (K, num_rounds, 2^x + 2^y) uint8 -> (K, num_rounds, 2^x + 2^y + 2, record_bytes), entry k
        what answer_shamir gives for keys[k].  Where it measured faster the queued rounds share
        passes over the shard (8 per read of it; $PIR_SH_SHARE, $PIR_SH_G: include/pir_engine.h),
        else each key has its own answer, back to back."""
        kl = self.shamir_key_len
        nq = self.num_rounds
        k = np.ascontiguousarray(np.asarray(keys, np.uint8).reshape(-1, nq, kl))
        nk = k.shape[0]
        nrec = self.num_rows // 2 - rec0 if nrec is None else nrec
        ptrs = (ctypes.c_void_p * max(nk * nq, 1))(*[k[i, a].ctypes.data
                                                     for i in range(nk) for a in range(nq)])
        out = np.empty((nk, nq, kl + 2, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_answer_shamir_queue(self._h, ptrs, nk, rec0, nrec,
                                                       out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_answer_shamir_queue")
        return out

    def answer_shamir_queue_dev(self, d_keys, key_pitch, key_stride, num_keys, rec0, nrec,
                                d_result, stream=None):
        check(self._lib.pir_engine_answer_shamir_queue_dev(self._h, d_keys, key_pitch, key_stride,
                                                           num_keys, rec0, nrec, d_result, stream),
              "answer_shamir_queue_dev")

    def reserve_shamir_queue(self, num_keys):
        """Pre-size the work buffers for Shamir queues of up to num_keys keys (no allocation
        inside later answer_shamir_queue[_dev] calls)."""
        check(self._lib.pir_engine_reserve_shamir_queue(self._h, num_keys),
              "reserve_shamir_queue")

    @property
    def woodruff_m(self):
        """The Woodruff key length M of this engine's 2^n records (pir_engine_woodruff_m)."""
        return woodruff_m(self.n)

    @property
    def woodruff_fused_tile(self):
        """Records per tile of the single-launch Woodruff path for this engine's whole domain
        (0: its shape is not served, every answer takes the coefficient kernel + scan)."""
        return int(self._lib.pir_engine_woodruff_fused_tile(self._h))

    def answer_woodruff(self, key, rec0=0, nrec=None):
        """Woodruff value answer (runWoodruffQueryThread, src/c/server.cpp:564-616) of a
        one-round engine: key is woodruff_m bytes; XOR over the records i of [rec0, rec0 + nrec)
        of key[a_i] * key[b_i] * row_i, (a_i, b_i) the i-th 2-subset of [0, M).
        -> (record_bytes,) uint8."""
        k = np.ascontiguousarray(np.asarray(key, np.uint8).reshape(-1))
        nrec = self.num_rows - rec0 if nrec is None else nrec
        out = np.empty(self.record_bytes, np.uint8)
        check(self._lib.pir_engine_answer_woodruff(self._h, k.ctypes.data_as(ctypes.c_void_p),
                                                   k.size, rec0, nrec,
                                                   out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_answer_woodruff")
        return out

    def answer_woodruff_deriv(self, key, rec0=0, nrec=None):
        """Woodruff derivative answers (WOODRUFF_DERIVATIVE = 1, server.cpp:618-644):
        -> (woodruff_m + 1, record_bytes): the value answer, then for j < M the XOR over the
        records whose pair holds j of key[the pair's other index] * row."""
        k = np.ascontiguousarray(np.asarray(key, np.uint8).reshape(-1))
        nrec = self.num_rows - rec0 if nrec is None else nrec
        out = np.empty((k.size + 1, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_answer_woodruff_deriv(self._h,
                                                         k.ctypes.data_as(ctypes.c_void_p),
                                                         k.size, rec0, nrec,
                                                         out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_answer_woodruff_deriv")
        return out

    def answer_woodruff_deriv_dev(self, d_key, key_len, rec0, nrec, d_result, stream=None):
        check(self._lib.pir_engine_answer_woodruff_deriv_dev(self._h, d_key, key_len, rec0, nrec,
                                                             d_result, stream),
              "answer_woodruff_deriv_dev")

    def answer_woodruff_dev(self, d_key, key_len, rec0, nrec, d_result, stream=None):
        check(self._lib.pir_engine_answer_woodruff_dev(self._h, d_key, key_len, rec0, nrec,
                                                       d_result, stream), "answer_woodruff_dev")

    def answer_woodruff_queue(self, keys, rec0=0, nrec=None):
        """A queue of independent Woodruff value queries over the records [rec0, rec0 + nrec):
        keys is a list of keys or a (K, woodruff_m) array -> (K, record_bytes) uint8, row k what
        answer_woodruff gives for key k.  Where it measured faster the queued keys share passes
        over the shard (8 keys per read of it; $PIR_WD_SHARE, $PIR_WD_G: include/pir_engine.h),
        else each key has its own answer, back to back."""
        ks = [np.asarray(k, np.uint8).reshape(-1) for k in keys]
        nk = len(ks)
        key_len = ks[0].size if nk else self.woodruff_m
        if any(k.size != key_len for k in ks):
            raise _lib.PirError("answer_woodruff_queue: keys of different lengths")
        k = np.ascontiguousarray(np.concatenate(ks)) if nk else np.zeros(1, np.uint8)
        nrec = self.num_rows - rec0 if nrec is None else nrec
        out = np.empty((nk, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_answer_woodruff_queue(self._h, k.ctypes.data_as(ctypes.c_void_p),
                                                         key_len, nk, rec0, nrec,
                                                         out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_answer_woodruff_queue")
        return out

    def answer_woodruff_queue_dev(self, d_keys, key_len, num_keys, rec0, nrec, d_result,
                                  stream=None):
        check(self._lib.pir_engine_answer_woodruff_queue_dev(self._h, d_keys, key_len, num_keys,
                                                             rec0, nrec, d_result, stream),
              "answer_woodruff_queue_dev")

    def reserve_woodruff_queue(self, num_keys):
        """Pre-size the work buffers for Woodruff queues of up to num_keys keys (no allocation
        inside later answer_woodruff_queue[_dev] calls)."""
        check(self._lib.pir_engine_reserve_woodruff_queue(self._h, num_keys),
              "reserve_woodruff_queue")

    def answer_woodruff_deriv_queue(self, keys, rec0=0, nrec=None):
        """A queue of independent Woodruff derivative queries over the records [rec0, rec0 +
        nrec): keys is a list of keys or a (K, woodruff_m) array -> (K, woodruff_m + 1,
        record_bytes) uint8, answer k what answer_woodruff_deriv gives for key k.  Where it
        measured faster the queued keys share the two passes over the shard (8 keys per read of
        it; $PIR_WDD_SHARE, $PIR_WDD_G: include/pir_engine.h), else each key has its own answer,
        back to back."""
        ks = [np.asarray(k, np.uint8).reshape(-1) for k in keys]
        nk = len(ks)
        key_len = ks[0].size if nk else self.woodruff_m
        if any(k.size != key_len for k in ks):
            raise _lib.PirError("answer_woodruff_deriv_queue: keys of different lengths")
        k = np.ascontiguousarray(np.concatenate(ks)) if nk else np.zeros(1, np.uint8)
        nrec = self.num_rows - rec0 if nrec is None else nrec
        out = np.empty((nk, key_len + 1, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_answer_woodruff_deriv_queue(
            self._h, k.ctypes.data_as(ctypes.c_void_p), key_len, nk, rec0, nrec,
            out.ctypes.data_as(ctypes.c_void_p)), "pir_engine_answer_woodruff_deriv_queue")
        return out

    def answer_woodruff_deriv_queue_dev(self, d_keys, key_len, num_keys, rec0, nrec, d_result,
                                        stream=None):
        check(self._lib.pir_engine_answer_woodruff_deriv_queue_dev(
            self._h, d_keys, key_len, num_keys, rec0, nrec, d_result, stream),
            "answer_woodruff_deriv_queue_dev")

    def reserve_woodruff_deriv_queue(self, num_keys):
        """Pre-size the work buffers for Woodruff derivative queues of up to num_keys keys (no
        allocation inside later answer_woodruff_deriv_queue[_dev] calls)."""
        check(self._lib.pir_engine_reserve_woodruff_deriv_queue(self._h, num_keys),
              "reserve_woodruff_deriv_queue")

    def answer_mp(self, key, p, t, thread_num=0, num_threads=1):
        """Multiparty sqrt(N) DPF answer (runOptimizedMultiPartyDPFQuery[Thread], src/c/
        server.cpp:136-176, :384-430): the key's NUM_RSS_KEYS shares of every record (the
        layout of multiparty_dpf.cpp:467-539) scanned against the shard.  The engine's
        num_rounds must be mp_num_keys(p, t).  -> (num_rounds, record_bytes)."""
        k = np.frombuffer(bytes(key), np.uint8) if not isinstance(key, np.ndarray) else \
            np.ascontiguousarray(key, np.uint8)
        out = np.empty((self.num_rounds, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_answer_mp(self._h, k.ctypes.data_as(ctypes.c_void_p), k.size,
                                             p, t, thread_num, num_threads,
                                             out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_answer_mp")
        return out

    def answer_mp_dev(self, d_key, p, t, d_result, thread_num=0, num_threads=1, stream=None):
        check(self._lib.pir_engine_answer_mp_dev(self._h, d_key, p, t, thread_num, num_threads,
                                                 d_result, stream), "answer_mp_dev")

    def answer_cd(self, key, num_cd_keys_needed, num_cd_keys, thread_num=0, num_threads=1):
        """Covering-design sqrt(N) DPF answer (runCDQueryThread, src/c/server.cpp:443-492): the
        key's NUM_CD_KEYS shares (evalAllCDThread's layout, multiparty_dpf.cpp:617-690) scanned
        against the shard.  The engine's num_rounds must be num_cd_keys.
        -> (num_rounds, record_bytes)."""
        k = np.frombuffer(bytes(key), np.uint8) if not isinstance(key, np.ndarray) else \
            np.ascontiguousarray(key, np.uint8)
        out = np.empty((self.num_rounds, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_answer_cd(self._h, k.ctypes.data_as(ctypes.c_void_p), k.size,
                                             num_cd_keys_needed, num_cd_keys, thread_num,
                                             num_threads, out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_answer_cd")
        return out

    def answer_cd_dev(self, d_key, num_cd_keys_needed, num_cd_keys, d_result, thread_num=0,
                      num_threads=1, stream=None):
        check(self._lib.pir_engine_answer_cd_dev(self._h, d_key, num_cd_keys_needed, num_cd_keys,
                                                 thread_num, num_threads, d_result, stream),
              "answer_cd_dev")

    # -- queues of explicit-coefficient, multiparty and covering-design queries ----------------
    def answer_coefs_queue(self, coefs, row0=0, nrows=None):
        """A queue of independent explicit-coefficient queries over the rows [row0, row0 +
        nrows): coefs is (K, num_rounds, rows) uint8 -> (K, num_rounds, record_bytes), row k what
        answer_coefs gives for coefs[k].  Where it measured faster the queued keys share passes
        over the shard (8 / nrp keys per read of it; $PIR_GQ_SHARE, $PIR_GQ_G:
        include/pir_engine.h), else each key has its own answer, back to back."""
        nk = len(coefs)
        c = np.ascontiguousarray(np.asarray(coefs, np.uint8).reshape(nk, self.num_rounds, -1)) \
            if nk else np.zeros((0, self.num_rounds, self.num_rows), np.uint8)
        nrows = c.shape[2] - row0 if nrows is None else nrows
        ptrs = (ctypes.c_void_p * max(1, nk * self.num_rounds))(
            *[c[k, a].ctypes.data for k in range(nk) for a in range(self.num_rounds)])
        out = np.empty((nk, self.num_rounds, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_answer_coefs_queue(self._h, ptrs, nk, row0, nrows,
                                                      out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_answer_coefs_queue")
        return out

    def answer_coefs_queue_dev(self, d_coefs, coef_pitch, key_stride, num_keys, row0, nrows,
                               d_result, stream=None):
        check(self._lib.pir_engine_answer_coefs_queue_dev(self._h, d_coefs, coef_pitch, key_stride,
                                                          num_keys, row0, nrows, d_result, stream),
              "answer_coefs_queue_dev")

    def _queue_keys(self, keys, what):
        ks = [np.frombuffer(bytes(k), np.uint8) if not isinstance(k, np.ndarray)
              else np.asarray(k, np.uint8).reshape(-1) for k in keys]
        if any(k.size != ks[0].size for k in ks):
            raise _lib.PirError("%s: keys of different lengths" % what)
        k = np.ascontiguousarray(np.concatenate(ks)) if ks else np.zeros(1, np.uint8)
        return k, len(ks), (ks[0].size if ks else 0)

    def answer_mp_queue(self, keys, p, t, thread_num=0, num_threads=1):
        """A queue of independent multiparty sqrt(N) DPF queries (keys of one length) over one
        thread slice -> (K, num_rounds, record_bytes), row k what answer_mp gives for keys[k];
        sharing as answer_coefs_queue."""
        k, nk, kb = self._queue_keys(keys, "answer_mp_queue")
        out = np.empty((nk, self.num_rounds, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_answer_mp_queue(self._h, k.ctypes.data_as(ctypes.c_void_p), kb,
                                                   nk, p, t, thread_num, num_threads,
                                                   out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_answer_mp_queue")
        return out

    def answer_mp_queue_dev(self, d_keys, key_stride, num_keys, p, t, d_result, thread_num=0,
                            num_threads=1, stream=None):
        check(self._lib.pir_engine_answer_mp_queue_dev(self._h, d_keys, key_stride, num_keys, p, t,
                                                       thread_num, num_threads, d_result, stream),
              "answer_mp_queue_dev")

    def answer_cd_queue(self, keys, num_cd_keys_needed, num_cd_keys, thread_num=0, num_threads=1):
        """A queue of independent covering-design sqrt(N) DPF queries -> (K, num_rounds,
        record_bytes), row k what answer_cd gives for keys[k]; sharing as answer_coefs_queue."""
        k, nk, kb = self._queue_keys(keys, "answer_cd_queue")
        out = np.empty((nk, self.num_rounds, self.record_bytes), np.uint8)
        check(self._lib.pir_engine_answer_cd_queue(self._h, k.ctypes.data_as(ctypes.c_void_p), kb,
                                                   nk, num_cd_keys_needed, num_cd_keys, thread_num,
                                                   num_threads,
                                                   out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_answer_cd_queue")
        return out

    def answer_cd_queue_dev(self, d_keys, key_stride, num_keys, num_cd_keys_needed, num_cd_keys,
                            d_result, thread_num=0, num_threads=1, stream=None):
        check(self._lib.pir_engine_answer_cd_queue_dev(self._h, d_keys, key_stride, num_keys,
                                                       num_cd_keys_needed, num_cd_keys, thread_num,
                                                       num_threads, d_result, stream),
              "answer_cd_queue_dev")

    def reserve_group_queue(self, num_keys):
        """Pre-size the work buffers for explicit-coefficient and sqrt(N) DPF queues of up to
        num_keys keys (no allocation inside later queue calls)."""
        check(self._lib.pir_engine_reserve_group_queue(self._h, num_keys), "reserve_group_queue")

    def eval_all(self, key):
        """(num_rounds, rows) DPF shares dataShare[a][i]."""
        k, kp = self._check_key(key)
        out = np.empty((self.num_rounds, self.num_rows), np.uint8)
        check(self._lib.pir_engine_eval_all(self._h, kp, out.ctypes.data_as(ctypes.c_void_p)),
              "pir_engine_eval_all")
        return out

    # -- device-resident path ----------------------------------------------------------------
    def alloc_dev(self, nbytes):
        p = ctypes.c_void_p()
        check(self._lib.pir_engine_alloc_dev(self._h, nbytes, ctypes.byref(p)), "alloc_dev")
        return p.value

    def free_dev(self, d_ptr):
        check(self._lib.pir_engine_free_dev(self._h, d_ptr), "free_dev")

    def set_party(self, party_index):
        """Answer later queries as party `party_index` over the same resident shard
        (server.partyIndex, src/c/server.h:16)."""
        check(self._lib.pir_engine_set_party_index(self._h, int(party_index)), "set_party_index")
        self.party_index = int(party_index)

    def fill_random_dev(self, d_ptr, nbytes, seed):
        """nbytes pseudo-random bytes from the engine's generator into device memory."""
        check(self._lib.pir_engine_fill_random_dev(self._h, d_ptr, nbytes, seed),
              "fill_random_dev")

    def h2d(self, d_ptr, host):
        h, hp = _buf(host)
        check(self._lib.pir_engine_memcpy_h2d(self._h, d_ptr, hp, h.size), "memcpy_h2d")

    def d2h(self, d_ptr, nbytes):
        out = np.empty(nbytes, np.uint8)
        check(self._lib.pir_engine_memcpy_d2h(self._h, out.ctypes.data_as(ctypes.c_void_p),
                                              d_ptr, nbytes), "memcpy_d2h")
        return out

    def answer_dev(self, d_key, d_result, stream=None):
        check(self._lib.pir_engine_answer_dev(self._h, d_key, d_result, stream), "answer_dev")

    def answer_batch_dev(self, d_keys, num_keys, d_result, stream=None):
        check(self._lib.pir_engine_answer_batch_dev(self._h, d_keys, num_keys, d_result, stream),
              "answer_batch_dev")

    def answer_stream_dev(self, d_keys, num_keys, d_result, stream=None):
        """A queue of independent queries (device pointers; asynchronous): each its own key and
        tree and the answer answer_dev would give.  Where it measured faster the queued keys
        share passes over the shard (8 keys per read of it; $PIR_STREAM_SHARE, $PIR_STREAM_G:
        include/pir_engine.h), else each has its own full pass, back to back in one launch."""
        check(self._lib.pir_engine_answer_stream_dev(self._h, d_keys, num_keys, d_result, stream),
              "answer_stream_dev")

    def reserve_queue(self, num_keys):
        """Pre-size the work buffers for queues of up to num_keys queries (no allocation, and
        so no device synchronisation, inside later answer_stream_dev calls)."""
        check(self._lib.pir_engine_reserve_queue(self._h, num_keys), "reserve_queue")

    def fold_image(self, op="report"):
        """The fold image (a bit-transposed second copy of the shard for the shared-queue scan;
        $PIR_FOLD_IMAGE, include/pir_engine.h): op = "report", "build" (now) or "drop".  Returns
        the bytes of a valid image held afterwards (0: none)."""
        held = ctypes.c_uint64(0)
        check(self._lib.pir_engine_fold_image(self._h, {"report": 0, "build": 1, "drop": 2}[op],
                                              ctypes.byref(held)), "fold_image")
        return held.value

    def answer_stream(self, keys):
        """Host form of answer_stream_dev: [num_keys, num_rounds, record_bytes]."""
        keys = [bytes(k) for k in keys]
        nk = len(keys)
        d_k = self.alloc_dev(max(1, nk * self.key_len))
        try:
            d_r = self.alloc_dev(max(1, nk * self.answer_bytes))
            try:
                if nk:
                    self.h2d(d_k, b"".join(keys))
                self.answer_stream_dev(d_k, nk, d_r)
                self.sync()
                out = self.d2h(d_r, nk * self.answer_bytes)
            finally:
                self.free_dev(d_r)
        finally:
            self.free_dev(d_k)
        return out.reshape(nk, self.num_rounds, self.record_bytes)

    @property
    def stream(self):
        return self._lib.pir_engine_stream(self._h)

    def sync(self):
        check(self._lib.pir_engine_sync(self._h), "pir_engine_sync")

    def set_profiling(self, slots=64):
        """Record per-phase HIP events for up to `slots` answers (0 turns profiling off)."""
        check(self._lib.pir_engine_set_profiling(self._h, int(slots)), "set_profiling")

    def last_timings(self):
        """{phase: mean ms} over the answers recorded since the previous call."""
        arr = (_lib.PirKernelTime * 16)()
        n = self._lib.pir_engine_last_timings(self._h, arr, 16)
        if n < 0:
            check(n, "last_timings")
        return {arr[i].name.decode(): float(arr[i].ms) for i in range(n)}

    def profile_phases(self, d_key, iters=10):
        """Each phase alone (diagnostics): {phase: mean ms}."""
        out = (ctypes.c_float * 5)()
        check(self._lib.pir_engine_profile_phases(self._h, d_key, iters, out), "profile_phases")
        names = ["key_prep", "tree_frontier", "tree_stages", "scan", "reduce"]
        return {n: float(out[i]) for i, n in enumerate(names)}

    TRACE_PHASES = ["start", "key_parsed", "first_tile_root", "tile0_ready", "last_tile_ready",
                    "scan_done", "end"]

    def trace_query(self, d_key, num_keys=1):
        """One single-launch answer of a queue of num_keys keys (at d_key, key_len apart) with
        per-workgroup phase stamps (diagnostics): an array [workgroups, 256] of microseconds
        since the earliest workgroup start (layout: pir_engine_trace_query in
        include/pir_engine.h; 0 = stamp not reached; columns 56-57, 59-61, 128-159 and 192-255
        are raw shader-clock ticks or counts, divided by 100 like the rest)."""
        out = np.zeros((4096, 256), np.uint64)
        n = self._lib.pir_engine_trace_query(self._h, d_key, num_keys,
                                             out.ctypes.data_as(ctypes.c_void_p), 4096)
        check(min(n, 0), "trace_query")
        return out[:n].astype(np.float64) / 100.0

    # -- split shard ---------------------------------------------------------------------------
    def attach_comm(self, unique_id, nranks, rank):
        uid, up = _buf(unique_id)
        check(self._lib.pir_comm_attach(self._h, up, nranks, rank), "pir_comm_attach")

    def detach_comm(self):
        """Drop the communicator (aborted): this engine answers its partition alone again."""
        check(self._lib.pir_comm_detach(self._h), "pir_comm_detach")

    def comm_info(self):
        """RCCL's own view of this engine's communicator (ncclCommCount, ncclCommUserRank,
        ncclCommCuDevice; -1 when none is attached) and the engine device's PCI bus id."""
        ci = _lib.PirCommInfo()
        check(self._lib.pir_comm_info(self._h, ctypes.byref(ci)), "pir_comm_info")
        return {"attached": bool(ci.attached), "rccl_count": ci.count,
                "rccl_user_rank": ci.user_rank, "rccl_device": ci.device,
                "engine_device": ci.engine_device,
                "pci_bus_id": ci.pci_bus_id.decode(errors="replace")}


def shamir_response_len(log_domain, record_bytes):
    """calcShamirResponseLength: (2^x + 2^y + 2) * record_bytes, x = ceil(n/2), y = n - x."""
    return int(_lib.load().pir_engine_shamir_response_len(log_domain, record_bytes))


def woodruff_m(log_num_records):
    """WOODRUFF_M: the smallest M >= 3 with M (M - 1) / 2 >= 2^n (params.cpp:621-628); host only."""
    return int(_lib.load().pir_engine_woodruff_m(log_num_records))


def woodruff_pair(m, i):
    """The i-th 2-subset (a, b), a < b, of [0, m) in lexicographic order; host only."""
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    check(_lib.load().pir_engine_woodruff_pair(m, i, ctypes.byref(a), ctypes.byref(b)),
          "pir_engine_woodruff_pair")
    return a.value, b.value


def mp_num_keys(p, t):
    """NUM_RSS_KEYS = choose(p, t) * (p - t) / p (params.cpp:618): shares per multiparty key."""
    return _lib.load().pir_engine_mp_num_keys(p, t)


def mp_key_len(p, n, t):
    """calcMultiPartyOptDPFKeyLength (utils.cpp:105-116)."""
    return _lib.load().pir_engine_mp_key_len(p, n, t)


def cd_key_len(p, n, t, num_cd_keys_needed, num_cd_keys):
    """calcCDDPFKeyLength (utils.cpp:118-129) = the bytes evalAllCDThread reads; 0: no layout."""
    return _lib.load().pir_engine_cd_key_len(p, n, t, num_cd_keys_needed, num_cd_keys)


def mp_eval_bytes(p, n, t):
    """Key bytes the multiparty evaluation reads (multiparty_dpf.cpp:485-511); -1: no layout."""
    return _lib.load().pir_engine_mp_eval_bytes(p, n, t)


def comm_unique_id():
    out = np.zeros(128, np.uint8)
    check(_lib.load().pir_comm_unique_id(out.ctypes.data_as(ctypes.c_void_p)), "pir_comm_unique_id")
    return out.tobytes()
