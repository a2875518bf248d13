/* pir_client.h -- client-side helpers of the tree-DPF PIR protocol, on the GPU.
 *
 * Key generation (the client's half of the hot path's input) runs the same device AES as the
 * engine.  Replaces (paths relative to /root/reference/src/c):
 *   pir_gen_keys       genOptimizedDPF          dpf_tree.cpp:142-274 (root seeds supplied by the
 *                                               caller; the reference draws them with RAND_bytes)
 *   pir_final_cw       generate_opt_DPF_tree_query's finalCW values   client.cpp:144-153
 *   pir_gen_hollanti_keys*  genHollantiDPF      shamir_dpf.cpp:190-237 (random bytes from an
 *                                               AES-CTR stream under a caller-supplied seed)
 *   pir_mac_files_*    the CheckMAC record tags of initialize_client  client.cpp:29-31
 *   pir_mac_check      the client's check of a decoded record         benchmark.go:190-207
 */
#ifndef PIR_CLIENT_H
#define PIR_CLIENT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* keys_out: p keys of pir_engine_key_len(p, n, nq) bytes, party j at keys_out + j*key_len.
 * fcw: nq*(p-1) bytes, fcw[a*(p-1) + j-1] = finalCW of party j (1 <= j < p) for round a.
 * root_seeds: p*16 bytes.  Synchronous; returns 0 or a negative PIR_E* code. */
int pir_gen_keys(int device, int n, uint64_t index, const uint8_t *fcw, int p, int nq,
                 const uint8_t *root_seeds, uint8_t *keys_out);
/* out[a*(p-1) + j-2] = gf_pow(j, rho*(a+1)) ^ 1 for j = 2..p, a < nq (GF(2^8)/0x11d) */
void pir_final_cw(int p, int nq, int rho, uint8_t *out);

/* ---- Hollanti (polynomial PIR, mode 3) coefficient vectors, generated on the GPU ----
 * genHollantiDPF (shamir_dpf.cpp:190-237) with the intended polynomial: for key k (record
 * indices[k], seed seeds + 16*k), party q < p, round a < nq and record x < num_records, over
 * GF(2^8)/0x11d,
 *   key[q][a][x] = (XOR_{m<t} rnd[a][m][x] * (q+1)^m) ^ ([x == index] * (q+1)^(t + (a+1)*rho - 1)).
 * The key stream: with G(key, n) = the first n bytes of AES-128-CTR under `key`, keystream block
 * j = AES_key(BE128(j)), j = 0, 1, ... (the reference's G, utils.cpp:37-51),
 *   sk = G(seed, 16*nq*t),  rnd[a][m][x] = G(sk[16*(a*t + m), +16), num_records)[x].
 * A seed is a secret of ONE query: the caller draws 16 fresh bytes per key from the OS CSPRNG
 * (getrandom, os.urandom), never a counter or a constant -- two queries under one seed differ
 * in the two records they ask for and nowhere else.
 *
 * party q, key k, round a, record x at d_keys[q*party_stride + k*key_stride + a*coef_pitch + x];
 * d_keys + q*party_stride is then the d_coefs of pir_engine_answer_coefs_queue_dev(coef_pitch,
 * key_stride) and, for one key, of pir_engine_answer_coefs_dev.  No byte at or past num_records
 * of a vector is written; vectors at 16-byte aligned addresses are written with 16-byte stores.
 * Asynchronous on `stream` (indices and seeds are read before the call returns).
 * PIR_EINVAL, checked before any device call: null pointers with num_keys > 0, num_keys < 0,
 * t < 1, nq < 1 or > PIR_MAX_ROUNDS, rho < 1, p < 1 or > PIR_MAX_PARTIES, t + rho*nq > 255,
 * num_records == 0 or > 2^36 (the 32-bit block counter), an index >= num_records,
 * coef_pitch < num_records, key_stride < nq*coef_pitch, party_stride < num_keys*key_stride.
 * num_keys == 0 returns PIR_OK and touches nothing. */
int pir_gen_hollanti_keys_dev(int device, uint64_t num_records, const uint64_t *indices,
                              int num_keys, int t, int p, int nq, int rho,
                              const uint8_t *seeds /* num_keys*16, host */, uint8_t *d_keys,
                              uint64_t coef_pitch, uint64_t key_stride, uint64_t party_stride,
                              void *stream);
/* host form: keys_out packed (p, num_keys, nq, num_records); synchronous */
int pir_gen_hollanti_keys(int device, uint64_t num_records, const uint64_t *indices, int num_keys,
                          int t, int p, int nq, int rho, const uint8_t *seeds, uint8_t *keys_out);

/* ---- record tags: HMAC-SHA256 under a 16-byte key (utils.cpp:32-34), computed on the GPU ---- */
#define PIR_MAC_BYTES 32
/* tag of row i (d_files + i*file_pitch, payload_bytes bytes) -> d_tags + i*tag_pitch, 32 bytes.
 * In place with d_tags = d_files + payload_bytes, tag_pitch = file_pitch (only [0, payload_bytes)
 * of a row is read).  Any alignment.  Asynchronous on `stream` (a hipStream_t of `device`, or
 * NULL).  num_files == 0 touches nothing; null pointers, payload_bytes == 0,
 * file_pitch < payload_bytes and tag_pitch < 32 are PIR_EINVAL. */
int pir_mac_files_dev(int device, const uint8_t *d_files, uint64_t file_pitch, uint64_t num_files,
                      uint32_t payload_bytes, const uint8_t key[16],
                      uint8_t *d_tags, uint64_t tag_pitch, void *stream);
/* host rows (client.unencoded_files): payloads staged through two pinned buffers in chunks of
 * ~64 MiB ($PIR_MAC_CHUNK_FILES, read per call: the chunk in files), tagged on the GPU, only the
 * tags copied back to files[i] + payload_bytes.  Synchronous. */
int pir_mac_files_rows(int device, uint8_t *const *files, uint64_t num_files,
                       uint32_t payload_bytes, const uint8_t key[16]);
/* host only, no GPU: 0 if record[payload_bytes, +32) is the tag of record[0, payload_bytes),
 * 1 if not, a negative PIR_E* code for bad arguments; the comparison does not exit early */
int pir_mac_check(const uint8_t *record, uint32_t payload_bytes, const uint8_t key[16]);

#ifdef __cplusplus
}
#endif
#endif
