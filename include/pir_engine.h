/* pir_engine.h -- C ABI of the MI355X tree-DPF PIR answer engine (libpir_engine.so).
 *
 * Plain pointers and sizes only.  One engine = one PIR server's shard (or one partition of
 * it) resident in the HBM of one GPU.  Every entry point returns 0 on success and a
 * negative PIR_E* code on failure (message: pir_engine_last_error()); the server.h-compatible
 * shim (pir_server.h) turns failures into abort(), like the reference's handleErrors()
 * (src/c/utils.cpp:11-15).
 *
 * Reference interfaces replaced (paths relative to /root/reference/src/c):
 *   pir_engine_create / _destroy     initializeServer / freeServer          server.cpp:17-52
 *   pir_engine_set_shard[_rows]      the indexList rows written by encode_across_files_server
 *                                                                           client.cpp:93-97
 *   pir_engine_answer                runOptimizedDPFTreeQuery               server.cpp:96-134
 *   pir_engine_answer_slice          runOptimizedDPFTreeQueryThread (intended semantics)
 *                                                                           server.cpp:505-549
 *   pir_engine_answer_slices[_dev]   the T concurrent ...Thread calls of one query
 *                                    (src/server_util/tree.go:60-76)        server.cpp:505-549
 *   pir_engine_eval_all              evalAllOptimizedDPF                    dpf_tree.cpp:473-598
 *   pir_engine_answer_coefs[_dev]    runHollantiQuery / ...Thread           server.cpp:321-371
 *   pir_engine_answer_shamir[_dev]   runOptShamirDPFQuery / ...Thread       server.cpp:203-302
 *   pir_engine_answer_shamir_queue[_dev]    K answers, 8 rounds per read of the shard
 *   pir_engine_reserve_shamir_queue         (no counterpart: the reference answers one key)
 *   pir_engine_encode_hermite_*      generate_hermite_within_file           client.cpp:57-68
 *   pir_engine_shamir_response_len   calcShamirResponseLength               utils.cpp:140-143
 *   pir_engine_answer_woodruff[_dev] runWoodruffQueryThread (value answer)  server.cpp:564-616
 *   pir_engine_answer_woodruff_deriv[_dev]  ... with WOODRUFF_DERIVATIVE    server.cpp:618-644
 *   pir_engine_answer_woodruff_queue[_dev]  K value answers, 8 keys per read of the shard
 *   pir_engine_reserve_woodruff_queue       (no counterpart: the reference answers one key)
 *   pir_engine_answer_woodruff_deriv_queue[_dev]  K derivative answers, 8 keys per read
 *   pir_engine_reserve_woodruff_deriv_queue (no counterpart: the reference answers one key)
 *   pir_engine_woodruff_m            calcWoodruffKeyLength / WOODRUFF_M     params.cpp:621-628
 *   pir_engine_woodruff_pair         makeCombi(M, 2)[i] - 1                 params.cpp:629-640
 *   pir_engine_answer_mp[_dev]       runOptimizedMultiPartyDPFQuery[Thread] server.cpp:136-176,
 *                                    (evalAllOptMultiPartyDPF[Thread])      :384-430,
 *                                                                 multiparty_dpf.cpp:467-615
 *   pir_engine_mp_key_len            calcMultiPartyOptDPFKeyLength          utils.cpp:105-116
 *   pir_engine_mp_num_keys           NUM_RSS_KEYS                           params.cpp:618
 *   pir_engine_answer_cd[_dev]       runCDQueryThread (evalAllCDThread)     server.cpp:443-492,
 *                                                                 multiparty_dpf.cpp:617-690
 *   pir_engine_cd_key_len            calcCDDPFKeyLength                     utils.cpp:118-129
 *   pir_engine_answer_coefs_queue[_dev]     K answers of one mode, 8 / nrp keys per read of the
 *   pir_engine_answer_mp_queue[_dev]        shard (no counterpart: the reference answers one key)
 *   pir_engine_answer_cd_queue[_dev]
 *   pir_engine_reserve_group_queue
 *   pir_engine_key_len               calcOptimizedDPFTreeKeyLength          utils.cpp:85-90
 *   pir_comm_* + partitions          (new) split-shard across GPUs, XOR all-reduce over RCCL
 */
#ifndef PIR_ENGINE_H
#define PIR_ENGINE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIR_OK 0
#define PIR_EINVAL (-1)  /* bad argument / unsupported shape          */
#define PIR_EHIP (-2)    /* a HIP runtime call failed                  */
#define PIR_ENOMEM (-3)  /* device or host allocation failed           */
#define PIR_ECOMM (-4)   /* RCCL failure                               */
#define PIR_ESTATE (-5)  /* call not valid in the engine's state       */

#define PIR_MAX_PARTIES 17 /* p - 1 <= 16 control bits                   */
#define PIR_MAX_ROUNDS 16  /* NUM_ROUNDS bytes come from one AES block   */
#define PIR_MAX_LOG_RECORDS 40

typedef struct pir_engine pir_engine_t;

typedef struct {
    int device;             /* HIP device ordinal                                     */
    int num_parties;        /* p = NUM_PARTIES (2..17)                                */
    int party_index;        /* 1-based, as server.partyIndex                          */
    int log_num_records;    /* n = LOG_NUM_ENCODED_FILES: depth of the DPF tree       */
    uint32_t record_bytes;  /* ENCODED_FILE_SIZE_BYTES                                */
    int num_rounds;         /* NUM_ROUNDS (1..16): output bytes per leaf              */
    int log_num_partitions; /* G: the logical shard is split into 2^G row partitions  */
    int partition_index;    /* which partition this engine holds (0 when G == 0)      */
    int is_byzantine;       /* answers are random bytes (server.cpp:116-119)          */
} pir_engine_config;

const char *pir_engine_last_error(void);
int pir_engine_create(const pir_engine_config *cfg, pir_engine_t **out);
void pir_engine_destroy(pir_engine_t *e);
int pir_engine_key_len(int num_parties, int log_num_records, int num_rounds);
/* records (rows) held by this engine = 2^(n - G) */
uint64_t pir_engine_num_rows(const pir_engine_t *e);
/* answer later queries as party `party_index` (1-based) over the same shard: the reference's
 * server.partyIndex (server.h:16), which only selects the root control bits of the DPF
 * evaluation (dpf_tree.cpp:496-502).  Lets one resident shard serve every party's key in
 * tests and benchmarks without a second copy of it. */
int pir_engine_set_party_index(pir_engine_t *e, int party_index);

/* ---- shard (device-resident; rows are this engine's partition, row 0 = its first) ---- */
/* rows [row0, row0+nrows) from a host buffer with src_pitch bytes between rows */
int pir_engine_set_shard(pir_engine_t *e, const uint8_t *host, uint64_t row0, uint64_t nrows,
                         uint64_t src_pitch);
/* rows [row0, row0+nrows) from an array of row pointers (server.indexList): host threads
 * ($PIR_GATHER_THREADS, default min(8, cores)) gather ~64 MiB chunks into two pinned buffers,
 * chunk c + 1 while the DMA of chunk c runs */
int pir_engine_set_shard_rows(pir_engine_t *e, const uint8_t *const *rows, uint64_t row0,
                              uint64_t nrows);
/* the reverse: rows [row0, row0+nrows) of the device shard into row pointers (record_bytes
 * each), DMA into two pinned buffers, host threads scattering one while the other fills */
int pir_engine_get_shard_rows(pir_engine_t *e, uint8_t *const *rows, uint64_t row0,
                              uint64_t nrows);
/* synthetic shard generated on the device (bench): byte b of GLOBAL row i is a function of
 * (seed, i, b), so every partition of a logical shard agrees with the whole */
int pir_engine_fill_shard_random(pir_engine_t *e, uint64_t seed);
/* the server's erasure-coded shard, computed on the GPU (client.cpp:70-97, the server setup of
 * src/server/server.go:299-331): global row r = XOR_{j<k, src = encdb*j + r < num_files}
 * gf_pow(party_index, j) * file[src], encdb = ceil(num_files / k), for this engine's rows.
 * d_files: num_files device rows file_pitch bytes apart (record_bytes used), or NULL for the
 * reference's synthetic database (client.cpp:16-33). */
int pir_engine_encode_across_dev(pir_engine_t *e, const uint8_t *d_files, uint64_t file_pitch,
                                 uint64_t num_files, int k);
/* pir_engine_encode_across_dev(e, NULL, 0, num_files, k) for a CheckMAC setup: the synthetic
 * files are record_bytes - 32 payload bytes followed by HMAC-SHA256(key[16], payload)
 * (client.cpp:29-31).  The payloads take 257 values, so 257 tags are computed on the GPU
 * (pir_mac_files_dev's kernel) and the encode reads them from that table.  record_bytes < 33 is
 * PIR_EINVAL. */
int pir_engine_encode_across_synthetic_mac(pir_engine_t *e, uint64_t num_files, int k,
                                           const uint8_t key[16]);
/* pir_engine_encode_across_dev from the client's HOST file rows (client.unencoded_files:
 * num_files row pointers, record_bytes read from each): the server setup of server.go:299-331
 * with the encode on the GPU.  Per ~64 MiB chunk of this engine's rows, host threads gather the
 * k source files of each row into pinned staging (chunk c + 1 while chunk c's DMA and encode
 * kernel run); the shard is left resident in HBM. */
int pir_engine_encode_across_rows(pir_engine_t *e, const uint8_t *const *files,
                                  uint64_t num_files, int k);
/* the same for pir_engine_encode_within_dev: num_files host rows of file_bytes each */
int pir_engine_encode_within_rows(pir_engine_t *e, const uint8_t *const *files,
                                  uint64_t num_files, uint32_t file_bytes, int k, int party);
/* the Hollanti-mode shard (MODE 3: encoded within files), computed on the GPU (client.cpp:43-56,
 * 99-103; replaces the host encode_within_files_server of the server setup): row r of this
 * engine's rows = XOR_{j<k} gf_pow(party, j) * part j of file r, part j = bytes
 * [j*record_bytes, (j+1)*record_bytes) of the file, zero past file_bytes; rows >= num_files are
 * zero.  d_files: num_files device rows file_pitch >= file_bytes bytes apart, or NULL for the
 * reference's synthetic database (client.cpp:16-33).  party: the server's party index (1..),
 * or 0 for the engine's party_index (a Hollanti engine is created with 2 parties: they only
 * size tree-DPF keys). */
int pir_engine_encode_within_dev(pir_engine_t *e, const uint8_t *d_files, uint64_t file_pitch,
                                 uint64_t num_files, uint32_t file_bytes, int k, int party);
int pir_engine_get_shard_row(pir_engine_t *e, uint64_t row, uint8_t *out);
/* rows [row0, row0+nrows) back to the host, record_bytes per row, packed */
int pir_engine_get_shard(pir_engine_t *e, uint64_t row0, uint64_t nrows, uint8_t *out);

/* ---- live record updates: changed files patched into the resident shard, and into the fold
 *      image, in place (k_update_rows) ----
 * Every encoding above is linear over GF(2^8), so a file that changes from `old` to `new` changes
 * its coded rows by coefficient * (old ^ new).  All forms therefore take DELTAS, old ^ new: the
 * engine cannot recover `old` from a coded row.  After the call the shard equals, byte for byte,
 * what the matching encode call gives from the new files (the coefficients are the encoders'
 * own); the same record may appear more than once in a batch, and records that share a row or a
 * block of 4 rows may come together.  Partition engines take the same global indices as the
 * whole and skip the rows of other partitions.
 * The fold image survives: an update is not a rewrite.  A valid image is patched with the rows
 * and stays valid (pir_engine_fold_image(REPORT) still reports its size); without a valid image
 * there is none afterwards either, but a pass that wanted one before the update still counts, so
 * under $PIR_FOLD_IMAGE=1 the next sharing pass builds it; with $PIR_FOLD_IMAGE=0 only the rows
 * are touched.
 * Ordering: an update runs after every answer enqueued before it, on any stream, and before
 * every answer enqueued after it.  The _dev forms are asynchronous on `stream` (NULL: the
 * engine's): the index array (host memory) is read before the call returns, the deltas (device
 * memory, any alignment, delta i at d_delta + i * delta_pitch) are read on the stream.  The forms
 * without _dev take host deltas, staged through an engine buffer, and wait for the update.
 * PIR_EINVAL, checked before any device call, the shard and the image untouched: null pointers
 * with num > 0, num < 0, an index at or beyond num_files (growing the database changes encdb: a
 * re-encode) or a row beyond the shard, k outside [1, 16], encdb beyond the domain, a pitch below
 * the bytes read, hermite on an engine with partitions or with one row, record_bytes < 33 for the
 * CheckMAC form.  num == 0: PIR_OK, nothing done. */
/* engine row rows[i] ^= delta i (record_bytes each); rows are this engine's row numbers */
int pir_engine_update_rows_dev(pir_engine_t *e, const uint64_t *rows, int num,
                               const uint8_t *d_delta, uint64_t delta_pitch, void *stream);
int pir_engine_update_rows(pir_engine_t *e, const uint64_t *rows, int num, const uint8_t *delta,
                           uint64_t delta_pitch);
/* file f = file_index[i] of an across-encoded database (pir_engine_encode_across_*): encdb =
 * ceil(num_files / k), j = f / encdb, global row r = f % encdb; row r ^= gf_pow(party_index, j) *
 * delta i (record_bytes) */
int pir_engine_update_across_dev(pir_engine_t *e, const uint64_t *file_index, int num,
                                 const uint8_t *d_delta, uint64_t delta_pitch, uint64_t num_files,
                                 int k, void *stream);
int pir_engine_update_across(pir_engine_t *e, const uint64_t *file_index, int num,
                             const uint8_t *delta, uint64_t delta_pitch, uint64_t num_files,
                             int k);
/* file r = file_index[i] of a within-encoded database (pir_engine_encode_within_*): global row r
 * ^= XOR_{j<k} gf_pow(party, j) * part j of delta i (file_bytes long, parts of record_bytes);
 * party as for the encode (0: the engine's).  hermite != 0 (a Shamir engine: no partitions, N =
 * rows / 2, num_files <= N): also row N + r ^= XOR_{odd j<k} gf_pow(party, j - 1) * part j
 * (pir_engine_encode_hermite_*) */
int pir_engine_update_within_dev(pir_engine_t *e, const uint64_t *file_index, int num,
                                 const uint8_t *d_delta, uint64_t delta_pitch, uint64_t num_files,
                                 uint32_t file_bytes, int k, int party, int hermite,
                                 void *stream);
int pir_engine_update_within(pir_engine_t *e, const uint64_t *file_index, int num,
                             const uint8_t *delta, uint64_t delta_pitch, uint64_t num_files,
                             uint32_t file_bytes, int k, int party, int hermite);
/* CheckMAC setups, across-encoded: d_old / d_new hold the old and new PAYLOADS (record_bytes - 32
 * bytes each, `pitch` apart, device memory); the engine tags both with HMAC-SHA256(key[16], .) on
 * the GPU, forms payload-delta || tag-delta and applies pir_engine_update_across_dev */
int pir_engine_update_across_mac_dev(pir_engine_t *e, const uint64_t *file_index, int num,
                                     const uint8_t *d_old, const uint8_t *d_new, uint64_t pitch,
                                     uint64_t num_files, int k, const uint8_t key[16],
                                     void *stream);

/* ---- answers, host buffers (synchronous; key_len bytes of key) ---- */
/* result: num_rounds * record_bytes bytes, round a at result + a*record_bytes.  With a
 * communicator attached (pir_comm_attach) every rank receives the XOR over partitions. */
int pir_engine_answer(pir_engine_t *e, const uint8_t *key, uint8_t *result);
/* partial answer over the engine rows [t*R/T, (t+1)*R/T), R = rows held, T a power of 2 */
int pir_engine_answer_slice(pir_engine_t *e, const uint8_t *key, int thread_num,
                            int num_threads, uint8_t *result);
/* every slice of one query at once: results[t] (t < num_threads, num_rounds * record_bytes
 * each, back to back) = pir_engine_answer_slice(e, key, t, num_threads, .) -- the T calls of
 * one query that src/server_util/tree.go:60-76 issues concurrently with the same key
 * (runOptimizedDPFTreeQueryThread, server.cpp:505-549), computed by ONE tree and ONE pass over
 * the shard where the shape allows (the pir_server.h shim serves its Thread calls from it) */
int pir_engine_answer_slices(pir_engine_t *e, const uint8_t *key, int num_threads,
                             uint8_t *results);
int pir_engine_answer_slices_dev(pir_engine_t *e, const uint8_t *d_key, int num_threads,
                                 uint8_t *d_results, void *stream);
/* ---- explicit-coefficient answers: the Hollanti/Goldberg polynomial-PIR server scan
 *      (runHollantiQuery / runHollantiQueryThread, server.cpp:321-371) -- no DPF, the client
 *      sends one coefficient vector per round ----
 * result[a] = XOR_{r in [row0, row0+nrows)} coefs[a][r] * shard row r over GF(2^8)/0x11d, for
 * a < num_rounds; coefs[a] is indexed by engine row (num_rounds host pointers).  Always the
 * honest answer: the reference's Thread variant ignores isByzantine (server.cpp:353-369). */
int pir_engine_answer_coefs(pir_engine_t *e, const uint8_t *const *coefs, uint64_t row0,
                            uint64_t nrows, uint8_t *result);
/* device form: round a's coefficient of engine row r at d_coefs[a * coef_pitch + r] */
int pir_engine_answer_coefs_dev(pir_engine_t *e, const uint8_t *d_coefs, uint64_t coef_pitch,
                                uint64_t row0, uint64_t nrows, uint8_t *d_result, void *stream);
/* ---- Shamir sqrt(N) mode (runOptShamirDPFQuery / ...Thread, server.cpp:203-319) ----
 * A Shamir engine is created with log_num_records = n + 1 and no partitions: rows [0, N), N =
 * 2^n, are the value rows and rows [N, 2N) the derivative ("Hermite") rows, the reference's
 * indexList layout (set_shard / get_shard address all 2N).  The value rows are a 2^x x 2^y
 * matrix, x = ceil(n/2), y = n - x, record i at delta = i >> y, gamma = i & (2^y - 1).  Round
 * a's key is 2^x + 2^y bytes: ky[delta] = key[a][delta], kx[gamma] = key[a][2^x + gamma].  Its
 * response is response_len = (2^x + 2^y + 2) * record_bytes bytes, over GF(2^8)/0x11d:
 *   record delta          Rx[delta] = XOR_gamma kx[gamma] * A[delta][gamma]
 *   record 2^x + gamma    Ry[gamma] = XOR_delta ky[delta] * A[delta][gamma]
 *   record 2^x + 2^y      XOR kx[gamma] ky[delta] * H[delta][gamma]
 *   record 2^x + 2^y + 1  XOR kx[gamma] ky[delta] * A[delta][gamma]
 * with every sum restricted to the records [rec0, rec0 + nrec) of the domain (the Thread form's
 * [startIndex, endIndex); partial responses XOR to the whole).  result: num_rounds x
 * response_len bytes.  A Byzantine engine answers the whole-domain call (rec0 = 0, nrec = N)
 * with random bytes and every other range honestly, as the reference's two entry points do.
 * Three shard-sized passes (value rows twice, Hermite rows once) per group of up to 4 rounds. */
uint64_t pir_engine_shamir_response_len(int log_domain, uint32_t record_bytes);
int pir_engine_answer_shamir(pir_engine_t *e, const uint8_t *const *keys, uint64_t rec0,
                             uint64_t nrec, uint8_t *result);
/* device form: round a's key at d_keys + a * key_pitch; asynchronous on `stream` */
int pir_engine_answer_shamir_dev(pir_engine_t *e, const uint8_t *d_keys, uint64_t key_pitch,
                                 uint64_t rec0, uint64_t nrec, uint8_t *d_result, void *stream);
/* A queue of num_keys independent Shamir queries over the records [rec0, rec0 + nrec): key k's
 * round a at d_keys + k * key_stride + a * key_pitch (any alignment; the host form takes
 * num_keys * num_rounds pointers, key-major), results num_keys x num_rounds x response_len bytes
 * back to back, result k byte for byte what pir_engine_answer_shamir[_dev] gives for key k and
 * the same range.  The refusals are those of the single answer; num_keys < 0 and, with num_keys
 * > 0, null pointers are PIR_EINVAL; num_keys == 0 touches nothing, nrec == 0 zeroes every
 * result.  A Byzantine engine answers the whole-domain queue with random bytes, fresh for each
 * key, and every other range honestly.  A shared queue takes the num_keys * num_rounds rounds as
 * independent virtual keys in ceil(K R / 8) groups of as equal sizes as possible (20 -> 7 + 7 +
 * 6); a group's 8 key bytes of a matrix row or column are one 64-bit word, each of the two value
 * passes reads the value rows once for the group (a transposed four-Russians fold per matrix row
 * / column, the sums stored straight into the responses), and one 8-round scan reads the Hermite
 * rows once.  $PIR_SH_SHARE, read at engine creation: 0 never shares (the single answers back to
 * back on the stream), unset or 1 follows the measured policy (Queued Shamir queries
 * share shard passes), 2 shares every queue of two or more virtual keys over records of at least
 * 256 bytes (narrower records always run unshared); $PIR_SH_G overrides the slots per pass (2, 4
 * or 8; default 8).  The device form is asynchronous on `stream`. */
int pir_engine_answer_shamir_queue_dev(pir_engine_t *e, const uint8_t *d_keys, uint64_t key_pitch,
                                       uint64_t key_stride, int num_keys, uint64_t rec0,
                                       uint64_t nrec, uint8_t *d_result, void *stream);
int pir_engine_answer_shamir_queue(pir_engine_t *e, const uint8_t *const *keys, int num_keys,
                                   uint64_t rec0, uint64_t nrec, uint8_t *results);
/* pre-size everything the queue touches for up to num_keys keys, so that a later queue call
 * allocates nothing */
int pir_engine_reserve_shamir_queue(pir_engine_t *e, int num_keys);
/* the Hermite rows [N, 2N) of a Shamir engine (client.cpp:57-68, 103-107): row N + r = XOR over
 * odd j, 1 <= j < k, of gf_pow(party, j - 1) * part j of file r -- the formal derivative of the
 * within-file polynomial that pir_engine_encode_within_* evaluates; rows past num_files are
 * zero.  Files, synthetic database (d_files = NULL) and party as for encode_within.  The value
 * rows are not touched.  pir_engine_encode_within_* knows nothing of the two halves and zeroes
 * the rows past num_files: on a Shamir engine call it first, then this. */
int pir_engine_encode_hermite_dev(pir_engine_t *e, const uint8_t *d_files, uint64_t file_pitch,
                                  uint64_t num_files, uint32_t file_bytes, int k, int party);
int pir_engine_encode_hermite_rows(pir_engine_t *e, const uint8_t *const *files,
                                   uint64_t num_files, uint32_t file_bytes, int k, int party);
/* ---- Woodruff mode (runWoodruffQueryThread, server.cpp:564-616, WOODRUFF_D = 2) ----
 * A Woodruff engine has num_rounds = 1, no partitions and no communicator; its N = 2^n rows are
 * the records.  The key is M bytes, M the smallest integer >= 3 with M (M - 1) / 2 >= N
 * (pir_engine_woodruff_m; 0 for n outside [0, 31]).  Record i belongs to the i-th pair (a, b),
 * 0 <= a < b < M, in lexicographic order (pir_engine_woodruff_pair, exact for every i < 2^32:
 * start(a) = a (2M - a - 1) / 2 <= i < start(a + 1), b = a + 1 + i - start(a)); pairs of rank
 * >= N are unused.  The value answer over the records [rec0, rec0 + nrec) (the Thread form's
 * [startIndex, endIndex); partial answers XOR to the whole), over GF(2^8)/0x11d:
 *     result = XOR_i key[a_i] * key[b_i] * row_i                   (record_bytes bytes)
 * The derivative answers (WOODRUFF_DERIVATIVE = 1, server.cpp:618-644) are M + 1 records of
 * record_bytes bytes:
 *     result[0]     = the value answer
 *     result[1 + j] = XOR_{i : j in {a_i, b_i}} key[the other index] * row_i,   j < M
 * All M + 1 are overwritten (the reference zeroes only the first and XORs into whatever the
 * caller's other M buffers held).  Two passes over the shard.
 * isByzantine changes nothing in the reference (both branches are the same) and nothing here.
 * Both helpers are host only and need no GPU. */
uint32_t pir_engine_woodruff_m(int log_num_records);
int pir_engine_woodruff_pair(uint32_t m, uint64_t i, uint32_t *a, uint32_t *b);
int pir_engine_answer_woodruff(pir_engine_t *e, const uint8_t *key, uint64_t key_len,
                               uint64_t rec0, uint64_t nrec, uint8_t *result);
/* device form: key and result in device memory (any alignment); asynchronous on `stream` */
int pir_engine_answer_woodruff_dev(pir_engine_t *e, const uint8_t *d_key, uint64_t key_len,
                                   uint64_t rec0, uint64_t nrec, uint8_t *d_result, void *stream);
int pir_engine_answer_woodruff_deriv(pir_engine_t *e, const uint8_t *key, uint64_t key_len,
                                     uint64_t rec0, uint64_t nrec, uint8_t *result);
int pir_engine_answer_woodruff_deriv_dev(pir_engine_t *e, const uint8_t *d_key, uint64_t key_len,
                                         uint64_t rec0, uint64_t nrec, uint8_t *d_result,
                                         void *stream);
/* A queue of num_keys independent Woodruff value queries over the records [rec0, rec0 + nrec):
 * keys of key_len = M bytes back to back, results num_keys x record_bytes back to back, result k
 * byte for byte what pir_engine_answer_woodruff[_dev] gives for key k and the same range.  The
 * refusals are those of the single answer; num_keys < 0 and, with num_keys > 0, null pointers are
 * PIR_EINVAL; num_keys == 0 writes nothing, nrec == 0 zeroes every result.  A shared queue goes
 * into ceil(K / G) groups of as equal sizes as possible (20 -> 7 + 7 + 6); one coefficient kernel
 * writes a group's pair products for every record (the keys interleaved, the group's products
 * one packed GF(2^8) multiply) and one G-round scan reads the shard once for the group.
 * $PIR_WD_SHARE, read at engine creation: 0 never shares (the single answers back to back on the
 * stream), unset or 1 follows the measured policy (Queued Woodruff queries share
 * shard passes), 2 shares every queue of two or more keys; $PIR_WD_G overrides the keys per pass
 * (2, 4 or 8; default 8).  The device form is asynchronous on `stream`; the keys may have any
 * alignment. */
int pir_engine_answer_woodruff_queue_dev(pir_engine_t *e, const uint8_t *d_keys, uint64_t key_len,
                                         int num_keys, uint64_t rec0, uint64_t nrec,
                                         uint8_t *d_result, void *stream);
int pir_engine_answer_woodruff_queue(pir_engine_t *e, const uint8_t *keys, uint64_t key_len,
                                     int num_keys, uint64_t rec0, uint64_t nrec, uint8_t *results);
/* pre-size everything the queue touches for up to num_keys keys, so that a later queue call
 * allocates nothing (as pir_engine_reserve_queue does for tree queues) */
int pir_engine_reserve_woodruff_queue(pir_engine_t *e, int num_keys);
/* A queue of num_keys independent Woodruff derivative queries over the records [rec0, rec0 +
 * nrec): keys of key_len = M bytes back to back (any alignment), results num_keys x (M + 1) x
 * record_bytes back to back, result k byte for byte what pir_engine_answer_woodruff_deriv[_dev]
 * gives for key k and the same range.  The refusals are those of the single answer; num_keys < 0
 * and, with num_keys > 0, null pointers are PIR_EINVAL; num_keys == 0 touches nothing, nrec == 0
 * zeroes every result.  A shared queue goes into ceil(K / G) groups of as equal sizes as possible
 * (20 -> 7 + 7 + 6); a group's 8 key bytes of an index are one 64-bit word, and each of the two
 * passes reads the shard once for the group: a transposed four-Russians fold per triangle row /
 * column, every key's sum put straight into its response (the rows pass stores, the columns pass
 * XORs into that), the totals kernel once per key between the two.  $PIR_WDD_SHARE, read at
 * engine creation: 0 never shares (the single answers back to back on the stream), unset or 1
 * follows the measured policy (Queued Woodruff derivative queries share shard passes),
 * 2 shares every queue of two or more keys over records of at least 256 bytes (narrower records
 * always run unshared); $PIR_WDD_G overrides the slots per pass (2, 4 or 8; default 8).  The
 * device form is asynchronous on `stream`. */
int pir_engine_answer_woodruff_deriv_queue_dev(pir_engine_t *e, const uint8_t *d_keys,
                                               uint64_t key_len, int num_keys, uint64_t rec0,
                                               uint64_t nrec, uint8_t *d_result, void *stream);
int pir_engine_answer_woodruff_deriv_queue(pir_engine_t *e, const uint8_t *keys, uint64_t key_len,
                                           int num_keys, uint64_t rec0, uint64_t nrec,
                                           uint8_t *results);
/* pre-size everything the queue touches for up to num_keys keys (the key table, the host form's
 * key and result staging), so that a later queue call allocates nothing */
int pir_engine_reserve_woodruff_deriv_queue(pir_engine_t *e, int num_keys);
/* the tile (records) of the single-launch path that answers this engine's whole domain when
 * $PIR_WD_FUSED selects it (k_query's Woodruff mode), 0 where its shape is not served and every
 * answer goes through the coefficient kernel + scan */
int pir_engine_woodruff_fused_tile(pir_engine_t *e);
/* Multiparty sqrt(N) DPF answer of party index 1..p with threshold t (the engine must have
 * num_rounds == pir_engine_mp_num_keys(p, t), one output share per round):
 *   result[a] = XOR_{r in rows} share[a][r] * shard row r,   a < NUM_RSS_KEYS,
 *   share[a][i*mu + x] = XOR_{j: toggle[a][i][j] != 0} G(seed[i][j], mu)[x] ^ cw[j][x]
 * over the key layout of multiparty_dpf.cpp:133-273 / :467-539 (seeds, toggle bytes, correction
 * words; mu = 2^ceil(log2(ceil(2^(n/2) * 2^((p-1)/2)))) records per row, nu = 2^n / mu rows).
 * rows: the thread slice [thread_num*S*mu, (thread_num+1)*S*mu), S = nu / num_threads, of
 * runOptimizedMultiPartyDPFQueryThread (num_threads = 1: the whole domain), within this engine's
 * partition.  key_bytes >= pir_engine_mp_eval_bytes(p, n, t) (the bytes the evaluation reads;
 * calcMultiPartyOptDPFKeyLength sizes the buffer the Go client sends).  Always the honest
 * answer (the Byzantine branch of server.cpp:157-160 is the caller's). */
int pir_engine_answer_mp(pir_engine_t *e, const uint8_t *key, uint64_t key_bytes, int p, int t,
                         int thread_num, int num_threads, uint8_t *result);
int pir_engine_answer_mp_dev(pir_engine_t *e, const uint8_t *d_key, int p, int t, int thread_num,
                             int num_threads, uint8_t *d_result, void *stream);
int pir_engine_mp_num_keys(int p, int t);
int pir_engine_mp_key_len(int p, int n, int t);
long long pir_engine_mp_eval_bytes(int p, int n, int t); /* -1: no layout for (p, n, t) */
/* Covering-design sqrt(N) DPF answer (runCDQueryThread, server.cpp:443-492): the multiparty
 * evaluation and scan above on the layout of evalAllCDThread (multiparty_dpf.cpp:617-690):
 * NUM_CD_KEYS output shares (the engine must have num_rounds == num_cd_keys), 2^(q-1) seeds per
 * row (q = NUM_CD_KEYS_NEEDED), mu = 2^(n/2 + 3) records per row (integer n / 2), nu = 2^n / mu
 * rows (0 when mu > 2^n: the answer is zero), the same thread slices.  key_bytes >=
 * pir_engine_cd_key_len(...) (= the bytes the evaluation reads).  Always the honest answer:
 * both branches of runCDQueryThread compute it (server.cpp:466-485). */
int pir_engine_answer_cd(pir_engine_t *e, const uint8_t *key, uint64_t key_bytes,
                         int num_cd_keys_needed, int num_cd_keys, int thread_num, int num_threads,
                         uint8_t *result);
int pir_engine_answer_cd_dev(pir_engine_t *e, const uint8_t *d_key, int num_cd_keys_needed,
                             int num_cd_keys, int thread_num, int num_threads, uint8_t *d_result,
                             void *stream);
/* calcCDDPFKeyLength(p, n, t, q, c) (p and t unused there too); 0 for no layout */
int pir_engine_cd_key_len(int p, int n, int t, int num_cd_keys_needed, int num_cd_keys);
/* ---- queues of explicit-coefficient, multiparty and covering-design queries ----
 * num_keys independent queries of one mode over one range or thread slice; results num_keys x
 * num_rounds x record_bytes back to back, result k byte for byte what the single call
 * (pir_engine_answer_coefs / _mp / _cd [_dev]) gives for key k with the same range or slice.  The
 * refusals are those of the single calls; num_keys < 0 and, with num_keys > 0, null pointers are
 * PIR_EINVAL; num_keys == 0 touches nothing; an empty range, an empty slice or nu == 0 zeroes
 * every result.  A shared queue goes into ceil(K / G) groups of as equal sizes as possible (20 ->
 * 7 + 7 + 6), G = 8 / nrp key slots per pass (nrp: num_rounds rounded up to a power of two; a
 * queue of an engine with nrp > 4 has one slot and runs unshared); one kernel writes a group's
 * W = G nrp share bytes of every record (k_interleave_coefs_g from the groups' vectors,
 * k_mp_shares_g from its sqrt(N) keys) and one W-round scan reads the shard once for the group.
 * $PIR_GQ_SHARE, read at engine creation: 0 never shares (the single answers back to back on the
 * stream), unset or 1 follows the measured policy (Queued Hollanti, multiparty and CD
 * queries), 2 shares every queue of two or more keys that has two or more slots; $PIR_GQ_G
 * overrides the slots per pass (2, 4 or 8, at most 8 / nrp).  A partition engine shares passes
 * over its partition; with a communicator attached the queue runs the single answers back to
 * back, each with its own exchange.
 * coefs_queue_dev: key k's round a coefficient of engine row r at d_coefs[k * key_stride + a *
 * coef_pitch + r] (any alignment; 16-byte aligned vectors are read fastest).  coefs_queue: coefs
 * holds num_keys * num_rounds host pointers, key-major (key k's round a at coefs[k * num_rounds +
 * a]), each a vector over the engine's rows; one group's vectors are staged at a time.
 * mp / cd _queue_dev: keys key_stride bytes apart (>= the bytes the evaluation reads), any
 * alignment and stride (keys whose address or stride is no multiple of 16 are copied to an aligned
 * staging buffer first, as the single answer does for one key).  mp / cd _queue: host keys
 * key_bytes apart (>= the bytes the evaluation reads). */
int pir_engine_answer_coefs_queue_dev(pir_engine_t *e, const uint8_t *d_coefs, uint64_t coef_pitch,
                                      uint64_t key_stride, int num_keys, uint64_t row0,
                                      uint64_t nrows, uint8_t *d_result, void *stream);
int pir_engine_answer_coefs_queue(pir_engine_t *e, const uint8_t *const *coefs, int num_keys,
                                  uint64_t row0, uint64_t nrows, uint8_t *results);
int pir_engine_answer_mp_queue_dev(pir_engine_t *e, const uint8_t *d_keys, uint64_t key_stride,
                                   int num_keys, int p, int t, int thread_num, int num_threads,
                                   uint8_t *d_result, void *stream);
int pir_engine_answer_mp_queue(pir_engine_t *e, const uint8_t *keys, uint64_t key_bytes,
                               int num_keys, int p, int t, int thread_num, int num_threads,
                               uint8_t *results);
int pir_engine_answer_cd_queue_dev(pir_engine_t *e, const uint8_t *d_keys, uint64_t key_stride,
                                   int num_keys, int num_cd_keys_needed, int num_cd_keys,
                                   int thread_num, int num_threads, uint8_t *d_result,
                                   void *stream);
int pir_engine_answer_cd_queue(pir_engine_t *e, const uint8_t *keys, uint64_t key_bytes,
                               int num_keys, int num_cd_keys_needed, int num_cd_keys,
                               int thread_num, int num_threads, uint8_t *results);
/* pre-size everything these queues touch for up to num_keys keys over the whole shard (the share
 * buffer of rows x 8 bytes, the slabs, the group answer, the host forms' staging, and the staging
 * of unaligned device keys for the longest sqrt(N) key a queue of this engine has brought so far),
 * so that a later queue call allocates nothing */
int pir_engine_reserve_group_queue(pir_engine_t *e, int num_keys);
/* DPF shares of this engine's rows: out[a*R + i] (dataShare[a][i]) */
int pir_engine_eval_all(pir_engine_t *e, const uint8_t *key, uint8_t *out);

/* ---- answers, device-resident (asynchronous on `stream`, a hipStream_t or NULL for the
 *      engine's own stream).  Answers share the engine's work buffers: one enqueued on a
 *      different stream than the previous answer waits on the device for that answer (an
 *      event recorded on the previous stream; answers that stay on one stream record none, so
 *      back-to-back launches there carry no event-record dispatch gap). ---- */
int pir_engine_answer_dev(pir_engine_t *e, const uint8_t *d_key, uint8_t *d_result,
                          void *stream);
/* `num_keys` keys of key_len bytes back to back; results num_keys x num_rounds x record_bytes.
 * Keys are answered in groups of pir_engine_batch_group() keys per pass over the shard (the
 * shard is read once per group, each key's tree is evaluated separately). */
int pir_engine_answer_batch_dev(pir_engine_t *e, const uint8_t *d_keys, int num_keys,
                                uint8_t *d_result, void *stream);
/* host-buffer form of the above (synchronous) */
int pir_engine_answer_batch(pir_engine_t *e, const uint8_t *keys, int num_keys,
                            uint8_t *results);
/* a queue of `num_keys` independent queries (keys of key_len bytes back to back; results
 * num_keys x num_rounds x record_bytes), each with its own DPF key and tree and the answer
 * pir_engine_answer_dev would give, byte for byte.  The queue is handed over whole and nothing
 * is returned before its end, so on shapes where that measured faster (one round, records of
 * 256 B - 1 KiB, >= 2^20 rows, >= 4 keys) the queued keys share passes over the shard: 8 keys
 * per read of it, as pir_engine_answer_batch_dev does.  Elsewhere every query has its own full
 * pass, back to back in one k_query launch where the shape allows (the tree of query k+1 built
 * while query k's rows stream).  $PIR_STREAM_SHARE, read at engine creation: 0 never shares,
 * unset or 1 follows that policy, 2 shares on every shape the batched path takes;
 * $PIR_STREAM_G overrides the keys per pass ($PIR_BATCH_G steers answer_batch only). */
int pir_engine_answer_stream_dev(pir_engine_t *e, const uint8_t *d_keys, int num_keys,
                                 uint8_t *d_result, void *stream);
/* pre-size the device work buffers of pir_engine_answer_stream_dev for queues of up to
 * `num_keys` queries (a server sizes its queue at setup), so that no answer call allocates
 * (k_query's slabs and scratch; for a shared queue the batch scan's slabs, both share buffers,
 * the batched node buffers, the parsed keys and, with a communicator, the partition buffers):
 * the reference has no counterpart (its buffers are host mallocs per call, server.cpp:108-114). */
int pir_engine_reserve_queue(pir_engine_t *e, int num_keys);
/* The fold image: a second copy of the shard (round_up(rows, 4) x padded record bytes of device
 * memory), bit-transposed once so that the shared-queue scan (k_scan_t) need not transpose it in
 * every pass.  Answers are the same with and without it.  $PIR_FOLD_IMAGE, read at engine
 * creation: 0 never; unset or 1 builds it in pir_engine_reserve_queue for a queue that shares
 * passes, and in a shared queue or batch that finds the shard unchanged since the previous one
 * wanted it (a shard rewritten between queries never pays a build), and only while a sixteenth
 * of the device's memory stays free afterwards -- else the answers run without it and
 * pir_engine_last_error says so once; 2 builds it wherever a pass can use it and fails where it
 * does not fit.  $PIR_FOLD_IMAGE_MAX_BYTES caps its size.  Every rewrite of the shard (set_shard,
 * fill, encode) drops it; a live update (pir_engine_update_*) patches it in place and keeps it.
 * op: report only, build now (synchronous; an error with $PIR_FOLD_IMAGE=0), or drop;
 * *bytes_held (may be NULL) = the bytes of a valid image afterwards, 0 without one. */
enum { PIR_FOLD_IMAGE_REPORT = 0, PIR_FOLD_IMAGE_BUILD = 1, PIR_FOLD_IMAGE_DROP = 2 };
int pir_engine_fold_image(pir_engine_t *e, int op, uint64_t *bytes_held);
/* keys per shard pass: 0 = automatic (8 / nrp), else a power of two <= 16 / nrp, where nrp =
 * num_rounds rounded up to a power of two.  Default from $PIR_BATCH_G. */
int pir_engine_set_batch_group(pir_engine_t *e, int keys_per_pass);
int pir_engine_batch_group(const pir_engine_t *e);
void *pir_engine_stream(pir_engine_t *e);
int pir_engine_sync(pir_engine_t *e);
/* device scratch the caller may use for keys/results (freed with the engine) */
int pir_engine_alloc_dev(pir_engine_t *e, size_t bytes, void **d_ptr);
/* release a pir_engine_alloc_dev buffer before the engine is destroyed (waits for the device) */
int pir_engine_free_dev(pir_engine_t *e, void *d_ptr);
/* `bytes` pseudo-random bytes, a function of (seed, position), written to d_dst by the engine's
 * generator on its stream (benchmarks: a device-resident database without a host copy) */
int pir_engine_fill_random_dev(pir_engine_t *e, void *d_dst, size_t bytes, uint64_t seed);
int pir_engine_memcpy_h2d(pir_engine_t *e, void *d_dst, const void *h_src, size_t bytes);
int pir_engine_memcpy_d2h(pir_engine_t *e, void *h_dst, const void *d_src, size_t bytes);

/* ---- per-phase device time of answers (HIP events on the answering stream) ---- */
/* phases: key_prep, tree_frontier, tree_leaves, scan, reduce, comm_fold, total, chunks, fused;
 * an answer in k_query (fused = 2) and a shared queue (fused = 0) have launch, scan, reduce,
 * comm_fold, total, fused, a shared queue's scan being its first kernel -> the end of its last
 * scan.  `slots` event sets are kept in a ring (0 = off), each remembering its answer's path;
 * last_timings averages the answers recorded since the previous read (at most `slots`), every
 * slot read by its own path and reported under the newest answer's phase names, fills up to
 * `max` {name, ms} pairs and returns the count.  A Shamir answer (fused = 4) reports k_query's
 * phase names: launch = start -> the response zeroed, scan = the rows pass, the strips pass and
 * the Hermite scan, reduce = the Hermite slabs' k_reduce + the totals kernel.  A Woodruff answer
 * (fused = 5: the single launch, 6: coefficient kernel + scan) reports them too: launch = start
 * -> the first kernel, scan = that kernel (6: both kernels), reduce = k_reduce; its derivative
 * answers (fused = 7): launch = start -> the answer zeroed, scan = the two passes, reduce = 0.
 * A shared Woodruff queue (fused = 8) has one event set: launch = start -> the first coefficient
 * kernel, scan = that -> the end of the last group's scan, reduce = the last group's k_reduce;
 * an unshared queue records what its single answers record.  A shared queue of
 * explicit-coefficient, multiparty or covering-design queries (fused = 9) has the same one event
 * set with its share kernel in the coefficient kernel's place; the single answers of these modes
 * record none.  A shared Shamir queue (fused = 10) has one event set: launch = start -> the
 * responses zeroed, scan = the first key table -> the end of the last group's Hermite scan,
 * reduce = the last group's k_reduce and totals kernels; an unshared one records what its single
 * answers record.  A shared Woodruff derivative queue (fused = 11) has one event set: launch =
 * start -> the responses zeroed, scan = the first key table -> the end of the last group's
 * columns pass, reduce = 0; an unshared one records what its single answers record (7). */
typedef struct {
    char name[32];
    float ms;
} pir_kernel_time;
int pir_engine_set_profiling(pir_engine_t *e, int slots);
int pir_engine_last_timings(pir_engine_t *e, pir_kernel_time *out, int max);
/* diagnostics: each phase run alone `iters` times back to back (no pipelining); out_ms[5] =
 * mean ms of key_prep, tree_frontier, tree_stages (all expand stages), scan (one launch over
 * all rows), reduce.  d_key: device pointer to one raw key. */
int pir_engine_profile_phases(pir_engine_t *e, const uint8_t *d_key, int iters, float *out_ms);
/* diagnostics: one single-launch answer (k_query) of a queue of num_keys keys with
 * per-workgroup phase stamps.  out holds max_wgs x 256 uint64 wall-clock ticks (100 MHz)
 * relative to the earliest start (0 = not reached): [0..6] start, key parsed, first tile root,
 * tile 0 shares ready, last tile of query 0 ready, query 0 scanned, query 0 slab written;
 * [8+d] descent level d of the first tile root (d < 32); [40+l] expansion level l of tile 0
 * (l < 16); [56], [57] shader clock (s_memtime) at start and at the first tile root; with
 * end-of-query work stealing (a lone query): [58] the tree waves' last chunk folded, [59] chunks
 * of other workgroups folded by this one's tree waves, [60] own chunks folded by the tree
 * waves, [61] own chunks folded by the scan waves (counts, not ticks); [64+g]
 * queue tile g ready, [96+g] queue tile g consumed by scan wave 0, [128+g] shader clock at
 * [64+g] (g < 32); [160+l] expansion level l of queue tile 1 (built by the tree waves beside
 * the scan), [176] its root ready; [192+8w+k] (diagnostic builds with -DPIR_FOLD_STAMPS=1
 * only) shader cycles of fold phase k of four-Russians scan wave w.  Returns the number
 * of workgroups (>= 0), or an error code; PIR_EINVAL when the shape does not use k_query. */
int pir_engine_trace_query(pir_engine_t *e, const uint8_t *d_key, int num_keys, uint64_t *out,
                           int max_wgs);

/* ---- split shard across GPUs: XOR all-reduce of partition answers over RCCL ---- */
#define PIR_COMM_ID_BYTES 128
int pir_comm_unique_id(uint8_t id[PIR_COMM_ID_BYTES]);
/* rank r of nranks; nranks must equal 2^G of the engine's config and r its partition.  Every
 * answer then ends with ONE ncclAllGather of the partition partials (all queued queries'
 * nq x efs answers, query-major) + the XOR fold below.  An exchange that fails or does not
 * enqueue within $PIR_COMM_TIMEOUT seconds (default 60) aborts the communicator; the engine
 * then refuses every later answer with PIR_ECOMM. */
int pir_comm_attach(pir_engine_t *e, const uint8_t id[PIR_COMM_ID_BYTES], int nranks, int rank);
/* drop the communicator (aborted, never waited on) and answer this partition alone again; also
 * clears the refusal state after a failed exchange.  For callers that fall back to exchanging
 * partition answers themselves when a communicator could not be set up on every rank.  Call it
 * with no answer in flight: it waits for the engine's own stream only, and an exchange enqueued
 * on a caller's stream would be cut off by the abort. */
int pir_comm_detach(pir_engine_t *e);
/* what RCCL and HIP report for this engine (a multi-GPU run's self-check): attached = 1 when a
 * communicator is attached; count, user_rank and device = ncclCommCount, ncclCommUserRank and
 * ncclCommCuDevice of that communicator (-1 when none); engine_device = the engine's HIP device;
 * pci_bus_id = hipDeviceGetPCIBusId of it (so N ranks can be checked to sit on N distinct GPUs). */
typedef struct pir_comm_info {
  int attached;
  int count;
  int user_rank;
  int device;
  int engine_device;
  char pci_bus_id[64];
} pir_comm_info_t;
int pir_comm_info(pir_engine_t *e, pir_comm_info_t *out);
/* the combine step after the all-gather, on its own: d_gathered = nranks blocks of
 * bytes_per_rank (rank r's partial answers at r * bytes_per_rank: ncclAllGather's output
 * layout); d_result[i] = XOR over r of d_gathered[r * bytes_per_rank + i] (the XOR assembly of
 * server.cpp:553-562 across partitions).  Exposed so that one GPU can check a multi-rank
 * combine against the whole-shard answer before any multi-GPU run. */
int pir_engine_fold_gathered_dev(pir_engine_t *e, const uint8_t *d_gathered, int nranks,
                                 uint64_t bytes_per_rank, uint8_t *d_result, void *stream);

#ifdef __cplusplus
}
#endif
#endif
