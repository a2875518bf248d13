// pir_engine_shamir.cpp -- explicit-coefficient answers, the Shamir sqrt(N) mode and its
// Hermite encode.
#include "pir_engine_internal.h"

using namespace eng;

int eng::check_rows(const pir_engine* e, uint64_t row0, uint64_t nrows) {
  if (row0 > e->rows || nrows > e->rows - row0)
    return fail(PIR_EINVAL, "rows [%llu,%llu) beyond the %llu held", (unsigned long long)row0,
                (unsigned long long)(row0 + nrows), (unsigned long long)e->rows);
  return PIR_OK;
}

// Explicit-coefficient answer (server.cpp:321-382): out[a] = XOR_{i < nrows} src[a*pitch + i] *
// shard[row0 + i].  The vectors are interleaved into the record-major share buffer, then the
// same GF(2^8) scan + slab reduce as the 2-kernel DPF path; with a communicator, the partition
// partials are combined like answers (all-gather + XOR fold).
int eng::answer_coefs_locked(pir_engine* e, const uint8_t* src, uint64_t pitch, uint64_t row0,
                             uint64_t nrows, uint8_t* d_result, hipStream_t s) {
  const auto& c = e->cfg;
  const size_t out_bytes = (size_t)c.num_rounds * c.record_bytes;
  uint8_t* out = e->comm ? e->d_part.p : d_result;
  e->ev = nullptr;
  if (nrows == 0) {
    HIP_TRY(hipMemsetAsync(out, 0, out_bytes, s));
  } else {
    const pir::ScanShape sh = pir::make_scan_shape(nrows, e->pitch, c.num_rounds, e->num_cus);
    int rc = e->d_slabs.reserve((size_t)sh.grid.x * sh.grid.y * sh.slab_bytes);
    if (rc) return rc;
    HIP_TRY(pir::launch_interleave_coefs(src, pitch, nrows, c.num_rounds, e->nrp, e->d_c, s));
    HIP_TRY(pir::launch_scan(sh, e->d_shard + row0 * e->pitch, nrows, e->d_c, e->d_slabs, false, s));
    HIP_TRY(pir::launch_reduce(sh, e->d_slabs, c.record_bytes, out, s));
  }
  if (e->comm) {
    if (int rc = exchange(e, e->d_part, out_bytes, e->d_gather, d_result, s)) return rc;
  }
  return PIR_OK;
}

namespace {

// Shamir sqrt(N) answer (server.cpp:203-319) over the records [rec0, rec0 + nrec) of the N =
// rows / 2 value rows (Hermite rows behind them): the response is zeroed, then per group of
// kShamirRounds rounds one rows pass (Rx) and one strips pass (Ry) over the value rows, one
// explicit-coefficient scan of the Hermite rows for every round's tot1, and k_shamir_totals
// (tot2 from the finished Rx).  d_result: num_rounds x response_len.
int answer_shamir_locked(pir_engine* e, const uint8_t* d_keys, uint64_t key_pitch, uint64_t rec0,
                         uint64_t nrec, uint8_t* d_result, hipStream_t s) {
  const auto& c = e->cfg;
  const uint64_t N = e->rows / 2;
  const pir::ShamirDims d = pir::shamir_dims(c.log_num_records - 1, c.record_bytes);
  const size_t out_bytes = (size_t)c.num_rounds * d.resp_len;
  e->ev = nullptr;
  hipEvent_t* ev = nullptr;
  if (!e->prof.empty()) {
    ev = prof_slot(e, 4, 1, true);
    HIP_TRY(hipEventRecord(ev[EV_START], s));
  }
  if (c.is_byzantine && rec0 == 0 && nrec == N) {  // server.cpp:214-217: random answer bytes
    HIP_TRY(pir::launch_fill_random(d_result, out_bytes, 0xB42u + (++e->byz_counter), s));
    if (ev)
      for (int i : {EV_SCAN_B, EV_SCAN_E, EV_RED, EV_END}) HIP_TRY(hipEventRecord(ev[i], s));
    return PIR_OK;
  }
  HIP_TRY(hipMemsetAsync(d_result, 0, out_bytes, s));
  if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_B], s));
  pir::ScanShape sh{};
  if (nrec) {
    sh = pir::make_scan_shape(nrec, e->pitch, c.num_rounds, e->num_cus);
    if (int rc = e->d_slabs.reserve((size_t)sh.grid.x * sh.grid.y * sh.slab_bytes)) return rc;
    for (int a0 = 0; a0 < c.num_rounds; a0 += pir::kShamirRounds) {
      const int nr = std::min(pir::kShamirRounds, c.num_rounds - a0);
      const uint8_t* k = d_keys + (uint64_t)a0 * key_pitch;
      uint8_t* out = d_result + (uint64_t)a0 * d.resp_len;
      HIP_TRY(pir::launch_shamir_rows(d, e->d_shard, e->pitch, c.record_bytes, k, key_pitch, nr,
                                      rec0, rec0 + nrec, out, s));
      HIP_TRY(pir::launch_shamir_strips(d, e->d_shard, e->pitch, c.record_bytes, k, key_pitch, nr,
                                        rec0, rec0 + nrec, out, s));
    }
    HIP_TRY(pir::launch_shamir_coefs(d, d_keys, key_pitch, c.num_rounds, e->nrp, rec0, rec0 + nrec,
                                     e->d_c, s));
    HIP_TRY(pir::launch_scan(sh, e->d_shard + (N + rec0) * e->pitch, nrec, e->d_c, e->d_slabs,
                             false, s));
  }
  if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_E], s));
  if (nrec) {
    HIP_TRY(pir::launch_reduce(sh, e->d_slabs, c.record_bytes, e->d_part, s));
  } else {
    HIP_TRY(hipMemsetAsync(e->d_part, 0, (size_t)c.num_rounds * c.record_bytes, s));
  }
  HIP_TRY(pir::launch_shamir_totals(d, c.record_bytes, d_keys, key_pitch, c.num_rounds, e->d_part,
                                    d_result, s));
  if (ev) {
    HIP_TRY(hipEventRecord(ev[EV_RED], s));
    HIP_TRY(hipEventRecord(ev[EV_END], s));
  }
  return PIR_OK;
}

// a Shamir engine holds value rows and Hermite rows (log_num_records = n + 1), unsplit
int check_shamir(const pir_engine* e, uint64_t rec0, uint64_t nrec) {
  if (e->cfg.log_num_partitions > 0)
    return fail(PIR_EINVAL, "the Shamir mode does not serve a split shard (2^%d partitions)",
                e->cfg.log_num_partitions);
  if (e->comm) return fail(PIR_EINVAL, "the Shamir mode does not answer through a communicator");
  if (e->cfg.log_num_records < 1)
    return fail(PIR_EINVAL, "a Shamir engine needs log_num_records = n + 1 >= 1 (value rows and "
                            "Hermite rows)");
  const uint64_t N = e->rows / 2;
  if (rec0 > N || nrec > N - rec0)
    return fail(PIR_EINVAL, "records [%llu,%llu) beyond the %llu value rows",
                (unsigned long long)rec0, (unsigned long long)(rec0 + nrec), (unsigned long long)N);
  return PIR_OK;
}

}  // namespace

extern "C" {

int pir_engine_answer_coefs_dev(pir_engine_t* e, const uint8_t* d_coefs, uint64_t coef_pitch,
                                uint64_t row0, uint64_t nrows, uint8_t* d_result, void* stream) {
  if (!e || !d_result || (!d_coefs && nrows)) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_rows(e, row0, nrows)) return rc;
  if (e->cfg.num_rounds > 1 && coef_pitch < row0 + nrows)
    return fail(PIR_EINVAL, "coef_pitch %llu < %llu rows", (unsigned long long)coef_pitch,
                (unsigned long long)(row0 + nrows));
  AnswerScope sc(e, stream);
  if (sc.rc()) return sc.rc();
  return sc.finish(answer_coefs_locked(e, d_coefs + row0, coef_pitch, row0, nrows, d_result,
                                       sc.stream()));
}

int pir_engine_answer_coefs(pir_engine_t* e, const uint8_t* const* coefs, uint64_t row0,
                            uint64_t nrows, uint8_t* result) {
  if (!e || !result || (!coefs && nrows)) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_rows(e, row0, nrows)) return rc;
  const auto& c = e->cfg;
  for (int a = 0; a < c.num_rounds && nrows; ++a)
    if (!coefs[a]) return fail(PIR_EINVAL, "null coefficient vector %d", a);
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  if (int rc = e->d_coef_stage.reserve(std::max<size_t>(1, (size_t)c.num_rounds * nrows))) return rc;
  for (int a = 0; a < c.num_rounds && nrows; ++a)  // only the rows answered travel
    HIP_TRY(hipMemcpyAsync(e->d_coef_stage + (size_t)a * nrows, coefs[a] + row0, nrows,
                           hipMemcpyHostToDevice, e->stream));
  if (int rc = sc.finish(answer_coefs_locked(e, e->d_coef_stage, nrows, row0, nrows, e->d_result,
                                             e->stream)))
    return rc;
  return download(result, e->d_result, (size_t)c.num_rounds * c.record_bytes, e->stream, e->h_res);
}

uint64_t pir_engine_shamir_response_len(int log_domain, uint32_t record_bytes) {
  if (log_domain < 0 || log_domain >= PIR_MAX_LOG_RECORDS) return 0;
  return pir::shamir_dims(log_domain, record_bytes).resp_len;
}

int pir_engine_answer_shamir_dev(pir_engine_t* e, const uint8_t* d_keys, uint64_t key_pitch,
                                 uint64_t rec0, uint64_t nrec, uint8_t* d_result, void* stream) {
  if (!e || !d_result || !d_keys) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_shamir(e, rec0, nrec)) return rc;
  const pir::ShamirDims d = pir::shamir_dims(e->cfg.log_num_records - 1, e->cfg.record_bytes);
  if (e->cfg.num_rounds > 1 && key_pitch < d.X + d.Y)
    return fail(PIR_EINVAL, "key_pitch %llu < the key's %llu bytes", (unsigned long long)key_pitch,
                (unsigned long long)(d.X + d.Y));
  AnswerScope sc(e, stream);
  if (sc.rc()) return sc.rc();
  return sc.finish(answer_shamir_locked(e, d_keys, key_pitch, rec0, nrec, d_result, sc.stream()));
}

int pir_engine_answer_shamir(pir_engine_t* e, const uint8_t* const* keys, uint64_t rec0,
                             uint64_t nrec, uint8_t* result) {
  if (!e || !result || !keys) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_shamir(e, rec0, nrec)) return rc;
  const auto& c = e->cfg;
  for (int a = 0; a < c.num_rounds; ++a)
    if (!keys[a]) return fail(PIR_EINVAL, "null key %d", a);
  const pir::ShamirDims d = pir::shamir_dims(c.log_num_records - 1, c.record_bytes);
  const uint64_t klen = d.X + d.Y;
  const size_t out_bytes = (size_t)c.num_rounds * d.resp_len;
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  int rc = e->d_coef_stage.reserve((size_t)c.num_rounds * klen);
  if (!rc) rc = e->d_shamir_res.reserve(out_bytes);
  if (rc) return rc;
  for (int a = 0; a < c.num_rounds; ++a)
    HIP_TRY(hipMemcpyAsync(e->d_coef_stage + (size_t)a * klen, keys[a], klen,
                           hipMemcpyHostToDevice, e->stream));
  rc = sc.finish(answer_shamir_locked(e, e->d_coef_stage, klen, rec0, nrec, e->d_shamir_res,
                                      e->stream));
  if (rc) return rc;
  return download(result, e->d_shamir_res, out_bytes, e->stream);
}

// Hermite rows of a Shamir engine: rows [N, 2N), N = rows / 2 (file r -> row N + r)
static int check_hermite(pir_engine_t* e, uint64_t num_files, uint32_t file_bytes, int k,
                         int party) {
  if (int rc = check_shamir(e, 0, 0)) return rc;
  if (k < 1 || k > 16) return fail(PIR_EINVAL, "k = %d outside [1,16]", k);
  if (party < 0 || party > 255) return fail(PIR_EINVAL, "party %d outside [0,255]", party);
  if ((uint64_t)file_bytes > (uint64_t)k * e->cfg.record_bytes)
    return fail(PIR_EINVAL, "file_bytes %u > k * record_bytes (%d * %u)", file_bytes, k,
                e->cfg.record_bytes);
  if (num_files > e->rows / 2)
    return fail(PIR_EINVAL, "%llu files > %llu value rows", (unsigned long long)num_files,
                (unsigned long long)(e->rows / 2));
  return PIR_OK;
}

int pir_engine_encode_hermite_dev(pir_engine_t* e, const uint8_t* d_files, uint64_t file_pitch,
                                  uint64_t num_files, uint32_t file_bytes, int k, int party) {
  if (!e) return fail(PIR_EINVAL, "null engine");
  if (int rc = check_hermite(e, num_files, file_bytes, k, party)) return rc;
  if (d_files && file_pitch < file_bytes) return fail(PIR_EINVAL, "file_pitch < file_bytes");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  const uint64_t N = e->rows / 2;
  HIP_TRY(pir::launch_encode_hermite(d_files, file_pitch, num_files, file_bytes, k,
                                     party ? party : e->cfg.party_index,
                                     e->d_shard + N * e->pitch, N, 0, e->pitch,
                                     e->cfg.record_bytes, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return PIR_OK;
}

int pir_engine_encode_hermite_rows(pir_engine_t* e, const uint8_t* const* files,
                                   uint64_t num_files, uint32_t file_bytes, int k, int party) {
  if (!e || (!files && num_files)) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_hermite(e, num_files, file_bytes, k, party)) return rc;
  // the files travel once, packed; the encode reads them from the device
  const uint32_t fb = std::max<uint32_t>(file_bytes, 1);
  DevBuf<> d_files;
  std::vector<uint8_t> packed((size_t)num_files * fb);
  for (uint64_t i = 0; i < num_files; ++i) memcpy(packed.data() + i * fb, files[i], file_bytes);
  {
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (d_files.reserve(std::max<size_t>(packed.size(), 1)))
      return fail(PIR_ENOMEM, "encode staging");
    if (hipMemcpy(d_files, packed.data(), packed.size(), hipMemcpyHostToDevice) != hipSuccess)
      return fail(PIR_EHIP, "encode staging copy");
  }
  const int rc = pir_engine_encode_hermite_dev(e, d_files, fb, num_files, file_bytes, k, party);
  std::lock_guard<std::mutex> lk(e->mu);
  d_files.release();
  return rc;
}

}  // extern "C"
