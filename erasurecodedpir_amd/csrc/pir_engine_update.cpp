// pir_engine_update.cpp -- live record updates: a batch of changed files becomes a table of terms
// (pir_update_plan.h) that k_update_rows (pir_update.hip) XORs into the resident shard's rows and,
// where the engine holds a valid fold image, into the image's blocks.  An update is not a rewrite:
// it holds no ShardWrite, the image stays valid through it, and a pass that wanted an image before
// it still gets one after it.
#include "pir_engine_internal.h"

using namespace eng;

namespace {

// what every form checks first (before any device call)
int check_batch(const pir_engine_t* e, const uint64_t* index, int num, const void* a,
                const void* b) {
  if (!e) return fail(PIR_EINVAL, "null engine");
  if (num < 0) return fail(PIR_EINVAL, "an update of %d records", num);
  if (num > 0 && (!index || !a || !b)) return fail(PIR_EINVAL, "null argument");
  return PIR_OK;
}

int check_k(int k) {
  if (k < 1 || k > 16) return fail(PIR_EINVAL, "k = %d outside [1,16]", k);
  return PIR_OK;
}

int check_indices(const uint64_t* index, int num, uint64_t bound, const char* what) {
  for (int i = 0; i < num; ++i)
    if (index[i] >= bound)
      return fail(PIR_EINVAL, "update %d: %s %llu at or beyond %llu", i, what,
                  (unsigned long long)index[i], (unsigned long long)bound);
  return PIR_OK;
}

int check_across(const pir_engine_t* e, const uint64_t* files, int num, uint64_t pitch,
                 uint64_t num_files, int k) {
  if (int rc = check_k(k)) return rc;
  const uint64_t encdb = (num_files + (uint64_t)k - 1) / (uint64_t)k;
  if (encdb > (1ull << e->cfg.log_num_records))
    return fail(PIR_EINVAL, "%llu files over k=%d need %llu rows > 2^%d",
                (unsigned long long)num_files, k, (unsigned long long)encdb,
                e->cfg.log_num_records);
  if (num > 0 && pitch < e->cfg.record_bytes) return fail(PIR_EINVAL, "delta_pitch < record_bytes");
  // growing the database would change encdb, and with it the row of every file: a re-encode
  return check_indices(files, num, num_files, "file");
}

int check_within(const pir_engine_t* e, const uint64_t* files, int num, uint64_t pitch,
                 uint64_t num_files, uint32_t file_bytes, int k, int party, int hermite) {
  if (int rc = check_k(k)) return rc;
  if (party < 0 || party > 255) return fail(PIR_EINVAL, "party %d outside [0,255]", party);
  if ((uint64_t)file_bytes > (uint64_t)k * e->cfg.record_bytes)
    return fail(PIR_EINVAL, "file_bytes %u > k * record_bytes (%d * %u)", file_bytes, k,
                e->cfg.record_bytes);
  if (hermite && (e->cfg.log_num_partitions > 0 || e->rows < 2))
    return fail(PIR_EINVAL, "Hermite rows: a Shamir engine has no partitions and value rows and "
                            "Hermite rows (2^%d partitions, %llu rows)",
                e->cfg.log_num_partitions, (unsigned long long)e->rows);
  const uint64_t domain = hermite ? e->rows / 2 : 1ull << e->cfg.log_num_records;
  if (num_files > domain)
    return fail(PIR_EINVAL, "%llu files > %llu rows", (unsigned long long)num_files,
                (unsigned long long)domain);
  if (num > 0 && pitch < file_bytes) return fail(PIR_EINVAL, "delta_pitch < file_bytes");
  return check_indices(files, num, num_files, "file");
}

// The terms, already made, onto the device and into the shard on s; then the epochs.  The table
// travels from one of two pinned buffers: a buffer is refilled only after the copy that read it
// has completed (ev_upd), so an update does not wait for the one before it
int apply_locked(pir_engine* e, std::vector<pir::UpdateTerm>& terms, const uint8_t* d_delta,
                 uint64_t dpitch, uint32_t limit, hipStream_t s) {
  if (terms.empty()) return PIR_OK;  // (every row in other partitions)
  if (terms.size() > 0xffffffffull) return fail(PIR_EINVAL, "an update of %zu terms", terms.size());
  std::vector<pir::UpdateBlock> blocks;
  pir::update_plan(terms, blocks);
  const size_t bbytes = blocks.size() * sizeof(pir::UpdateBlock);
  const size_t tbytes = terms.size() * sizeof(pir::UpdateTerm);
  size_t cap = 1 << 16;  // grown by doubling: a run of growing batches regrows rarely
  while (cap < bbytes + tbytes) cap *= 2;
  const int b = e->upd_next;
  if (!e->ev_upd[b]) {
    HIP_TRY(hipEventCreateWithFlags(&e->ev_upd[b], hipEventDisableTiming));
  } else {
    HIP_TRY(hipEventSynchronize(e->ev_upd[b]));
  }
  if (int rc = e->h_upd[b].reserve(cap)) return rc;
  if (int rc = e->d_upd.reserve(cap)) return rc;
  memcpy(e->h_upd[b], blocks.data(), bbytes);
  memcpy(e->h_upd[b] + bbytes, terms.data(), tbytes);
  HIP_TRY(hipMemcpyAsync(e->d_upd, e->h_upd[b], bbytes + tbytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(e->ev_upd[b], s));
  e->upd_next = b ^ 1;
  // the image is patched where it is valid; a pass that wanted one keeps wanting it
  const bool had = e->fold_image && e->d_image.p && e->image_epoch == e->shard_epoch;
  const bool wanted = e->image_wanted == e->shard_epoch;
  const hipError_t err = pir::launch_update_rows(
      reinterpret_cast<const pir::UpdateBlock*>(e->d_upd.p), (uint32_t)blocks.size(),
      reinterpret_cast<const pir::UpdateTerm*>(e->d_upd.p + bbytes), d_delta, dpitch, limit,
      e->d_shard, e->rows, e->pitch, e->cfg.record_bytes, had ? e->d_image.p : nullptr, s);
  ++e->shard_epoch;
  if (err != hipSuccess) {
    e->image_epoch = 0;
    return fail(PIR_EHIP, "update_rows: %s", hipGetErrorString(err));
  }
  if (had) e->image_epoch = e->shard_epoch;
  if (wanted) e->image_wanted = e->shard_epoch;
  return PIR_OK;
}

// One update under an AnswerScope: after every answer enqueued before it, before every later
// one.  host: the deltas (num x width bytes, pitch apart) are staged through the engine's buffer
// and the call waits; else they are read on the stream.  make(terms) is called under the
// engine's lock (the party index is the engine's at that moment)
template <class Make>
int update(pir_engine_t* e, int num, const uint8_t* delta, uint64_t pitch, uint32_t width,
           uint32_t limit, bool host, void* stream, Make&& make) {
  if (num == 0) return PIR_OK;
  AnswerScope sc(e, host ? nullptr : stream);
  if (sc.rc()) return sc.rc();
  const hipStream_t s = sc.stream();
  if (host) {
    const size_t dp = ((size_t)width + 3) & ~(size_t)3;
    if (int rc = stage2d(e->d_upd_delta, dp, delta, pitch, width, (size_t)num,
                         hipMemcpyHostToDevice, s))
      return rc;
    delta = e->d_upd_delta;
    pitch = dp;
  }
  std::vector<pir::UpdateTerm> terms;
  make(terms);
  int rc = apply_locked(e, terms, delta, pitch, limit, s);
  if (host && !rc && hipStreamSynchronize(s) != hipSuccess) rc = fail(PIR_EHIP, "update: sync");
  return sc.finish(rc);
}

int update_rows(pir_engine_t* e, const uint64_t* rows, int num, const uint8_t* delta,
                uint64_t pitch, bool host, void* stream) {
  if (int rc = check_batch(e, rows, num, delta, delta)) return rc;
  if (num > 0 && pitch < e->cfg.record_bytes) return fail(PIR_EINVAL, "delta_pitch < record_bytes");
  if (int rc = check_indices(rows, num, e->rows, "row")) return rc;
  const uint32_t efs = e->cfg.record_bytes;
  return update(e, num, delta, pitch, efs, efs, host, stream,
                [&](std::vector<pir::UpdateTerm>& t) { pir::update_terms_rows(rows, num, t); });
}

int update_across(pir_engine_t* e, const uint64_t* files, int num, const uint8_t* delta,
                  uint64_t pitch, uint64_t num_files, int k, bool host, void* stream) {
  if (int rc = check_batch(e, files, num, delta, delta)) return rc;
  if (int rc = check_across(e, files, num, pitch, num_files, k)) return rc;
  const uint32_t efs = e->cfg.record_bytes;
  return update(e, num, delta, pitch, efs, efs, host, stream, [&](std::vector<pir::UpdateTerm>& t) {
    pir::update_terms_across(files, num, num_files, k, e->cfg.party_index,
                             (uint64_t)e->cfg.partition_index * e->rows, e->rows, t);
  });
}

int update_within(pir_engine_t* e, const uint64_t* files, int num, const uint8_t* delta,
                  uint64_t pitch, uint64_t num_files, uint32_t file_bytes, int k, int party,
                  int hermite, bool host, void* stream) {
  if (int rc = check_batch(e, files, num, delta, delta)) return rc;
  if (int rc = check_within(e, files, num, pitch, num_files, file_bytes, k, party, hermite))
    return rc;
  return update(e, num, delta, pitch, file_bytes, file_bytes, host, stream,
                [&](std::vector<pir::UpdateTerm>& t) {
                  pir::update_terms_within(files, num, file_bytes, e->cfg.record_bytes, k,
                                           party ? party : e->cfg.party_index,
                                           (uint64_t)e->cfg.partition_index * e->rows, e->rows,
                                           hermite ? e->rows / 2 : 0, t);
                });
}

}  // namespace

extern "C" {

int pir_engine_update_rows_dev(pir_engine_t* e, const uint64_t* rows, int num,
                               const uint8_t* d_delta, uint64_t delta_pitch, void* stream) {
  return update_rows(e, rows, num, d_delta, delta_pitch, false, stream);
}
int pir_engine_update_rows(pir_engine_t* e, const uint64_t* rows, int num, const uint8_t* delta,
                           uint64_t delta_pitch) {
  return update_rows(e, rows, num, delta, delta_pitch, true, nullptr);
}

int pir_engine_update_across_dev(pir_engine_t* e, const uint64_t* file_index, int num,
                                 const uint8_t* d_delta, uint64_t delta_pitch, uint64_t num_files,
                                 int k, void* stream) {
  return update_across(e, file_index, num, d_delta, delta_pitch, num_files, k, false, stream);
}
int pir_engine_update_across(pir_engine_t* e, const uint64_t* file_index, int num,
                             const uint8_t* delta, uint64_t delta_pitch, uint64_t num_files,
                             int k) {
  return update_across(e, file_index, num, delta, delta_pitch, num_files, k, true, nullptr);
}

int pir_engine_update_within_dev(pir_engine_t* e, const uint64_t* file_index, int num,
                                 const uint8_t* d_delta, uint64_t delta_pitch, uint64_t num_files,
                                 uint32_t file_bytes, int k, int party, int hermite,
                                 void* stream) {
  return update_within(e, file_index, num, d_delta, delta_pitch, num_files, file_bytes, k, party,
                       hermite, false, stream);
}
int pir_engine_update_within(pir_engine_t* e, const uint64_t* file_index, int num,
                             const uint8_t* delta, uint64_t delta_pitch, uint64_t num_files,
                             uint32_t file_bytes, int k, int party, int hermite) {
  return update_within(e, file_index, num, delta, delta_pitch, num_files, file_bytes, k, party,
                       hermite, true, nullptr);
}

int pir_engine_update_across_mac_dev(pir_engine_t* e, const uint64_t* file_index, int num,
                                     const uint8_t* d_old, const uint8_t* d_new, uint64_t pitch,
                                     uint64_t num_files, int k, const uint8_t key[16],
                                     void* stream) {
  if (int rc = check_batch(e, file_index, num, d_old, d_new)) return rc;
  if (!key) return fail(PIR_EINVAL, "null argument");
  const uint32_t efs = e->cfg.record_bytes;
  if (efs <= PIR_MAC_BYTES)
    return fail(PIR_EINVAL, "record_bytes %u leaves no payload before the %d-byte tag", efs,
                PIR_MAC_BYTES);
  const uint32_t payload = efs - PIR_MAC_BYTES;
  if (int rc = check_across(e, file_index, num, efs, num_files, k)) return rc;
  if (num > 0 && pitch < payload) return fail(PIR_EINVAL, "pitch < the payload's bytes");
  if (num == 0) return PIR_OK;
  AnswerScope sc(e, stream);
  if (sc.rc()) return sc.rc();
  const hipStream_t s = sc.stream();
  // both payloads tagged, then payload-delta || tag-delta as the records' deltas
  if (int rc = e->d_upd_tags.reserve((size_t)2 * num * PIR_MAC_BYTES)) return rc;
  if (int rc = e->d_upd_delta.reserve((size_t)num * efs)) return rc;
  const pir::HmacStates st = pir::hmac_states(key);
  HIP_TRY(pir::launch_hmac_sha256_files(d_old, pitch, (uint64_t)num, payload, st, e->d_upd_tags,
                                        PIR_MAC_BYTES, s));
  HIP_TRY(pir::launch_hmac_sha256_files(d_new, pitch, (uint64_t)num, payload, st,
                                        e->d_upd_tags + (size_t)num * PIR_MAC_BYTES, PIR_MAC_BYTES,
                                        s));
  HIP_TRY(pir::launch_update_mac_delta(d_old, d_new, pitch, e->d_upd_tags, (uint64_t)num, payload,
                                       e->d_upd_delta, s));
  std::vector<pir::UpdateTerm> terms;
  pir::update_terms_across(file_index, num, num_files, k, e->cfg.party_index,
                           (uint64_t)e->cfg.partition_index * e->rows, e->rows, terms);
  return sc.finish(apply_locked(e, terms, e->d_upd_delta, efs, efs, s));
}

}  // extern "C"
