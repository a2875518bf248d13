// pir_engine_woodruff.cpp -- the Woodruff mode: value answers, derivative answers, and the queues
// of value queries and of derivative queries that share shard passes.
#include "pir_engine_internal.h"

using namespace eng;

namespace {

// Woodruff value answer (server.cpp:564-616) over the records [rec0, rec0 + nrec): out = XOR_i
// key[a_i] * key[b_i] * row_i, (a_i, b_i) the i-th 2-subset of [0, M) (pir_woodruff.h).
// The whole domain of a shape k_query tiles: ONE launch, its builder waves writing each tile's
// pair products into the LDS ring while the scan waves stream the shard (fused = 5).  Every
// other range or shape: k_woodruff_coefs, then the explicit-coefficient scan (fused = 6).
// $PIR_WD_FUSED: 0 = never k_query, 2 = always (an answer it cannot take fails: tests), default
// = the policy: k_query wherever it takes the answer.  Measured with tools/bench_woodruff.py on
// one MI355X, the three legs alternated in one process (profiles/woodruff/): 2^24 x 1 KiB
// k_query 2.456 ms against 2.554 (coefficient kernel + scan) and 2.539 (answer_coefs), the
// spread between repeats of one leg 0.05 ms; 2^24 x 256 B 0.634 against 0.746 / 0.715; 2^20 x
// 1 KiB 0.178 against 0.188 / 0.181 and 2^22 x 2 KiB 1.258 against 1.255 / 1.251, both inside
// the spread (0.01 / 0.04 ms).
// Both paths use the five-event profiling layout: "launch" = answer start -> the first kernel,
// "scan" = k_woodruff_coefs + the scan, or k_query, "reduce" = k_reduce.
constexpr bool kWdFusedDefault = true;

bool woodruff_fused_takes(const pir_engine* e, pir::QueryPlan* qp) {
  const auto& c = e->cfg;
  *qp = pir::make_query_plan(c.log_num_records, 0, 2, 1, e->pitch, e->num_cus);
  return e->allow_query && pir::query_wd_takes(*qp);
}

int answer_woodruff_locked(pir_engine* e, const uint8_t* d_key, uint32_t M, uint64_t rec0,
                           uint64_t nrec, uint8_t* d_result, hipStream_t s) {
  const auto& c = e->cfg;
  e->ev = nullptr;
  const char* fv = getenv("PIR_WD_FUSED");
  const int fmode = fv ? atoi(fv) : 1;
  pir::QueryPlan qp{};
  const bool whole = rec0 == 0 && nrec == e->rows;
  const bool takes = fmode != 0 && whole && woodruff_fused_takes(e, &qp);
  if (!takes && fmode == 2)
    return fail(PIR_EINVAL, "k_query's Woodruff mode does not take this answer ($PIR_WD_FUSED=2)");
  const bool fused = takes && (fmode == 2 || kWdFusedDefault);
  hipEvent_t* ev = nullptr;
  if (!e->prof.empty()) {
    ev = prof_slot(e, fused ? 5 : 6, 1, true);
    HIP_TRY(hipEventRecord(ev[EV_START], s));
  }
  if (fused) {
    if (int rc = e->d_slabs.reserve(pir::query_slab_bytes(qp))) return rc;
    if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_B], s));
    HIP_TRY(pir::launch_query_wd(qp, d_key, M, c.log_num_records, e->d_shard, e->d_slabs, s));
    if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_E], s));
    HIP_TRY(pir::launch_reduce(qp.shape, e->d_slabs, c.record_bytes, d_result, s));
    e->last_fused = 5;
  } else if (nrec == 0) {
    if (ev)
      for (int i : {EV_SCAN_B, EV_SCAN_E}) HIP_TRY(hipEventRecord(ev[i], s));
    HIP_TRY(hipMemsetAsync(d_result, 0, c.record_bytes, s));
  } else {
    const pir::ScanShape sh = pir::make_scan_shape(nrec, e->pitch, 1, e->num_cus);
    if (int rc = e->d_slabs.reserve((size_t)sh.grid.x * sh.grid.y * sh.slab_bytes)) return rc;
    if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_B], s));
    HIP_TRY(pir::launch_woodruff_coefs(d_key, M, e->nrp, rec0, rec0 + nrec, e->d_c, s));
    HIP_TRY(pir::launch_scan(sh, e->d_shard + rec0 * e->pitch, nrec, e->d_c, e->d_slabs, false, s));
    if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_E], s));
    HIP_TRY(pir::launch_reduce(sh, e->d_slabs, c.record_bytes, d_result, s));
    e->last_fused = 6;
  }
  if (ev) {
    HIP_TRY(hipEventRecord(ev[EV_RED], s));
    HIP_TRY(hipEventRecord(ev[EV_END], s));
  }
  return PIR_OK;
}

// Woodruff derivative answers (server.cpp:618-644): M + 1 records at d_result, all overwritten
// (the reference zeroes only the first and XORs into whatever the caller's other M held).  Two
// passes over the shard (pir_woodruff.h).  Five-event layout, fused = 7: "launch" = answer start
// -> the answer zeroed, "scan" = the rows pass, the totals kernel and the columns pass, "reduce"
// = 0.
int answer_woodruff_deriv_locked(pir_engine* e, const uint8_t* d_key, uint32_t M, uint64_t rec0,
                                 uint64_t nrec, uint8_t* d_result, hipStream_t s) {
  const auto& c = e->cfg;
  e->ev = nullptr;
  hipEvent_t* ev = nullptr;
  if (!e->prof.empty()) {
    ev = prof_slot(e, 7, 1, true);
    HIP_TRY(hipEventRecord(ev[EV_START], s));
  }
  HIP_TRY(hipMemsetAsync(d_result, 0, (size_t)(M + 1) * c.record_bytes, s));
  if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_B], s));
  HIP_TRY(pir::launch_woodruff_deriv(e->d_shard, e->pitch, c.record_bytes, d_key, M, rec0,
                                     rec0 + nrec, d_result, s));
  e->last_fused = 7;
  if (ev)
    for (int i : {EV_SCAN_E, EV_RED, EV_END}) HIP_TRY(hipEventRecord(ev[i], s));
  return PIR_OK;
}

// a Woodruff engine holds the N = 2^n records unsplit and answers one round
int check_woodruff(const pir_engine* e, uint64_t key_len, uint64_t rec0, uint64_t nrec) {
  const auto& c = e->cfg;
  if (c.num_rounds != 1)
    return fail(PIR_EINVAL, "the Woodruff mode answers one round (the engine has %d)", c.num_rounds);
  if (c.log_num_partitions > 0)
    return fail(PIR_EINVAL, "the Woodruff mode does not serve a split shard (2^%d partitions)",
                c.log_num_partitions);
  if (e->comm) return fail(PIR_EINVAL, "the Woodruff mode does not answer through a communicator");
  const uint32_t M = pir::wd_key_len(c.log_num_records);
  if (!M || key_len != M)
    return fail(PIR_EINVAL, "Woodruff key of %llu bytes; 2^%d records take M = %u",
                (unsigned long long)key_len, c.log_num_records, M);
  if (rec0 > e->rows || nrec > e->rows - rec0)
    return fail(PIR_EINVAL, "records [%llu,%llu) beyond the %llu records", (unsigned long long)rec0,
                (unsigned long long)(rec0 + nrec), (unsigned long long)e->rows);
  return PIR_OK;
}

// Keys per shard pass of a queue of nk Woodruff value queries by default; 0: every key its own
// answer (answer_woodruff_locked), back to back.  A pure function of the shape, on only for the
// families where the shared queue measured faster than the parent build's back-to-back single
// answers by more than the largest spread of any leg of that run (tools/bench_woodruff.py
// --queue, profiles/woodruff_queue/README.md); a family nobody measured stays off.
int woodruff_share_policy(uint32_t pitch, uint64_t rows, int nk) {
  // measured: queues of 2, 4, 8 and 20 keys over 2^20 and 2^24 rows of 1 KiB, 2^24 of 256 B and
  // 2^22 of 2 KiB, 8 keys per pass.  4 keys and more: 1.9-2.3x the parent at 4, 3.8-4.6x at 8,
  // 3.3-3.8x at 20 (7 + 7 + 6), on every shape.  2 keys: 1.0-1.19x, inside the spread on three
  // of the four shapes (a pass of 8 key slots costs 1.8 single answers), so they stay unshared
  if (nk < 4) return 0;
  const bool measured = (pitch == 1024 && rows >= (1ull << 20)) ||
                        (pitch == 256 && rows >= (1ull << 24)) ||
                        (pitch == 2048 && rows >= (1ull << 22));
  return measured ? 8 : 0;
}

// the group size of a Woodruff queue of nk keys (0: unshared).  $PIR_WD_SHARE: 0 never shares, 1
// (default) follows woodruff_share_policy, 2 shares every queue of two or more keys (every shape
// has a group scan: one round, so at most 8 rounds per pass); $PIR_WD_G overrides the group size
int woodruff_group(const pir_engine* e, int nk) {
  if (e->wd_share == 0 || nk < 2) return 0;
  int g = woodruff_share_policy(e->pitch, e->rows, nk);
  if (g == 0 && e->wd_share < 2) return 0;
  if (g == 0) g = 8;
  return e->wd_group > 0 ? e->wd_group : g;
}
// every buffer a Woodruff queue of up to nk keys over up to nrec records touches, shared or not
int ensure_woodruff_queue(pir_engine* e, uint32_t M, int nk, uint64_t nrec) {
  pir::ScanShape sh = pir::make_scan_shape(std::max<uint64_t>(nrec, 1), e->pitch, 1, e->num_cus);
  size_t slab = (size_t)sh.grid.x * sh.grid.y * sh.slab_bytes;
  pir::QueryPlan qp{};
  if (woodruff_fused_takes(e, &qp)) slab = std::max(slab, pir::query_slab_bytes(qp));
  int rc = PIR_OK;
  if (const int G = nrec ? woodruff_group(e, nk) : 0) {
    sh = woodruff_group_shape(e, nrec, G);
    slab = std::max(slab, (size_t)sh.grid.x * sh.grid.y * sh.slab_bytes);
    // the share buffer, then the interleaved key table of the shapes whose table outgrows LDS
    rc = e->d_cb.reserve(wd_share_bytes(nrec, sh.nrp) + (size_t)M * sh.nrp);
    if (!rc) rc = e->d_gtmp.reserve((size_t)16 * e->cfg.record_bytes);
  }
  if (!rc) rc = e->d_slabs.reserve(slab);
  return rc;
}

// A queue of nk Woodruff value queries over the records [rec0, rec0 + nrec): d_keys nk x M bytes,
// d_result nk x efs, result k what answer_woodruff_locked gives for key k.  Shared (woodruff_group
// > 0): the keys go into ceil(nk / G) groups of as equal sizes as possible, as answer_batch_core's
// queue does, and every group takes one full-width pass, all on s: launch_woodruff_coefs_g into
// the share buffer, the G-round scan, k_reduce (slots past the group's size have zero shares;
// their rounds are dropped).  The coefficient kernel is 0.15 ms beside a 4.5 ms scan at 2^24 x
// 1 KiB, and running it on s beside the previous group's scan on aux (two share buffers, as
// answer_batch_core overlaps its leaf stages) measured no faster on any shape and slower for
// three groups (16.3 against 14.8 ms for 20 keys: profiles/woodruff_queue/overlap/), so there is
// one stream and one share buffer.  Five-event layout, fused = 8: "launch" = start -> the first
// coefficient kernel, "scan" = that -> the end of the last scan, "reduce" = the last group's
// reduce.  Unshared, and empty ranges: the single answers back to back on s, each with its own
// slot.
int answer_woodruff_queue_locked(pir_engine* e, const uint8_t* d_keys, uint32_t M, int nk,
                                 uint64_t rec0, uint64_t nrec, uint8_t* d_result, hipStream_t s) {
  const auto& c = e->cfg;
  const int G = nrec ? woodruff_group(e, nk) : 0;
  if (int rc = ensure_woodruff_queue(e, M, nk, nrec)) return rc;
  if (G == 0) {
    for (int k = 0; k < nk; ++k)
      if (int rc = answer_woodruff_locked(e, d_keys + (size_t)k * M, M, rec0, nrec,
                                          d_result + (size_t)k * c.record_bytes, s))
        return rc;
    return PIR_OK;
  }
  const int W = G * e->nrp;
  uint8_t* const d_keyT = e->d_cb + wd_share_bytes(nrec, W);
  return answer_group_queue(e, nk, G, 8, rec0, nrec, d_result, s,
                            [&](int q0, int ng, uint8_t* d_cb, hipStream_t st) {
                              return pir::launch_woodruff_coefs_g(d_keys + (size_t)q0 * M, M, ng, W,
                                                                  rec0, rec0 + nrec, d_cb, st,
                                                                  d_keyT);
                            });
}

// Key slots per pass of a queue of nk Woodruff derivative queries by default; 0: every key its
// own answer (answer_woodruff_deriv_locked), back to back.  A pure function of the shape, on only
// where the shared queue measured faster than the parent build's back-to-back single answers by
// more than the largest spread of any leg of that run (tools/bench_woodruff.py --deriv-queue,
// profiles/woodruff_deriv_queue/README.md); everything nobody measured stays off.
int woodruff_deriv_share_policy(uint32_t pitch, uint64_t rows, int nk) {
  // measured: queues of 2, 4, 8 and 20 keys over 2^20 and 2^24 rows of 1 KiB, 2^24 of 256 B and
  // 2^22 of 2 KiB, 8 slots per pass.  2 keys: 1.5-3.4x the parent, 4: 2.9-6.3x, 8: 5.5-11.3x, 20
  // (7 + 7 + 6): 4.7-10.1x, every one by more than the spread (the two passes of 8 slots cost
  // 1.3 single answers at 2^24 x 1 KiB)
  if (nk < 2) return 0;
  const bool measured = (pitch == 1024 && rows >= (1ull << 20)) ||
                        (pitch == 256 && rows >= (1ull << 24)) ||
                        (pitch == 2048 && rows >= (1ull << 22));
  return measured ? pir::kWdDerivSlots : 0;
}

// the slots per pass of a Woodruff derivative queue of nk keys (0: unshared).  $PIR_WDD_SHARE: 0
// never shares, 1 (default) follows woodruff_deriv_share_policy, 2 shares every queue of two or
// more keys on a shape k_woodruff_seg takes (records of >= 256 B); $PIR_WDD_G overrides the slots
int woodruff_deriv_group(const pir_engine* e, int nk) {
  if (e->wdd_share == 0 || nk < 2 || !pir::woodruff_seg_takes(e->pitch)) return 0;
  int g = woodruff_deriv_share_policy(e->pitch, e->rows, nk);
  if (g == 0 && e->wdd_share < 2) return 0;
  if (g == 0) g = pir::kWdDerivSlots;
  return e->wdd_group > 0 ? e->wdd_group : g;
}
// the one buffer a shared derivative queue touches: a group's interleaved key table (the single
// answers need none); sized wherever some queue could share, whatever the policy says of nk keys
int ensure_woodruff_deriv_queue(pir_engine* e, uint32_t M) {
  if (e->wdd_share == 0 || !pir::woodruff_seg_takes(e->pitch)) return PIR_OK;
  return e->d_cb.reserve((size_t)M * 8);
}

// Which pass hands a wave a long segment and then a short one (bit 0: rows, bit 1: columns); the
// others hand the segments out longest first.  Longest first measured faster in both passes on
// all four shapes (8 keys at 2^24 x 1 KiB: 7.99 ms against 8.71 / 8.76 for pairing in one pass
// and 9.19 in both), so neither pairs.  $PIR_WDD_PAIR (diagnostics, read per answer) overrides it.
constexpr int kWdDerivPair = 0;

// A queue of nk Woodruff derivative queries over the records [rec0, rec0 + nrec): d_keys nk x M
// bytes, d_result nk x (M + 1) x efs, result k what answer_woodruff_deriv_locked gives for key k.
// Shared (woodruff_deriv_group > 0): one memset zeroes every response, the keys go into ceil(nk /
// G) groups of as equal sizes as possible, and per group, all on s: the key table, the rows pass
// (k_woodruff_seg<false>: R[a] stored into every key's record 1 + a), k_woodruff_totals once per
// key (record 0 from the key's finished rows pass), the columns pass (k_woodruff_seg<true>: C[b]
// XORed into record 1 + b).  Five-event layout, fused = 11: "launch" = start -> the responses
// zeroed, "scan" = the first key table -> the end of the last group's columns pass, "reduce" = 0.
// Unshared and empty ranges: the single answers back to back on s, each with its own slot.
int answer_woodruff_deriv_queue_locked(pir_engine* e, const uint8_t* d_keys, uint32_t M, int nk,
                                       uint64_t rec0, uint64_t nrec, uint8_t* d_result,
                                       hipStream_t s) {
  const auto& c = e->cfg;
  const size_t out_bytes = (size_t)(M + 1) * c.record_bytes;
  const int G = nrec ? woodruff_deriv_group(e, nk) : 0;
  if (G == 0) {
    for (int k = 0; k < nk; ++k)
      if (int rc = answer_woodruff_deriv_locked(e, d_keys + (size_t)k * M, M, rec0, nrec,
                                                d_result + (size_t)k * out_bytes, s))
        return rc;
    return PIR_OK;
  }
  if (int rc = ensure_woodruff_deriv_queue(e, M)) return rc;
  e->ev = nullptr;
  hipEvent_t* ev = nullptr;
  if (!e->prof.empty()) {
    ev = prof_slot(e, 11, 1, true);
    HIP_TRY(hipEventRecord(ev[EV_START], s));
  }
  HIP_TRY(hipMemsetAsync(d_result, 0, (size_t)nk * out_bytes, s));
  if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_B], s));
  const char* pv = getenv("PIR_WDD_PAIR");
  const int pair = pv && pv[0] ? atoi(pv) & 3 : kWdDerivPair;
  const uint64_t lo = rec0, hi = rec0 + nrec;
  const int ngroups = (nk + G - 1) / G;
  for (int q0 = 0, j = 0, ng = 0; q0 < nk; q0 += ng, ++j) {
    ng = nk / ngroups + (j < nk % ngroups ? 1 : 0);
    const uint8_t* const keys = d_keys + (size_t)q0 * M;
    uint8_t* const out = d_result + (size_t)q0 * out_bytes;
    HIP_TRY(pir::launch_woodruff_key_table(keys, M, ng, e->d_cb, s));
    HIP_TRY(pir::launch_woodruff_seg(e->d_shard, e->pitch, c.record_bytes, e->d_cb, M, ng, lo, hi,
                                     false, (pair & 1) != 0, out, s));
    for (int g = 0; g < ng; ++g)
      HIP_TRY(pir::launch_woodruff_totals(c.record_bytes, keys + (size_t)g * M, M, lo, hi,
                                          out + (size_t)g * out_bytes, s));
    HIP_TRY(pir::launch_woodruff_seg(e->d_shard, e->pitch, c.record_bytes, e->d_cb, M, ng, lo, hi,
                                     true, (pair & 2) != 0, out, s));
  }
  e->last_fused = 11;
  if (ev)
    for (int i : {EV_SCAN_E, EV_RED, EV_END}) HIP_TRY(hipEventRecord(ev[i], s));
  return PIR_OK;
}

}  // namespace

extern "C" {

uint32_t pir_engine_woodruff_m(int log_num_records) { return pir::wd_key_len(log_num_records); }

int pir_engine_woodruff_pair(uint32_t m, uint64_t i, uint32_t* a, uint32_t* b) {
  if (!a || !b) return fail(PIR_EINVAL, "null argument");
  if (m < 3 || m >= (1u << 17) || i >= (uint64_t)m * (m - 1) / 2)
    return fail(PIR_EINVAL, "no pair of rank %llu among the 2-subsets of [0,%u)",
                (unsigned long long)i, m);
  const pir::WdPair p = pir::wd_pair(m, i);
  *a = p.a;
  *b = p.b;
  return PIR_OK;
}

int pir_engine_woodruff_fused_tile(pir_engine_t* e) {
  if (!e || e->cfg.num_rounds != 1 || e->cfg.log_num_partitions > 0) return 0;
  pir::QueryPlan qp{};
  return woodruff_fused_takes(e, &qp) ? qp.tile : 0;
}

int pir_engine_answer_woodruff_dev(pir_engine_t* e, const uint8_t* d_key, uint64_t key_len,
                                   uint64_t rec0, uint64_t nrec, uint8_t* d_result,
                                   void* stream) {
  if (!e || !d_result || !d_key) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_woodruff(e, key_len, rec0, nrec)) return rc;
  AnswerScope sc(e, stream);
  if (sc.rc()) return sc.rc();
  return sc.finish(answer_woodruff_locked(e, d_key, (uint32_t)key_len, rec0, nrec, d_result,
                                          sc.stream()));
}

int pir_engine_answer_woodruff(pir_engine_t* e, const uint8_t* key, uint64_t key_len,
                               uint64_t rec0, uint64_t nrec, uint8_t* result) {
  if (!e || !result || !key) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_woodruff(e, key_len, rec0, nrec)) return rc;
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  if (int rc = stage(e->d_coef_stage, key, key_len, hipMemcpyHostToDevice, e->stream)) return rc;
  if (int rc = sc.finish(answer_woodruff_locked(e, e->d_coef_stage, (uint32_t)key_len, rec0, nrec,
                                                e->d_result, e->stream)))
    return rc;
  return download(result, e->d_result, e->cfg.record_bytes, e->stream, e->h_res);
}

int pir_engine_answer_woodruff_queue_dev(pir_engine_t* e, const uint8_t* d_keys, uint64_t key_len,
                                         int num_keys, uint64_t rec0, uint64_t nrec,
                                         uint8_t* d_result, void* stream) {
  if (int rc = check_queue_args(e, num_keys, d_keys, d_result)) return rc;
  if (int rc = check_woodruff(e, key_len, rec0, nrec)) return rc;
  if (num_keys == 0) return PIR_OK;
  AnswerScope sc(e, stream);
  if (sc.rc()) return sc.rc();
  return sc.finish(answer_woodruff_queue_locked(e, d_keys, (uint32_t)key_len, num_keys, rec0, nrec,
                                                d_result, sc.stream()));
}

int pir_engine_answer_woodruff_queue(pir_engine_t* e, const uint8_t* keys, uint64_t key_len,
                                     int num_keys, uint64_t rec0, uint64_t nrec,
                                     uint8_t* results) {
  if (int rc = check_queue_args(e, num_keys, keys, results)) return rc;
  if (int rc = check_woodruff(e, key_len, rec0, nrec)) return rc;
  if (num_keys == 0) return PIR_OK;
  const size_t rb = (size_t)num_keys * e->cfg.record_bytes;
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  int rc = e->d_shamir_res.reserve(rb);
  if (!rc) rc = stage(e->d_coef_stage, keys, (size_t)num_keys * key_len, hipMemcpyHostToDevice, e->stream);
  if (rc) return rc;
  rc = sc.finish(answer_woodruff_queue_locked(e, e->d_coef_stage, (uint32_t)key_len, num_keys, rec0,
                                              nrec, e->d_shamir_res, e->stream));
  if (rc) return rc;
  return download(results, e->d_shamir_res, rb, e->stream);
}

int pir_engine_reserve_woodruff_queue(pir_engine_t* e, int num_keys) {
  if (!e || num_keys < 1) return fail(PIR_EINVAL, "bad argument");
  if (int rc = check_woodruff(e, pir::wd_key_len(e->cfg.log_num_records), 0, 0)) return rc;
  const uint32_t M = pir::wd_key_len(e->cfg.log_num_records);
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  int rc = ensure_woodruff_queue(e, M, num_keys, e->rows);
  if (const int G = rc ? 0 : woodruff_group(e, num_keys))
    rc = fold_image_reserve(e, woodruff_group_shape(e, e->rows, G));
  // the host form's staging
  if (!rc) rc = e->d_coef_stage.reserve((size_t)num_keys * M);
  if (!rc)
    rc = e->d_shamir_res.reserve((size_t)num_keys * e->cfg.record_bytes);
  return rc;
}

int pir_engine_answer_woodruff_deriv_dev(pir_engine_t* e, const uint8_t* d_key, uint64_t key_len,
                                         uint64_t rec0, uint64_t nrec, uint8_t* d_result,
                                         void* stream) {
  if (!e || !d_result || !d_key) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_woodruff(e, key_len, rec0, nrec)) return rc;
  AnswerScope sc(e, stream);
  if (sc.rc()) return sc.rc();
  return sc.finish(answer_woodruff_deriv_locked(e, d_key, (uint32_t)key_len, rec0, nrec, d_result,
                                                sc.stream()));
}

int pir_engine_answer_woodruff_deriv(pir_engine_t* e, const uint8_t* key, uint64_t key_len,
                                     uint64_t rec0, uint64_t nrec, uint8_t* result) {
  if (!e || !result || !key) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_woodruff(e, key_len, rec0, nrec)) return rc;
  const size_t out_bytes = (size_t)(key_len + 1) * e->cfg.record_bytes;
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  int rc = e->d_shamir_res.reserve(out_bytes);
  if (!rc) rc = stage(e->d_coef_stage, key, key_len, hipMemcpyHostToDevice, e->stream);
  if (rc) return rc;
  rc = sc.finish(answer_woodruff_deriv_locked(e, e->d_coef_stage, (uint32_t)key_len, rec0, nrec,
                                              e->d_shamir_res, e->stream));
  if (rc) return rc;
  return download(result, e->d_shamir_res, out_bytes, e->stream);
}

int pir_engine_answer_woodruff_deriv_queue_dev(pir_engine_t* e, const uint8_t* d_keys,
                                               uint64_t key_len, int num_keys, uint64_t rec0,
                                               uint64_t nrec, uint8_t* d_result, void* stream) {
  if (int rc = check_queue_args(e, num_keys, d_keys, d_result)) return rc;
  if (int rc = check_woodruff(e, key_len, rec0, nrec)) return rc;
  if (num_keys == 0) return PIR_OK;
  AnswerScope sc(e, stream);
  if (sc.rc()) return sc.rc();
  return sc.finish(answer_woodruff_deriv_queue_locked(e, d_keys, (uint32_t)key_len, num_keys, rec0,
                                                      nrec, d_result, sc.stream()));
}

int pir_engine_answer_woodruff_deriv_queue(pir_engine_t* e, const uint8_t* keys, uint64_t key_len,
                                           int num_keys, uint64_t rec0, uint64_t nrec,
                                           uint8_t* results) {
  if (int rc = check_queue_args(e, num_keys, keys, results)) return rc;
  if (int rc = check_woodruff(e, key_len, rec0, nrec)) return rc;
  if (num_keys == 0) return PIR_OK;
  const size_t rb = (size_t)num_keys * (key_len + 1) * e->cfg.record_bytes;
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  int rc = e->d_shamir_res.reserve(rb);
  if (!rc) rc = stage(e->d_coef_stage, keys, (size_t)num_keys * key_len, hipMemcpyHostToDevice, e->stream);
  if (rc) return rc;
  rc = sc.finish(answer_woodruff_deriv_queue_locked(e, e->d_coef_stage, (uint32_t)key_len, num_keys,
                                                    rec0, nrec, e->d_shamir_res, e->stream));
  if (rc) return rc;
  return download(results, e->d_shamir_res, rb, e->stream);
}

int pir_engine_reserve_woodruff_deriv_queue(pir_engine_t* e, int num_keys) {
  if (!e || num_keys < 1) return fail(PIR_EINVAL, "bad argument");
  if (int rc = check_woodruff(e, pir::wd_key_len(e->cfg.log_num_records), 0, 0)) return rc;
  const uint32_t M = pir::wd_key_len(e->cfg.log_num_records);
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  int rc = ensure_woodruff_deriv_queue(e, M);
  // the host form's staging
  if (!rc) rc = e->d_coef_stage.reserve((size_t)num_keys * M);
  if (!rc) rc = e->d_shamir_res.reserve((size_t)num_keys * (M + 1) * e->cfg.record_bytes);
  return rc;
}

}  // extern "C"
