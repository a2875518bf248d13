// pir_engine_group.cpp -- the sqrt(N) DPF modes (multiparty, covering-design) and the queues
// that share shard passes between their keys or between explicit-coefficient queries.
#include "pir_engine_internal.h"

using namespace eng;

namespace {

// Multiparty sqrt(N) DPF answer (server.cpp:384-430): the thread's rows of the domain
// [thr * slice * mu, (thr + 1) * slice * mu), slice = nu / num_threads (the reference drops the
// nu % num_threads remainder rows; so does this), intersected with this engine's partition:
// shares (k_mp_shares) -> GF(2^8) scan -> slab reduce [-> all-gather + XOR fold].
int answer_mp_locked(pir_engine* e, const pir::MpLayout& L, const uint8_t* d_key, int thread_num,
                     int num_threads, uint8_t* d_result, hipStream_t s) {
  const auto& c = e->cfg;
  const size_t out_bytes = (size_t)c.num_rounds * c.record_bytes;
  uint8_t* out = e->comm ? e->d_part.p : d_result;
  e->ev = nullptr;
  // the whole domain of a layout k_query tiles (the plan's tile divides mu; few seeds per row):
  // ONE launch, its tree waves building each tile's shares from the key while the scan waves
  // stream the shard.  $PIR_MP_FUSED: 0 = never (k_mp_shares, then the scan), 2 = always (an
  // answer k_query cannot take fails: tests), default: where it applies with >= 3 shares, or
  // with 1-2 shares and <= 8 seeds a row (4 share waves + 12 scan waves, query_nq_mp).
  // Measured on 2^24 x 1 KiB (profiles/r04/r4o_ab.jsonl, r4q_ab.jsonl, r4ae_ab.jsonl): CD842 (3
  // shares) 3.19 -> 2.79 ms, CD732 (4) 4.19 -> 3.67 ms, multiparty p = 3 (2 shares, 4 seeds)
  // 2.70 -> 2.52 ms (with 8 share waves it was 2.77: r4p_ab.jsonl)
  const char* fv = getenv("PIR_MP_FUSED");
  const int fmode = fv ? atoi(fv) : 1;
  if (fmode != 0) {
    const pir::QueryPlan qp = pir::make_query_plan(c.log_num_records, c.log_num_partitions, 2,
                                                   c.num_rounds, e->pitch, e->num_cus);
    // more than 32 seeds per row (CD732: 64): the 4 share waves beside the scan fall behind and
    // the separate share kernel + scan is faster (3.77 -> 3.56 ms; CD842's 32 seeds and the
    // multiparty shapes stay fused: 2.82 / 2.51 / 2.64 against 3.15 / 2.66 / 2.81,
    // profiles/r06/r7i_ccd7_fused_ab.*, r7j_mp_fused_ab.*); $PIR_MP_FUSED=2 forces up to 64
    const bool takes = thread_num == 0 && num_threads == 1 && L.nu && L.p2 <= (fmode == 2 ? 64u : 32u) &&
                       e->allow_query && qp.tile && qp.shape.uniform &&
                       L.mu % (uint64_t)qp.tile == 0 &&
                       (fmode == 2 || L.nrk >= 3 || L.p2 <= 8);
    if (!takes && fmode == 2)
      return fail(PIR_EINVAL, "k_query's sqrt(N) mode does not take this answer ($PIR_MP_FUSED=2)");
    if (takes) {
      if (int rc = e->d_slabs.reserve(pir::query_slab_bytes(qp))) return rc;
      HIP_TRY(pir::launch_query_mp(qp, d_key, 0, 1, L, c.log_num_records, c.log_num_partitions,
                                   (uint64_t)c.partition_index, e->d_shard, e->d_slabs, s));
      HIP_TRY(pir::launch_reduce(qp.shape, e->d_slabs, c.record_bytes, out, s));
      e->last_fused = 3;
      if (e->comm) {
        if (int rc = exchange(e, e->d_part, out_bytes, e->d_gather, d_result, s)) return rc;
      }
      return PIR_OK;
    }
  }
  const uint64_t slice = L.nu / (uint64_t)num_threads;
  const uint64_t p0 = (uint64_t)c.partition_index * e->rows;
  const uint64_t lo = std::max<uint64_t>((uint64_t)thread_num * slice * L.mu, p0);
  const uint64_t hi = std::min<uint64_t>((uint64_t)(thread_num + 1) * slice * L.mu, p0 + e->rows);
  if (hi <= lo) {
    HIP_TRY(hipMemsetAsync(out, 0, out_bytes, s));
  } else {
    const uint64_t nrows = hi - lo;
    const pir::ScanShape sh = pir::make_scan_shape(nrows, e->pitch, c.num_rounds, e->num_cus);
    int rc = e->d_slabs.reserve((size_t)sh.grid.x * sh.grid.y * sh.slab_bytes);
    if (rc) return rc;
    HIP_TRY(pir::launch_mp_shares(L, d_key, lo, hi, e->nrp, e->d_c, e->num_cus, s));
    HIP_TRY(pir::launch_scan(sh, e->d_shard + (lo - p0) * e->pitch, nrows, e->d_c, e->d_slabs,
                             false, s));
    HIP_TRY(pir::launch_reduce(sh, e->d_slabs, c.record_bytes, out, s));
  }
  if (e->comm) {
    if (int rc = exchange(e, e->d_part, out_bytes, e->d_gather, d_result, s)) return rc;
  }
  return PIR_OK;
}

// the layout's share count against the engine's rounds, the thread slot
int check_layout(const pir_engine* e, const pir::MpLayout& L, int thread_num, int num_threads,
                 const char* what) {
  if (L.nrk != e->cfg.num_rounds)
    return fail(PIR_EINVAL, "the %s layout gives %d shares but the engine has %d rounds", what,
                L.nrk, e->cfg.num_rounds);
  if (num_threads < 1 || thread_num < 0 || thread_num >= num_threads)
    return fail(PIR_EINVAL, "thread_num %d of %d", thread_num, num_threads);
  return PIR_OK;
}

int check_mp(const pir_engine* e, int p, int t, int thread_num, int num_threads,
             pir::MpLayout* L) {
  if (!pir::mp_layout(p, e->cfg.log_num_records, t, L))
    return fail(PIR_EINVAL, "no multiparty DPF layout for p=%d t=%d n=%d", p, t,
                e->cfg.log_num_records);
  return check_layout(e, *L, thread_num, num_threads, "multiparty (NUM_RSS_KEYS)");
}

int check_cd(const pir_engine* e, int q_needed, int num_cd_keys, int thread_num,
             int num_threads, pir::MpLayout* L) {
  if (!pir::cd_layout(e->cfg.log_num_records, q_needed, num_cd_keys, L))
    return fail(PIR_EINVAL, "no covering-design DPF layout for NUM_CD_KEYS_NEEDED=%d "
                "NUM_CD_KEYS=%d n=%d", q_needed, num_cd_keys, e->cfg.log_num_records);
  return check_layout(e, *L, thread_num, num_threads, "covering-design (NUM_CD_KEYS)");
}

// ---- queues of explicit-coefficient and sqrt(N) DPF keys (fused == 9) --------------------------
// Key slots per shard pass of a queue of nk keys by default; 0: every key its own answer, back to
// back.  mode 0: explicit-coefficient vectors, 1: multiparty / covering-design keys.  A pure
// function of the shape, on only for the families where the shared queue measured faster than the
// parent build's back-to-back single answers by more than the largest spread of any leg of that
// run (tools/bench_group_queue.py, profiles/group_queue/README.md); a family nobody measured
// stays off.
// seeds: the sqrt(N) layout's seeds per row (0 for mode 0).
int group_share_policy(int mode, int num_rounds, uint32_t seeds, uint32_t pitch, uint64_t rows,
                       int nk) {
  // measured: queues of 2, 4, 8 and 20 keys over 2^20 and 2^24 rows of 1 KiB and 2^24 of 256 B;
  // vectors of 1 and 2 rounds, multiparty p = 3 / t = 1 (2 shares, 4 seeds), CD842 (3 shares, 32
  // seeds).  Vectors and multiparty, 4 keys and more: 2.1-2.7x the parent at 4, 4.5-4.7x (1
  // round) and 2.1-2.7x (2 rounds / shares: 4 slots) at 8 and 20, on every shape; 2 keys: 1.07-
  // 1.36x, inside the spread on one or two of the three shapes, so they stay unshared.  CD842 (2
  // slots): 1.67-1.70x at 256 B for every length (its single answer there is bound by the AES of
  // its 32 seeds, which a group does once per key all the same, but beside one scan); 0.97-1.00x
  // at 2^24 x 1 KiB and 0.69x at 2^20 x 1 KiB, where the single answer's k_query hides the share
  // waves under its scan and the group's share kernel (1.28 ms for two keys) does not: off
  const bool kib = pitch == 1024 && rows >= (1ull << 20);
  const bool b256 = pitch == 256 && rows >= (1ull << 24);
  if (mode == 0) return num_rounds <= 2 && nk >= 4 && (kib || b256) ? 8 / num_rounds : 0;
  if (num_rounds == 2 && seeds == 4) return nk >= 4 && (kib || b256) ? 4 : 0;
  if (num_rounds == 3 && seeds == 32) return nk >= 2 && b256 ? 2 : 0;
  return 0;
}

// the key slots per pass of a group queue of nk keys (0: unshared).  $PIR_GQ_SHARE: 0 never
// shares, 1 (default) follows group_share_policy, 2 shares every queue of two or more keys that
// has two or more slots (nrp <= 4; 8 / nrp slots); $PIR_GQ_G overrides the slots per pass.  A
// communicator's queue runs the single answers, each with its own exchange.
int group_queue_slots(const pir_engine* e, int mode, int nk, uint32_t seeds = 0) {
  const auto& c = e->cfg;
  if (e->gq_share == 0 || nk < 2 || e->nrp > 4 || e->comm) return 0;
  int g = group_share_policy(mode, c.num_rounds, seeds, e->pitch, e->rows, nk);
  if (g == 0 && e->gq_share < 2) return 0;
  const int gmax = 8 / e->nrp;
  if (g == 0 || g > gmax) g = gmax;
  if (e->gq_group > 0) g = std::min(e->gq_group, gmax);
  return g >= 2 ? g : 0;
}

// the buffers a shared group queue over nrec rows touches, G slots per pass
int ensure_group_queue(pir_engine* e, uint64_t nrec, int G) {
  const pir::ScanShape sh = woodruff_group_shape(e, nrec, G);
  int rc = e->d_slabs.reserve((size_t)sh.grid.x * sh.grid.y * sh.slab_bytes);
  if (!rc) rc = e->d_cb.reserve(wd_share_bytes(nrec, G * e->nrp));
  if (!rc) rc = e->d_gtmp.reserve((size_t)16 * e->cfg.record_bytes);
  return rc;
}

// A queue of nk explicit-coefficient queries over the engine rows [row0, row0 + nrows): key k's
// round a coefficient of row row0 + i at src[k * key_stride + a * coef_pitch + i]; d_result nk x
// num_rounds x efs, result k what answer_coefs_locked gives for key k.  G > 0 (group_queue_slots):
// k_interleave_coefs_g writes each group's share rows (answer_group_queue); G == 0, and empty
// ranges: the single answers back to back on s.
int answer_coefs_queue_locked(pir_engine* e, const uint8_t* src, uint64_t coef_pitch,
                              uint64_t key_stride, int nk, int G, uint64_t row0, uint64_t nrows,
                              uint8_t* d_result, hipStream_t s) {
  const auto& c = e->cfg;
  const size_t out_bytes = (size_t)c.num_rounds * c.record_bytes;
  if (G == 0 || nrows == 0) {
    for (int k = 0; k < nk; ++k)
      if (int rc = answer_coefs_locked(e, src + (size_t)k * key_stride, coef_pitch, row0, nrows,
                                       d_result + (size_t)k * out_bytes, s))
        return rc;
    return PIR_OK;
  }
  if (int rc = ensure_group_queue(e, nrows, G)) return rc;
  const int W = G * e->nrp;
  return answer_group_queue(e, nk, G, 9, row0, nrows, d_result, s,
                            [&](int q0, int ng, uint8_t* d_cb, hipStream_t st) {
                              return pir::launch_interleave_coefs_g(
                                  src + (size_t)q0 * key_stride, coef_pitch, key_stride, ng,
                                  c.num_rounds, e->nrp, W, nrows, d_cb, st);
                            });
}

// A queue of nk sqrt(N) DPF keys of one layout (multiparty or covering-design), 16-byte aligned
// and key_stride (a multiple of 16) apart, over the thread slice of answer_mp_locked; result k
// what answer_mp_locked gives for key k.  Shared: k_mp_shares_g writes each group's share rows.
// Unshared, an empty slice and nu == 0: the single answers back to back on s.
int answer_mp_queue_locked(pir_engine* e, const pir::MpLayout& L, const uint8_t* d_keys,
                           uint64_t key_stride, int nk, int thread_num, int num_threads,
                           uint8_t* d_result, hipStream_t s) {
  const auto& c = e->cfg;
  const size_t out_bytes = (size_t)c.num_rounds * c.record_bytes;
  const uint64_t slice = L.nu / (uint64_t)num_threads;
  const uint64_t p0 = (uint64_t)c.partition_index * e->rows;
  const uint64_t lo = std::max<uint64_t>((uint64_t)thread_num * slice * L.mu, p0);
  const uint64_t hi = std::min<uint64_t>((uint64_t)(thread_num + 1) * slice * L.mu, p0 + e->rows);
  const int G = hi > lo ? group_queue_slots(e, 1, nk, L.p2) : 0;
  if (G == 0) {
    for (int k = 0; k < nk; ++k)
      if (int rc = answer_mp_locked(e, L, d_keys + (size_t)k * key_stride, thread_num, num_threads,
                                    d_result + (size_t)k * out_bytes, s))
        return rc;
    return PIR_OK;
  }
  if (int rc = ensure_group_queue(e, hi - lo, G)) return rc;
  const int W = G * e->nrp;
  return answer_group_queue(e, nk, G, 9, lo - p0, hi - lo, d_result, s,
                            [&](int q0, int ng, uint8_t* d_cb, hipStream_t st) {
                              return pir::launch_mp_shares_g(L, d_keys + (size_t)q0 * key_stride,
                                                             key_stride, ng, W, e->nrp, lo, hi,
                                                             d_cb, e->num_cus, st);
                            });
}

uint64_t mp_stage_stride(const pir::MpLayout& L) { return (L.eval_bytes + 15) & ~15ull; }

// a validated layout's queue from device keys of any alignment and stride: keys the share
// kernels cannot read as 16-byte words go through the aligned staging buffer
int answer_layout_queue_dev(pir_engine* e, const pir::MpLayout& L, const uint8_t* d_keys,
                            uint64_t key_stride, int nk, int thread_num, int num_threads,
                            uint8_t* d_result, void* stream) {
  if (nk > 1 && key_stride < L.eval_bytes)
    return fail(PIR_EINVAL, "key_stride %llu < the %llu bytes the evaluation reads",
                (unsigned long long)key_stride, (unsigned long long)L.eval_bytes);
  AnswerScope sc(e, stream);
  if (sc.rc()) return sc.rc();
  e->gq_key_bytes = std::max(e->gq_key_bytes, L.eval_bytes);
  if (L.eval_bytes && (((uintptr_t)d_keys & 15) || (nk > 1 && (key_stride & 15)))) {
    const uint64_t st = mp_stage_stride(L);
    if (int rc = stage2d(e->d_mpkey, st, d_keys, nk > 1 ? key_stride : st, L.eval_bytes, nk,
                         hipMemcpyDeviceToDevice, sc.stream()))
      return rc;
    d_keys = e->d_mpkey;
    key_stride = st;
  }
  return sc.finish(answer_mp_queue_locked(e, L, d_keys, key_stride, nk, thread_num, num_threads,
                                          d_result, sc.stream()));
}

// ... and from host keys key_bytes apart, answers copied back to host memory
int answer_layout_queue_host(pir_engine* e, const pir::MpLayout& L, const uint8_t* keys,
                             uint64_t key_bytes, int nk, int thread_num, int num_threads,
                             uint8_t* results, const char* what) {
  if (key_bytes < L.eval_bytes)
    return fail(PIR_EINVAL, "%s key of %llu bytes; the evaluation reads %llu", what,
                (unsigned long long)key_bytes, (unsigned long long)L.eval_bytes);
  const size_t rb = (size_t)nk * e->cfg.num_rounds * e->cfg.record_bytes;
  const uint64_t st = std::max<uint64_t>(16, mp_stage_stride(L));
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  e->gq_key_bytes = std::max(e->gq_key_bytes, L.eval_bytes);
  int rc = e->d_shamir_res.reserve(rb);
  if (!rc) rc = stage2d(e->d_mpkey, st, keys, key_bytes, L.eval_bytes, nk, hipMemcpyHostToDevice, e->stream);
  if (rc) return rc;
  rc = sc.finish(answer_mp_queue_locked(e, L, e->d_mpkey, st, nk, thread_num, num_threads,
                                        e->d_shamir_res, e->stream));
  if (rc) return rc;
  return download(results, e->d_shamir_res, rb, e->stream);
}

// a validated sqrt(N) layout's answer from a device key (any alignment)
int answer_layout_dev(pir_engine* e, const pir::MpLayout& L, const uint8_t* d_key, int thread_num,
                      int num_threads, uint8_t* d_result, void* stream) {
  AnswerScope sc(e, stream);
  if (sc.rc()) return sc.rc();
  if (((uintptr_t)d_key & 15) && L.eval_bytes) {  // the seeds are read as 16-byte words
    if (int rc = stage(e->d_mpkey, d_key, L.eval_bytes, hipMemcpyDeviceToDevice, sc.stream()))
      return rc;
    d_key = e->d_mpkey;
  }
  return sc.finish(answer_mp_locked(e, L, d_key, thread_num, num_threads, d_result, sc.stream()));
}

// ... and from a host key of key_bytes bytes, answer copied back to host memory
int answer_layout_host(pir_engine* e, const pir::MpLayout& L, const uint8_t* key,
                       uint64_t key_bytes, int thread_num, int num_threads, uint8_t* result,
                       const char* what) {
  if (key_bytes < L.eval_bytes)
    return fail(PIR_EINVAL, "%s key of %llu bytes; the evaluation reads %llu", what,
                (unsigned long long)key_bytes, (unsigned long long)L.eval_bytes);
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  if (int rc = stage(e->d_mpkey, key, L.eval_bytes, hipMemcpyHostToDevice, e->stream)) return rc;
  if (int rc = sc.finish(answer_mp_locked(e, L, e->d_mpkey, thread_num, num_threads, e->d_result,
                                          e->stream)))
    return rc;
  return download(result, e->d_result, (size_t)e->cfg.num_rounds * e->cfg.record_bytes, e->stream,
                  e->h_res);
}

}  // namespace

extern "C" {

int pir_engine_mp_num_keys(int p, int t) {  // params.cpp:618
  if (p < 1 || t < 0 || t > p) return 0;
  return pir::mp_choose(p, t) * (p - t) / p;
}

int pir_engine_mp_key_len(int p, int n, int t) {  // utils.cpp:105-116 (its own mu = 2^(n/2))
  if (p < 1 || t < 0 || t > p || n < 0 || n > 62) return 0;
  const int c = pir::mp_choose(p, t), q = (p - t) * c / p;
  if (c < 1 || c > 32) return 0;
  const uint64_t p2 = 1ull << (c - 1), mu = 1ull << (n / 2), nu = 1ull << (n - n / 2);
  return (int)(16 * p2 * nu + (uint64_t)q * nu * p2 + p2 * mu);
}

long long pir_engine_mp_eval_bytes(int p, int n, int t) {
  pir::MpLayout L;
  return pir::mp_layout(p, n, t, &L) ? (long long)L.eval_bytes : -1;
}

int pir_engine_answer_mp_dev(pir_engine_t* e, const uint8_t* d_key, int p, int t, int thread_num,
                             int num_threads, uint8_t* d_result, void* stream) {
  if (!e || !d_result) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_key_ptr(d_key)) return rc;
  pir::MpLayout L;
  if (int rc = check_mp(e, p, t, thread_num, num_threads, &L)) return rc;
  return answer_layout_dev(e, L, d_key, thread_num, num_threads, d_result, stream);
}

int pir_engine_answer_mp(pir_engine_t* e, const uint8_t* key, uint64_t key_bytes, int p, int t,
                         int thread_num, int num_threads, uint8_t* result) {
  if (!e || !result) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_key_ptr(key)) return rc;
  pir::MpLayout L;
  if (int rc = check_mp(e, p, t, thread_num, num_threads, &L)) return rc;
  return answer_layout_host(e, L, key, key_bytes, thread_num, num_threads, result, "multiparty");
}

int pir_engine_cd_key_len(int p, int n, int t, int num_cd_keys_needed, int num_cd_keys) {
  (void)p; (void)t;  // utils.cpp:118-129 takes them and does not use them
  pir::MpLayout L;
  return pir::cd_layout(n, num_cd_keys_needed, num_cd_keys, &L) ? (int)L.eval_bytes : 0;
}

int pir_engine_answer_cd_dev(pir_engine_t* e, const uint8_t* d_key, int num_cd_keys_needed,
                             int num_cd_keys, int thread_num, int num_threads, uint8_t* d_result,
                             void* stream) {
  if (!e || !d_result) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_key_ptr(d_key)) return rc;
  pir::MpLayout L;
  if (int rc = check_cd(e, num_cd_keys_needed, num_cd_keys, thread_num, num_threads, &L)) return rc;
  return answer_layout_dev(e, L, d_key, thread_num, num_threads, d_result, stream);
}

int pir_engine_answer_cd(pir_engine_t* e, const uint8_t* key, uint64_t key_bytes,
                         int num_cd_keys_needed, int num_cd_keys, int thread_num, int num_threads,
                         uint8_t* result) {
  if (!e || !result) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_key_ptr(key)) return rc;
  pir::MpLayout L;
  if (int rc = check_cd(e, num_cd_keys_needed, num_cd_keys, thread_num, num_threads, &L)) return rc;
  return answer_layout_host(e, L, key, key_bytes, thread_num, num_threads, result,
                            "covering-design");
}

int pir_engine_answer_coefs_queue_dev(pir_engine_t* e, const uint8_t* d_coefs, uint64_t coef_pitch,
                                      uint64_t key_stride, int num_keys, uint64_t row0,
                                      uint64_t nrows, uint8_t* d_result, void* stream) {
  if (int rc = check_queue_args(e, num_keys, d_coefs, d_result)) return rc;
  if (int rc = check_rows(e, row0, nrows)) return rc;
  const auto& c = e->cfg;
  if (c.num_rounds > 1 && coef_pitch < row0 + nrows)
    return fail(PIR_EINVAL, "coef_pitch %llu < %llu rows", (unsigned long long)coef_pitch,
                (unsigned long long)(row0 + nrows));
  if (num_keys > 1 && key_stride < (uint64_t)(c.num_rounds - 1) * coef_pitch + row0 + nrows)
    return fail(PIR_EINVAL, "key_stride %llu < the %d vectors of one key",
                (unsigned long long)key_stride, c.num_rounds);
  if (num_keys == 0) return PIR_OK;
  AnswerScope sc(e, stream);
  if (sc.rc()) return sc.rc();
  return sc.finish(answer_coefs_queue_locked(e, d_coefs + row0, coef_pitch, key_stride, num_keys,
                                             group_queue_slots(e, 0, num_keys), row0, nrows,
                                             d_result, sc.stream()));
}

int pir_engine_answer_coefs_queue(pir_engine_t* e, const uint8_t* const* coefs, int num_keys,
                                  uint64_t row0, uint64_t nrows, uint8_t* results) {
  if (int rc = check_queue_args(e, num_keys, coefs, results)) return rc;
  if (int rc = check_rows(e, row0, nrows)) return rc;
  const auto& c = e->cfg;
  for (int v = 0; v < num_keys * c.num_rounds && nrows; ++v)
    if (!coefs[v]) return fail(PIR_EINVAL, "null coefficient vector %d", v);
  if (num_keys == 0) return PIR_OK;
  const size_t out_bytes = (size_t)c.num_rounds * c.record_bytes;
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  // one group's vectors are staged at a time (16-byte aligned rows: the group kernel's wide
  // loads): G num_rounds <= 8 vectors shared, one key's vectors unshared
  const int G = nrows ? group_queue_slots(e, 0, num_keys) : 0;
  const int per = G ? G : 1, ngroups = (num_keys + per - 1) / per;
  const size_t vp = ((size_t)nrows + 15) & ~(size_t)15, ks = vp * c.num_rounds;
  int rc = e->d_coef_stage.reserve(std::max<size_t>(16, ks * per));
  if (!rc) rc = e->d_shamir_res.reserve(out_bytes * num_keys);
  if (rc) return rc;
  for (int q0 = 0, j = 0, ng = 0; q0 < num_keys; q0 += ng, ++j) {
    ng = num_keys / ngroups + (j < num_keys % ngroups ? 1 : 0);
    for (int v = 0; v < ng * c.num_rounds && nrows; ++v)  // only the rows answered travel
      HIP_TRY(hipMemcpyAsync(e->d_coef_stage + (size_t)v * vp, coefs[q0 * c.num_rounds + v] + row0,
                             nrows, hipMemcpyHostToDevice, e->stream));
    rc = answer_coefs_queue_locked(e, e->d_coef_stage, vp, ks, ng, G, row0, nrows,
                                   e->d_shamir_res + (size_t)q0 * out_bytes, e->stream);
    if (rc) return rc;
  }
  if (int rc2 = sc.finish(PIR_OK)) return rc2;
  return download(results, e->d_shamir_res, out_bytes * num_keys, e->stream);
}

int pir_engine_answer_mp_queue_dev(pir_engine_t* e, const uint8_t* d_keys, uint64_t key_stride,
                                   int num_keys, int p, int t, int thread_num, int num_threads,
                                   uint8_t* d_result, void* stream) {
  if (int rc = check_queue_args(e, num_keys, d_keys, d_result)) return rc;
  pir::MpLayout L;
  if (int rc = check_mp(e, p, t, thread_num, num_threads, &L)) return rc;
  if (num_keys == 0) return PIR_OK;
  return answer_layout_queue_dev(e, L, d_keys, key_stride, num_keys, thread_num, num_threads,
                                 d_result, stream);
}

int pir_engine_answer_mp_queue(pir_engine_t* e, const uint8_t* keys, uint64_t key_bytes,
                               int num_keys, int p, int t, int thread_num, int num_threads,
                               uint8_t* results) {
  if (int rc = check_queue_args(e, num_keys, keys, results)) return rc;
  pir::MpLayout L;
  if (int rc = check_mp(e, p, t, thread_num, num_threads, &L)) return rc;
  if (num_keys == 0) return PIR_OK;
  return answer_layout_queue_host(e, L, keys, key_bytes, num_keys, thread_num, num_threads, results,
                                  "multiparty");
}

int pir_engine_answer_cd_queue_dev(pir_engine_t* e, const uint8_t* d_keys, uint64_t key_stride,
                                   int num_keys, int num_cd_keys_needed, int num_cd_keys,
                                   int thread_num, int num_threads, uint8_t* d_result,
                                   void* stream) {
  if (int rc = check_queue_args(e, num_keys, d_keys, d_result)) return rc;
  pir::MpLayout L;
  if (int rc = check_cd(e, num_cd_keys_needed, num_cd_keys, thread_num, num_threads, &L)) return rc;
  if (num_keys == 0) return PIR_OK;
  return answer_layout_queue_dev(e, L, d_keys, key_stride, num_keys, thread_num, num_threads,
                                 d_result, stream);
}

int pir_engine_answer_cd_queue(pir_engine_t* e, const uint8_t* keys, uint64_t key_bytes,
                               int num_keys, int num_cd_keys_needed, int num_cd_keys,
                               int thread_num, int num_threads, uint8_t* results) {
  if (int rc = check_queue_args(e, num_keys, keys, results)) return rc;
  pir::MpLayout L;
  if (int rc = check_cd(e, num_cd_keys_needed, num_cd_keys, thread_num, num_threads, &L)) return rc;
  if (num_keys == 0) return PIR_OK;
  return answer_layout_queue_host(e, L, keys, key_bytes, num_keys, thread_num, num_threads, results,
                                  "covering-design");
}

int pir_engine_reserve_group_queue(pir_engine_t* e, int num_keys) {
  if (!e || num_keys < 1) return fail(PIR_EINVAL, "bad argument");
  const auto& c = e->cfg;
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(c.device));
  // the single answers an unshared queue runs: the explicit-coefficient scan, k_query's sqrt(N) mode
  pir::ScanShape sh = pir::make_scan_shape(e->rows, e->pitch, c.num_rounds, e->num_cus);
  size_t slab = (size_t)sh.grid.x * sh.grid.y * sh.slab_bytes;
  const pir::QueryPlan qp = pir::make_query_plan(c.log_num_records, c.log_num_partitions, 2,
                                                 c.num_rounds, e->pitch, e->num_cus);
  if (qp.tile) slab = std::max(slab, pir::query_slab_bytes(qp));
  int rc = e->d_slabs.reserve(slab);
  // a shared queue at the widest share row (rows x 8 bytes whatever $PIR_GQ_G says)
  if (!rc && e->nrp <= 4) rc = ensure_group_queue(e, e->rows, 8 / e->nrp);
  if (!rc && e->nrp <= 4 && e->gq_share && !e->comm)
    rc = fold_image_reserve(e, woodruff_group_shape(e, e->rows, 8 / e->nrp));
  // the host forms' staging: one group's vectors, the keys, the results; the device form's
  // staging of unaligned keys, for the longest key a queue of this engine has brought so far
  const size_t vp = ((size_t)e->rows + 15) & ~(size_t)15;
  if (!rc) rc = e->d_coef_stage.reserve(vp * std::max(8, c.num_rounds));
  if (!rc)
    rc = e->d_shamir_res.reserve((size_t)num_keys * c.num_rounds * c.record_bytes);
  if (!rc && e->gq_key_bytes)
    rc = e->d_mpkey.reserve((size_t)num_keys * ((e->gq_key_bytes + 15) & ~15ull));
  return rc;
}

}  // extern "C"
