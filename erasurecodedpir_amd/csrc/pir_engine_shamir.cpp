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

// ---- queued keys that share shard passes ----------------------------------------------------
// The K x num_rounds rounds of a queue are independent virtual keys (pir_shamir.h).  Slots per
// pass of a queue of nv virtual keys by default; 0: every key its own answer.  A pure function of
// the shape, on only where the shared queue measured faster than the parent build's single
// answers back to back by more than the largest spread of any leg of that run
// (tools/bench_shamir.py --queue, profiles/shamir_queue/README.md); everything unmeasured is off.
int shamir_share_policy(uint32_t pitch, uint64_t rows, int nv) {
  // measured: queues of 2, 3, 4, 8 and 20 one-round keys over 2^20 and 2^24 value rows of 1 KiB,
  // 2^24 of 256 B and 2^22 of 2 KiB (the engine holds twice as many rows), 8 slots per pass.
  // 2 keys: 1.4-2.0x the parent, 4: 2.8-4.0x, 8: 5.1-7.5x, 20 (7 + 7 + 6): 4.6-6.0x, every one
  // by more than the spread (a pass of 8 slots costs 1.4 single answers at 2^24 x 1 KiB)
  if (nv < 2) return 0;
  const bool measured = (pitch == 1024 && rows >= (1ull << 21)) ||
                        (pitch == 256 && rows >= (1ull << 25)) ||
                        (pitch == 2048 && rows >= (1ull << 23));
  return measured ? pir::kShamirSlots : 0;
}
// which value passes of a group of ng virtual keys run k_shamir_seg (bit 0: Rx, bit 1: Ry); the
// others run k_shamir_rows / k_shamir_strips over the group's virtual keys, up to kShamirRounds
// per launch.  A transposed pass costs the same for 2 slots as for 8; the four-round kernels
// grow with the keys.  Measured pass by pass ($PIR_SH_PASS legs of the same run): the transposed
// pass beat the four-round kernels by more than the spread for every group of 3 and more on all
// four shapes, and for groups of 2 at 2^20 x 1 KiB and 2^24 x 256 B; for groups of 2 at 2^24 x
// 1 KiB it lost (Rx 12.11 against 10.93 ms, Ry against 10.68; both on the four-round kernels
// 10.26; spread 1.01) and at 2^22 x 2 KiB it lost or stayed inside the spread (5.96 against
// 5.48 / 5.28, both 5.06; spread 0.55): there both passes run the existing kernels
int shamir_pass_policy(uint32_t pitch, uint64_t rows, int ng) {
  const bool lost = (pitch == 1024 && rows >= (1ull << 25)) || (pitch == 2048 && rows >= (1ull << 23));
  return ng <= 2 && lost ? 0 : 3;
}

// the slots per pass of a Shamir queue of nv virtual keys (0: unshared).  $PIR_SH_SHARE: 0 never
// shares, 1 (default) follows shamir_share_policy, 2 shares every queue of two or more virtual
// keys on a shape k_shamir_seg takes (records of >= 256 B); $PIR_SH_G overrides the slots
int shamir_group(const pir_engine* e, int nv) {
  if (e->sh_share == 0 || nv < 2 || !pir::shamir_seg_takes(e->pitch) || e->nrp > 8) return 0;
  int g = shamir_share_policy(e->pitch, e->rows, nv);
  if (g == 0 && e->sh_share < 2) return 0;
  if (g == 0) g = pir::kShamirSlots;
  return e->sh_group > 0 ? e->sh_group : g;
}

// the 8-round scan of a group's share rows over nrec Hermite rows
pir::ScanShape shamir_group_shape(const pir_engine* e, uint64_t nrec) {
  return woodruff_group_shape(e, nrec, pir::kShamirSlots / e->nrp);
}

// every buffer a Shamir queue of up to nk keys over up to nrec records touches, shared or not
int ensure_shamir_queue(pir_engine* e, const pir::ShamirDims& d, int nk, uint64_t nrec) {
  const auto& c = e->cfg;
  pir::ScanShape sh = pir::make_scan_shape(std::max<uint64_t>(nrec, 1), e->pitch, c.num_rounds,
                                           e->num_cus);
  size_t slab = (size_t)sh.grid.x * sh.grid.y * sh.slab_bytes;
  int rc = PIR_OK;
  if (nrec && shamir_group(e, nk * c.num_rounds)) {
    sh = shamir_group_shape(e, nrec);
    slab = std::max(slab, (size_t)sh.grid.x * sh.grid.y * sh.slab_bytes);
    // the share rows, then the group's interleaved key table
    rc = e->d_cb.reserve(wd_share_bytes(nrec, pir::kShamirSlots) + (size_t)(d.X + d.Y) * 8);
    if (!rc) rc = e->d_gtmp.reserve((size_t)16 * c.record_bytes);
  }
  if (!rc) rc = e->d_slabs.reserve(slab);
  return rc;
}

// A queue of nk Shamir keys over the records [rec0, rec0 + nrec): key k's round a at d_keys +
// k * key_stride + a * key_pitch, d_result nk x num_rounds x response_len, result k what
// answer_shamir_locked gives for key k.  Shared (shamir_group > 0): the nk * num_rounds virtual
// keys go into groups of as equal sizes as possible, and per group, all on s: the key table, the
// two value passes (k_shamir_seg, or k_shamir_rows / _strips where shamir_pass_policy says so)
// straight into the responses, k_shamir_coefs_g + the 8-round scan of the Hermite rows + k_reduce
// into d_gtmp, and k_shamir_totals per run of virtual keys that are equally spaced.  Five-event
// layout, fused = 10: "launch" = start -> the responses zeroed, "scan" = the first key table ->
// the end of the last Hermite scan, "reduce" = the last group's k_reduce and totals.  Unshared,
// empty ranges and a Byzantine engine's whole domain: the single answers back to back on s.
int answer_shamir_queue_locked(pir_engine* e, const uint8_t* d_keys, uint64_t key_pitch,
                               uint64_t key_stride, int nk, uint64_t rec0, uint64_t nrec,
                               uint8_t* d_result, hipStream_t s) {
  const auto& c = e->cfg;
  const int R = c.num_rounds;
  const uint64_t N = e->rows / 2;
  const pir::ShamirDims d = pir::shamir_dims(c.log_num_records - 1, c.record_bytes);
  const size_t out_bytes = (size_t)R * d.resp_len;
  const bool random = c.is_byzantine && rec0 == 0 && nrec == N;
  const int G = nrec && !random ? shamir_group(e, nk * R) : 0;
  if (int rc = ensure_shamir_queue(e, d, nk, nrec)) return rc;
  if (G == 0) {
    for (int k = 0; k < nk; ++k)
      if (int rc = answer_shamir_locked(e, d_keys + (uint64_t)k * key_stride, key_pitch, rec0, nrec,
                                        d_result + (size_t)k * out_bytes, s))
        return rc;
    return PIR_OK;
  }
  e->ev = nullptr;
  hipEvent_t* ev = nullptr;
  if (!e->prof.empty()) {
    ev = prof_slot(e, 10, 1, true);
    HIP_TRY(hipEventRecord(ev[EV_START], s));
  }
  HIP_TRY(hipMemsetAsync(d_result, 0, (size_t)nk * out_bytes, s));
  if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_B], s));
  const pir::ScanShape sh = shamir_group_shape(e, nrec);
  uint8_t* const d_kT = e->d_cb + wd_share_bytes(nrec, pir::kShamirSlots);
  // $PIR_SH_PASS (diagnostics, read per answer): the passes on k_shamir_seg, whatever the policy
  const char* pv = getenv("PIR_SH_PASS");
  const uint64_t lo = rec0, hi = rec0 + nrec;
  auto key_of = [&](int v) { return d_keys + (uint64_t)(v / R) * key_stride + (uint64_t)(v % R) * key_pitch; };
  // the virtual keys [v, v + n) that are equally spaced from v on, at most `most`: one round
  // per key: key_stride apart; else the rounds of one key, key_pitch apart
  auto run_of = [&](int v, int end, int most, uint64_t* pitch) {
    *pitch = R == 1 ? key_stride : key_pitch;
    const int n = R == 1 ? end - v : std::min(end - v, R - v % R);
    return std::min(n, most);
  };
  const int nv = nk * R, ngroups = (nv + G - 1) / G;
  for (int v0 = 0, j = 0, ng = 0; v0 < nv; v0 += ng, ++j) {
    ng = nv / ngroups + (j < nv % ngroups ? 1 : 0);
    uint8_t* const out = d_result + (size_t)v0 * d.resp_len;
    const int passes = pv && pv[0] ? atoi(pv) & 3 : shamir_pass_policy(e->pitch, e->rows, ng);
    HIP_TRY(pir::launch_shamir_key_table(d, d_keys, key_pitch, key_stride, R, v0, ng, d_kT, s));
    for (int strided = 0; strided < 2; ++strided) {
      if (passes >> strided & 1) {
        HIP_TRY(pir::launch_shamir_seg(d, e->d_shard, e->pitch, c.record_bytes, d_kT, ng, lo, hi,
                                       strided != 0, out, s));
        continue;
      }
      for (int v = v0, n = 0; v < v0 + ng; v += n) {
        uint64_t kp = 0;
        n = run_of(v, v0 + ng, pir::kShamirRounds, &kp);
        uint8_t* const o = d_result + (size_t)v * d.resp_len;
        if (strided)
          HIP_TRY(pir::launch_shamir_strips(d, e->d_shard, e->pitch, c.record_bytes, key_of(v), kp, n,
                                            lo, hi, o, s));
        else
          HIP_TRY(pir::launch_shamir_rows(d, e->d_shard, e->pitch, c.record_bytes, key_of(v), kp, n,
                                          lo, hi, o, s));
      }
    }
    HIP_TRY(pir::launch_shamir_coefs_g(d, d_kT, lo, hi, e->d_cb, s));
    HIP_TRY(pir::launch_scan(sh, e->d_shard + (N + rec0) * e->pitch, nrec, e->d_cb, e->d_slabs,
                             false, s));
    if (ev && v0 + ng >= nv) HIP_TRY(hipEventRecord(ev[EV_SCAN_E], s));
    HIP_TRY(pir::launch_reduce(sh, e->d_slabs, c.record_bytes, e->d_gtmp, s));
    for (int v = v0, n = 0; v < v0 + ng; v += n) {
      uint64_t kp = 0;
      n = run_of(v, v0 + ng, pir::kShamirSlots, &kp);
      HIP_TRY(pir::launch_shamir_totals(d, c.record_bytes, key_of(v), kp, n,
                                        e->d_gtmp + (size_t)(v - v0) * c.record_bytes,
                                        d_result + (size_t)v * d.resp_len, s));
    }
  }
  e->last_fused = 10;
  if (ev) {
    HIP_TRY(hipEventRecord(ev[EV_RED], s));
    HIP_TRY(hipEventRecord(ev[EV_END], s));
  }
  return PIR_OK;
}

int check_shamir_queue(const pir_engine* e, uint64_t key_pitch, uint64_t key_stride, int nk) {
  const pir::ShamirDims d = pir::shamir_dims(e->cfg.log_num_records - 1, e->cfg.record_bytes);
  if (e->cfg.num_rounds > 1 && key_pitch < d.X + d.Y)
    return fail(PIR_EINVAL, "key_pitch %llu < the key's %llu bytes", (unsigned long long)key_pitch,
                (unsigned long long)(d.X + d.Y));
  if (nk > 1 && key_stride < d.X + d.Y)
    return fail(PIR_EINVAL, "key_stride %llu < the key's %llu bytes",
                (unsigned long long)key_stride, (unsigned long long)(d.X + d.Y));
  return PIR_OK;
}

}  // namespace

extern "C" {

int pir_engine_answer_shamir_queue_dev(pir_engine_t* e, const uint8_t* d_keys, uint64_t key_pitch,
                                       uint64_t key_stride, int num_keys, uint64_t rec0,
                                       uint64_t nrec, uint8_t* d_result, void* stream) {
  if (int rc = check_queue_args(e, num_keys, d_keys, d_result)) return rc;
  if (int rc = check_shamir(e, rec0, nrec)) return rc;
  if (int rc = check_shamir_queue(e, key_pitch, key_stride, num_keys)) return rc;
  if (num_keys == 0) return PIR_OK;
  AnswerScope sc(e, stream);
  if (sc.rc()) return sc.rc();
  return sc.finish(answer_shamir_queue_locked(e, d_keys, key_pitch, key_stride, num_keys, rec0,
                                              nrec, d_result, sc.stream()));
}

int pir_engine_answer_shamir_queue(pir_engine_t* e, const uint8_t* const* keys, int num_keys,
                                   uint64_t rec0, uint64_t nrec, uint8_t* results) {
  if (int rc = check_queue_args(e, num_keys, keys, results)) return rc;
  if (int rc = check_shamir(e, rec0, nrec)) return rc;
  if (num_keys == 0) return PIR_OK;
  const auto& c = e->cfg;
  const size_t nv = (size_t)num_keys * c.num_rounds;
  for (size_t v = 0; v < nv; ++v)
    if (!keys[v]) return fail(PIR_EINVAL, "null key %zu", v);
  const pir::ShamirDims d = pir::shamir_dims(c.log_num_records - 1, c.record_bytes);
  const uint64_t klen = d.X + d.Y;
  const size_t out_bytes = nv * d.resp_len;
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  int rc = e->d_coef_stage.reserve(nv * klen);
  if (!rc) rc = e->d_shamir_res.reserve(out_bytes);
  if (rc) return rc;
  for (size_t v = 0; v < nv; ++v)
    HIP_TRY(hipMemcpyAsync(e->d_coef_stage + v * klen, keys[v], klen, hipMemcpyHostToDevice,
                           e->stream));
  rc = sc.finish(answer_shamir_queue_locked(e, e->d_coef_stage, klen, c.num_rounds * klen, num_keys,
                                            rec0, nrec, e->d_shamir_res, e->stream));
  if (rc) return rc;
  return download(results, e->d_shamir_res, out_bytes, e->stream);
}

int pir_engine_reserve_shamir_queue(pir_engine_t* e, int num_keys) {
  if (!e || num_keys < 1) return fail(PIR_EINVAL, "bad argument");
  if (int rc = check_shamir(e, 0, 0)) return rc;
  const auto& c = e->cfg;
  const pir::ShamirDims d = pir::shamir_dims(c.log_num_records - 1, c.record_bytes);
  const size_t nv = (size_t)num_keys * c.num_rounds;
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(c.device));
  int rc = ensure_shamir_queue(e, d, num_keys, e->rows / 2);
  // the host form's staging
  if (!rc) rc = e->d_coef_stage.reserve(nv * (d.X + d.Y));
  if (!rc) rc = e->d_shamir_res.reserve(nv * d.resp_len);
  return rc;
}

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
  ShardWrite sw(e);
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
