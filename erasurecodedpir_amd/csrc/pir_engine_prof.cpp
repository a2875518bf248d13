// pir_engine_prof.cpp -- the engine's profiling: per-answer event slots and their phase times,
// the per-kernel phase loop, k_query's per-workgroup trace.
#include "pir_engine_internal.h"

#ifndef PIR_TRACE_TREE_TILES
#define PIR_TRACE_TREE_TILES 0  // diagnostics build only (pir_kernels.hip)
#endif

using namespace eng;

namespace {

const char* const kPhaseNames[] = {"key_prep", "tree_frontier", "tree_leaves", "scan",
                                   "reduce", "comm_fold", "total", "chunks", "fused"};
constexpr int kNumPhases = 9;
// the k_query path (fused == 2: key, tree and scan are one kernel): "launch" = answer start ->
// k_query start (key upload, workspace ordering, dispatch), "scan" = the k_query launch,
// "reduce" = k_reduce (0 with an in-kernel reduce), "comm_fold" = the split-shard exchange and
// whatever follows; they add up to "total"
// A Shamir answer (fused == 4) uses the same five events: "launch" = answer start -> the response
// zeroed, "scan" = the rows pass, the strips pass and the Hermite scan, "reduce" = k_reduce of
// the Hermite slabs + k_shamir_totals
// A Woodruff answer (fused == 5: k_query's Woodruff mode, 6: k_woodruff_coefs + the scan) too:
// "launch" = answer start -> its first kernel, "scan" = that kernel (with 6, both), "reduce" =
// k_reduce; its derivative answers (fused == 7): "launch" = start -> the answer zeroed, "scan" =
// the rows pass, the totals kernel and the columns pass, "reduce" = 0; a shared Woodruff queue
// (fused == 8) and a shared queue of explicit-coefficient or sqrt(N) DPF keys (fused == 9):
// answer_group_queue; a shared Shamir queue (fused == 10): "launch" = start -> the responses
// zeroed, "scan" = the first key table -> the end of the last group's Hermite scan, "reduce" =
// the last group's k_reduce + k_shamir_totals; a shared Woodruff derivative queue (fused == 11):
// "launch" = start -> the responses zeroed, "scan" = the first key table -> the end of the last
// group's columns pass, "reduce" = 0
const char* const kQueryPhaseNames[] = {"launch", "scan", "reduce", "comm_fold", "total", "fused"};
constexpr int kNumQueryPhases = 6;

// Mean per-phase device times over the answers recorded since the last read.  tree_leaves and
// scan are the summed kernel durations of the C pipelined chunks (they overlap each other).
// Every slot is read with the layout of its own answer (only events recorded in it); the
// phases reported are those of the latest answer's path, a slot of the other layout adding to
// the phases the two share (scan, reduce, comm_fold, total).  A shared queue reports k_query's
// phases with fused = 0: "scan" = its first kernel -> the end of its last scan.
int read_timings(pir_engine* e, pir_kernel_time* out, int max) {
  if (e->prof.empty() || e->prof_count == 0) return 0;
  const int cnt = e->prof_count, sz = (int)e->prof.size();
  const pir_engine::ProfSlot& newest = e->prof[(e->prof_next + sz - 1) % sz];
  HIP_TRY(hipEventSynchronize(newest.ev[EV_END]));
  auto five = [](const pir_engine::ProfSlot& sl) { return sl.queue || sl.fused == 2; };
  // accumulators in kPhaseNames' order; "launch" (the five-event layout) beside them
  double acc[kNumPhases] = {}, launch = 0;
  auto el = [](hipEvent_t a, hipEvent_t b, double& sum) -> hipError_t {
    float ms = 0;
    hipError_t r = hipEventElapsedTime(&ms, a, b);
    sum += ms;
    return r;
  };
  for (int k = 0; k < cnt; ++k) {
    const pir_engine::ProfSlot& sl = e->prof[(e->prof_next + sz - cnt + k) % sz];
    const hipEvent_t* v = sl.ev;
    if (five(sl)) {
      HIP_TRY(el(v[EV_START], v[EV_SCAN_B], launch));
      HIP_TRY(el(v[EV_SCAN_B], v[EV_SCAN_E], acc[3]));
      HIP_TRY(el(v[EV_SCAN_E], v[EV_RED], acc[4]));
    } else {
      HIP_TRY(el(v[EV_START], v[EV_KEY], acc[0]));
      HIP_TRY(el(v[EV_KEY], v[EV_FRONT], acc[1]));
      for (int j = 0; j < sl.chunks; ++j) {
        HIP_TRY(el(v[EV_LEAF_B + j], v[EV_LEAF_E + j], acc[2]));
        HIP_TRY(el(v[EV_SCAN_B + j], v[EV_SCAN_E + j], acc[3]));
      }
      HIP_TRY(el(v[EV_PRERED], v[EV_RED], acc[4]));
    }
    HIP_TRY(el(v[EV_RED], v[EV_END], acc[5]));
    HIP_TRY(el(v[EV_START], v[EV_END], acc[6]));
    acc[7] += sl.chunks;
    acc[8] += sl.fused;
  }
  e->prof_count = 0;
  if (five(newest)) {
    const int nq = std::min(max, kNumQueryPhases);
    const double q[kNumQueryPhases] = {launch, acc[3], acc[4], acc[5], acc[6], acc[8]};
    for (int i = 0; i < nq; ++i) {
      snprintf(out[i].name, sizeof out[i].name, "%s", kQueryPhaseNames[i]);
      out[i].ms = (float)(q[i] / cnt);
    }
    return nq;
  }
  const int n = std::min(max, kNumPhases);
  for (int i = 0; i < n; ++i) {
    snprintf(out[i].name, sizeof out[i].name, "%s", kPhaseNames[i]);
    out[i].ms = (float)(acc[i] / cnt);
  }
  return n;
}

}  // namespace

// the next profiling slot, labelled with the path whose events it will hold
hipEvent_t* eng::prof_slot(pir_engine* e, int fused, int chunks, bool queue) {
  pir_engine::ProfSlot& sl = e->prof[e->prof_next];
  sl.fused = fused;
  sl.chunks = chunks;
  sl.queue = queue;
  e->prof_next = (e->prof_next + 1) % (int)e->prof.size();
  e->prof_count = std::min(e->prof_count + 1, (int)e->prof.size());
  return sl.ev;
}

extern "C" {

int pir_engine_set_profiling(pir_engine_t* e, int slots) {
  if (!e || slots < 0) return fail(PIR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (auto& sl : e->prof)
    for (auto& ev : sl.ev) (void)hipEventDestroy(ev);
  e->prof.assign((size_t)slots, {});
  e->prof_next = e->prof_count = 0;
  for (auto& sl : e->prof)
    // timing-only stamps: no system-scope fence (its cache write-back / invalidate at every
    // record slowed the bracketed k_query by ~2 % against the unprofiled answer)
    for (auto& ev : sl.ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableSystemFence));
  return PIR_OK;
}

int pir_engine_last_timings(pir_engine_t* e, pir_kernel_time* out, int max) {
  if (!e || !out) return fail(PIR_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  return read_timings(e, out, max);
}

int pir_engine_profile_phases(pir_engine_t* e, const uint8_t* d_key, int iters, float* out_ms) {
  if (!e || !d_key || !out_ms || iters < 1) return fail(PIR_EINVAL, "bad argument");
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  const auto& c = e->cfg;
  hipStream_t s = e->stream;
  const pir::TreePlan pl =
      pir::make_plan(c.log_num_records, c.log_num_partitions, (uint64_t)c.partition_index, -1, c.num_parties);
  const pir::ScanShape sh = pir::make_scan_shape(pl.nleaves, e->pitch, c.num_rounds, e->num_cus);
  int rc = e->d_slabs.reserve((size_t)sh.grid.x * sh.grid.y * sh.slab_bytes);
  if (rc) return rc;
  hipEvent_t ev[6];
  for (auto& x : ev) HIP_TRY(hipEventCreate(&x));
  HIP_TRY(hipEventRecord(ev[0], s));
  for (int i = 0; i < iters; ++i)
    HIP_TRY(pir::launch_key_prep(d_key, e->key_len, 1, c.num_parties, c.log_num_records,
                                 c.num_rounds, c.party_index - 1, e->d_keys, s));
  HIP_TRY(hipEventRecord(ev[1], s));
  for (int i = 0; i < iters; ++i)
    HIP_TRY(pir::launch_frontier(pl, key_src(e, nullptr), e->nodes, s));
  HIP_TRY(hipEventRecord(ev[2], s));
  for (int i = 0; i < iters; ++i)
    HIP_TRY(pir::launch_stages(pl, e->d_keys, e->nodes, 0, 1, e->d_c, e->nrp, s));
  HIP_TRY(hipEventRecord(ev[3], s));
  for (int i = 0; i < iters; ++i)
    HIP_TRY(pir::launch_scan(sh, e->d_shard, pl.nleaves, e->d_c, e->d_slabs, false, s));
  HIP_TRY(hipEventRecord(ev[4], s));
  for (int i = 0; i < iters; ++i) HIP_TRY(pir::launch_reduce(sh, e->d_slabs, c.record_bytes, e->d_result, s));
  HIP_TRY(hipEventRecord(ev[5], s));
  HIP_TRY(hipEventSynchronize(ev[5]));
  sc.synced();
  for (int i = 0; i < 5; ++i) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
    out_ms[i] = ms / iters;
  }
  for (auto& x : ev) (void)hipEventDestroy(x);
  return PIR_OK;
}

int pir_engine_trace_query(pir_engine_t* e, const uint8_t* d_key, int num_keys, uint64_t* out,
                           int max_wgs) {
  if (!e || !d_key || !out || max_wgs < 0 || num_keys < 1) return fail(PIR_EINVAL, "bad argument");
  const auto& c = e->cfg;
  const pir::QueryPlan qp = pir::make_query_plan(c.log_num_records, c.log_num_partitions,
                                                 c.num_parties, c.num_rounds, e->pitch, e->num_cus,
                                                 num_keys);
  if (!qp.tile) return fail(PIR_EINVAL, "shape does not use the single-launch query kernel");
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  const pir::ScanShape& sh = qp.shape;
  int rc = e->d_slabs.reserve((size_t)num_keys * pir::query_slab_bytes(qp));
  if (!rc) rc = e->d_qscratch.reserve(pir::query_scratch_bytes(qp));
  pir::StealArgs steal;
  if (!rc) rc = steal_args(e, qp, num_keys, 1, e->stream, &steal);
  if (rc) return rc;
  const int nwg = (int)sh.grid.x;
  const size_t bytes = (size_t)nwg * pir::kQueryTraceSlots * sizeof(uint64_t);
  DevBuf<uint64_t> d_tr;
  if (int rc2 = d_tr.reserve(bytes + sizeof(uint64_t))) return rc2;
  std::vector<uint64_t> h((size_t)nwg * pir::kQueryTraceSlots);
  hipError_t err = hipMemsetAsync(d_tr, 0, bytes, e->stream);
  const char* dbg = getenv("PIR_TRACE_NOSCAN");  // diagnostics: scan waves skip their rows
  uint64_t flags = (dbg && dbg[0] == '1') ? 1u : 0u;
#if PIR_TRACE_TREE_TILES
  if (const char* tv = getenv("PIR_TRACE_TILES")) {  // "a,b": two queue tiles' tree phases
    unsigned a = 0, b = 0;
    if (sscanf(tv, "%u,%u", &a, &b) >= 1) flags |= ((uint64_t)(a & 0xffu) << 8) | ((uint64_t)(b & 0xffu) << 16);
  }
#endif
  if (err == hipSuccess)
    err = hipMemcpyAsync(d_tr + (size_t)nwg * pir::kQueryTraceSlots, &flags, sizeof flags,
                         hipMemcpyHostToDevice, e->stream);
  if (err == hipSuccess)
    err = pir::launch_query(qp, d_key, (uint32_t)e->key_len, num_keys, c.num_parties, c.log_num_records,
                            c.party_index - 1, c.log_num_partitions, (uint64_t)c.partition_index,
                            e->d_shard, e->d_slabs, e->d_qscratch, e->stream, d_tr, nullptr,
                            nullptr, 0u, 0u, steal);
  if (err == hipSuccess) err = hipMemcpyAsync(h.data(), d_tr, bytes, hipMemcpyDeviceToHost, e->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  if (err != hipSuccess) return fail(PIR_EHIP, "trace_query: %s", hipGetErrorString(err));
  sc.synced();
  uint64_t t0 = ~0ull;
  for (int w = 0; w < nwg; ++w) t0 = std::min(t0, h[(size_t)w * pir::kQueryTraceSlots]);
  const int n = std::min(nwg, max_wgs);
  for (int w = 0; w < n; ++w)
    for (int k = 0; k < pir::kQueryTraceSlots; ++k) {
      const uint64_t v = h[(size_t)w * pir::kQueryTraceSlots + k];
      // shader-clock ticks and counts as they are
      const bool raw = k == 56 || k == 57 || k == 59 || k == 60 || k == 61 ||
                       (k >= 128 && k < 160) || (k >= 192 && !(PIR_TRACE_TREE_TILES && k >= 208));
      out[(size_t)w * pir::kQueryTraceSlots + k] = raw ? v : (v ? v - t0 : 0);
    }
  return nwg;
}

}  // extern "C"
