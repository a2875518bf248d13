// pir_engine.cpp -- host side of the C ABI in include/pir_engine.h.
//
// One engine = one GPU holding one shard (or one 2^-G partition of a logical shard) in HBM,
// laid out as rows of `pitch` = round_up(record_bytes, 16) bytes (zero padding), so every
// lane of the scan reads aligned 16-byte chunks.  An answer is four kernels on one stream:
//   key prep -> tree (frontier + leaves) -> GF(2^8) scan -> slab reduce
// plus, for a split shard, an RCCL all-gather of the per-partition answers and an XOR fold
// (RCCL has no XOR reduction op).
//
// This file: create / destroy, the workspace ordering between answers (AnswerScope), the DPF-tree
// answers and the small device utilities.  The rest of the host code is in
// pir_engine_{comm,shard,shamir,woodruff,group,prof}.cpp, pir_engine_internal.h between them.
#include <stdarg.h>

#include <string>

#include "pir_engine_internal.h"

using namespace eng;

static thread_local std::string g_err;

int eng::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

pir::KeySrc eng::key_src(pir_engine* e, const uint8_t* d_raw) {
  const auto& c = e->cfg;
  return pir::KeySrc{d_raw, c.num_parties, c.log_num_records, c.num_rounds, c.party_index - 1,
                     e->d_keys};
}

namespace {

constexpr int kFrontBatch = 256;  // batched answers: keys whose upper tree levels run together
constexpr uint64_t kBatchNodeBytes = 4ull << 30;  // ... within this much node memory

int ilog2_exact(uint64_t v) {
  if (v == 0 || (v & (v - 1))) return -1;
  int l = 0;
  while ((1ull << l) < v) ++l;
  return l;
}

int ensure_batch(pir_engine* e, int nk) {
  if (nk <= e->max_batch) return PIR_OK;
  e->d_key_raw.release();
  e->d_keys.release();
  e->max_batch = 0;
  if (int rc = e->d_key_raw.reserve((size_t)nk * e->key_len)) return rc;
  if (int rc = e->d_keys.reserve((size_t)nk * sizeof(pir::DevKey))) return rc;
  e->max_batch = nk;
  return PIR_OK;
}

int pick_chunks(const pir::TreePlan& pl, int num_cus) {
  // pipeline the leaf stage only while each chunk's launch still covers every CU
  const int blocks = pir::final_stage_blocks(pl);
  int c = 1;
  while (2 * c <= kMaxChunks && blocks % (2 * c) == 0 && blocks / (2 * c) >= num_cus) c *= 2;
  return c;
}

// Answer one partition slice: rows [row0, row0 + 2^(n - log_parts_total)) of this engine
// with the tree rooted at `prefix` (depth log_parts_total).  d_key points at ONE parsed key.
//   s  : key prep, frontier, leaves(0..C-1), [join], reduce
//   aux: scan(j) after leaves(j)  -- so leaves(j+1) overlaps scan(j)
int answer_fused(pir_engine* e, const uint8_t* d_raw, int log_parts_total, uint64_t prefix,
                 uint64_t row0, uint8_t* d_out, hipStream_t s, int tile) {
  const pir::DevKey* d_key = e->d_keys;
  const auto& c = e->cfg;
  const pir::TreePlan pl =
      pir::make_plan(c.log_num_records, log_parts_total, prefix, pir::fused_k(tile), c.num_parties);
  const pir::ScanShape sh =
      pir::make_fused_shape(pl.nleaves, e->pitch, c.num_rounds, e->num_cus, tile);
  int rc = e->d_slabs.reserve((size_t)sh.grid.x * sh.grid.y * sh.slab_bytes);
  if (rc) return rc;
  e->last_chunks = 1;
  e->last_fused = 1;
  hipEvent_t* ev = e->ev;
  if (ev) HIP_TRY(hipEventRecord(ev[EV_KEY], s));
  HIP_TRY(pir::launch_frontier(pl, key_src(e, d_raw), e->nodes, s));
  HIP_TRY(pir::launch_stages(pl, d_key, e->nodes, 0, 1, e->d_c, e->nrp, s, 0, pl.nstages - 1));
  if (ev) {
    HIP_TRY(hipEventRecord(ev[EV_FRONT], s));
    HIP_TRY(hipEventRecord(ev[EV_LEAF_B], s));
    HIP_TRY(hipEventRecord(ev[EV_LEAF_E], s));
    HIP_TRY(hipEventRecord(ev[EV_SCAN_B], s));
  }
  HIP_TRY(pir::launch_fused(pl, d_key, e->nodes, e->d_shard + row0 * e->pitch, sh, e->d_slabs,
                            tile, s));
  if (ev) {
    HIP_TRY(hipEventRecord(ev[EV_SCAN_E], s));
    HIP_TRY(hipEventRecord(ev[EV_PRERED], s));
  }
  HIP_TRY(pir::launch_reduce(sh, e->d_slabs, c.record_bytes, d_out, s));
  if (ev) HIP_TRY(hipEventRecord(ev[EV_RED], s));
  return PIR_OK;
}

// grow a buffer that is kept zeroed between launches (k_query's slab counters, its stealing
// flags: no flag equals a generation >= 1): a launch still in flight on s may read the old one
template <class T>
int reserve_zeroed(DevBuf<T>& b, size_t bytes, hipStream_t s) {
  if (bytes <= b.cap) return PIR_OK;
  if (b) HIP_TRY(hipStreamSynchronize(s));
  if (int rc = b.reserve(bytes)) return rc;
  HIP_TRY(hipMemsetAsync(b, 0, bytes, s));
  return PIR_OK;
}
// nk zeroed slab counters for k_query's fused reduce (the kernel leaves them zero)
int ensure_qcnt(pir_engine* e, int nk, hipStream_t s) {
  return reserve_zeroed(e->d_qcnt, (size_t)nk * sizeof(uint32_t), s);
}

}  // namespace

// the work-stealing arguments of a k_query launch (empty = static tiles): a lone query (nk == 1)
// answered whole (nslices == 1: a stolen chunk is folded into the thief's region slab) with one
// column group, on at most one workgroup per CU (every workgroup resident, so the bounded wait
// for unpublished last tiles never outlasts a late one's dispatch)
int eng::steal_args(pir_engine* e, const pir::QueryPlan& qp, int nk, int nslices, hipStream_t s,
                    pir::StealArgs* out) {
  *out = pir::StealArgs{};
  if (!PIR_QUERY_STEAL || !e->steal || nk != 1 || nslices != 1 || qp.shape.nq > 2 || !qp.shape.uniform ||
      qp.shape.grid.y != 1 || (int)qp.shape.grid.x > e->num_cus || qp.m4r)
    return PIR_OK;
  // a captured launch would replay one generation: flags left equal to it by the previous
  // replay would read as published shares
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIP_TRY(hipStreamIsCapturing(s, &cap));
  if (cap != hipStreamCaptureStatusNone) return PIR_OK;
  if (int rc = reserve_zeroed(e->d_steal, pir::query_steal_bytes(qp), s)) return rc;
  if (++e->steal_gen == 0) e->steal_gen = 1;
  out->buf = e->d_steal;
  out->gen = e->steal_gen;
  out->mode = (uint32_t)e->steal;
  return PIR_OK;
}

namespace {

// one launch: key parse, tree and scan of nk queued keys (key_len apart) in k_query; then the
// slab reduce of all nk answers (d_out: nk x nq x efs)
// nslices > 1 (a power of two <= 2^qp.lr, nk == 1): d_out gets the nslices partial answers
// over equal consecutive row ranges instead of the whole answer (runOptimizedDPFTreeQueryThread
// for every thread of a query at once: the slices are runs of k_query's region slabs)
int answer_query(pir_engine* e, const pir::QueryPlan& qp, const uint8_t* d_raw, int nk,
                 int log_parts_total, uint64_t prefix, uint64_t row0, uint8_t* d_out,
                 hipStream_t s, int nslices = 1) {
  const auto& c = e->cfg;
  const pir::ScanShape& sh = qp.shape;
  int rc = e->d_slabs.reserve((size_t)nk * pir::query_slab_bytes(qp));
  if (!rc) rc = e->d_qscratch.reserve(pir::query_scratch_bytes(qp));
  // modes 2 and 3 need whole answer words at aligned addresses, mode 3 at least 8 slabs;
  // otherwise k_reduce (always for slices)
  int fred = e->fused_reduce;
  if (fred >= 2 && (c.record_bytes % 4 != 0 || reinterpret_cast<uintptr_t>(d_out) % 4 != 0)) fred = 0;
  if (fred == 3 && qp.lr < 3) fred = 1;
  if (nslices > 1) fred = 0;
  if (!rc && fred) rc = ensure_qcnt(e, nk * (fred == 3 ? 8 : 1), s);
  pir::StealArgs steal;
  if (!rc) rc = steal_args(e, qp, nk, nslices, s, &steal);
  if (rc) return rc;
  if (fred >= 2)  // the workgroups (mode 2) or slab groups (mode 3) XOR into zeroed answers
    HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)nk * c.num_rounds * c.record_bytes, s));
  e->last_chunks = 1;
  e->last_fused = 2;
  // profiling: k_query has no separate key / tree / scan kernels, so only its own bounds and
  // the reduce are stamped (each event record between two launches costs the next one a few us
  // of dispatch: fewer stamps keep the profiled answer close to the unprofiled one)
  hipEvent_t* ev = e->ev;
  if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_B], s));
  HIP_TRY(pir::launch_query(qp, d_raw, (uint32_t)e->key_len, nk, c.num_parties,
                            c.log_num_records, c.party_index - 1, log_parts_total, prefix,
                            e->d_shard + row0 * e->pitch, e->d_slabs, e->d_qscratch, s, nullptr,
                            fred ? d_out : nullptr, e->d_qcnt, c.record_bytes, (uint32_t)fred,
                            steal));
  if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_E], s));
  if (!fred) HIP_TRY(pir::launch_reduce(sh, e->d_slabs, c.record_bytes, d_out, s, nk, nslices));
  if (ev) HIP_TRY(hipEventRecord(ev[EV_RED], s));
  return PIR_OK;
}

int answer_core(pir_engine* e, const uint8_t* d_raw, int log_parts_total, uint64_t prefix,
                uint64_t row0, uint8_t* d_out, hipStream_t s) {
  const auto& c = e->cfg;
  const pir::DevKey* d_key = e->d_keys;
  const uint64_t nleaves = 1ull << (c.log_num_records - log_parts_total);
  if (e->allow_query && e->allow_fused) {
    const pir::QueryPlan qp = pir::make_query_plan(c.log_num_records, log_parts_total,
                                                   c.num_parties, c.num_rounds, e->pitch, e->num_cus);
    if (qp.tile) return answer_query(e, qp, d_raw, 1, log_parts_total, prefix, row0, d_out, s);
  }
  const int tile = e->allow_fused ? pir::fused_tile(c.num_rounds, e->pitch, nleaves, e->num_cus) : 0;
  if (tile) return answer_fused(e, d_raw, log_parts_total, prefix, row0, d_out, s, tile);
  e->last_fused = 0;
  const pir::TreePlan pl = pir::make_plan(c.log_num_records, log_parts_total, prefix, -1, c.num_parties);
  const int C = pick_chunks(pl, e->num_cus);
  e->last_chunks = C;
  const uint64_t nrec = pl.nleaves / C;
  const pir::ScanShape sh = pir::make_scan_shape(nrec, e->pitch, c.num_rounds, e->num_cus);
  int rc = e->d_slabs.reserve((size_t)sh.grid.x * sh.grid.y * sh.slab_bytes);
  if (rc) return rc;
  hipEvent_t* ev = e->ev;
  if (ev) HIP_TRY(hipEventRecord(ev[EV_KEY], s));
  HIP_TRY(pir::launch_frontier(pl, key_src(e, d_raw), e->nodes, s));
  HIP_TRY(pir::launch_stages(pl, d_key, e->nodes, 0, 1, e->d_c, e->nrp, s, 0, pl.nstages - 1));
  if (ev) HIP_TRY(hipEventRecord(ev[EV_FRONT], s));
  for (int j = 0; j < C; ++j) {
    if (ev) HIP_TRY(hipEventRecord(ev[EV_LEAF_B + j], s));
    HIP_TRY(pir::launch_stages(pl, d_key, e->nodes, j, C, e->d_c, e->nrp, s, pl.nstages - 1));
    if (ev) HIP_TRY(hipEventRecord(ev[EV_LEAF_E + j], s));
    HIP_TRY(hipEventRecord(e->ev_leaf[j], s));
    HIP_TRY(hipStreamWaitEvent(e->aux, e->ev_leaf[j], 0));
    if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_B + j], e->aux));
    HIP_TRY(pir::launch_scan(sh, e->d_shard + (row0 + j * nrec) * e->pitch, nrec,
                             e->d_c + j * nrec * e->nrp, e->d_slabs, j > 0, e->aux));
    if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_E + j], e->aux));
  }
  HIP_TRY(hipEventRecord(e->ev_join, e->aux));
  HIP_TRY(hipStreamWaitEvent(s, e->ev_join, 0));
  if (ev) HIP_TRY(hipEventRecord(ev[EV_PRERED], s));
  HIP_TRY(pir::launch_reduce(sh, e->d_slabs, c.record_bytes, d_out, s));
  if (ev) HIP_TRY(hipEventRecord(ev[EV_RED], s));
  return PIR_OK;
}

// keys answered per shard pass: G keys x nrp share bytes per record (a power of two <= 16)
int clamp_group(const pir_engine* e, int g) {
  g = std::max(1, std::min(g, 16 / e->nrp));
  while (g & (g - 1)) g &= g - 1;  // power of two
  return g;
}
int batch_group(const pir_engine* e) {
  return clamp_group(e, e->batch_group > 0 ? e->batch_group : 8 / std::min(e->nrp, 8));
}

// Keys per shard pass of a queue (answer_stream) by default; 0: every query its own pass in
// k_query.  A pure function of the shape, enabled only where the shared queue measured faster
// than k_query's queue of the parent build on the same machine, alternating runs
// (profiles/stream_share/README.md).
int stream_share_policy(int rounds, uint32_t pitch, uint64_t rows, int nk) {
  // measured: one round, 8 keys per pass (k_scan_t), 2^20 / 2^24 / 2^27 rows of 1 KiB and 2^24
  // of 256 B, all 1.5-1.8x k_query's queue of 20; 4 and 2 keys per pass gain less, 16 lose; a
  // pass of 8 key slots costs about two of k_query's, so queues of fewer than 4 keys stay there;
  // five rounds (two keys per pass) lose by 15x
  if (rounds != 1 || nk < 4) return 0;
  if (pitch < 256 || pitch > 1024 || pitch % 256 != 0 || rows < (1ull << 20)) return 0;
  return 8;
}

// the group size answer_stream uses for a queue of nk keys (0: k_query).  $PIR_STREAM_SHARE: 0
// never shares, 1 (default) follows stream_share_policy, 2 shares wherever the batched path
// takes the shape; $PIR_STREAM_G overrides the group size (diagnostics)
int stream_group(const pir_engine* e, int nk) {
  const auto& c = e->cfg;
  if (e->stream_share == 0 || nk < 2 || c.is_byzantine || e->nrp > 8) return 0;
  int g = stream_share_policy(c.num_rounds, e->pitch, e->rows, nk);
  if (g == 0 && e->stream_share < 2) return 0;
  if (g == 0) g = std::max(2, 8 / e->nrp);
  if (e->stream_group > 0) g = e->stream_group;
  g = clamp_group(e, g);
  return g >= 2 ? g : 0;
}
}  // namespace

// the scan of a group of gw <= G key slots (gw * nrp rounds); key-major shares for k_scan_t,
// which a narrowed group (gw < G) takes wherever it can
pir::ScanShape eng::group_scan_shape(const pir_engine* e, uint64_t nleaves, int gw, int G,
                                     bool* kmaj) {
  pir::ScanShape sh = pir::make_scan_shape(nleaves, e->pitch, gw * e->nrp, e->num_cus,
                                           e->batch_scan_bpc, gw < G);
  // k_scan_t reads the group's shares key-major (key g's nrp bytes of leaf i at g * nleaves *
  // nrp + i * nrp), so each tree's leaf stage writes its shares contiguously (packed 16-byte
  // stores); the other scans read them interleaved per record (cb[i][W], key g at g * nrp).
  // One key slot: the two layouts are the same one
  *kmaj = sh.tfold && gw > 1 && !(getenv("PIR_BATCH_KMAJOR") && atoi(getenv("PIR_BATCH_KMAJOR")) == 0);
  if (*kmaj) {
    sh.ckey = (uint32_t)e->nrp;
    sh.ckoff = (uint64_t)nleaves * e->nrp;
  }
  return sh;
}
namespace {

// the tree plan and super-group of a batched answer
pir::TreePlan batch_plan(const pir_engine* e, int log_parts_total, uint64_t prefix, int G, int* FB) {
  const auto& c = e->cfg;
  const pir::TreePlan pl = pir::make_plan(c.log_num_records, log_parts_total, prefix, e->batch_k_last, c.num_parties, 8);
  // super-group: as many keys as kBatchNodeBytes of upper-level nodes hold (a multiple of G)
  const uint64_t per_key = 2 * pl.max_nodes * (sizeof(uint4) + sizeof(uint32_t));
  int fb = (int)std::min<uint64_t>(kFrontBatch, std::max<uint64_t>(1, kBatchNodeBytes / per_key));
  *FB = std::max(G, fb / G * G);
  return pl;
}

// every buffer a batched answer of nk keys, G per pass, touches (narrow: a ragged last group
// may take a narrower scan with its own slab shape)
int ensure_batched(pir_engine* e, const pir::TreePlan& pl, int FB, int nk, int G, bool narrow) {
  size_t slab = 0;
  for (int gw = narrow ? 1 : G; gw <= G; gw *= 2) {
    bool km;
    const pir::ScanShape sh = group_scan_shape(e, pl.nleaves, gw, G, &km);
    slab = std::max(slab, (size_t)sh.grid.x * sh.grid.y * sh.slab_bytes);
  }
  int rc = e->d_slabs.reserve(slab);
  if (!rc) rc = e->d_cb.reserve(2 * (size_t)pl.nleaves * G * e->nrp);
  if (!rc) rc = ensure_batch(e, nk);
  if (!rc) rc = e->bnode_store.reserve(&e->bnodes, (uint64_t)std::min(nk, FB) * pl.max_nodes);
  if (!rc) rc = e->d_gtmp.reserve((size_t)16 * e->cfg.record_bytes);
  return rc;
}

// nk keys (raw, key_len apart) against one partition slice, one shard pass per group of G
// keys: each key's tree writes its shares into slot g of the interleaved coefficient rows
// cb[i][G*nrp]; one multi-round scan of G*nrp rounds answers the group (round g*nrp + a =
// key g, round a).  d_out: nk x nq x efs.
//   s  : per super-group of FB keys: frontier + all but the last tree stage of the FB keys
//        (one launch per stage, keys along grid y); then per group of G keys the last
//        (leaf) stage into share buffer j%2 (after scan j-2 has read it)
//   aux: scan + reduce of group j (after its leaf stage)
// so the leaf stage of group j+1 runs beside the scan of group j.  (Node-writing stages beside
// a scan are starved of the CU's memory pipeline, hence the up-front upper stages.)
// queue (answer_stream's shared queue, G keys per pass): the nk keys go into ceil(nk / G) groups
// of as equal sizes as possible (20 keys at G = 8: 7 + 7 + 6, not 8 + 8 + 4: every group keeps the
// full-width scan and its key-major packed leaf stores, and the leaf stages, which bound the
// pipeline, are spread evenly; $PIR_STREAM_NARROW=1 instead gives a group of ng < G keys the
// narrowest scan that holds it, the next power of two >= ng key slots -- measured slower,
// profiles/stream_share/README.md); the last group's reduce runs on s after the join, and a
// profiled queue stamps EV_SCAN_B before its first kernel and EV_SCAN_E after its last scan
// (both on s)
int answer_batch_core(pir_engine* e, const uint8_t* d_raw, int nk, int log_parts_total,
                      uint64_t prefix, uint64_t row0, uint8_t* d_out, hipStream_t s, int G,
                      bool queue) {
  const auto& c = e->cfg;
  e->last_batch_group = G;
  e->last_fused = 0;
  e->last_chunks = 1;
  int FB = G;
  const pir::TreePlan pl = batch_plan(e, log_parts_total, prefix, G, &FB);
  bool kmaj_full = false;
  const pir::ScanShape sh_full = group_scan_shape(e, pl.nleaves, G, G, &kmaj_full);
  const size_t cb_bytes = (size_t)pl.nleaves * G * e->nrp;
  if (int rc = ensure_batched(e, pl, FB, nk, G, queue && e->stream_narrow)) return rc;
  const size_t out_bytes = (size_t)c.num_rounds * c.record_bytes;
  const int last = pl.nstages - 1;
  // the fold image of the rows from row0, for the full-width k_scan_t passes (built here, on s,
  // ahead of the fork, where the rule says so: fold_image_for)
  const uint8_t* d_img = nullptr;
  if (int rc = fold_image_at(e, sh_full, row0, s, &d_img)) return rc;
  hipEvent_t* ev = queue ? e->ev : nullptr;
  if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_B], s));
  HIP_TRY(hipEventRecord(e->ev_fork, s));
  HIP_TRY(hipStreamWaitEvent(e->aux, e->ev_fork, 0));
  const int ngroups = (nk + G - 1) / G;
  for (int q0 = 0, j = 0, ng = 0, fb0 = 0, fb_end = 0; q0 < nk; q0 += ng, ++j) {
    ng = queue && !e->stream_narrow ? nk / ngroups + (j < nk % ngroups ? 1 : 0) : std::min(G, nk - q0);
    const int b = j & 1;
    if (q0 + ng > fb_end) {  // frontier + upper stages of the next FB keys
      const int nf = std::min(FB, nk - q0);
      fb0 = q0;
      fb_end = q0 + nf;
      const pir::KeySrc ks{d_raw + (size_t)q0 * e->key_len, c.num_parties, c.log_num_records,
                           c.num_rounds, c.party_index - 1, e->d_keys + q0};
      HIP_TRY(pir::launch_frontier(pl, ks, e->bnodes, s, nf, (size_t)e->key_len, pl.max_nodes));
      if (last > 0) {
        const pir::StageBatch up{nf, pl.max_nodes, 0, nullptr, nullptr, 0};
        HIP_TRY(pir::launch_stages(pl, e->d_keys + q0, e->bnodes, 0, 1, nullptr, e->nrp, s, 0,
                                   last, 0, &up));
      }
    }
    // the group's key slots and their scan
    const int r0 = q0 - fb0;
    int gw = G;
    if (queue && e->stream_narrow)
      for (gw = 1; gw < ng;) gw *= 2;
    bool kmaj = kmaj_full;
    const pir::ScanShape sh = gw == G ? sh_full : group_scan_shape(e, pl.nleaves, gw, G, &kmaj);
    const int W = gw * e->nrp;
    const bool tail_on_s = queue && q0 + ng >= nk;
    uint8_t* cb = e->d_cb + b * cb_bytes;
    if (j >= 2) HIP_TRY(hipStreamWaitEvent(s, e->ev_cb_free[b], 0));
    // the leaf stage of the ng trees of the group side by side: grid row y = key q0 + y
    const uint64_t off = (uint64_t)r0 * pl.max_nodes;
    const pir::NodeBufs nbg{{e->bnodes.s[0] + off, e->bnodes.s[1] + off},
                            {e->bnodes.t[0] + off, e->bnodes.t[1] + off}};
    const pir::StageBatch sb{ng, pl.max_nodes, kmaj ? (uint32_t)sh.ckoff : (uint32_t)e->nrp,
                             nullptr, nullptr, 0};
    HIP_TRY(pir::launch_stages(pl, e->d_keys + q0, nbg, 0, 1, cb, e->nrp, s, last, last + 1,
                               kmaj ? e->nrp : W, &sb));
    HIP_TRY(hipEventRecord(e->ev_cb_ready[b], s));
    HIP_TRY(hipStreamWaitEvent(e->aux, e->ev_cb_ready[b], 0));
    // slots g >= ng hold stale shares: their rounds are computed and dropped
    HIP_TRY(pir::launch_scan(sh, e->d_shard + row0 * e->pitch, pl.nleaves, cb, e->d_slabs, false,
                             e->aux, sh.tfold ? d_img : nullptr));
    HIP_TRY(hipEventRecord(e->ev_cb_free[b], e->aux));
    hipStream_t rs = e->aux;
    if (tail_on_s) {
      HIP_TRY(hipEventRecord(e->ev_join, e->aux));
      HIP_TRY(hipStreamWaitEvent(s, e->ev_join, 0));
      if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_E], s));
      rs = s;
    }
    uint8_t* dst = d_out + (size_t)q0 * out_bytes;
    if (e->nrp == c.num_rounds && ng == gw) {
      HIP_TRY(pir::launch_reduce(sh, e->d_slabs, c.record_bytes, dst, rs));
    } else {
      HIP_TRY(pir::launch_reduce(sh, e->d_slabs, c.record_bytes, e->d_gtmp, rs));
      HIP_TRY(hipMemcpy2DAsync(dst, out_bytes, e->d_gtmp, (size_t)e->nrp * c.record_bytes,
                               out_bytes, ng, hipMemcpyDeviceToDevice, rs));
    }
  }
  if (!queue) {
    HIP_TRY(hipEventRecord(e->ev_join, e->aux));
    HIP_TRY(hipStreamWaitEvent(s, e->ev_join, 0));
  }
  if (ev) HIP_TRY(hipEventRecord(ev[EV_RED], s));
  return PIR_OK;
}

int check_comm(const pir_engine* e) {
  return e->comm_failed ? fail(PIR_ECOMM, "the engine's communicator was aborted after a failed "
                                          "exchange (%s)", "re-create the engine")
                        : PIR_OK;
}

// the key of a host form, through the pinned h_key into d_key_raw on the engine's stream
int upload_key(pir_engine* e, const uint8_t* key) {
  memcpy(e->h_key, key, e->key_len);
  HIP_TRY(hipMemcpyAsync(e->d_key_raw, e->h_key, e->key_len, hipMemcpyHostToDevice, e->stream));
  return PIR_OK;
}

}  // namespace

int eng::check_key_ptr(const void* p) { return p ? PIR_OK : fail(PIR_EINVAL, "null key"); }

// before an answer on stream s: order it after the previous answer's use of the workspace.
// The engine's own stream records that answer's event only now, when another stream needs it
// (everything enqueued on it so far, the previous answer included): an event record between
// two launches on one stream delays the second by ~5.6 us of dispatch (the lone-query gap of
// profiles/r05/r5af_lone_gaps_depth4_depth16.txt; tools/micro/dispatch_gap.hip, mode 7).  A
// caller's stream records at finish(), while it is known to exist.
eng::AnswerScope::AnswerScope(pir_engine* e, void* stream) : lk_(e->mu), e_(e) {
  rc_ = [&]() -> int {
    HIP_TRY(hipSetDevice(e->cfg.device));
    s_ = stream ? (hipStream_t)stream : e->stream;
    if (int rc = check_comm(e)) return rc;
    if (e->ws_stream && e->ws_stream != s_) {
      if (e->ws_stream == e->stream) HIP_TRY(hipEventRecord(e->ev_ws, e->stream));
      HIP_TRY(hipStreamWaitEvent(s_, e->ev_ws, 0));
    }
    held_ = true;
    return PIR_OK;
  }();
}
// after it: the next answer, on whatever stream, waits for this one -- also when the answer
// failed part-way (rc != 0: work may already use the workspace on s; the record is best effort
// and the answer's own error code and message stand)
int eng::AnswerScope::finish(int rc) {
  if (!held_) return rc;
  held_ = false;
  const hipError_t r = s_ != e_->stream ? hipEventRecord(e_->ev_ws, s_) : hipSuccess;
  e_->ws_stream = s_;
  if (rc || r == hipSuccess) return rc;
  return fail(PIR_EHIP, "hipEventRecord(ev_ws) failed: %s", hipGetErrorString(r));
}
void eng::AnswerScope::synced() {
  held_ = false;
  e_->ws_stream = nullptr;
}

int eng::stage(DevBuf<>& buf, const void* src, size_t n, hipMemcpyKind kind, hipStream_t s) {
  if (int rc = buf.reserve(std::max<size_t>(n, 16))) return rc;
  if (n) HIP_TRY(hipMemcpyAsync(buf, src, n, kind, s));
  return PIR_OK;
}
int eng::stage2d(DevBuf<>& buf, size_t dst_pitch, const void* src, size_t src_pitch, size_t width,
                 size_t rows, hipMemcpyKind kind, hipStream_t s) {
  if (int rc = buf.reserve(std::max<size_t>(rows * dst_pitch, 16))) return rc;
  if (width) HIP_TRY(hipMemcpy2DAsync(buf, dst_pitch, src, src_pitch, width, rows, kind, s));
  return PIR_OK;
}
int eng::download(void* dst, const void* d_src, size_t n, hipStream_t s, uint8_t* via) {
  HIP_TRY(hipMemcpyAsync(via ? via : dst, d_src, n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (via) memcpy(dst, via, n);
  return PIR_OK;
}

namespace {

int answer_dev_locked(pir_engine* e, const uint8_t* d_key, uint8_t* d_result, hipStream_t s) {
  const auto& c = e->cfg;
  const size_t out_bytes = (size_t)c.num_rounds * c.record_bytes;
  e->ev = nullptr;
  pir_engine::ProfSlot* slot = nullptr;
  if (!e->prof.empty()) {
    slot = &e->prof[e->prof_next];
    e->ev = prof_slot(e, 0, 1, false);
  }
  hipEvent_t* ev = e->ev;
  if (ev) HIP_TRY(hipEventRecord(ev[EV_START], s));
  if (c.is_byzantine) {  // server.cpp:116-119: random answer bytes
    HIP_TRY(pir::launch_fill_random(d_result, out_bytes, 0xB42u + (++e->byz_counter), s));
    if (ev)
      for (int i = 1; i < kNumEv; ++i) HIP_TRY(hipEventRecord(ev[i], s));
    e->last_chunks = 1;
    e->ev = nullptr;
    return PIR_OK;
  }
  uint8_t* part_out = e->comm ? e->d_part.p : d_result;
  // the key is parsed inside the frontier kernel (k_key_prep only when the tree is very deep)
  int rc = answer_core(e, d_key, c.log_num_partitions, (uint64_t)c.partition_index, 0,
                       part_out, s);
  if (rc) return rc;
  if (slot) {  // the path answer_core took: which events the slot holds
    slot->fused = e->last_fused;
    slot->chunks = e->last_chunks;
  }
  if (e->comm) {
    if (int rc = exchange(e, e->d_part, out_bytes, e->d_gather, d_result, s)) return rc;
  }
  if (ev) HIP_TRY(hipEventRecord(ev[EV_END], s));
  e->ev = nullptr;
  return PIR_OK;
}

// a split shard's batch of `total` answer bytes: this partition's part and every rank's
int ensure_bparts(pir_engine* e, size_t total) {
  if (!e->comm) return PIR_OK;
  if (int rc = e->d_bpart.reserve(total)) return rc;
  return e->d_bgather.reserve(total * e->nranks);
}

int answer_batch_locked(pir_engine* e, const uint8_t* d_keys, int nk, uint8_t* d_result,
                        hipStream_t s) {
  const auto& c = e->cfg;
  const size_t out_bytes = (size_t)c.num_rounds * c.record_bytes;
  e->ev = nullptr;
  if (nk == 0) return PIR_OK;
  if (c.is_byzantine) {
    HIP_TRY(pir::launch_fill_random(d_result, out_bytes * nk, 0xB42u + (++e->byz_counter), s));
    return PIR_OK;
  }
  if (nk == 1 || batch_group(e) == 1) {  // one key per shard pass: the single-query path
    for (int q = 0; q < nk; ++q) {
      int rc = answer_dev_locked(e, d_keys + (size_t)q * e->key_len, d_result + q * out_bytes, s);
      if (rc) return rc;
    }
    return PIR_OK;
  }
  const size_t total = out_bytes * nk;
  if (int rc = ensure_bparts(e, total)) return rc;
  uint8_t* part_out = e->comm ? e->d_bpart.p : d_result;
  int rc = answer_batch_core(e, d_keys, nk, c.log_num_partitions, (uint64_t)c.partition_index, 0,
                             part_out, s, batch_group(e), false);
  if (rc) return rc;
  if (e->comm) {
    if (int rc = exchange(e, e->d_bpart, total, e->d_bgather, d_result, s)) return rc;
  }
  return PIR_OK;
}

// nk independent queries (each its own key and tree) handed over at once.  Where stream_group
// gives a group size, G queued keys share each pass over the shard (answer_batch_core's leaf
// stage -> share buffer -> one scan of G * nrp rounds; no answer is due before the queue's
// last reduce, so none comes later than with a pass each).  Otherwise every query has its own
// full shard pass: one k_query launch when the shape allows (the tree of query k+1 overlaps
// the scan of query k), else one answer after another.  d_result: nk x nq x efs.
int answer_stream_locked(pir_engine* e, const uint8_t* d_keys, int nk, uint8_t* d_result,
                         hipStream_t s) {
  const auto& c = e->cfg;
  const size_t out_bytes = (size_t)c.num_rounds * c.record_bytes;
  e->ev = nullptr;
  if (nk == 0) return PIR_OK;
  const pir::QueryPlan qp = pir::make_query_plan(c.log_num_records, c.log_num_partitions,
                                                 c.num_parties, c.num_rounds, e->pitch, e->num_cus,
                                                 nk);
  const int G = stream_group(e, nk);
  if (!G && (c.is_byzantine || !qp.tile || !e->allow_query || !e->allow_fused)) {
    for (int k = 0; k < nk; ++k) {
      int rc = answer_dev_locked(e, d_keys + (size_t)k * e->key_len, d_result + k * out_bytes, s);
      if (rc) return rc;
    }
    return PIR_OK;
  }
  const size_t total = out_bytes * nk;
  if (int rc = ensure_bparts(e, total)) return rc;
  uint8_t* part_out = e->comm ? e->d_bpart.p : d_result;
  if (!e->prof.empty()) {  // one event set for the whole queue (phases of the one launch)
    e->ev = prof_slot(e, G ? 0 : 2, 1, true);
    HIP_TRY(hipEventRecord(e->ev[EV_START], s));
  }
  int rc = G ? answer_batch_core(e, d_keys, nk, c.log_num_partitions,
                                 (uint64_t)c.partition_index, 0, part_out, s, G, true)
             : answer_query(e, qp, d_keys, nk, c.log_num_partitions,
                            (uint64_t)c.partition_index, 0, part_out, s);
  if (rc) return rc;
  if (e->comm) {
    if (int rc = exchange(e, e->d_bpart, total, e->d_bgather, d_result, s)) return rc;
  }
  if (e->ev) HIP_TRY(hipEventRecord(e->ev[EV_END], s));
  e->ev = nullptr;
  return PIR_OK;
}

// Every slice of one query: d_result[t] (t < 2^lt, num_rounds x record_bytes each) = the
// partial answer over this engine's rows [t*R/2^lt, (t+1)*R/2^lt) -- what the T calls
// runOptimizedDPFTreeQueryThread(t, T) of one query return (server.cpp:505-549, intended
// semantics; tree.go:60-76 issues them concurrently with the same key).  One k_query launch over
// the whole shard when its 2^lr regions split evenly into the slices (one tree, one pass, a
// slab reduce per run of regions); else one answer per slice.  Partials stay per engine: no
// all-gather (the Thread form has none either).
int answer_slices_locked(pir_engine* e, const uint8_t* d_key, int lt, uint8_t* d_result,
                         hipStream_t s) {
  const auto& c = e->cfg;
  const size_t out_bytes = (size_t)c.num_rounds * c.record_bytes;
  const int T = 1 << lt;
  e->ev = nullptr;
  const pir::QueryPlan qp = pir::make_query_plan(c.log_num_records, c.log_num_partitions,
                                                 c.num_parties, c.num_rounds, e->pitch, e->num_cus);
  if (qp.tile && lt <= qp.lr && e->allow_query && e->allow_fused)
    return answer_query(e, qp, d_key, 1, c.log_num_partitions, (uint64_t)c.partition_index, 0,
                        d_result, s, T);
  for (int t = 0; t < T; ++t) {
    const uint64_t prefix = ((uint64_t)c.partition_index << lt) | (uint64_t)t;
    const uint64_t row0 = (uint64_t)t * (e->rows >> lt);
    int rc = answer_core(e, d_key, c.log_num_partitions + lt, prefix, row0,
                         d_result + (size_t)t * out_bytes, s);
    if (rc) return rc;
  }
  return PIR_OK;
}

int check_slices(const pir_engine* e, int num_threads, int* lt) {
  *lt = ilog2_exact((uint64_t)(num_threads > 0 ? num_threads : 0));
  if (*lt < 0 || e->cfg.log_num_partitions + *lt > e->cfg.log_num_records)
    return fail(PIR_EINVAL, "num_threads %d must be a power of two <= 2^%d", num_threads,
                e->cfg.log_num_records - e->cfg.log_num_partitions);
  return PIR_OK;
}

}  // namespace

extern "C" {

const char* pir_engine_last_error(void) { return g_err.c_str(); }

int pir_engine_key_len(int p, int n, int nq) {  // utils.cpp:85-90
  return 16 + n * (p - 1) * (16 + 2 * p - 2) + nq * (p - 1);
}

int pir_engine_create(const pir_engine_config* cfg, pir_engine_t** out) {
  if (!cfg || !out) return fail(PIR_EINVAL, "null argument");
  const auto& c = *cfg;
  if (c.num_parties < 2 || c.num_parties > PIR_MAX_PARTIES)
    return fail(PIR_EINVAL, "num_parties %d outside [2,%d]", c.num_parties, PIR_MAX_PARTIES);
  if (c.party_index < 1 || c.party_index > c.num_parties)
    return fail(PIR_EINVAL, "party_index %d outside [1,%d]", c.party_index, c.num_parties);
  if (c.num_rounds < 1 || c.num_rounds > PIR_MAX_ROUNDS)
    return fail(PIR_EINVAL, "num_rounds %d outside [1,%d]", c.num_rounds, PIR_MAX_ROUNDS);
  if (c.log_num_records < 0 || c.log_num_records > PIR_MAX_LOG_RECORDS)
    return fail(PIR_EINVAL, "log_num_records %d", c.log_num_records);
  if (c.record_bytes < 1) return fail(PIR_EINVAL, "record_bytes must be >= 1");
  if (c.log_num_partitions < 0 || c.log_num_partitions > c.log_num_records ||
      c.partition_index < 0 || (uint64_t)c.partition_index >= (1ull << c.log_num_partitions))
    return fail(PIR_EINVAL, "bad partition %d of 2^%d", c.partition_index, c.log_num_partitions);
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (c.device < 0 || c.device >= ndev) return fail(PIR_EINVAL, "device %d of %d", c.device, ndev);
  HIP_TRY(hipSetDevice(c.device));

  auto* e = new pir_engine;
  e->cfg = c;
  e->nrp = c.num_rounds == 1 ? 1 : (c.num_rounds == 2 ? 2 : (c.num_rounds <= 4 ? 4 : (c.num_rounds <= 8 ? 8 : 16)));
  e->pitch = (c.record_bytes + 15u) & ~15u;
  e->rows = 1ull << (c.log_num_records - c.log_num_partitions);
  e->key_len = pir_engine_key_len(c.num_parties, c.log_num_records, c.num_rounds);
  auto cleanup = [&](int rc) { pir_engine_destroy(e); return rc; };
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, c.device) == hipSuccess) e->num_cus = prop.multiProcessorCount;
  if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&e->aux, hipStreamNonBlocking) != hipSuccess)
    return cleanup(fail(PIR_EHIP, "hipStreamCreate failed"));
  for (auto& ev : e->ev_leaf)
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess)
      return cleanup(fail(PIR_EHIP, "hipEventCreate failed"));
  if (hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&e->ev_ws, hipEventDisableTiming) != hipSuccess)
    return cleanup(fail(PIR_EHIP, "hipEventCreate failed"));
  for (int i = 0; i < 2; ++i)
    if (hipEventCreateWithFlags(&e->ev_cb_ready[i], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_cb_free[i], hipEventDisableTiming) != hipSuccess)
      return cleanup(fail(PIR_EHIP, "hipEventCreate failed"));
  const size_t shard_bytes = (size_t)e->rows * e->pitch;
  if (e->d_shard.reserve(shard_bytes))
    return cleanup(fail(PIR_ENOMEM, "hipMalloc shard %zu bytes", shard_bytes));
  if (hipMemsetAsync(e->d_shard, 0, shard_bytes, e->stream) != hipSuccess)
    return cleanup(fail(PIR_EHIP, "hipMemset shard"));
  pir::TreePlan pl = pir::make_plan(c.log_num_records, c.log_num_partitions, 0, -1, c.num_parties);
  {
    const char* f = getenv("PIR_FUSED");
    e->allow_fused = !(f && f[0] == '0');
    const char* qy = getenv("PIR_QUERY");
    e->allow_query = !(qy && qy[0] == '0');
    const char* fr = getenv("PIR_FUSED_REDUCE");
    if (fr) e->fused_reduce = std::max(0, std::min(3, atoi(fr)));
    // $PIR_QUERY_STEAL: 0 = off; else the kernel's StealArgs::mode (default 3)
    const char* st = getenv("PIR_QUERY_STEAL");
    if (st) e->steal = std::max(0, std::min(3, atoi(st)));
    const char* bg = getenv("PIR_BATCH_G");
    if (bg) e->batch_group = atoi(bg);
    const char* bb = getenv("PIR_BATCH_SCAN_BPC");
    if (bb) e->batch_scan_bpc = std::max(1, atoi(bb));
    // $PIR_STREAM_SHARE / $PIR_STREAM_G: queued keys per shard pass (stream_group)
    const char* ss = getenv("PIR_STREAM_SHARE");
    if (ss && ss[0]) e->stream_share = std::max(0, std::min(2, atoi(ss)));
    const char* sg = getenv("PIR_STREAM_G");
    if (sg) e->stream_group = std::max(0, std::min(16, atoi(sg)));
    const char* sn = getenv("PIR_STREAM_NARROW");
    e->stream_narrow = sn && atoi(sn) == 1;
    // $PIR_WD_SHARE / $PIR_WD_G: queued Woodruff keys per shard pass (woodruff_group)
    const char* ws = getenv("PIR_WD_SHARE");
    if (ws && ws[0]) e->wd_share = std::max(0, std::min(2, atoi(ws)));
    const char* wg = getenv("PIR_WD_G");
    if (wg && wg[0]) e->wd_group = atoi(wg) >= 8 ? 8 : (atoi(wg) >= 4 ? 4 : 2);
    // $PIR_GQ_SHARE / $PIR_GQ_G: queued explicit-coefficient and sqrt(N) DPF keys per shard pass
    // (group_queue_slots)
    const char* gs = getenv("PIR_GQ_SHARE");
    if (gs && gs[0]) e->gq_share = std::max(0, std::min(2, atoi(gs)));
    const char* gg = getenv("PIR_GQ_G");
    if (gg && gg[0]) e->gq_group = atoi(gg) >= 8 ? 8 : (atoi(gg) >= 4 ? 4 : 2);
    // $PIR_SH_SHARE / $PIR_SH_G: queued Shamir virtual keys per shard pass (shamir_group)
    const char* shs = getenv("PIR_SH_SHARE");
    if (shs && shs[0]) e->sh_share = std::max(0, std::min(2, atoi(shs)));
    const char* shg = getenv("PIR_SH_G");
    if (shg && shg[0]) e->sh_group = atoi(shg) >= 8 ? 8 : (atoi(shg) >= 4 ? 4 : 2);
    // $PIR_WDD_SHARE / $PIR_WDD_G: queued Woodruff derivative keys per shard pass
    // (woodruff_deriv_group)
    const char* wds = getenv("PIR_WDD_SHARE");
    if (wds && wds[0]) e->wdd_share = std::max(0, std::min(2, atoi(wds)));
    const char* wdg = getenv("PIR_WDD_G");
    if (wdg && wdg[0]) e->wdd_group = atoi(wdg) >= 8 ? 8 : (atoi(wdg) >= 4 ? 4 : 2);
    // $PIR_FOLD_IMAGE / $PIR_FOLD_IMAGE_MAX_BYTES: the fold image (include/pir_engine.h)
    const char* fi = getenv("PIR_FOLD_IMAGE");
    if (fi && fi[0]) e->fold_image = std::max(0, std::min(2, atoi(fi)));
    const char* fm = getenv("PIR_FOLD_IMAGE_MAX_BYTES");
    if (fm && fm[0]) e->fold_image_max = strtoull(fm, nullptr, 10);
    const char* bk = getenv("PIR_BATCH_KLAST");
    if (bk) e->batch_k_last = std::max(1, std::min(12, atoi(bk)));
    const int tile = pir::fused_tile(c.num_rounds, e->pitch, e->rows, e->num_cus);
    if (tile) {
      const pir::TreePlan pf =
          pir::make_plan(c.log_num_records, c.log_num_partitions, 0, pir::fused_k(tile), c.num_parties);
      if (pf.max_nodes > pl.max_nodes) pl = pf;
    }
  }
  const size_t out_bytes = (size_t)c.num_rounds * c.record_bytes;
  if (e->node_store.reserve(&e->nodes, pl.max_nodes) || e->d_c.reserve((size_t)e->rows * e->nrp) ||
      e->d_part.reserve(out_bytes) || e->d_result.reserve(out_bytes) ||
      e->h_key.reserve(e->key_len) || e->h_res.reserve(out_bytes))
    return cleanup(fail(PIR_ENOMEM, "workspace allocation failed"));
  int rc = ensure_batch(e, 1);
  if (rc) return cleanup(rc);
  if (hipStreamSynchronize(e->stream) != hipSuccess) return cleanup(fail(PIR_EHIP, "sync"));
  *out = e;
  return PIR_OK;
}

void pir_engine_destroy(pir_engine_t* e) {
  if (!e) return;
  (void)hipSetDevice(e->cfg.device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  if (e->aux) (void)hipStreamSynchronize(e->aux);
  if (e->comm) (void)ncclCommDestroy(e->comm);
  for (auto& b : e->user) (void)hipFree(b.p);
  for (auto& sl : e->prof)
    for (auto& ev : sl.ev) (void)hipEventDestroy(ev);
  delete e;  // the members free their buffers; then ~StreamSet destroys the events and streams
}

uint64_t pir_engine_num_rows(const pir_engine_t* e) { return e ? e->rows : 0; }

int pir_engine_answer_dev(pir_engine_t* e, const uint8_t* d_key, uint8_t* d_result,
                          void* stream) {
  if (!e || !d_result) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_key_ptr(d_key)) return rc;
  AnswerScope sc(e, stream);
  if (sc.rc()) return sc.rc();
  return sc.finish(answer_dev_locked(e, d_key, d_result, sc.stream()));
}

int pir_engine_answer_batch_dev(pir_engine_t* e, const uint8_t* d_keys, int num_keys,
                                uint8_t* d_result, void* stream) {
  if (!e || !d_result || num_keys < 0) return fail(PIR_EINVAL, "bad argument");
  if (int rc = check_key_ptr(d_keys)) return rc;
  AnswerScope sc(e, stream);
  if (sc.rc()) return sc.rc();
  return sc.finish(answer_batch_locked(e, d_keys, num_keys, d_result, sc.stream()));
}

// the keys and results of one call live in buffers of its own: nothing is held between calls
int pir_engine_answer_batch(pir_engine_t* e, const uint8_t* keys, int num_keys,
                            uint8_t* results) {
  if (!e || (num_keys > 0 && (!keys || !results)) || num_keys < 0)
    return fail(PIR_EINVAL, "bad argument");
  if (num_keys == 0) return PIR_OK;
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  const size_t rb = (size_t)num_keys * e->cfg.num_rounds * e->cfg.record_bytes;
  DevBuf<> d_k, d_r;  // freed on every way out (hipFree waits for the device)
  if (d_r.reserve(rb)) return fail(PIR_ENOMEM, "batch result buffer %zu bytes", rb);
  if (int rc = stage(d_k, keys, (size_t)num_keys * e->key_len, hipMemcpyHostToDevice, e->stream))
    return rc;
  if (int rc = sc.finish(answer_batch_locked(e, d_k, num_keys, d_r, e->stream))) return rc;
  return download(results, d_r, rb, e->stream);
}

int pir_engine_answer_stream_dev(pir_engine_t* e, const uint8_t* d_keys, int num_keys,
                                 uint8_t* d_result, void* stream) {
  if (!e || !d_result || num_keys < 0) return fail(PIR_EINVAL, "bad argument");
  if (int rc = check_key_ptr(d_keys)) return rc;
  AnswerScope sc(e, stream);
  if (sc.rc()) return sc.rc();
  return sc.finish(answer_stream_locked(e, d_keys, num_keys, d_result, sc.stream()));
}

int pir_engine_reserve_queue(pir_engine_t* e, int num_keys) {
  if (!e || num_keys < 1) return fail(PIR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  const auto& c = e->cfg;
  const pir::QueryPlan qp = pir::make_query_plan(c.log_num_records, c.log_num_partitions,
                                                 c.num_parties, c.num_rounds, e->pitch, e->num_cus,
                                                 num_keys);
  const size_t total = (size_t)num_keys * c.num_rounds * c.record_bytes;
  int rc = PIR_OK;
  if (const int G = stream_group(e, num_keys)) {  // a shared queue: the batched path's buffers
    int FB = G;
    const pir::TreePlan pl = batch_plan(e, c.log_num_partitions, (uint64_t)c.partition_index, G, &FB);
    rc = ensure_batched(e, pl, FB, num_keys, G, e->stream_narrow);
    if (!rc) rc = ensure_bparts(e, total);
    // the fold image, where the queue's passes are k_scan_t's
    bool km = false;
    if (!rc) rc = fold_image_reserve(e, group_scan_shape(e, pl.nleaves, G, G, &km));
    if (rc) return rc;
  }
  if (!qp.tile) return PIR_OK;  // shapes k_query does not take allocate per answer
  // k_query's own (a queue of one, or a shorter queue the policy leaves to it): the slabs
  // only ever grow
  rc = e->d_slabs.reserve((size_t)num_keys * pir::query_slab_bytes(qp));
  if (!rc) rc = e->d_qscratch.reserve(pir::query_scratch_bytes(qp));
  if (!rc && e->fused_reduce) rc = ensure_qcnt(e, num_keys * 8, e->stream);
  if (!rc && num_keys == 1) {  // the stealing buffer (this advances the generation once: harmless)
    pir::StealArgs st;
    rc = steal_args(e, qp, 1, 1, e->stream, &st);
    // its zeroing ran on the engine stream: done before an answer on any other stream reads it
    if (!rc) HIP_TRY(hipStreamSynchronize(e->stream));
  }
  if (!rc) rc = ensure_bparts(e, total);
  return rc;
}

int pir_engine_set_batch_group(pir_engine_t* e, int keys_per_pass) {
  if (!e || keys_per_pass < 0 || keys_per_pass > 16) return fail(PIR_EINVAL, "bad argument");
  e->batch_group = keys_per_pass;
  return PIR_OK;
}

int pir_engine_batch_group(const pir_engine_t* e) { return e ? batch_group(e) : 0; }

int pir_engine_answer(pir_engine_t* e, const uint8_t* key, uint8_t* result) {
  if (!e || !result) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_key_ptr(key)) return rc;
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  if (int rc = upload_key(e, key)) return rc;
  if (int rc = sc.finish(answer_dev_locked(e, e->d_key_raw, e->d_result, e->stream))) return rc;
  return download(result, e->d_result, (size_t)e->cfg.num_rounds * e->cfg.record_bytes, e->stream,
                  e->h_res);
}

int pir_engine_answer_slice(pir_engine_t* e, const uint8_t* key, int thread_num, int num_threads,
                            uint8_t* result) {
  if (!e || !result) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_key_ptr(key)) return rc;
  const int lt = ilog2_exact((uint64_t)num_threads);
  const auto& c = e->cfg;
  if (lt < 0 || c.log_num_partitions + lt > c.log_num_records)
    return fail(PIR_EINVAL, "num_threads %d must be a power of two <= 2^%d", num_threads,
                c.log_num_records - c.log_num_partitions);
  if (thread_num < 0 || thread_num >= num_threads)
    return fail(PIR_EINVAL, "thread_num %d of %d", thread_num, num_threads);
  // NB: the reference's Thread variant computes the honest answer even when isByzantine is
  // set (both branches of server.cpp:526-541 are identical); mirrored here.
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  if (int rc = upload_key(e, key)) return rc;
  const uint64_t prefix = ((uint64_t)c.partition_index << lt) | (uint64_t)thread_num;
  const uint64_t row0 = (uint64_t)thread_num * (e->rows >> lt);
  if (int rc = sc.finish(answer_core(e, e->d_key_raw, c.log_num_partitions + lt, prefix, row0,
                                     e->d_result, e->stream)))
    return rc;
  return download(result, e->d_result, (size_t)c.num_rounds * c.record_bytes, e->stream, e->h_res);
}

int pir_engine_answer_slices_dev(pir_engine_t* e, const uint8_t* d_key, int num_threads,
                                 uint8_t* d_results, void* stream) {
  if (!e || !d_results) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_key_ptr(d_key)) return rc;
  int lt = 0;
  if (int rc = check_slices(e, num_threads, &lt)) return rc;
  AnswerScope sc(e, stream);
  if (sc.rc()) return sc.rc();
  return sc.finish(answer_slices_locked(e, d_key, lt, d_results, sc.stream()));
}

int pir_engine_answer_slices(pir_engine_t* e, const uint8_t* key, int num_threads,
                             uint8_t* results) {
  if (!e || !results) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_key_ptr(key)) return rc;
  int lt = 0;
  if (int rc = check_slices(e, num_threads, &lt)) return rc;
  const size_t bytes = (size_t)num_threads * e->cfg.num_rounds * e->cfg.record_bytes;
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  if (int rc = e->d_slices.reserve(bytes)) return rc;
  if (int rc = e->h_slices.reserve(bytes)) return rc;
  if (int rc = upload_key(e, key)) return rc;
  if (int rc = sc.finish(answer_slices_locked(e, e->d_key_raw, lt, e->d_slices, e->stream)))
    return rc;
  return download(results, e->d_slices, bytes, e->stream, e->h_slices);
}

int pir_engine_eval_all(pir_engine_t* e, const uint8_t* key, uint8_t* out) {
  if (!e || !out) return fail(PIR_EINVAL, "null argument");
  if (int rc = check_key_ptr(key)) return rc;
  AnswerScope sc(e);
  if (sc.rc()) return sc.rc();
  const auto& c = e->cfg;
  if (int rc = upload_key(e, key)) return rc;
  const pir::TreePlan pl =
      pir::make_plan(c.log_num_records, c.log_num_partitions, (uint64_t)c.partition_index, -1, c.num_parties);
  HIP_TRY(pir::launch_frontier(pl, key_src(e, e->d_key_raw), e->nodes, e->stream));
  HIP_TRY(pir::launch_stages(pl, e->d_keys, e->nodes, 0, 1, e->d_c, e->nrp, e->stream));
  std::vector<uint8_t> ct((size_t)e->rows * e->nrp);
  if (int rc = download(ct.data(), e->d_c, ct.size(), e->stream)) return rc;
  sc.synced();
  for (uint64_t i = 0; i < e->rows; ++i)
    for (int a = 0; a < c.num_rounds; ++a) out[(size_t)a * e->rows + i] = ct[i * e->nrp + a];
  return PIR_OK;
}

void* pir_engine_stream(pir_engine_t* e) { return e ? (void*)e->stream : nullptr; }

int pir_engine_sync(pir_engine_t* e) {
  if (!e) return fail(PIR_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return PIR_OK;
}

int pir_engine_alloc_dev(pir_engine_t* e, size_t bytes, void** d_ptr) {
  if (!e || !d_ptr) return fail(PIR_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, bytes ? bytes : 1));
  e->user.push_back({p, bytes});
  *d_ptr = p;
  return PIR_OK;
}

int pir_engine_free_dev(pir_engine_t* e, void* d_ptr) {
  if (!e) return fail(PIR_EINVAL, "null engine");
  if (!d_ptr) return PIR_OK;
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  for (size_t i = 0; i < e->user.size(); ++i)
    if (e->user[i].p == d_ptr) {
      // answers still queued on any stream may read it: hipFree waits for the device
      HIP_TRY(hipFree(d_ptr));
      e->user.erase(e->user.begin() + (long)i);
      return PIR_OK;
    }
  return fail(PIR_EINVAL, "%p was not allocated by pir_engine_alloc_dev", d_ptr);
}

int pir_engine_set_party_index(pir_engine_t* e, int party_index) {
  if (!e) return fail(PIR_EINVAL, "null engine");
  if (party_index < 1 || party_index > e->cfg.num_parties)
    return fail(PIR_EINVAL, "party_index %d outside [1,%d]", party_index, e->cfg.num_parties);
  std::lock_guard<std::mutex> lk(e->mu);
  e->cfg.party_index = party_index;  // read at enqueue time (a kernel argument), not by kernels
  return PIR_OK;                     // already queued
}

int pir_engine_fill_random_dev(pir_engine_t* e, void* d_dst, size_t bytes, uint64_t seed) {
  if (!e || (!d_dst && bytes)) return fail(PIR_EINVAL, "null argument");
  if (!bytes) return PIR_OK;
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(pir::launch_fill_random(static_cast<uint8_t*>(d_dst), bytes, seed, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return PIR_OK;
}

int pir_engine_memcpy_h2d(pir_engine_t* e, void* d_dst, const void* h_src, size_t bytes) {
  if (!e) return fail(PIR_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return PIR_OK;
}

int pir_engine_memcpy_d2h(pir_engine_t* e, void* h_dst, const void* d_src, size_t bytes) {
  if (!e) return fail(PIR_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return PIR_OK;
}

}  // extern "C"
