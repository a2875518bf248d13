// pir_update_plan.h -- the host side of a live update (k_update_rows, pir_update.hip): the terms
// a batch of changed files contributes to the shard's rows, and their grouping by 4-row block.
// Plain C++ with no HIP types (tests/test_update_plan_cpu.py builds it with the host compiler).
//
// Every encoding of the shard is linear over GF(2^8), so a file that changes by delta = old ^ new
// changes a coded row by coefficient * (a slice of delta): one term.  k_update_rows gives each
// block of 4 rows (the unit of the fold image, pir_bits.h) to one workgroup per column group,
// which applies all of the block's terms; so the terms are sorted by block here, and the terms
// of one block keep the order they were made in.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace pir {

// row `row` of the engine ^= coef * (bytes [off, off + record_bytes) of delta number `delta`; the
// bytes at or past the launch's limit count as zero)
struct UpdateTerm {
  uint64_t row;
  uint32_t delta;
  uint32_t off;
  uint32_t coef;
  uint32_t pad_;
};
// the terms [t0, t1) of the sorted table all lie in rows [4 blk, 4 blk + 4)
struct UpdateBlock {
  uint64_t blk;
  uint32_t t0, t1;
};
static_assert(sizeof(UpdateTerm) == 24 && sizeof(UpdateBlock) == 16, "device layout");

// gf_pow(party, j) over GF(2^8), poly 0x11d, as the encoders have it (coding.cpp:46-60;
// pow(0, e) == 1 there)
inline uint8_t update_gf_pow(int party, int j) {
  uint32_t r = 1;
  for (int t = 0; t < j && party; ++t) {
    uint32_t a = r, b = (uint32_t)party & 0xffu, m = 0;
    while (b) {
      if (b & 1) m ^= a;
      a = ((a << 1) ^ ((a & 0x80) ? 0x11d : 0)) & 0xff;
      b >>= 1;
    }
    r = m;
  }
  return (uint8_t)r;
}

// The engine holds the global rows [row0, row0 + rows) as its rows [0, rows): a term of global
// row g is kept (as row g - row0) only inside, so that every partition engine can be given the
// same global batch
inline void update_push(std::vector<UpdateTerm>& out, uint64_t g, uint64_t row0, uint64_t rows,
                        uint32_t delta, uint32_t off, uint32_t coef) {
  if (g < row0 || g - row0 >= rows) return;
  out.push_back(UpdateTerm{g - row0, delta, off, coef, 0});
}

// rows form: engine row rows[i] ^= delta i
inline void update_terms_rows(const uint64_t* rows, int num, std::vector<UpdateTerm>& out) {
  for (int i = 0; i < num; ++i) out.push_back(UpdateTerm{rows[i], (uint32_t)i, 0, 1, 0});
}

// across-encoded files (k_encode_across): file f = encdb j + r -> global row r, gf_pow(party, j)
inline void update_terms_across(const uint64_t* files, int num, uint64_t num_files, int k,
                                int party, uint64_t row0, uint64_t rows,
                                std::vector<UpdateTerm>& out) {
  const uint64_t encdb = (num_files + (uint64_t)k - 1) / (uint64_t)k;
  for (int i = 0; i < num; ++i) {
    const uint64_t j = files[i] / encdb, r = files[i] - j * encdb;
    update_push(out, r, row0, rows, (uint32_t)i, 0, update_gf_pow(party, (int)j));
  }
}

// within-encoded files (k_encode_within): file r -> global row r, part j (bytes [j efs,
// (j + 1) efs) of the file, those past file_bytes absent) times gf_pow(party, j); hermite_row0
// != 0: also the Hermite row hermite_row0 + r (launch_encode_hermite), the odd parts j times
// gf_pow(party, j - 1).  The terms of one file are adjacent, value row first
inline void update_terms_within(const uint64_t* files, int num, uint32_t file_bytes, uint32_t efs,
                                int k, int party, uint64_t row0, uint64_t rows,
                                uint64_t hermite_row0, std::vector<UpdateTerm>& out) {
  for (int i = 0; i < num; ++i) {
    for (int j = 0; j < k && (uint64_t)j * efs < file_bytes; ++j)
      update_push(out, files[i], row0, rows, (uint32_t)i, (uint32_t)j * efs,
                  update_gf_pow(party, j));
    if (!hermite_row0) continue;
    for (int j = 1; j < k && (uint64_t)j * efs < file_bytes; j += 2)
      update_push(out, hermite_row0 + files[i], row0, rows, (uint32_t)i, (uint32_t)j * efs,
                  update_gf_pow(party, j - 1));
  }
}

// sort the terms by block (stable: a block's terms stay in their order) and list the blocks
inline void update_plan(std::vector<UpdateTerm>& terms, std::vector<UpdateBlock>& blocks) {
  std::stable_sort(terms.begin(), terms.end(),
                   [](const UpdateTerm& a, const UpdateTerm& b) { return a.row / 4 < b.row / 4; });
  blocks.clear();
  for (size_t t = 0; t < terms.size(); ++t) {
    const uint64_t blk = terms[t].row / 4;
    if (blocks.empty() || blocks.back().blk != blk)
      blocks.push_back(UpdateBlock{blk, (uint32_t)t, (uint32_t)t});
    blocks.back().t1 = (uint32_t)t + 1;
  }
}

}  // namespace pir
