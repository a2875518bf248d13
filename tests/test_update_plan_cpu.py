"""The host side of a live update (csrc/pir_update_plan.h) on the CPU: the terms a batch of
changed records contributes to the shard's rows -- rows form, across-encoded files, within-encoded
files with and without Hermite rows, whole engines and partitions -- and their grouping by 4-row
block.  A small stand-alone program built with the host compiler against the header prints the
sorted term table and the block ranges of the batch on its command line; both are checked against
a Python restatement.  The same program, built once more with the address and undefined-behaviour
sanitizers, must print the same and report nothing."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "erasurecodedpir_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "pir_update_plan.h"
// argv: form (rows | across | within) row0 rows num_files k party file_bytes efs hermite_row0
//       index...; prints "T row delta off coef" per sorted term, then "B blk t0 t1" per block
int main(int argc, char** argv) {
  if (argc < 10) return 2;
  const char* form = argv[1];
  auto u = [&](int i) { return strtoull(argv[i], nullptr, 10); };
  const uint64_t row0 = u(2), rows = u(3), num_files = u(4);
  const int k = (int)u(5), party = (int)u(6);
  const uint32_t file_bytes = (uint32_t)u(7), efs = (uint32_t)u(8);
  const uint64_t hermite_row0 = u(9);
  std::vector<uint64_t> index;
  for (int i = 10; i < argc; ++i) index.push_back(u(i));
  std::vector<pir::UpdateTerm> terms;
  if (!strcmp(form, "rows"))
    pir::update_terms_rows(index.data(), (int)index.size(), terms);
  else if (!strcmp(form, "across"))
    pir::update_terms_across(index.data(), (int)index.size(), num_files, k, party, row0, rows, terms);
  else if (!strcmp(form, "within"))
    pir::update_terms_within(index.data(), (int)index.size(), file_bytes, efs, k, party, row0, rows,
                             hermite_row0, terms);
  else
    return 2;
  std::vector<pir::UpdateBlock> blocks;
  pir::update_plan(terms, blocks);
  for (const auto& t : terms)
    printf("T %llu %u %u %u\n", (unsigned long long)t.row, t.delta, t.off, t.coef);
  for (const auto& b : blocks) printf("B %llu %u %u\n", (unsigned long long)b.blk, b.t0, b.t1);
  return 0;
}
"""


def _build(d, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src, exe = d / "plan.cpp", d / name
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + extra +
                          ["-o", str(exe), str(src)])

    def run(form, index, row0=0, rows=1 << 40, num_files=0, k=1, party=1, file_bytes=0, efs=0,
            hermite_row0=0):
        args = [form] + [str(int(v)) for v in (row0, rows, num_files, k, party, file_bytes, efs,
                                               hermite_row0)] + [str(int(i)) for i in index]
        r = subprocess.run([str(exe)] + args, capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr)
        terms = [tuple(int(w) for w in ln.split()[1:]) for ln in r.stdout.splitlines()
                 if ln.startswith("T ")]
        blocks = [tuple(int(w) for w in ln.split()[1:]) for ln in r.stdout.splitlines()
                  if ln.startswith("B ")]
        return terms, blocks

    return run


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("update_plan_" + request.param)
    extra = [] if request.param == "plain" else \
        ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    return _build(d, "plan_" + request.param, extra)


# ------------------------------------------------------------------------- the restatement
def _terms(form, index, row0, rows, num_files, k, party, file_bytes, efs, hermite_row0):
    """(row, delta, off, coef) in the order the batch gives them, rows of this engine only"""
    out = []

    def push(g, i, off, coef):
        if row0 <= g < row0 + rows:
            out.append((g - row0, i, off, coef))

    for i, f in enumerate(index):
        if form == "rows":
            out.append((f, i, 0, 1))
        elif form == "across":
            encdb = (num_files + k - 1) // k
            push(f % encdb, i, 0, O.gf_pow(party, f // encdb))
        else:
            live = [j for j in range(k) if j * efs < file_bytes]
            for j in live:
                push(f, i, j * efs, O.gf_pow(party, j))
            if hermite_row0:
                for j in live:
                    if j % 2:
                        push(hermite_row0 + f, i, j * efs, O.gf_pow(party, j - 1))
    return out


def _plan(terms):
    """stable by block; [blk, t0, t1) ranges"""
    order = sorted(range(len(terms)), key=lambda t: terms[t][0] // 4)
    st = [terms[t] for t in order]
    blocks = []
    for t, term in enumerate(st):
        if not blocks or blocks[-1][0] != term[0] // 4:
            blocks.append([term[0] // 4, t, t])
        blocks[-1][2] = t + 1
    return st, [tuple(b) for b in blocks]


def _check(plan, form, index, **kw):
    args = dict(row0=0, rows=1 << 40, num_files=0, k=1, party=1, file_bytes=0, efs=0,
                hermite_row0=0)
    args.update(kw)
    got_t, got_b = plan(form, index, **args)
    want_t, want_b = _plan(_terms(form, index, **args))
    assert got_t == want_t
    assert got_b == want_b
    # the ranges tile the table, each within one block, blocks ascending
    t = 0
    for blk, t0, t1 in got_b:
        assert t0 == t and t1 > t0
        assert all(got_t[i][0] // 4 == blk for i in range(t0, t1))
        t = t1
    assert t == len(got_t)
    assert [b[0] for b in got_b] == sorted({b[0] for b in got_b})
    return got_t, got_b


# ---------------------------------------------------------------------------------- the tests
def test_rows_duplicates_and_quadruples(plan):
    # a quadruple in block 3, a row twice, row 0, a far row, out of order
    _check(plan, "rows", [13, 12, 1 << 33, 15, 0, 14, 13, 7, (1 << 33) + 3, 13])


def test_empty(plan):
    assert plan("rows", []) == ([], [])


def test_across_same_row_pairs(plan):
    num_files, k, party = 3 * 2048 - 5, 3, 2
    encdb = (num_files + k - 1) // k
    batch = [5, 5 + encdb, 5 + 2 * encdb,      # one row, three coefficients
             40, 41, 42, 43,                  # one block
             77, 77,                          # one file twice
             0, num_files - 1, encdb - 1, 6]  # first, last, last row
    got_t, got_b = _check(plan, "across", batch, num_files=num_files, k=k, party=party,
                          rows=2048)
    assert [t[3] for t in got_t if t[0] == 5] == [1, 2, 4]      # gf_pow(2, j), in batch order
    assert sum(1 for t in got_t if t[0] == 77) == 2
    assert any(b == (10, b[1], b[1] + 4) for b in got_b)


def test_across_partitions_split_the_batch(plan):
    num_files, k, party, rows = 2 * 4096 - 5, 2, 3, 2048
    encdb = (num_files + k - 1) // k
    rng = np.random.default_rng(3)
    batch = [int(v) for v in rng.integers(0, num_files, 200)] + [0, num_files - 1, 2047, 2048,
                                                                 2047 + encdb, 2048 + encdb]
    whole, _ = _check(plan, "across", batch, num_files=num_files, k=k, party=party, rows=4096)
    parts = []
    for part in range(2):
        t, _ = _check(plan, "across", batch, num_files=num_files, k=k, party=party,
                      row0=part * rows, rows=rows)
        assert all(term[0] < rows for term in t)
        parts += [(term[0] + part * rows,) + term[1:] for term in t]
    assert sorted(parts) == sorted(whole)
    assert len(whole) == len(batch)


def test_within_parts_and_hermite(plan):
    efs, k, party = 256, 3, 5
    for file_bytes in (3 * efs, 2 * efs + 7, efs, 1, 0):
        for hermite_row0 in (0, 1024):
            batch = [8, 9, 700, 8, 0, 1023]
            t, _ = _check(plan, "within", batch, num_files=1024, k=k, party=party,
                          file_bytes=file_bytes, efs=efs, hermite_row0=hermite_row0,
                          rows=2048 if hermite_row0 else 1024)
            parts = -(-file_bytes // efs)
            want = len(batch) * (parts + (parts // 2 if hermite_row0 else 0))
            assert len(t) == want, (file_bytes, hermite_row0)
            assert all(term[2] % efs == 0 and term[2] < max(file_bytes, 1) for term in t)


def test_within_out_of_partition(plan):
    t, b = _check(plan, "within", [5, 600, 511, 512], num_files=1024, k=2, party=1,
                  file_bytes=100, efs=64, row0=512, rows=512)
    assert sorted({term[0] for term in t}) == [0, 88]
    assert [blk for blk, _, _ in b] == [0, 22]
