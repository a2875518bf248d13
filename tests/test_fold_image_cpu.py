"""The fold image's bit order (csrc/pir_bits.h: fold_image4, fold_image4_rows, fold_image_nibble)
on the CPU: a small stand-alone program built with the host compiler against the header turns
the 4 x 32-bit rows given on its command line into image words.  Checked here, against the
layout stated independently in Python: for every bit position j = 4 i + k the nibble whose bit r
is row r's bit j sits in image word k at the bits (4 i + 3 + r) mod 32; fold_image_nibble reads
that nibble; and the way back (fold_image4_rows) returns the rows."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "erasurecodedpir_amd", "csrc")

ROT = 3  # kFoldImageRot

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "pir_bits.h"
// argv: hex words, four rows a group; per group one line: kFoldImageRot, the 4 image words, the
// 4 words fold_image4_rows makes of them, the 32 nibbles fold_image_nibble reads
int main(int argc, char** argv) {
  for (int i = 1; i + 3 < argc; i += 4) {
    uint32_t x[4];
    for (int r = 0; r < 4; ++r) x[r] = (uint32_t)strtoul(argv[i + r], nullptr, 16);
    pir::fold_image4(x);
    printf("%d", pir::kFoldImageRot);
    for (int k = 0; k < 4; ++k) printf(" %08x", x[k]);
    uint32_t y[4] = {x[0], x[1], x[2], x[3]};
    pir::fold_image4_rows(y);
    for (int k = 0; k < 4; ++k) printf(" %08x", y[k]);
    for (int j = 0; j < 32; ++j) printf(" %x", pir::fold_image_nibble(x, j));
    printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def image4(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("fold_image")
    src, exe = d / "fi.cpp", d / "fi"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", str(exe), str(src)])

    def run(groups):
        args = ["%08x" % w for g in groups for w in g]
        out = subprocess.check_output([str(exe)] + args, text=True)
        res = []
        for ln in out.splitlines():
            f = ln.split()
            assert len(f) == 1 + 4 + 4 + 32
            res.append((int(f[0]), [int(v, 16) for v in f[1:5]], [int(v, 16) for v in f[5:9]],
                        [int(v, 16) for v in f[9:]]))
        return res

    return run


def _groups():
    rng = np.random.default_rng(4)
    groups = [[int(w) for w in g] for g in rng.integers(0, 1 << 32, (200, 4), dtype=np.uint64)]
    # single rows, single bits, the bits at the rotation's wrap, all ones
    groups += [[0xFFFFFFFF if r == q else 0 for r in range(4)] for q in range(4)]
    groups += [[1 << j if r == (j & 3) else 0 for r in range(4)] for j in range(32)]
    groups += [[0xE0000007] * 4, [0xFFFFFFFF] * 4, [0] * 4]
    return groups


def _nibble(rows, j):
    return sum(((rows[r] >> j) & 1) << r for r in range(4))


def test_layout_and_way_back(image4):
    groups = _groups()
    got = image4(groups)
    assert len(got) == len(groups)
    for rows, (rot, words, back, nibbles) in zip(groups, got):
        assert rot == ROT
        want = [0, 0, 0, 0]
        for j in range(32):
            i, k = j >> 2, j & 3
            for r in range(4):
                want[k] |= ((rows[r] >> j) & 1) << ((4 * i + ROT + r) % 32)
        assert words == want, rows
        assert nibbles == [_nibble(rows, j) for j in range(32)], rows
        assert back == rows, rows
