"""transpose4x32 (csrc/pir_bits.h), the 4-row bit transpose behind k_scan_t's nibble indices, on
the CPU: a small stand-alone program built with the host compiler against the header applies it
to the words given on its command line, and the result is checked against the definition bit by
bit -- nibble i of word k holds bit 4 i + k of the four rows, row r in bit r -- for random
inputs and for every single-bit input."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "erasurecodedpir_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "pir_bits.h"
// argv: groups of four rows (hex words); prints each group transposed, four hex words a line
int main(int argc, char** argv) {
  for (int i = 1; i + 3 < argc; i += 4) {
    uint32_t x[4];
    for (int k = 0; k < 4; ++k) x[k] = (uint32_t)strtoul(argv[i + k], nullptr, 16);
    pir::transpose4x32(x);
    printf("%08x %08x %08x %08x\n", x[0], x[1], x[2], x[3]);
  }
  return 0;
}
"""


def _by_definition(rows):
    out = [0, 0, 0, 0]
    for k in range(4):
        for i in range(8):
            for r in range(4):
                out[k] |= ((rows[r] >> (4 * i + k)) & 1) << (4 * i + r)
    return out


@pytest.fixture(scope="module")
def transpose(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("bits_nibble")
    src, exe = d / "t4.cpp", d / "t4"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", str(exe), str(src)])

    def run(groups):
        args = ["%08x" % w for g in groups for w in g]
        lines = subprocess.check_output([str(exe)] + args, text=True).split("\n")
        return [[int(w, 16) for w in ln.split()] for ln in lines if ln]

    return run


def test_random_inputs(transpose):
    rng = np.random.default_rng(4)
    groups = [[int(w) for w in rng.integers(0, 1 << 32, 4, dtype=np.uint64)] for _ in range(200)]
    groups += [[0, 0, 0, 0], [0xFFFFFFFF] * 4]
    got = transpose(groups)
    assert len(got) == len(groups)
    for g, t in zip(groups, got):
        assert t == _by_definition(g), ["%08x" % w for w in g]


def test_single_bits(transpose):
    """Row r, bit 4 i + k alone -> bit 4 i + r of word k alone."""
    groups, want = [], []
    for r in range(4):
        for bit in range(32):
            g = [0, 0, 0, 0]
            g[r] = 1 << bit
            groups.append(g)
            w = [0, 0, 0, 0]
            w[bit % 4] = 1 << (4 * (bit // 4) + r)
            want.append(w)
    assert transpose(groups) == want
