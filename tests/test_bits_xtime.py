"""gf_xtime4 (csrc/pir_bits.h), the packed "times alpha" every bit-plane fold ends with, on the
CPU: a small stand-alone program built with the host compiler against the header applies it to
the words given on its command line, and the result is checked against the bytewise product with
alpha modulo 0x11d -- for each of the four byte positions and all 256 byte values, the other
three bytes random: the byte's product is right and its neighbours' are what they would be
without it (no bit crosses a byte)."""
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
// argv: hex words; prints gf_xtime4 of each, one hex word a line
int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i)
    printf("%08x\n", pir::gf_xtime4((uint32_t)strtoul(argv[i], nullptr, 16)));
  return 0;
}
"""


def _xtime(b):
    """b * alpha in GF(2^8) modulo x^8 + x^4 + x^3 + x^2 + 1 (0x11d), by the definition."""
    b <<= 1
    return b ^ 0x11D if b & 0x100 else b


@pytest.fixture(scope="module")
def xtime4(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("bits_xtime")
    src, exe = d / "x4.cpp", d / "x4"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", str(exe), str(src)])

    def run(words):
        out = subprocess.check_output([str(exe)] + ["%08x" % w for w in words], text=True)
        return [int(ln, 16) for ln in out.split()]

    return run


@pytest.mark.parametrize("pos", range(4))
def test_every_byte_value(xtime4, pos):
    """Byte `pos` takes all 256 values beside three random bytes."""
    rng = np.random.default_rng(40 + pos)
    others = [int(w) & ~(0xFF << (8 * pos)) for w in rng.integers(0, 1 << 32, 256, dtype=np.uint64)]
    words = [o | (v << (8 * pos)) for v, o in enumerate(others)]
    got = xtime4(words + others)
    assert len(got) == 512
    for v, (w, g, g0) in enumerate(zip(words, got[:256], got[256:])):
        want = sum(_xtime((w >> (8 * k)) & 0xFF) << (8 * k) for k in range(4))
        assert g == want, "%08x" % w
        # the neighbours' bytes do not depend on this byte: the same as with it zero
        assert (g ^ g0) == _xtime(v) << (8 * pos), "%08x" % w
