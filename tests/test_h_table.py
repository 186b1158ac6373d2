"""The helix kernel's table of face values (csrc/h_table.h, read by scalar
loads: TSA_H_TAB in csrc/pencil_kernel.hip): entry v holds the IEEE f16 bits
of the integer v in both halves for v < 2048, and every later entry repeats
the 2047 entry (padding positions clamp their index into that tail).

The header is plain C++17, so a host program that includes it alone prints the
table the device code is built from.

TSA_H_TAB is off by default (it measured slower), so no default
build compiles the kernel code that reads the table: a syntax-only device
compile of csrc/pencil_kernel.hip with the switch set keeps that form
building."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "hw-accelerator-three-sequence-alignment_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "h_table.h"
static constexpr tsa::HTable T = tsa::make_h_table();  // built at compile time
static_assert(T.v[0] == 0u && T.v[1] == 0x3C003C00u && T.v[2047] == T.v[tsa::H_TAB_N - 1], "h_table");
int main() {
  std::printf("%d %d\n", tsa::H_TAB_N, tsa::H_TAB_SAT);
  for (int i = 0; i < tsa::H_TAB_N; ++i) std::printf("%u\n", T.v[i]);
  return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler builds the library; the table test uses the same one"
    d = tmp_path_factory.mktemp("h_table")
    src, exe = d / "dump.cpp", d / "dump"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{HEADER_DIR}", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    n, sat = int(out[0]), int(out[1])
    return n, sat, np.array([int(x) for x in out[2:]], dtype=np.uint64)


def test_table_is_float16_bit_for_bit(table):
    n, sat, v = table
    assert sat == 2047 and len(v) == n
    want = np.arange(2048).astype(np.float16).view(np.uint16).astype(np.uint64) * 0x00010001
    assert np.array_equal(v[:2048], want)
    # exact: every integer below 2048 is an f16 value
    assert np.array_equal(np.arange(2048).astype(np.float16).astype(np.int64), np.arange(2048))


def test_table_tail_saturates(table):
    n, sat, v = table
    # a four-entry read whose first index is clamped to sat + 1 stays inside
    assert n >= sat + 1 + 4
    assert np.all(v[sat:] == v[sat])


def test_table_form_of_the_kernel_still_compiles():
    """-DTSA_H_TAB=1: the front end instantiates every helix kernel with the
    table form's code (no code generation: a few seconds)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the Makefile's compiler
    assert os.path.exists(hipcc), hipcc
    r = subprocess.run([hipcc, "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-fsyntax-only",
                        "-Wall", "-Wno-unused-function", "-DTSA_H_TAB=1",
                        os.path.join(HEADER_DIR, "pencil_kernel.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
