"""piece_weights_from (ogbench_amd/csrc/piece_weights.h): the lean contact loop
builds the integer weights of an active-edge set from the edge activities as
doubles (adds and one fma) instead of taking the integer mask apart and
converting.  Every weight is an integer of magnitude <= 4, so the two builders
must agree bit for bit on every mask.  The header is plain C++, so both are
compiled here (no GPU, no HIP) into a small program that prints, for each of
the 512 masks of three slots, the weights from the activities; the expected
values are the integer definition, restated in Python.
"""
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, 'ogbench_amd', 'csrc')

FIELDS = ['S0', 'T0', 'D0', 'S1', 'T1', 'D1', 'S2', 'T2', 'D2', 'A2', 'C2']

# per mask: one line for piece_weights_from of the mask's activities, one for
# the header's own integer builder; values as the 64-bit patterns of the doubles
MAIN = r'''
#include <cstdio>
#include <cstring>
#include "piece_weights.h"
static void show(const ogbx::PieceWeights& p) {
  const double v[11] = {p.S0, p.T0, p.D0, p.S1, p.T1, p.D1, p.S2, p.T2, p.D2, p.A2, p.C2};
  for (int k = 0; k < 11; ++k) {
    unsigned long long b;
    std::memcpy(&b, &v[k], sizeof b);
    std::printf("%016llx%c", b, k == 10 ? '\n' : ' ');
  }
}
int main() {
  for (unsigned A = 0; A < 512; ++A) {
    ogbx::EdgeActs e;
    for (int i = 0; i < 9; ++i) e.a[i] = ogbx::edge_on((A >> i) & 1u);
    ogbx::PieceWeights p, q;
    ogbx::piece_weights_from(e, p);
    ogbx::piece_weights(A, q);
    show(p);
    show(q);
  }
  return 0;
}
'''


def weights_py(A):
    """The integer definition: per slot T = a0 + a1, D = a0 - a1, S = T + 2 a2; A2 = a0 + a1 + a2, C2 = a2 of slot 2."""
    out = {}
    for s in range(3):
        a0, a1, a2 = (A >> (3 * s)) & 1, (A >> (3 * s + 1)) & 1, (A >> (3 * s + 2)) & 1
        out['T%d' % s], out['D%d' % s], out['S%d' % s] = a0 + a1, a0 - a1, a0 + a1 + 2 * a2
    out['A2'] = ((A >> 6) & 1) + ((A >> 7) & 1) + ((A >> 8) & 1)
    out['C2'] = (A >> 8) & 1
    return out


def _bits(v):
    return struct.unpack('<Q', struct.pack('<d', float(v)))[0]


@pytest.fixture(scope='module')
def host_rows(tmp_path_factory):
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'),
                            '/opt/rocm/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx is not None, 'no host C++ compiler found'
    d = tmp_path_factory.mktemp('piece_weights')
    src, exe = d / 'main.cpp', d / 'main'
    src.write_text(MAIN)
    subprocess.run([cxx, '-O2', '-std=c++17', '-ffp-contract=off', '-I', HEADER_DIR, str(src), '-o', str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True)
    rows = [[int(w, 16) for w in line.split()] for line in out.stdout.splitlines()]
    assert len(rows) == 1024 and all(len(r) == len(FIELDS) for r in rows)
    return rows


def test_weights_from_activities_match_the_integer_definition(host_rows):
    for A in range(512):
        want = weights_py(A)
        got = dict(zip(FIELDS, host_rows[2 * A]))
        for f in FIELDS:
            assert got[f] == _bits(want[f]), (A, f, hex(got[f]), want[f])


def test_mask_builder_matches_the_integer_definition(host_rows):
    """The header's own integer builder (the full loop's) states the same definition."""
    for A in range(512):
        want = weights_py(A)
        got = dict(zip(FIELDS, host_rows[2 * A + 1]))
        for f in FIELDS:
            assert got[f] == _bits(want[f]), (A, f, hex(got[f]), want[f])


def test_zero_weights_are_positive_zero(host_rows):
    """D = a0 - a1 of equal activities is +0.0 (not -0.0), as the conversion of integer 0 gives."""
    assert all(w != _bits(-0.0) for row in host_rows for w in row)
