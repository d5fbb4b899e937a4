"""goal_s2max (ogbench_amd/csrc/goal_threshold.h): the step kernels test success
as dist^2 <= goal_s2max(goal_tol) instead of sqrt(dist^2) <= goal_tol.  That
is the same test for every input exactly when goal_s2max(tol) is the largest
double whose correctly rounded square root is <= tol.  The header is plain
C++, so the host function itself is compiled here (no GPU, no HIP) into a
small program that prints its value for each tolerance.
"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, 'ogbench_amd', 'csrc')

# the registry's tolerances (maze.py:86: 1.0 for the point mass, 0.5 otherwise), then awkward ones
TOLS = [1.0, 0.5, 0.3, 0.7, 0.1, 1.0 / 3.0, math.pi, 1e-3, 2.5, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52, 1e-160, 1e150]

MAIN = r'''
#include <cstdio>
#include <cstdlib>
#include "goal_threshold.h"
int main(int argc, char** argv) {
  for (int k = 1; k < argc; ++k) std::printf("%a\n", ogbx::goal_s2max(std::strtod(argv[k], nullptr)));
  return 0;
}
'''


def s2max_py(tol):
    """The header's rule restated: start at fl(tol * tol), walk with nextafter."""
    tol = np.float64(tol)
    s = tol * tol
    while s > 0 and np.sqrt(s) > tol:
        s = np.nextafter(s, np.float64(0))
    while np.sqrt(np.nextafter(s, np.float64(np.inf))) <= tol:
        s = np.nextafter(s, np.float64(np.inf))
    return s


def _is_exact(tol, s):
    tol, s = np.float64(tol), np.float64(s)
    return bool(np.sqrt(s) <= tol) and bool(np.sqrt(np.nextafter(s, np.float64(np.inf))) > tol)


@pytest.fixture(scope='module')
def host_values(tmp_path_factory):
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'),
                            '/opt/rocm/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx is not None, 'no host C++ compiler found'
    d = tmp_path_factory.mktemp('goal_s2max')
    src, exe = d / 'main.cpp', d / 'main'
    src.write_text(MAIN)
    subprocess.run([cxx, '-O2', '-std=c++17', '-ffp-contract=off', '-I', HEADER_DIR, str(src), '-o', str(exe)],
                   check=True)
    out = subprocess.run([str(exe)] + [float(t).hex() for t in TOLS], check=True, capture_output=True, text=True)
    vals = [float.fromhex(line) for line in out.stdout.split()]
    assert len(vals) == len(TOLS)
    return dict(zip(TOLS, vals))


@pytest.mark.parametrize('tol', TOLS)
def test_host_threshold_is_exact(host_values, tol):
    s = host_values[tol]
    assert np.sqrt(np.float64(s)) <= tol
    assert np.sqrt(np.nextafter(np.float64(s), np.float64(np.inf))) > tol
    assert s == s2max_py(tol)


def test_threshold_decides_every_neighbour_like_the_square_root(host_values):
    """dist^2 <= s2max and sqrt(dist^2) <= tol agree on the 64 doubles on either side of the threshold."""
    for tol in TOLS:
        s = np.float64(host_values[tol])
        lo = hi = s
        for _ in range(64):
            lo, hi = np.nextafter(lo, np.float64(0)), np.nextafter(hi, np.float64(np.inf))
            assert bool(np.sqrt(lo) <= tol) == bool(lo <= s)
            assert bool(np.sqrt(hi) <= tol) == bool(hi <= s)
    assert not (np.float64(np.nan) <= np.float64(host_values[1.0]))  # a NaN distance fails both forms


def test_zero_tolerance():
    assert s2max_py(0.0) == 0.0 and _is_exact(0.0, 0.0)
