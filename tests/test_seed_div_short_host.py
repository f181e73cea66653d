"""The short seeded division of the chi-square kernels (csrc/pm_seed_short.h: div_seeded_short — the table seed used as the
reciprocal, no Newton step) on the host: tools/microbench/seed_short_host.cpp evaluates seed_short_pair_ok, the predicate the
device certifies each launch with (pm_chi2.hip: seed_cert_kernel), with std::fma and IEEE division over every count pair
(ca, cb) with ca + cb < 94^2, for five totals.

No proof says the short quotient is correctly rounded; the sweep observes 0 failures for these totals, and the product relies on
the per-launch certificate, not on this list.  That the predicate can say no is shown by degrading every seed to
fl(R[s] (1 + 2^-K)): K = 39 is the largest K at which the sweep fails at all (2 pairs, both for T = 999; none at K = 40 and
above — the seed's own error is 2^-51; K = 38: 12 pairs, K = 36: 172, K = 32: 77 200)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tools", "microbench", "seed_short_host.cpp")
TOTALS = [999, 4096, 19999, 49999, 199999]
PAIRS = 94 * 94 * (94 * 94 + 1) // 2
K_FAILS = 39
LINE = re.compile(r"T (\d+) degrade (\d+) pairs (\d+) short_bad (\d+)")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    out = str(tmp_path_factory.mktemp("seed_short") / "seed_short_host")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", SRC, "-o", out])
    return out


def sweep(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300, check=True).stdout
    print(out)
    rows = [tuple(int(x) for x in m) for m in LINE.findall(out)]
    assert [r[0] for r in rows] == TOTALS and all(r[2] == PAIRS for r in rows), out
    return rows


def test_the_short_quotient_has_the_bits_of_ieee_division(exe):
    assert [r[3] for r in sweep(exe)] == [0] * len(TOTALS)


def test_the_predicate_rejects_a_degraded_seed(exe):
    rows = sweep(exe, K_FAILS)
    assert all(r[1] == K_FAILS for r in rows) and sum(r[3] for r in rows) >= 1


def test_the_kernels_divide_as_the_predicate_does():
    """One definition: the kernel's seeded term and the certificate both go through pm_seed_short.h."""
    chi2 = open(os.path.join(ROOT, "platymatch_amd", "csrc", "pm_chi2.hip")).read()
    assert "div_seeded_short(df * df, a[p] + b[q], Rc[k])" in chi2 and "seed_short_pair_ok(" in chi2
