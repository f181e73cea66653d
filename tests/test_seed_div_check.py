"""The table-seeded division of the chi-square kernels (pm_common.h: div_seeded, seed_offset) against IEEE division, exhaustively
over every count pair (ca, cb) with ca + cb < 94^2 for four totals: tools/microbench/seed_div_check.hip, one source built for the
device (gpu-marked) and, with std::fma, for the host.  The table index must be exact and the term must carry the bits of
(df * df) / d in every case, zero counts on either side and on both included.  The control without the Newton step is printed,
not asserted: nobody has shown that it fails on this domain."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tools", "microbench", "seed_div_check.hip")
TOTALS = [999, 19999, 49999, 199999]
PAIRS = 94 * 94 * (94 * 94 + 1) // 2
LINE = re.compile(r"T (\d+) pairs (\d+) index_bad (\d+) term_bad (\d+) recip_bad (\d+) control_bad (\d+)")


def verdict(out):
    print(out)
    rows = [tuple(int(x) for x in m) for m in LINE.findall(out)]
    assert [r[0] for r in rows] == TOTALS, out
    for _, pairs, index_bad, term_bad, _recip_bad, _control_bad in rows:
        assert pairs == PAIRS and index_bad == 0 and term_bad == 0, out


def fresh(exe):
    return os.path.exists(exe) and os.path.getmtime(exe) >= os.path.getmtime(SRC)


def test_seeded_division_on_the_host(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "seed_div_check_host")
    subprocess.check_call([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", SRC, "-o", exe])
    verdict(subprocess.run([exe], capture_output=True, text=True, timeout=300, check=True).stdout)


@pytest.mark.gpu
def test_seeded_division_on_the_device():
    exe = os.path.join(ROOT, "tools", "microbench", "seed_div_check")
    if not fresh(exe):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        subprocess.check_call([hipcc, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", SRC, "-o", exe])
    verdict(subprocess.run([exe], capture_output=True, text=True, timeout=300, check=True).stdout)
    hdr = open(os.path.join(ROOT, "platymatch_amd", "csrc", "pm_common.h")).read()
    assert "__builtin_fma(-d, r0, 1.0)" in hdr and "__builtin_fma(r0, e, r0)" in hdr and "__builtin_fma(d, T, magic)" in hdr
