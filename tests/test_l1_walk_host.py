"""The register-resident Knuth-Yao walk and low popcount of `ob_spec.h` against the bit-at-a-time
`ob_bitstream`, on the host (no GPU).

Builds tests/l1_walk_host.cpp (a stand-alone program; its header says what it walks) against
`ob_spec.h` and runs it. Per table it compares 200,000 uniform streams, at least 16 streams found
by search whose walk leaves the nine hot columns (the fallback to the generic stream), and one
crafted stream that runs past the first word, the first call and a refill; then the low popcount
at every length 1 .. 127. The program fails on the first differing sample or final bit position,
and when fewer than four of the six tables reach their 16 found streams.

The floor is reachable: the generic walk alone leaves the hot columns in 0.4-0.7 % of uniform
streams, so the search finds 16 per table within about 5,000 candidates of its 5 * 10^7, on all six
tables. A walk of more than 32 bits has a probability below 10^-7 per stream, so the search does
not find one (the program prints how many it saw); the crafted streams cover that path instead.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    pytest.fail("no C++ compiler found (CXX, g++, clang++)")


def test_l1_walk_fast_equals_generic(tmp_path):
    exe = str(tmp_path / "l1_walk_host")
    subprocess.run([_compiler(), "-O2", "-std=c++17", "-I", os.path.join(ROOT, "oaxaca-blinder-rs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "l1_walk_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert "MISMATCH" not in r.stdout
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "popcount: m = 1 .. 127" in r.stdout
