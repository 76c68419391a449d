"""device::unique of include/simd_sort/radix_sort.hpp driven from C++
(tests/cpp/test_unique.cpp): 100 000 records of 300 distinct keys, two payload
pairs, up and down, with every optional output and with none, checked against
std::stable_sort of the same data plus a run scan, the slots past U against
their fill."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BIN = os.path.join(CPP, "_build", "test_unique")


@pytest.mark.gpu
def test_unique_header_form_on_gpu():
    subprocess.run(["make", "-C", CPP, "-f", "unique.mk", "_build/test_unique"],
                   check=True)  # (incremental)
    r = subprocess.run([BIN, "100000", "300"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "unique ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
