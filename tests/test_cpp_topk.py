"""device::top_k of include/simd_sort/radix_sort.hpp driven from C++
(tests/cpp/test_topk.cpp): the separate-array form with two payload pairs
and the DataElement form, up and down, at n = 10000, k = 100, each checked
against std::stable_sort of the same data."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BIN = os.path.join(CPP, "_build", "test_topk")


@pytest.mark.gpu
def test_top_k_header_forms_on_gpu():
    subprocess.run(["make", "-C", CPP, "-f", "topk.mk", "_build/test_topk"], check=True)  # (incremental)
    r = subprocess.run([BIN, "10000", "100"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "top_k ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
