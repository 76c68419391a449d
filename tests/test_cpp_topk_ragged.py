"""device::top_k_ragged of include/simd_sort/radix_sort.hpp driven from C++
(tests/cpp/test_topk_ragged.cpp): 1000 segments of 0 .. 600 records plus one of
9000, two payload pairs, up and down, with and without indices and counts,
k = 10 (the kernels) and k = 3000 (the sort route), each segment's head checked
against std::stable_sort of the same data and every other slot against its
fill."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BIN = os.path.join(CPP, "_build", "test_topk_ragged")


@pytest.mark.gpu
def test_topk_ragged_header_form_on_gpu():
    subprocess.run(["make", "-C", CPP, "-f", "topk_ragged.mk", "_build/test_topk_ragged"],
                   check=True)  # (incremental)
    r = subprocess.run([BIN, "1000", "600", "9000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "topk_ragged ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
