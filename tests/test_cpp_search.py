"""Both forms of device::search_sorted of include/simd_sort/radix_sort.hpp
driven from C++ (tests/cpp/test_search.cpp): 100 000 table keys of 300
distinct values and 50 000 queries, up and down, the flat form with and
without the hint and the segmented form with some bad segment ids, checked
against std::lower_bound and std::upper_bound on the transformed keys."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BIN = os.path.join(CPP, "_build", "test_search")


@pytest.mark.gpu
def test_search_sorted_header_forms_on_gpu():
    subprocess.run(["make", "-C", CPP, "-f", "search.mk", "_build/test_search"],
                   check=True)  # (incremental)
    r = subprocess.run([BIN, "100000", "300", "50000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "search ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
