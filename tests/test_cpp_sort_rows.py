"""device::sort_rows of include/simd_sort/radix_sort.hpp driven from C++
(tests/cpp/test_sort_rows.cpp): a 37 x 1000 matrix of padded rows with two
payload pairs, up and down, each row checked against std::stable_sort of the
same data; then 3 rows of 9000 records (the global levels)."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BIN = os.path.join(CPP, "_build", "test_sort_rows")


@pytest.mark.gpu
def test_sort_rows_header_form_on_gpu():
    subprocess.run(["make", "-C", CPP, "-f", "sort_rows.mk", "_build/test_sort_rows"],
                   check=True)  # (incremental)
    for args in (["37", "1000"], ["3", "9000"]):
        r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "sort_rows ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
