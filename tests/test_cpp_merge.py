"""Both forms of device::merge of include/simd_sort/radix_sort.hpp driven from
C++ (tests/cpp/test_merge.cpp): 100 000 + 60 000 records of 300 distinct float
keys with two payloads, up and down, with and without source_out, checked
against std::stable_sort of the concatenation on the transformed keys."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BIN = os.path.join(CPP, "_build", "test_merge")


@pytest.mark.gpu
def test_merge_header_forms_on_gpu():
    subprocess.run(["make", "-C", CPP, "-f", "merge.mk", "_build/test_merge"],
                   check=True)  # (incremental)
    r = subprocess.run([BIN, "100000", "60000", "300"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "merge ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
