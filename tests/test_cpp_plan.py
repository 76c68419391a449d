"""The first level's host planner (csrc/srs_plan.hip: digit table, key
clusters, range arithmetic) under AddressSanitizer and UBSan, on its own
(tests/cpp/plan_check.cpp, built for the host by tests/cpp/plan.mk): edge
histograms for 32- and 64-bit keys, with the properties tests/test_table_plan.py
checks asserted in C++. No GPU, no library: a child process."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")


def test_planner_under_address_and_ub_sanitizers():
    b = subprocess.run(["make", "-C", CPP, "-f", "plan.mk", "_build/plan_check"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([os.path.join(CPP, "_build", "plan_check")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "plan_check ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
