"""The packed LDL^T solve of the one-workgroup solvers (orb_slam3-1_amd/csrc/dense_lm_device.h), compiled with g++ for the CPU
(tests/ldlt_check.cpp): the two instantiations the kernels use against long-double Gaussian elimination."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ldlt_solve_against_long_double_elimination(tmp_path):
    exe = str(tmp_path / "ldlt_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "orb_slam3-1_amd", "csrc"),
                           os.path.join(ROOT, "tests", "ldlt_check.cpp"), "-o", exe])
    rows = [l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert [(r[0], r[1]) for r in rows] == [("6", "1"), ("7", "0")]         # ldlt_solve<6, true> (pose), ldlt_solve<7, false> (Sim3)
    for n, recip, solved, worst, rejected in rows:
        print("ldlt_solve<%s, %s>: worst component error / max|x| = %s" % (n, recip, worst))
        assert solved == "1"                        # eigenvalues in [1, 1e3], lambda 0.25: every pivot is positive
        # N^2 * eps * cond = 49 * 2.2e-16 * 1e3 ~ 1e-11
        assert float(worst) <= 1e-11
        assert rejected == "1"                      # a non-positive first pivot returns false
