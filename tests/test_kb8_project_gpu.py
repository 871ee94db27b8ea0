"""orbx_kb8_project: the device's KannalaBrandt8::project and projectJac (csrc/camera_kb8.h) against tests/kb8_reference.py."""
import importlib

import numpy as np
import pytest

import kb8_reference as kr
from dense_ba_reference import LD

pytestmark = pytest.mark.gpu


def test_project_and_jacobian_on_4096_points(pkg):
    sk = importlib.import_module("orb_slam3-1_amd.synth_kb8")
    cam = sk.tumvi_camera()
    X = sk.make_camera_points(0, 4096)              # 0.5 .. 85 degrees off axis, depths 0.3 .. 30, sqrt(x^2 + y^2) >= 0.01 z
    uv, J = pkg.kb8_project(cam, X)
    # the device's theta and psi are within one float ulp of the host's (the f64 atan2 rounded to float against glibc's atan2f):
    # |du| <= fx (fd ulp32(theta) + r ulp32(psi)) + 1e-9, likewise dv -- derived, not measured
    ref = kr.project(cam, X)
    bound = kr.project_bound(cam, X)
    err = np.abs(uv - ref)
    print("largest |uv - reference| / bound: %.3f; exact agreement on %d of %d points" % (float((err / bound).max()), int((err == 0).all(1).sum()), len(X)))
    assert (err <= bound).all()
    # the Jacobian is all double: a few ulp, amplified by at most 1 / r^3 at the generator's floor
    Jr = kr.project_jac(cam, X)
    row = np.abs(Jr).max(2, keepdims=True)
    print("largest Jacobian error relative to its row: %.3g" % float((np.abs(J - Jr) / row).max()))
    assert (np.abs(J - Jr) <= 1e-10 * row).all()
    # uv alone (jac == NULL) gives the same bits
    np.testing.assert_array_equal(pkg.kb8_project(cam, X, want_jac=False), uv)
