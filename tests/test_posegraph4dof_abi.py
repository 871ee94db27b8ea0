"""The 4-DoF pose-graph additions of the C ABI (include/orbslam3_hip_4dof.h, which include/orbslam3_hip.h includes; no GPU): both
functions are declared there and exported, the ctypes mirrors have the layout of the C structs, every argument check of
essg_optimize_4dof answers before anything touches a device, and without a device the entry point fails loudly."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "orbslam3_hip.h")
HEADER_4DOF = os.path.join(ROOT, "include", "orbslam3_hip_4dof.h")
EXPECTED = ["essg_check_4dof", "essg_optimize_4dof"]


@pytest.fixture(scope="module")
def capi(pkg):
    return importlib.import_module("orb_slam3-1_amd.capi")


@pytest.fixture(scope="module")
def sp(pkg):
    return importlib.import_module("orb_slam3-1_amd.synth_posegraph")


def test_symbols_declared_and_exported(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_4DOF).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(essg_[a-z0-9_]+)\s*\(", src))) == EXPECTED
    assert '#include "orbslam3_hip_4dof.h"' in open(HEADER).read()
    for n in EXPECTED:
        assert hasattr(pkg.lib, n), "symbol %s declared in include/orbslam3_hip_4dof.h is not exported" % n
    assert callable(pkg.EssentialGraph.optimize_4dof)


def test_struct_layout_matches_header(capi):
    structs = {"Essg4DofProblem": ["n_vertices", "rcw", "tcw", "rwb", "twb", "rcb", "tcb", "fixed", "n_edges", "edge_vertices", "edge_rot",
                                   "edge_trans", "information", "max_iters", "lambda_init", "n_points", "points", "point_ref", "scw"],
               "Essg4DofResult": ["rcw_out", "tcw_out", "pose_q", "pose_t", "points_out", "stats"]}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "orbslam3_hip.h"', "int main(void) {"]
    for s, fields in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for f in fields:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        out = subprocess.check_output([exe], text=True)
    seen = dict(l.split() for l in out.strip().splitlines())
    for s, fields in structs.items():
        cls = getattr(capi, s)
        assert [f for f, _ in cls._fields_] == fields
        assert int(seen[s]) == C.sizeof(cls), s
        for f in fields:
            assert int(seen["%s.%s" % (s, f)]) == getattr(cls, f).offset, "%s.%s" % (s, f)


def _call(pkg, prep, problem=True, result=True):
    return pkg.lib.essg_optimize_4dof(None, C.byref(prep["problem"]) if problem else None, C.byref(prep["result"]) if result else None, None)


def _graph(sp, **kw):
    return sp.make_posegraph4dof(3, n=12, n_points=6, **kw)


def test_check_accepts_a_good_problem(pkg, capi, sp):
    for kw in (dict(), dict(n_fixed=3, duplicates=2, float_inputs=True, identity_tcb=False), dict(lambda_init=1e-3)):
        good = capi.essg4dof_prepare(_graph(sp, **kw))
        assert pkg.lib.essg_check_4dof(C.byref(good["problem"]), C.byref(good["result"])) == 0
    nopts = capi.essg4dof_prepare(dict(_graph(sp), points=np.zeros((0, 3), np.float32), point_ref=np.zeros(0, np.int32)))
    assert nopts["problem"].scw is None and nopts["problem"].n_points == 0
    assert pkg.lib.essg_check_4dof(C.byref(nopts["problem"]), C.byref(nopts["result"])) == 0
    nopose = capi.essg4dof_prepare(_graph(sp))
    nopose["result"].pose_q = None; nopose["result"].pose_t = None       # optional outputs
    assert pkg.lib.essg_check_4dof(C.byref(nopose["problem"]), C.byref(nopose["result"])) == 0


def test_every_argument_check(pkg, capi, sp):
    """each refusal of the header, with the message that names it; the handle is NULL throughout, so nothing can have run"""
    good = capi.essg4dof_prepare(_graph(sp))
    assert _call(pkg, good, problem=False) == -3 and b"NULL problem" in pkg.lib.orbx_last_error()
    assert pkg.lib.essg_check_4dof(None, C.byref(good["result"])) == -3
    assert _call(pkg, good, result=False) == -3 and b"NULL result" in pkg.lib.orbx_last_error()

    def refused(change, text, on="problem"):
        prep = capi.essg4dof_prepare(_graph(sp))
        change(prep[on], prep["arrays"])
        assert pkg.lib.essg_check_4dof(C.byref(prep["problem"]), C.byref(prep["result"])) == -3, text
        assert _call(pkg, prep) == -3, text
        assert text.encode() in pkg.lib.orbx_last_error(), (text, pkg.lib.orbx_last_error())

    def info(p, r, c, v):
        p.information[6 * r + c] = v

    refused(lambda p, a: setattr(p, "n_vertices", 0), "bad problem sizes")
    refused(lambda p, a: setattr(p, "n_edges", -1), "bad problem sizes")
    refused(lambda p, a: setattr(p, "n_points", -1), "bad problem sizes")
    for f in ("rcw", "tcw", "rwb", "twb", "rcb", "tcb", "fixed"):
        refused(lambda p, a, f=f: setattr(p, f, None), "NULL vertex arrays")
    for f in ("edge_vertices", "edge_rot", "edge_trans"):
        refused(lambda p, a, f=f: setattr(p, f, None), "NULL edge arrays")
    for f in ("points", "point_ref", "scw"):
        refused(lambda p, a, f=f: setattr(p, f, None), "NULL point arrays")
    refused(lambda r, a: setattr(r, "rcw_out", None), "NULL rcw_out / tcw_out", on="result")
    refused(lambda r, a: setattr(r, "tcw_out", None), "NULL rcw_out / tcw_out", on="result")
    refused(lambda r, a: setattr(r, "points_out", None), "NULL points_out", on="result")
    refused(lambda p, a: setattr(p, "max_iters", -1), "max_iters")
    refused(lambda p, a: setattr(p, "lambda_init", float("nan")), "lambda_init")
    refused(lambda p, a: setattr(p, "lambda_init", float("inf")), "lambda_init")
    refused(lambda p, a: a["ev"].__setitem__((4, 1), 12), "vertex index out of range")
    refused(lambda p, a: a["ev"].__setitem__((4, 0), -1), "vertex index out of range")
    refused(lambda p, a: a["ev"].__setitem__((5, slice(None)), 7), "to itself")
    refused(lambda p, a: a["fixed"].__setitem__(slice(None), 1), "no free vertex")
    for k in ("rcw", "tcw", "rwb", "twb", "rcb", "tcb"):
        refused(lambda p, a, k=k: a[k].__setitem__((5, 2), np.inf), "vertex 5 is not finite")
    refused(lambda p, a: a["edge_rot"].__setitem__((6, 4), np.nan), "measurement of edge 6 is not finite")
    refused(lambda p, a: a["edge_trans"].__setitem__((6, 1), -np.inf), "measurement of edge 6 is not finite")
    refused(lambda p, a: a["points"].__setitem__((1, 1), np.nan), "point 1 is not finite")
    refused(lambda p, a: a["ref"].__setitem__(2, 12), "reference index out of range")
    refused(lambda p, a: a["ref"].__setitem__(2, -1), "reference index out of range")
    refused(lambda p, a: a["scw"].__setitem__((3, 5), np.nan), "scw of vertex 3 is not finite")
    refused(lambda p, a: a["scw"].__setitem__((3, 7), 0.0), "scale that is not positive")
    refused(lambda p, a: info(p, 1, 4, 0.25), "not symmetric")
    refused(lambda p, a: info(p, 3, 3, 0.0), "diagonal entry that is not positive")
    refused(lambda p, a: info(p, 0, 0, -1e3), "diagonal entry that is not positive")
    refused(lambda p, a: info(p, 2, 2, np.nan), "information matrix is not finite")


def test_capacity_is_an_error_of_its_own(pkg, capi):
    """more free vertices than the documented capacity: ORBX_ERR_CAPACITY (the adapter falls back on it), before any device work"""
    n = capi.ESSG_MAX_FREE_VERTICES + 2
    eye, zero = np.tile(np.eye(3), (n, 1, 1)), np.zeros((n, 3))
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    ev = np.stack([np.arange(1, n), np.arange(0, n - 1)], 1).astype(np.int32)
    w = dict(rcw=eye, tcw=zero, rwb=eye, twb=zero, rcb=eye, tcb=zero, fixed=fixed, edge_vertices=ev, edge_rot=eye[:n - 1], edge_trans=zero[:n - 1])
    prep = capi.essg4dof_prepare(w)
    assert _call(pkg, prep) == -2 and pkg.lib.essg_check_4dof(C.byref(prep["problem"]), C.byref(prep["result"])) == -2
    assert b"capacity" in pkg.lib.orbx_last_error()
    fixed[1] = 1                                    # exactly the capacity: accepted as far as the arguments go
    prep = capi.essg4dof_prepare(w)
    assert pkg.lib.essg_check_4dof(C.byref(prep["problem"]), C.byref(prep["result"])) == 0
    assert _call(pkg, prep) in (-3, -4)
    assert b"capacity" not in pkg.lib.orbx_last_error()


def test_mirror_rejects_arrays_of_unequal_length(capi, sp):
    w = _graph(sp)
    for key in ("fixed", "twb", "rcb", "edge_trans", "point_ref", "scw"):
        bad = dict(w); bad[key] = w[key][:-1]
        with pytest.raises(ValueError):
            capi.essg4dof_prepare(bad)


def test_no_device_fails_loudly(pkg, capi, sp):
    if pkg.device_count() > 0:
        pytest.skip("a HIP device is present")
    prep = capi.essg4dof_prepare(_graph(sp))
    assert _call(pkg, prep) == -4                   # valid arguments, no device, no CPU fallback
    assert not prep["arrays"]["rcw_out"].any()


def test_generator_is_seeded_and_has_what_the_graph_needs(sp):
    a, b, c = sp.make_posegraph4dof(5, n=40, n_points=9), sp.make_posegraph4dof(5, n=40, n_points=9), sp.make_posegraph4dof(6, n=40, n_points=9)
    keys = ("rcw", "tcw", "rwb", "twb", "rcb", "tcb", "fixed", "edge_vertices", "edge_rot", "edge_trans", "points", "point_ref", "scw")
    for k in keys:
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["tcw"], c["tcw"])
    ev = a["edge_vertices"]
    assert a["rcw"].shape == (40, 3, 3) and ev.dtype == np.int32 and a["points"].dtype == np.float32 and a["lambda_init"] == 0.0
    assert 3.0 <= len(ev) / 40 <= 5.0 and (ev[:, 0] != ev[:, 1]).all() and a["fixed"].sum() == 1 and a["fixed"][0] == 1
    assert {(i, i - 1) for i in range(1, 40)} <= set(map(tuple, ev))            # the inertial edges
    assert tuple(ev[0]) == (35, 0) or (39, 0) in set(map(tuple, ev[:15]))       # loop connections come first
    assert np.array_equal(a["information"], np.diag([1e3, 1e3, 1, 1, 1, 1]))
    # gravity-aligned: the drift is a rotation about the world's z and a translation, so Rcw Rcw_truth^T maps z to z (identity Tcb)
    D = np.einsum("nij,nkj->nik", a["rcw"].transpose(0, 2, 1), a["truth_rcw"].transpose(0, 2, 1))      # Rwc Rwc_truth^T
    assert np.abs(D[:, 2, 2] - 1).max() < 1e-12 and np.abs(D[:, 0, 1]).max() > 1e-3
    # consistent inputs: camera pose and body pose agree to rounding; float inputs: to float rounding only
    for g, lo, hi in ((a, 0.0, 1e-14), (sp.make_posegraph4dof(5, n=40, float_inputs=True, identity_tcb=False), 1e-9, 1e-5)):
        Rcw = np.einsum("nij,nkj->nik", g["rcb"], g["rwb"])
        tcw = np.einsum("nij,nj->ni", g["rcb"], -np.einsum("nji,nj->ni", g["rwb"], g["twb"])) + g["tcb"]
        err = max(np.abs(Rcw - g["rcw"]).max(), np.abs(tcw - g["tcw"]).max())
        assert lo <= err <= hi, err
    f = sp.make_posegraph4dof(5, n=40, n_fixed=6, duplicates=4, identity_tcb=False, corrected_scale=1.05, n_points=5)
    assert f["fixed"].sum() == 6 and f["fixed"][f["edge_vertices"]].all(1).sum() >= 5
    pairs = [tuple(e) for e in f["edge_vertices"]]
    assert len(pairs) - len(set(pairs)) >= 1
    assert not np.allclose(f["rcb"][0], np.eye(3)) and np.abs(f["tcb"][0]).max() > 0.01
    assert (f["scw"][-5:, 7] == 1.05).all() and (f["scw"][:-5, 7] == 1).all()
    assert np.allclose(f["scw"][-5:, 4:7], 1.05 * f["tcw"][-5:], rtol=1e-15)    # the vertex drops the scale, scw keeps it
