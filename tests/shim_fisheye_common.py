"""Shared by tests/test_shim_fisheye.py and tests/test_fisheye_stereo_gpu.py: builds tests/stubs/shim_fisheye_toy.cpp (with its
recording fake, or against the library), writes a frame case as the toy's case file and parses what the toy prints.  A test helper."""
import os
import subprocess

import numpy as np

import fisheye_stereo_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "orb_slam3-1_amd")


def build_toy(d, real):
    exe = os.path.join(str(d), "shim_fisheye_toy")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, os.path.join(STUBS, "shim_fisheye_toy.cpp"), "-o", exe]
    if real:
        cmd += ["-DSHIM_FISHEYE_REAL", "-L", LIBDIR, "-lorbslam3_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def keypoints(capi, kps):
    """(n, 3) of x, y, octave -> KP_DTYPE, the other fields as the extractor leaves them"""
    kps = np.asarray(kps, np.float64).reshape(-1, 3)
    k = np.zeros(len(kps), capi.KP_DTYPE)
    k["x"], k["y"], k["octave"] = kps[:, 0], kps[:, 1], kps[:, 2].astype(np.int32)
    k["size"], k["angle"], k["response"], k["class_id"] = 31.0, 45.0, 20.0, -1
    return k


def case_bytes(capi, c):
    head = np.array([len(c["kps_l"]), c["mono_l"], len(c["kps_r"]), c["mono_r"], cases.N_LEVELS], np.int32)
    return b"".join([head.tobytes(), cases.rig_floats(c["rig"]).tobytes(), cases.LEVEL_SIGMA2.tobytes(),
                     keypoints(capi, c["kps_l"]).tobytes(), np.ascontiguousarray(c["desc_l"], np.uint8).tobytes(),
                     keypoints(capi, c["kps_r"]).tobytes(), np.ascontiguousarray(c["desc_r"], np.uint8).tobytes()])


def run_toy(exe, scenario, case, tmp_path):
    path = os.path.join(str(tmp_path), "case.bin")
    with open(path, "wb") as f:
        f.write(case)
    r = subprocess.run(["timeout", "-k", "10", "120", exe, scenario, path, os.path.join(str(tmp_path), "dump.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = dict(calls=[], left=[], right=[])
    for tok in (ln.split() for ln in r.stdout.strip().splitlines()):
        if tok[0] == "reference_calls":
            out["reference_calls"], out["close"], out["sizes"] = int(tok[1]), int(tok[3]), [int(v) for v in tok[5:]]
        elif tok[0] == "left":
            out["left"].append([int(tok[2])] + [float.fromhex(v) for v in tok[3:]])
        elif tok[0] == "right":
            out["right"].append(int(tok[2]))
        else:
            out["calls"].append(tok)
    left = np.array(out["left"], np.float64).reshape(-1, 6)
    out["left_to_right"], out["depth"], out["u_right"], out["p3d"] = left[:, 0].astype(np.int32), left[:, 1].astype(np.float32), left[:, 2], left[:, 3:].astype(np.float32)
    out["right_to_left"] = np.array(out["right"], np.int32)
    return out
