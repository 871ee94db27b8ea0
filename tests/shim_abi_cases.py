"""The scenarios behind tests/golden/shim_abi/: for each toy of tests/stubs/ whose recording fakes dump their problem structs through
tests/stubs/record_abi.hpp, how it is built and the argument lists it is run with.  Shared by tools/make_shim_abi_golden.py, which
records the dumps against any checkout's include/ directory, and tests/test_shim_abi_golden.py, which compares the tree's with them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
LIBDIR = os.path.join(ROOT, "orb_slam3-1_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "shim_abi")

INERTIAL = ["liba_window", "liba_recinit", "liba_large", "liba_diverged", "liba_large_diverged", "liba_no_prev", "liba_stop",
            "pose_keyframe", "pose_lastframe", "pose_keyframe_recinit", "pose_lastframe_recinit", "pose_rig"]
KB8 = ["pose_kb8", "pose_pinhole", "pose_rig", "pose_stereo_obs", "lba_kb8", "lba_mixed", "lba_rig", "lba_fixed_pinhole", "lba_stereo_obs"]


def _inertial(_work):
    return [(s, [s]) for s in INERTIAL]


def _kb8(_work):
    return [(s, [s]) for s in KB8]


def _fullba(work):
    """the maps of tests/test_shim_fullba.py: every combination of bInit, bFixLocal and the loop id that reaches fiba_solve"""
    import test_shim_fullba as t
    case = work / "fullba.txt"
    t.write_case(case, t.make_map())
    out = []
    for init in (0, 1):
        for fix_local in (0, 1):
            for loop_id in (0, 9):
                out.append(("init%d_fixlocal%d_loop%d" % (init, fix_local, loop_id), [str(case), "7", str(fix_local), str(loop_id), "0", str(init), "100.0", "1000000.0"]))
    out.append(("no_stop_flag_100_iterations", [str(case), "100", "0", "0", "-1", "1", "50.0", "2000.0"]))
    return out


def _imu_init(work):
    """the map of tests/test_shim_imu_init.py (with the clamped eigenvalue) through the walk of each overload"""
    import test_shim_imu_init as t
    case = t.write_case(work / "imu_init.txt", t.make_map())
    return [("walk_overload%d" % o, ["walk", case, str(o)]) for o in (1, 2, 3)]


# toy -> (scenarios, links the library, its stdout is part of the golden)
TOYS = {
    "shim_inertial_toy": (_inertial, False, True),
    "shim_kb8_toy": (_kb8, False, False),
    "shim_fullba_toy": (_fullba, True, False),
    "shim_imu_init_toy": (_imu_init, True, False),
}


def record(toy, include_dir, work):
    """Builds tests/stubs/<toy>.cpp against include_dir in the directory `work` and returns the text of all its scenarios."""
    scenarios, needs_lib, with_stdout = TOYS[toy]
    exe = work / toy
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", str(include_dir), os.path.join(STUBS, toy + ".cpp"), "-o", str(exe)]
    if needs_lib:
        cmd += ["-L", LIBDIR, "-lorbslam3_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    text = []
    for name, args in scenarios(work):
        r = subprocess.run([str(exe)] + args, capture_output=True, text=True)
        assert r.returncode == 0, (toy, name, r.returncode, r.stderr[-2000:])
        text.append("== %s\n%s" % (name, r.stderr))
        if with_stdout:
            text.append("-- stdout\n%s" % r.stdout)
    return "".join(text)
