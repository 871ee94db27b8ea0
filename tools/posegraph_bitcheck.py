"""Do the pose-graph solvers of this build return the bits another build returned?  Needs a GPU.

    python tools/posegraph_bitcheck.py record FILE      # in a checkout of the other commit, built
    python tools/posegraph_bitcheck.py compare FILE     # here

Every case of tests/posegraph_cases.py (EssentialGraph.optimize) and tests/posegraph4dof_cases.py (EssentialGraph.optimize_4dof)
runs on ONE handle, Sim3 and 4-DoF calls alternating, through the public Python API alone, so the same file runs in either
checkout.  The results involve no atomics and the assembly sums in a fixed order: identical kernels launched in the identical
sequence reproduce every bit.  record stores each output array and the stats of each call (an .npz); compare runs the cases again
and wants every array equal under np.array_equal and every stats dictionary equal under ==, with no tolerance.
Exit status 0: all equal; 1: something differs (each difference is listed)."""
import importlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
try:
    import torch  # noqa: F401  (one HIP runtime per process: see tests/conftest.py)
except Exception:
    pass
import numpy as np  # noqa: E402


def run_cases():
    """{"<solver>/<case>/<output>": array} and {"<solver>/<case>": stats} of every case"""
    pkg = importlib.import_module("orb_slam3-1_amd")
    sp = importlib.import_module("orb_slam3-1_amd.synth_posegraph")
    sim3_cases = importlib.import_module("posegraph_cases").CASES
    dof4_cases = importlib.import_module("posegraph4dof_cases").CASES
    calls = [c for pair in itertools.zip_longest((("sim3", n) for n in sim3_cases), (("4dof", n) for n in dof4_cases)) for c in pair if c]
    arrays, stats = {}, {}
    g = pkg.EssentialGraph()
    for kind, name in calls:
        if kind == "sim3":
            out = g.optimize(sp.make_posegraph(**sim3_cases[name]))
        else:
            out = g.optimize_4dof(sp.make_posegraph4dof(**dof4_cases[name]))
        stats["%s/%s" % (kind, name)] = out.pop("stats")
        for k, v in out.items():
            arrays["%s/%s/%s" % (kind, name, k)] = np.array(v)
        print("%s/%s: %d iterations, %d trials, chi2 %r" % (kind, name, stats[kind + "/" + name]["iterations"], stats[kind + "/" + name]["trials"],
                                                           stats[kind + "/" + name]["chi2_final"]), flush=True)
    g.close()
    return arrays, stats


def jsonable(v):
    return v.tolist() if isinstance(v, np.ndarray) else v.item() if isinstance(v, np.generic) else v


def main():
    if len(sys.argv) != 3 or sys.argv[1] not in ("record", "compare"):
        print(__doc__)
        return 2
    mode, path = sys.argv[1:]
    arrays, stats = run_cases()
    stats = {k: {f: jsonable(v) for f, v in st.items()} for k, st in stats.items()}
    if mode == "record":
        np.savez(path, __stats__=np.array(json.dumps(stats)), **arrays)
        print("recorded %d arrays of %d calls" % (len(arrays), len(stats)))
        return 0
    with np.load(path) as f:
        base = {k: f[k] for k in f.files if k != "__stats__"}
        base_stats = json.loads(str(f["__stats__"]))
    bad = ["set of outputs: %s" % sorted(set(base) ^ set(arrays))] if set(base) != set(arrays) else []
    bad += ["%s: %d of %d entries differ" % (k, int((base[k] != arrays[k]).sum()) if base[k].shape == arrays[k].shape else -1, arrays[k].size)
            for k in sorted(set(base) & set(arrays)) if not np.array_equal(base[k], arrays[k])]
    bad += ["stats of %s: %r recorded, %r here" % (k, base_stats.get(k), stats.get(k)) for k in sorted(set(base_stats) | set(stats)) if base_stats.get(k) != stats.get(k)]
    for b in bad:
        print("DIFFERS  " + b)
    print("%d arrays and %d stats compared: %s" % (len(arrays), len(stats), "bit-identical" if not bad else "%d differences" % len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
