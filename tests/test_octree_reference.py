"""The Python restatement of DistributeOctTree (octree_reference.py) against the CPU oracle on the dot images of octree_cases.py, and
the COVERAGE of those images: their traces together must reach every situation in which the octree kernel's waves share work, so
that the GPU test (test_octree_waves_gpu.py) cannot pass by never getting there.

Two items of the list this suite was written to cover cannot exist, and are asserted as such instead of being dropped silently:
  * a one-by-one node of exactly ONE key: a node of one key is bNoMore and is never divided, on any path;
  * a pass with MORE than 64 one-by-one nodes: a one-by-one node holds at least 33 keys once more than 6 lanes are active, dots are
    4 pixels apart, and an image of at most 320 x 240 has 64 nodes of 36 x 26 (54 dots at most) but 256 nodes of 18 x 13 (20 dots at
    most) one level further down.  The reachable end of that item is checked: a FULL list of 64 one-by-one nodes in one batch, and
    passes of two and more batches."""
import numpy as np
import pytest

import octree_cases as oc
import octree_reference as oref

WAVES = (2, 4)


@pytest.fixture(scope="module")
def traces():
    out = {}
    for c in oc.CASES:
        x, y, r = c.candidates()
        out[c.name] = oref.distribute(x, y, r, c.w - 32, c.h - 32, c.N)
    return out


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.name)
def test_reference_is_the_oracle(oracle, case, traces):
    oex = oracle.extractor(*case.args)
    oex.extract(case.image(), (0, 1000))
    cand = oex.level_candidates(0)
    x, y, r = case.candidates()
    assert len(cand) == len(case.dots), "one candidate per dot"
    np.testing.assert_array_equal(cand["x"], x)
    np.testing.assert_array_equal(cand["y"], y)
    np.testing.assert_array_equal(cand["response"], r)
    chosen, _ = traces[case.name]
    kps = oex.level_keypoints(0)
    assert len(kps) == len(chosen)
    np.testing.assert_array_equal(kps["x"], x[chosen] + oc.BORDER)
    np.testing.assert_array_equal(kps["y"], y[chosen] + oc.BORDER)
    np.testing.assert_array_equal(kps["response"], r[chosen])


def test_cases_cover_the_kernel(traces):
    batches = [(name, b) for name, (_, t) in traces.items() for b in t["batches"]]
    passes = [(name, p) for name, (_, t) in traces.items() for p in t["passes"]]
    tr = {name: t for name, (_, t) in traces.items()}
    missing = []

    def need(what, ok):
        if not ok:
            missing.append(what)

    # key counts of one-by-one nodes
    counts_few = {k for _, b in batches if b["active"] <= 6 for k in b["one_by_one"]}
    counts_all = {k for _, b in batches for k in b["one_by_one"]}
    assert 1 not in counts_all, "a node of one key is never divided"
    for k in (2, 32):
        need("one-by-one node of %d keys (at most 6 active)" % k, k in counts_few)
    for k in (33, 64, 65, 256, 257):
        need("one-by-one node of %d keys" % k, k in counts_all)
    need("33 keys one by one beside lane-per-node nodes", any(33 in b["one_by_one"] and b["active"] > 6 for _, b in batches))
    need("6 active lanes", any(b["active"] == 6 for _, b in batches))
    need("7 active lanes", any(b["active"] == 7 for _, b in batches))
    # length of the one-by-one list
    lens = {len(b["one_by_one"]) for _, b in batches}
    for n in sorted({0, 1, 2} | {w + d for w in WAVES for d in (-1, 0, 1)}):
        need("a batch with %d one-by-one nodes" % n, n in lens)
    assert max(p["one_by_one"] for _, p in passes) <= 64, "more than 64 one-by-one nodes in a pass (see the module's docstring)"
    need("a full list of 64 one-by-one nodes", 64 in lens)
    need("a pass of two batches", any(p["batches"] == 2 for _, p in passes))
    need("a pass of more than two batches", any(p["batches"] > 2 for _, p in passes))
    # empty children
    need("three empty children", any(3 in b["empty_children"] for _, b in batches))
    need("end by size == prev_size", any(t["end"] == "no_change" for t in tr.values()))
    # the sorted phase
    hits = [(b["hit_lane"], b) for _, b in batches if b["hit_lane"] is not None]
    need("N reached at lane 0", any(l == 0 for l, _ in hits))
    need("N reached at lane 63", any(l == 63 for l, _ in hits))
    for w in WAVES:
        def between(l, b):
            ll = b["one_by_one_lanes"]
            return l in ll and ll.index(l) + 1 < len(ll) and ll.index(l) % w != (ll.index(l) + 1) % w
        need("N reached between the one-by-one nodes of two of %d waves" % w, any(between(l, b) for l, b in hits))
    need("N reached in the first pass, no sort", any(t["end"] == "n" and not t["sorted"] for t in tr.values()))
    need("the sorted phase", any(t["sorted"] for t in tr.values()))
    need("a batch in several rounds", any(b["rounds"] > 1 for _, b in batches))
    # roots
    for n in (1, 2, 4):
        need("nIni = %d" % n, any(t["n_ini"] == n for t in tr.values()))
    need("an empty root", any(t["empty_roots"] == 1 and t["n_ini"] > 1 for t in tr.values()))
    # ties: the first key wins, also in the second block of 64 nodes of the selection
    need("equal responses inside a node", any(t.get("ties") for t in tr.values()))
    need("equal responses beyond node 64", any(any(i >= 64 for i in t.get("ties", [])) and any(i < 64 for i in t["ties"]) for t in tr.values()))
    for n in (0, 1, 63, 64, 65):
        need("total = %d" % n, any(t["total"] == n for t in tr.values()))
    assert not missing, "no case reaches: " + "; ".join(missing)
