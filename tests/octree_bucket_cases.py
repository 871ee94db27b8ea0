"""Images for the octree's bucket table (test_octree_buckets_gpu.py), and the ANALYSIS that shows what each of them makes the kernel do:
per pyramid level the candidates as the CPU oracle lists them, their cell codes in the level's table (octree_buckets.py), the trace
of the Python restatement of DistributeOctTree (octree_reference.py) and the key lists of its final nodes.  A case asserts on that
analysis that the situation it was built for occurs, so that the GPU test cannot pass by never getting there."""
import numpy as np

import octree_buckets as ob
import octree_cases as oc
import octree_reference as ref


def final_nodes(x, y, r, width, height, N):
    """distribute(), plus the key lists (candidate indices, ascending) of the nodes the list ends with -- except roots never divided"""
    created, divided = [], set()
    orig = ref._divide

    def recording(p, xs, ys):
        divided.add(id(p))
        ch = orig(p, xs, ys)
        created.extend(c for c in ch if c.keys)
        return ch
    ref._divide = recording
    try:
        chosen, trace = ref.distribute(x, y, r, width, height, N)
    finally:
        ref._divide = orig
    final = [list(n.keys) for n in created if id(n) not in divided]
    # (the recording hangs on distribute() calling the module's _divide for every divide: should that change, this fails loudly
    # instead of the cases' checks going blind -- the list ends with these nodes plus the roots that were never divided)
    assert trace["n_out"] - trace["n_ini"] <= len(final) <= trace["n_out"] == len(chosen), (len(final), trace["n_out"])
    return chosen, trace, final


def analyse(oex, nlevels, depth_max=ob.MAX_DEPTH):
    """oex: an oracle extractor that has just extracted the image.  One record per level."""
    nfeat = oex.tables()["nfeat"]
    levels = []
    for l in range(nlevels):
        c = oex.level_candidates(l)
        w, h = oex.level_size(l)
        N = int(nfeat[l])
        D, n_ini, xb, yb = ob.level_table(w, h, N, depth_max)
        x, y, r = c["x"].astype(np.float32), c["y"].astype(np.float32), c["response"].astype(np.float32)
        rec = dict(total=len(c), N=N, D=D, n_ini=n_ini, xb=xb, yb=yb, x=x, y=y, r=r, codes=[], trace=None, final=[])
        if n_ini > 0 and len(c):
            hx = ob.F32(w - 32) / ob.F32(n_ini)
            rec["codes"] = [ob.cell_code(int(x[k]), int(y[k]), int(ob.F32(x[k]) / hx), xb[int(ob.F32(x[k]) / hx)], yb, D) for k in range(len(c))]
            _, rec["trace"], rec["final"] = final_nodes(x, y, r, w - 32, h - 32, N)
        levels.append(rec)
    return levels


# ---- what a case is built for
def on_split_lines(lv):
    """(a) at every depth of the table a key with x == midx and one with y == midy"""
    D = lv["D"]
    xs, ys = set(int(v) for v in lv["x"]), set(int(v) for v in lv["y"])
    for d in range(1, D + 1):
        idx = [(2 * i + 1) << (D - d) for i in range(1 << (d - 1))]
        if not any(int(lv["xb"][r][i]) in xs for r in range(lv["n_ini"]) for i in idx) or not any(int(lv["yb"][i]) in ys for i in idx):
            return False
    return D >= 1


def deep_cluster(lv):
    """(b) a cell of the table with more than 64 keys, divided below the table by the whole wave (one-by-one nodes) and by single lanes.
    Dots are at least 4 pixels apart and a level's natural depth gives about four cells per feature, so no dot image puts 65 keys
    into a cell of a natural table and still divides it: the case caps the depth at 2 (ORBX_OCT_TAB_DEPTH).  Divides below a table
    of natural depth are `split_below_table` (a patch of noise: uniform noise never gets there)."""
    cnt = np.bincount(lv["codes"])
    t = lv["trace"]
    first_deep = sum(p["batches"] for p in t["passes"][:lv["D"]])          # pass k divides the nodes of depth k (first phase)
    deep = t["batches"][first_deep:]
    return (cnt.max() > 64 and any(b["one_by_one"] for b in deep) and
            any(b["small_max"] == 32 and b["active"] > len(b["one_by_one"]) for b in deep))


def split_below_table(lv):
    """two final nodes inside one cell of the table: that cell was divided by the partition code, at the level's natural depth"""
    per_cell = {}
    for keys in lv["final"]:
        codes = {lv["codes"][k] for k in keys}
        if len(codes) == 1:
            c = codes.pop()
            per_cell[c] = per_cell.get(c, 0) + 1
    return lv["D"] >= 4 and any(v > 1 for v in per_cell.values())


def tie_not_first_in_cell_order(lv):
    """(c) a final node whose first key of maximal response in candidate order is not the one with the smallest cell code"""
    for keys in lv["final"]:
        best = max(lv["r"][k] for k in keys)
        top = [k for k in keys if lv["r"][k] == best]
        if len(top) > 1 and min(lv["codes"][k] for k in top[1:]) < lv["codes"][top[0]]:
            return True
    return False


def breaks_inside_a_batch(lv):
    """(f) the sorted phase reaches N at a lane that is not the batch's last"""
    return any(b["hit_lane"] is not None and b["hit_lane"] < b["lanes"] - 1 for b in lv["trace"]["batches"])


# ---- the images
def _fill(dots, w, h, step=4):
    """a grid of dots `step` apart around the given ones, none closer than 4 to them"""
    out = list(dots)
    for p in oc.grid(8, 8, w - 32 - 8, h - 32 - 8, step):
        if all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= 4 for q in dots):
            out.append(p)
    return out


def _line_dots():
    """320 x 240, D = 5 (N = 217) and D = 6 (N = 1000) share these boundaries: one root of 288 x 208"""
    xb, yb = ob.cell_bounds(0, 288, 5), ob.cell_bounds(0, 208, 5)
    return [(xb[i], yb[j]) for j in (2, 3, 4, 8, 16, 24, 30) for i in (1, 2, 4, 8, 16, 24, 31)]


def _fast_cell_pattern():
    """one dot per FAST cell of 36 x 42 pixels, low in the even cell columns and high in the odd ones: inside a node the first
    candidate (cell row-major) lies BELOW a later one, which therefore has the smaller cell code"""
    dots = []
    for i in range(5):
        for j in range(8):
            p = (3 + 36 * j + 20, 3 + 42 * i + (30 if j % 2 == 0 else 6))
            if 8 <= p[0] < 280 and 8 <= p[1] < 200:
                dots.append(p)
    return dots


def _wide_dots():
    """320 x 100: four roots of 72 x 68; many, few, none and some keys"""
    return oc.grid(8, 8, 70, 58) + oc.block(80, 10, 7, 4, 8) + oc.grid(220, 8, 280, 58)


def sparse_levels_image():
    """dots of different brightness on black, eight levels: the faint ones fade out on the way up the pyramid, so the levels hold
    fewer and fewer candidates down to one and none"""
    img = np.zeros((120, 160), np.uint8)
    for k, v in enumerate((255, 120, 60, 30, 16)):
        img[40 + 9 * (k % 2), 30 + 22 * k] = v
    return img


def noise(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w)).astype(np.uint8)


def noise_patch_image():
    """320 x 240: 64 x 64 pixels of noise -- more corners than N = 217 inside some 60 cells of the depth-5 table -- in a sparse grid of
    dots, which keeps the list growing pass after pass (a pass that adds no node ends the reference's loop) until the patch divides"""
    img = np.zeros((240, 320), np.uint8)
    img[28:212:24, 28:292:24] = 200
    img[84:160, 124:200] = 0
    img[90:154, 130:194] = noise(64, 64, 11)
    return img


class BCase:
    def __init__(self, name, image, args, env=None, check=None, level=0):
        self.name, self.image, self.args, self.env, self.check, self.level = name, image, args, env or {}, check, level

    @property
    def depth_max(self):
        return int(self.env.get("ORBX_OCT_TAB_DEPTH", ob.MAX_DEPTH))


def _dot_case(name, w, h, N, dots, mode="mixed", **kw):
    c = oc.Case(name, w, h, N, dots, mode)
    return BCase(name, c.image(), c.args, **kw)


def build_cases():
    lines = _fill(_line_dots(), 320, 240)
    c = [
        _dot_case("split_lines_n217", 320, 240, 217, lines, check=on_split_lines),
        _dot_case("split_lines_n1000", 320, 240, 1000, lines, check=on_split_lines),
        BCase("cluster_below_depth2", oc.BY_NAME["grid_n1000"].image(), oc.BY_NAME["grid_n1000"].args, {"ORBX_OCT_TAB_DEPTH": "2"}, deep_cluster),
        BCase("no_table", oc.BY_NAME["sub_7_flat"].image(), oc.BY_NAME["sub_7_flat"].args, {"ORBX_OCT_TAB_DEPTH": "0"}, lambda lv: lv["D"] == 0),
        _dot_case("ties_across_fast_cells", 320, 240, 6, _fast_cell_pattern(), "flat", check=tie_not_first_in_cell_order),
        _dot_case("wide_four_roots", 320, 100, 60, _wide_dots(),
                  check=lambda lv: lv["n_ini"] == 4 and lv["trace"]["empty_roots"] == 1 and lv["D"] == 3),
        BCase("sorted_break", oc.BY_NAME["sorted_cut_lane1"].image(), oc.BY_NAME["sorted_cut_lane1"].args, None, breaks_inside_a_batch),
        BCase("sparse_levels", sparse_levels_image(), (100, 1.2, 8, 20, 7)),
        BCase("noise_patch_natural_depth", noise_patch_image(), (217,) + oc.ARGS_TAIL, None, lambda lv: lv["D"] == 5 and split_below_table(lv)),
        BCase("noise_67x67", noise(67, 67, 5), (60, 1.2, 2, 20, 7), None, lambda lv: lv["total"] > lv["N"]),
        BCase("noise_160x120", noise(160, 120, 6), (300, 1.2, 4, 20, 7), None, lambda lv: lv["total"] > lv["N"] and lv["D"] >= 4),
        BCase("noise_320x240_8_levels", noise(320, 240, 7), (1000, 1.2, 8, 20, 7), None, lambda lv: lv["total"] < lv["N"], level=7),
    ]
    return c


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}
