"""The bucket table of octree_buckets.py against DivideNode itself (octree_reference._divide, applied recursively): every cell's box
is the box the reference's node of the same path has, and every key lands in the cell whose path the reference's divides send it
down -- for odd and even boxes, boxes narrower than 2^D (repeated boundaries: empty cells) and several roots of non-integer width."""
import numpy as np
import pytest

import octree_buckets as ob
import octree_reference as ref

# (width, height) of the tree's area, i.e. level size minus 32
BOXES = [(67, 67), (100, 100), (321, 321), (100, 67), (67, 100), (608, 448), (321, 100), (5, 3), (1, 1), (13, 40), (288, 208)]
WIDE = [(100, 67, 1), (160 - 32, 96 - 32, 2), (250, 100, 2), (301, 100, 3), (288 - 32, 96 - 32, 4), (411, 100, 4), (70, 33, 2)]


def _reference_cells(ulx, brx, height, depth):
    """{code inside the root: (node, key indices)} after `depth` rounds of DivideNode on a root that holds every pixel as a key"""
    xs, ys = [], []
    for y in range(-2, height + 2):              # (a key may lie outside its root's box: roots are cut by float arithmetic)
        for x in range(ulx - 2, brx + 2):
            xs.append(float(x))
            ys.append(float(y))
    root = ref._Node(ulx, 0, brx, height)
    root.keys = list(range(len(xs)))
    level = {0: root}
    for _ in range(depth):
        nxt = {}
        for code, n in level.items():
            for q, c in enumerate(ref._divide(n, xs, ys)):
                nxt[4 * code + q] = c
        level = nxt
    return level, xs, ys


@pytest.mark.parametrize("depth", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("box", BOXES, ids=lambda b: "%dx%d" % b)
def test_cells_are_the_reference_nodes(box, depth):
    width, height = box
    if width * height > 20000 and depth > 3:
        depth = 4                       # (keeps the all-pixels reference of the large boxes quick; 4 is not otherwise in the list)
    xb, yb = ob.cell_bounds(0, width, depth), ob.cell_bounds(0, height, depth)
    assert xb[0] == 0 and xb[-1] == width and all(a <= b for a, b in zip(xb, xb[1:]))
    if width < (1 << depth):
        assert len(set(xb)) < len(xb)           # repeated boundaries
    cells, xs, ys = _reference_cells(0, width, height, depth)
    assert len(cells) == 4 ** depth
    for code, n in cells.items():
        assert ob.cell_box(code, xb, yb, depth) == (n.ulx, n.uly, n.brx, n.bry), code
        for k in n.keys:
            assert ob.cell_code(xs[k], ys[k], 0, xb, yb, depth) == code
    assert sum(len(n.keys) for n in cells.values()) == len(xs)


@pytest.mark.parametrize("case", WIDE, ids=lambda c: "%dx%d_%droots" % c)
def test_roots_of_non_integer_width(case):
    width, height, n_ini = case
    assert ob.n_roots(width, height) == n_ini
    depth = 3
    hx = ob.F32(width) / ob.F32(n_ini)
    boxes = ob.root_boxes(width, height)
    yb = ob.cell_bounds(0, height, depth)
    for r, (ulx, brx) in enumerate(boxes):
        assert (ulx, brx) == (int(hx * ob.F32(r)), int(hx * ob.F32(r + 1)))
        xb = ob.cell_bounds(ulx, brx, depth)
        cells, xs, ys = _reference_cells(ulx, brx, height, depth)
        for code, n in cells.items():
            assert ob.cell_box(code, xb, yb, depth) == (n.ulx, n.uly, n.brx, n.bry)
            for k in n.keys:
                assert ob.cell_code(xs[k], ys[k], r, xb, yb, depth) == (r << (2 * depth)) + code


def test_level_table_of_the_benchmark_frame():
    """640 x 480, 217 features at level 0: one root, D = 5, cells of 19 x 14 pixels"""
    d, n, xb, yb = ob.level_table(640, 480, 217)
    assert (d, n) == (5, 1) and xb.shape == (1, 33) and yb.shape == (33,)
    assert xb[0, 0] == 0 and xb[0, -1] == 608 and yb[-1] == 448
    assert set(np.diff(xb[0])) == {19} and set(np.diff(yb)) == {14}
    # the counters and the two coordinate maps fit the node pool that lends them its bytes
    assert 4 * (4 ** d + 1) + 2 * (608 + 448) <= ob.pool_bytes(217 + 16)


@pytest.mark.parametrize("nfeat,n_ini,expect", [(1, 1, 1), (4, 1, 2), (8, 1, 3), (40, 1, 4), (60, 1, 4), (217, 1, 5), (1000, 1, 6), (30, 2, 3), (100, 4, 4)])
def test_table_depth(nfeat, n_ini, expect):
    assert ob.table_depth(n_ini, nfeat) == expect
    assert ob.table_depth(n_ini, nfeat, 2) == min(expect, 2)


def test_maps_when_the_pool_is_small():
    """six features on 640 x 480: a pool of 22 nodes (1 352 bytes) holds the counters of 64 cells but not the maps (2 112 bytes)"""
    assert ob.pool_bytes(22) == 1352 and ob.table_depth(1, 6) == 3
    assert not ob.maps_in_lds(1, 6, 608, 448, 3)
    assert ob.maps_in_lds(1, 217, 608, 448, 5)


def test_levels_without_roots():
    assert ob.level_table(32, 200, 50)[:2] == (0, 0)            # no width
    assert ob.level_table(40, 400, 50)[:2] == (0, 0)            # round(8 / 368) = 0 roots
