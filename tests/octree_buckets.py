"""The octree's bucket table (k_octree: OctTabDesc, setup_geometry) restated in plain Python.

DistributeOctTree's splits are fixed before any key is looked at: a node's box depends only on its path from its root, every divide
cuts at ulx + ceil(w / 2) and uly + ceil(h / 2).  Applying that D times to a root gives 2^D columns and 2^D rows of cells; a key's
cell code is its root, then per depth (x >= midx) + 2 * (y >= midy), most significant depth first.  The device places every key
once by that code and divides nodes of depth < D by differences of the prefix sums over the cells."""
import numpy as np

F32 = np.float32
MAX_DEPTH = 6
POOL_EXTRA = 16
EDGE = 19


def cell_bounds(lo, hi, depth):
    """boundaries b[0 .. 2^depth] of the cells [lo, hi) is cut into; a box narrower than 2^depth repeats boundaries (empty cells)"""
    b = [0] * ((1 << depth) + 1)
    b[0], b[1 << depth] = lo, hi
    step = 1 << depth
    while step > 1:
        for i in range(0, 1 << depth, step):
            b[i + step // 2] = b[i] + -(-(b[i + step] - b[i]) // 2)
        step //= 2
    return b


def n_roots(width, height):
    return int(np.round(F32(width) / F32(height))) if height > 0 else 0


def root_boxes(width, height):
    """(ulx, brx) of the nIni roots (ORBextractor.cc:564-577), float32 arithmetic as the reference's"""
    n = n_roots(width, height)
    hx = F32(width) / F32(n)
    return [(int(hx * F32(i)), int(hx * F32(i + 1))) for i in range(n)]


def pool_bytes(pool):
    """bytes of the device's node pool, which lends the placement its counters"""
    return pool * (2 * 12 + 8 + 16 + 2 * 6) + ((pool + 15) & ~15)


def table_depth(n_ini, nfeat, depth_max=MAX_DEPTH):
    """the deepest table the level's budget can use (about four cells per feature) whose counters fit its node pool"""
    pool = pool_bytes(max(nfeat, 4 * n_ini) + POOL_EXTRA)
    d = 0
    while d < depth_max and (n_ini << (2 * d)) < 4 * nfeat and (n_ini << (2 * (d + 1))) <= 65536 and 4 * ((n_ini << (2 * (d + 1))) + 1) <= pool:
        d += 1
    return d


def maps_in_lds(n_ini, nfeat, width, height, depth):
    """do the two coordinate maps (2 bytes per column and row of the tree's area) fit the pool beside the counters?"""
    return 4 * ((n_ini << (2 * depth)) + 1) + 2 * (width + height) <= pool_bytes(max(nfeat, 4 * n_ini) + POOL_EXTRA)


def level_table(level_w, level_h, nfeat, depth_max=MAX_DEPTH):
    """(D, n_ini, x boundaries [n_ini][2^D + 1], y boundaries [2^D + 1]) of a pyramid level of level_w x level_h pixels"""
    width, height = level_w - 2 * (EDGE - 3), level_h - 2 * (EDGE - 3)
    n = max(n_roots(width, height), 0)
    if n < 1:
        return 0, 0, np.zeros((0, 2), np.int16), np.zeros(0, np.int16)
    d = table_depth(n, nfeat, depth_max)
    xb = np.array([cell_bounds(a, b, d) for a, b in root_boxes(width, height)], np.int16)
    return d, n, xb, np.array(cell_bounds(0, height, d), np.int16)


def cell_code(x, y, root, xb, yb, depth):
    ix = iy = 0
    code = root
    for d in range(depth - 1, -1, -1):
        bx = 1 if x >= xb[(2 * ix + 1) << d] else 0
        by = 1 if y >= yb[(2 * iy + 1) << d] else 0
        ix, iy, code = 2 * ix + bx, 2 * iy + by, 4 * code + bx + 2 * by
    return code


def cell_box(code, xb, yb, depth):
    """(ulx, uly, brx, bry) of the cell with this code inside its root"""
    ix = iy = 0
    for d in range(depth - 1, -1, -1):
        q = (code >> (2 * d)) & 3
        ix, iy = 2 * ix + (q & 1), 2 * iy + (q >> 1)
    return xb[ix], yb[iy], xb[ix + 1], yb[iy + 1]
