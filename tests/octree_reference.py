"""DistributeOctTree (ORBextractor.cc:555-779) restated in plain Python over a list of candidates, together with a TRACE of how the
device kernel (k_octree) walks the same computation: a pass of the reference's loops is cut into batches of up to 64 consecutive
list entries (first phase) or entries of the sorted to-expand vector (sorted phase), a lane per entry.  Inside a batch the nodes with
more than `small_max` keys (32, or 0 when at most 6 lanes are active) are the ONE-BY-ONE nodes: the whole wave takes them one at a
time, and with several waves per workgroup they are the PARTITION job that the waves share.

The trace holds, per batch: the phase, the active lanes, the key counts of the one-by-one nodes, the lane at which the list reached
N (sorted phase) and the rounds the batch needed because its children did not fit the free list of the N + 16 node pool.

std::sort is libstdc++'s introsort, restated here as well: the order of nodes that compare equal (same key count, same left edge)
is part of the result."""
import math

import numpy as np

F32 = np.float32
POOL_EXTRA = 16


# ---- libstdc++ std::sort (bits/stl_algo.h): introsort loop, median of three, unguarded partition, final insertion sort
def _std_sort(v, less):
    n = len(v)
    if n == 0:
        return

    def swap(a, b):
        v[a], v[b] = v[b], v[a]

    def median_to_first(result, a, b, c):
        if less(v[a], v[b]):
            if less(v[b], v[c]):
                swap(result, b)
            elif less(v[a], v[c]):
                swap(result, c)
            else:
                swap(result, a)
        elif less(v[a], v[c]):
            swap(result, a)
        elif less(v[b], v[c]):
            swap(result, c)
        else:
            swap(result, b)

    def partition(first, last, pivot):
        while True:
            while less(v[first], v[pivot]):
                first += 1
            last -= 1
            while less(v[pivot], v[last]):
                last -= 1
            if not first < last:
                return first
            swap(first, last)
            first += 1

    def loop(first, last, depth):
        while last - first > 16:
            if depth == 0:
                raise NotImplementedError("heapsort fallback of introsort: no case of this suite gets here")
            depth -= 1
            mid = first + (last - first) // 2
            median_to_first(first, first + 1, mid, last - 1)
            cut = partition(first + 1, last, first)
            loop(cut, last, depth)
            last = cut

    def linear_insert(last):
        val = v[last]
        nxt = last - 1
        while less(val, v[nxt]):
            v[last] = v[nxt]
            last = nxt
            nxt -= 1
        v[last] = val

    def insertion(first, last):
        for i in range(first + 1, last):
            if less(v[i], v[first]):
                val = v[i]
                v[first + 1:i + 1] = v[first:i]
                v[first] = val
            else:
                linear_insert(i)

    loop(0, n, 2 * int(math.floor(math.log2(n))))
    if n > 16:
        insertion(0, 16)
        for i in range(16, n):
            linear_insert(i)
    else:
        insertion(0, n)


class _Node:
    __slots__ = ("ulx", "uly", "brx", "bry", "keys", "no_more", "alive")

    def __init__(self, ulx, uly, brx, bry):
        self.ulx, self.uly, self.brx, self.bry = ulx, uly, brx, bry
        self.keys = []
        self.no_more = False
        self.alive = True


def _divide(p, xs, ys):
    half_x = -(-(p.brx - p.ulx) // 2)
    half_y = -(-(p.bry - p.uly) // 2)
    mx, my = p.ulx + half_x, p.uly + half_y
    c = [_Node(p.ulx, p.uly, mx, my), _Node(mx, p.uly, p.brx, my), _Node(p.ulx, my, mx, p.bry), _Node(mx, my, p.brx, p.bry)]
    for k in p.keys:
        if xs[k] < mx:
            c[0 if ys[k] < my else 2].keys.append(k)
        else:
            c[1 if ys[k] < my else 3].keys.append(k)
    for n in c:
        if len(n.keys) == 1:
            n.no_more = True
    return c


def _batch_record(phase, nodes, size, N, trace):
    """what the kernel does with one batch: nodes[l] is the node of lane l or None"""
    active = [n for n in nodes if n is not None]
    small_max = 0 if len(active) <= 6 else 32
    rec = {"phase": phase, "lanes": len(nodes), "active": len(active), "small_max": small_max,
           "one_by_one": [len(n.keys) for n in active if len(n.keys) > small_max],
           "one_by_one_lanes": [l for l, n in enumerate(nodes) if n is not None and len(n.keys) > small_max],
           "hit_lane": None, "rounds": 0, "empty_children": []}
    trace["batches"].append(rec)
    return rec


def distribute(x, y, resp, width, height, N):
    """x, y, resp: the level's candidates in vToDistributeKeys order, coordinates relative to the border (as the oracle's
    level_candidates returns them).  Returns (indices of the chosen candidates in list order, trace)."""
    xs = [float(v) for v in x]
    ys = [float(v) for v in y]
    trace = {"total": len(xs), "n_ini": 0, "empty_roots": 0, "passes": [], "batches": [], "sorted": False,
             "end": None, "first_pass_reached_n": False}
    if height <= 0:
        return [], trace
    n_ini = int(np.round(F32(width) / F32(height)))
    trace["n_ini"] = n_ini
    if n_ini <= 0 or not xs:
        return [], trace
    hx = F32(width) / F32(n_ini)
    roots = [_Node(int(hx * F32(i)), 0, int(hx * F32(i + 1)), height) for i in range(n_ini)]
    for k in range(len(xs)):
        roots[int(F32(xs[k]) / hx)].keys.append(k)
    lst = []                # front of the std::list is index 0
    for r in roots:
        if len(r.keys) == 1:
            r.no_more = True
        if r.keys:
            lst.append(r)
        else:
            trace["empty_roots"] += 1
    pool = max(N, 4 * n_ini) + POOL_EXTRA

    def rounds_needed(rec, parents, size_before):
        """the batch's children take their node slots before the parents return theirs: the longest prefix that fits, again and again"""
        nfree = pool - size_before
        i, rounds = 0, 0
        while i < len(parents):
            take, need = 0, 0
            while i + take < len(parents) and need + parents[i + take] <= nfree:
                need += parents[i + take]
                take += 1
            assert take > 0, "the pool cannot hold one node's children"
            nfree += take - need
            i += take
            rounds += 1
        rec["rounds"] = rounds

    finish = False
    while not finish:
        prev_size = len(lst)
        start = list(lst)                       # children pushed in front of the iterator are not visited by this pass
        expandable = []
        n_to_expand = 0
        pass_rec = {"phase": "first", "divided": [], "batches": 0, "one_by_one": 0}
        trace["passes"].append(pass_rec)
        for b0 in range(0, len(start), 64):
            lanes = [None if n.no_more else n for n in start[b0:b0 + 64]]
            if not any(n is not None for n in lanes):
                continue
            rec = _batch_record("first", lanes, len(lst), N, trace)
            pass_rec["batches"] += 1
            pass_rec["one_by_one"] += len(rec["one_by_one"])
            size_before, per_parent = len(lst), []
            for n in lanes:
                if n is None:
                    continue
                pass_rec["divided"].append(len(n.keys))
                ch = [c for c in _divide(n, xs, ys) if c.keys]
                rec["empty_children"].append(4 - len(ch))
                per_parent.append(len(ch))
                for c in ch:
                    lst.insert(0, c)
                    if len(c.keys) > 1:
                        n_to_expand += 1
                        expandable.append(c)
                n.alive = False
                lst.remove(n)
            rounds_needed(rec, per_parent, size_before)
        if len(lst) >= N or len(lst) == prev_size:
            finish = True
            trace["end"] = "n" if len(lst) >= N else "no_change"
            if len(lst) >= N:
                trace["first_pass_reached_n"] = True
        elif len(lst) + n_to_expand * 3 > N:
            trace["sorted"] = True
            while not finish:
                prev_size = len(lst)
                prev = expandable
                expandable = []
                _std_sort(prev, lambda a, b: (len(a.keys), a.ulx) < (len(b.keys), b.ulx))
                order = prev[::-1]              # for (j = size - 1; j >= 0; j--)
                pass_rec = {"phase": "sorted", "divided": [], "batches": 0, "one_by_one": 0}
                trace["passes"].append(pass_rec)
                reached = False
                for b0 in range(0, len(order), 64):
                    lanes = order[b0:b0 + 64]
                    rec = _batch_record("sorted", lanes, len(lst), N, trace)
                    pass_rec["batches"] += 1
                    pass_rec["one_by_one"] += len(rec["one_by_one"])
                    size_before, per_parent = len(lst), []
                    for l, n in enumerate(lanes):
                        pass_rec["divided"].append(len(n.keys))
                        ch = [c for c in _divide(n, xs, ys) if c.keys]
                        rec["empty_children"].append(4 - len(ch))
                        per_parent.append(len(ch))
                        for c in ch:
                            lst.insert(0, c)
                            if len(c.keys) > 1:
                                expandable.append(c)
                        lst.remove(n)
                        if len(lst) >= N:
                            rec["hit_lane"] = l
                            reached = True
                            break
                    rounds_needed(rec, per_parent, size_before)
                    if reached:
                        break
                if len(lst) >= N or len(lst) == prev_size:
                    finish = True
                    trace["end"] = "n" if len(lst) >= N else "no_change"
    out = []
    for n in lst:
        best = n.keys[0]
        for k in n.keys[1:]:
            if resp[k] > resp[best]:
                best = k
        out.append(best)
    trace["n_out"] = len(out)
    trace["ties"] = [i for i, n in enumerate(lst) if len(n.keys) > 1 and max(resp[k] for k in n.keys[1:]) == resp[n.keys[0]]
                     and resp[n.keys[0]] == max(resp[k] for k in n.keys)]
    return out, trace
