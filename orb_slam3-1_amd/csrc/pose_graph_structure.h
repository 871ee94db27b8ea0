// The block structure of a pose graph's normal equations, as the assembly kernels of essential_graph.inc and
// essential_graph_4dof.inc take it.  Host only, standard library only (tests/pose_graph_structure_dump.cpp compiles it with g++).
//
// THE ORDER IS PART OF THE RESULT: an assembly kernel sums the records of a block in the order of blk_ent, so every bit of a
// solution depends on it.
//   * free vertices are numbered in vertex order (col[v]; -1: fixed);
//   * the n_free diagonal blocks come first, block c for free vertex c, then the off-diagonal blocks in ascending (row, column)
//     order with row > column;
//   * inside a block the entries are in edge order;
//   * an entry is 4 * edge + kind: 0 Hii, 1 Hjj (diagonal blocks), 2 Hij when col[i] > col[j], 3 its transpose otherwise;
//   * an edge between two fixed vertices contributes nothing, every duplicate of an edge contributes.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace pgraph {

struct Structure {
    std::vector<int> col;           // [n_vertices] index among the free vertices, -1: fixed
    std::vector<int> blk_i, blk_j;  // [blocks] block row / column (free-vertex indices, row >= column)
    std::vector<int> blk_off;       // [blocks + 1] into blk_ent
    std::vector<int> blk_ent;
    int n_free = 0;
};

inline Structure build_structure(int n_vertices, const uint8_t* fixed, int n_edges, const int* edge_vertices)
{
    Structure g;
    g.col.resize((size_t)n_vertices);
    for (int v = 0; v < n_vertices; v++) g.col[v] = fixed[v] ? -1 : g.n_free++;
    std::vector<std::vector<int>> diag((size_t)g.n_free);
    std::vector<std::pair<std::pair<int, int>, int>> off;       // ((row, column), entry)
    for (int e = 0; e < n_edges; e++) {
        const int ci = g.col[edge_vertices[2 * (size_t)e]], cj = g.col[edge_vertices[2 * (size_t)e + 1]];
        if (ci >= 0) diag[ci].push_back(4 * e);
        if (cj >= 0) diag[cj].push_back(4 * e + 1);
        if (ci >= 0 && cj >= 0) off.push_back(ci > cj ? std::make_pair(std::make_pair(ci, cj), 4 * e + 2) : std::make_pair(std::make_pair(cj, ci), 4 * e + 3));
    }
    std::stable_sort(off.begin(), off.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    for (int c = 0; c < g.n_free; c++) {
        g.blk_i.push_back(c); g.blk_j.push_back(c); g.blk_off.push_back((int)g.blk_ent.size());
        g.blk_ent.insert(g.blk_ent.end(), diag[c].begin(), diag[c].end());
    }
    for (size_t k = 0; k < off.size(); k++) {
        if (k == 0 || off[k].first != off[k - 1].first) { g.blk_i.push_back(off[k].first.first); g.blk_j.push_back(off[k].first.second); g.blk_off.push_back((int)g.blk_ent.size()); }
        g.blk_ent.push_back(off[k].second);
    }
    g.blk_off.push_back((int)g.blk_ent.size());
    return g;
}

}  // namespace pgraph
