// orbx_device.h -- POD descriptors shared between the host driver and the gfx950 kernels.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/orbslam3_hip.h"

namespace orbx {

constexpr int kEdge = 19;          // EDGE_THRESHOLD   (reference src/ORBextractor.cc:73)
constexpr int kHalfPatch = 15;     // HALF_PATCH_SIZE  (:72)
constexpr int kPatch = 31;         // PATCH_SIZE       (:71)
constexpr int kMaxLevels = 16;
constexpr int kOctLogFactor = 6;     // octree push log capacity = 6 x node pool (<= 4 pushes per alive node between compactions)

// One pyramid level of one frame inside the per-frame pyramid buffer.
struct LevelDesc {
    int32_t w, h, stride;      // stride: bytes, multiple of 64
    int32_t nfeat;             // mnFeaturesPerLevel[level]
    int64_t off;               // byte offset inside the per-frame buffer, multiple of 64
    int32_t cell_begin, cell_count;   // range in the cell table
    int32_t cand_off, cand_cap;       // candidate slots of this level inside the per-frame candidate buffer
    int32_t sel_off, sel_cap;         // selected-keypoint slots (nfeat + 3)
    float scale;               // mvScaleFactor[level]
    int32_t patch_size;        // int(PATCH_SIZE * scale)   (:880)
};

// One FAST cell (reference :797-822): sub-image [x0,x1) x [y0,y1) in level coordinates.
struct CellDesc {
    int16_t level;
    int16_t x0, y0, x1, y1;
    int32_t slot_off, slot_cap;    // where this cell's keypoints go in the per-frame candidate buffer
};

// One level's quadtree bucket table (k_octree).  DistributeOctTree's splits are fixed before any key is looked at: a node's box
// depends only on its path from its root (halfX = ceil(w / 2)), so the cell a key reaches after `depth` divides is a function of
// its coordinates and these boundaries alone.  x boundaries: (2^depth + 1) per root, root after root; the y boundaries
// (2^depth + 1, every root spans the level's height) follow them.  Boundaries repeat where a box is narrower than 2^depth:
// such cells are empty, as the reference's empty children are.  Cell code of a key: its root, then per depth
// (x >= midx) + 2 * (y >= midy), most significant depth first.
constexpr int kOctTabMaxDepth = 6;   // (a node's depth takes three bits of its flags; 7 marks a node below the table)
struct OctTabDesc {
    int32_t depth, n_ini;
    int32_t bounds_off;            // first boundary of the level in the int16 boundary array
    int32_t prefix_off;            // the level's (n_ini << 2 depth) + 1 prefix sums inside the per-frame prefix buffer
    int32_t w_cell_inv, h_cell_inv;    // ceil(2^20 / FAST cell pitch): candidate order is (cell row, cell column, y, x), cell = (coordinate - 3) / pitch
    // The same table as two maps, so that a key finds its cell with two loads: per x (0 .. width) the root and the x bits of the cell
    // code in place, per y (0 .. height) the y bits; cell code = xmap[x] | ymap[y].  uint16 entries, x map first.
    int32_t map_off;
    int32_t maps_lds;              // the maps fit the node pool beside the counters: the kernel stages them in LDS
};

struct TileDesc {
    int16_t level, x0, y0;     // x0: a multiple of the tile width
    int16_t edge;              // bit 0: a stored output reads columns left of column 0, bit 1: right of the last column
};

// One destination row of the table-driven resize (k_resize, k_resize_tail): the two source rows clamped to the source image
// (sy0 | sy1 << 16) and the two vertical coefficients (0 .. 2048) shifted left by 12.  The host pads the table to whole tiles of
// 64 rows with copies of the last row, so that a thread reads its rows without a bound test.
// `plan` says which of the row's two source rows the previous destination row has filtered already, for a kernel that walks the
// rows in order and keeps the previous row's two horizontal results (resize_band): bits 0-1 the top row -- kResizeTopFresh, or
// the previous row's bottom / top source row; bit 2 (kResizeBottomIsTop) the bottom row is the top row, otherwise it is fresh.
// Computed on the clamped source rows.  resize_band reuses the previous BOTTOM row (five rows out of six at scale 1.2); the other
// two plans only arise where source rows are clamped, and it filters such a row again.
constexpr uint32_t kResizeTopFresh = 0, kResizeTopPrevBottom = 1, kResizeTopPrevTop = 2, kResizeBottomIsTop = 4;
constexpr int kResizeBand = 16;      // output rows a wave walks with the horizontal results in registers
struct __attribute__((aligned(16))) ResizeRow {
    uint32_t sy, b0, b1, plan;
};

// Workgroups are dispatched round-robin over the 8 XCDs, so workgroups b and b+8 share an L2 (MI355X_MICROARCH.md,
// "Workgroup dispatch").  With a grid of 8*chunk workgroups per frame this gives every XCD a contiguous run of `chunk` items
// (neighbouring items share image rows / 128-B lines: they stay in one L2); the run an XCD gets rotates with the frame, so
// that cheap and expensive runs (pyramid levels differ) spread evenly over the XCDs.  A speed-only mapping: any placement
// yields the same results.  The grid is padded to a multiple of 8 only -- empty workgroups still cost a dispatch slot, and the
// dispatcher starts only about two workgroups per nanosecond.
__host__ __device__ inline int xcd_grid(int n_items) { return 8 * ((n_items + 7) / 8); }
__host__ __device__ inline int xcd_remap(int block, int grid, int frame)
{
    const int chunk = grid >> 3;
    return (((block & 7) + frame) & 7) * chunk + (block >> 3);
}

// candidate / key record: x (12 bits), y (12 bits) relative to minBorder, FAST response (8 bits)
__host__ __device__ inline uint32_t pack_key(uint32_t x, uint32_t y, uint32_t resp) { return (x << 20) | (y << 8) | resp; }
__host__ __device__ inline uint32_t key_x(uint32_t e) { return e >> 20; }
__host__ __device__ inline uint32_t key_y(uint32_t e) { return (e >> 8) & 0xFFFu; }
__host__ __device__ inline uint32_t key_resp(uint32_t e) { return e & 0xFFu; }

}  // namespace orbx
