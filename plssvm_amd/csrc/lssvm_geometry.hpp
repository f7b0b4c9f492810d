/*
 * lssvm_geometry.hpp -- which tiles of the implicit matrix are evaluated, by whom and in what order: the row blocks of a rank, the row-block bands, the column chunks
 * and the work items of a launch.  Integer arithmetic on the host (lssvm_geometry.cpp; no HIP header, no device: tests/cpp/test_geometry_sanitized.cpp drives it on the
 * CPU); chunk_begin / chunk_len are shared with the kernels.
 */
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define LSSVM_HOST_DEVICE __host__ __device__
#else
#define LSSVM_HOST_DEVICE
#endif

namespace lssvm {

constexpr int TILE = 128;                     // rows / columns of one workgroup tile of the implicit matrix
constexpr int ITEM_ORDER = 3;                 // symmetric variant: the work items of a column chunk on ONE XCD at a time (list position 8 k + x = lane x; the hardware deals
                                              // workgroups round-robin over the 8 XCDs), the items cut short by the diagonal last, longest first.  Against plain
                                              // column-chunk major order (1): bit-identical results, fabric traffic 116 -> 97 GB per matvec at 1 000 000 x 128, time -0.3 %
                                              // (profiles/r04_ab_xcd_item_order.log)

/* a work item of a launch: .x = row block (the even block of a pair), .y = column chunk.  The kernels read the list as int2 (Problem<T>::build_shard_lists checks the layout) */
struct WorkItem {
    int x, y;
};

/* the option values the geometry reads (Options, lssvm_problem.hip.hpp: geometry_options) */
struct GeometryOptions {
    int64_t j_chunk_tiles, j_chunk_head, colslab_band_mb, colslab_limit_mb;
};

/* column chunk jc of a launch covers the tiles [chunk_begin, chunk_begin + chunk_len): a head of `head_count` short chunks, then chunks of `tiles` */
LSSVM_HOST_DEVICE inline int chunk_begin(int jc, int tiles, int head_tiles, int head_count) {
    return jc < head_count ? jc * head_tiles : head_count * head_tiles + (jc - head_count) * tiles;
}
LSSVM_HOST_DEVICE inline int chunk_len(int jc, int tiles, int head_tiles, int head_count) { return jc < head_count ? head_tiles : tiles; }
int num_chunks(int num_tiles, int tiles, int head_tiles, int head_count);

int sym_block_boundary(int num_tiles, int r, int world, const std::vector<double> *weights = nullptr);
void shard_blocks(int num_tiles, int world, int rank, bool symmetric, int &begin, int &end, const std::vector<double> *weights = nullptr);

inline long pairs_below(long b) { return b * (b - 1) / 2; }
/* tiles on and below the diagonal in the row blocks [ib_begin, ib_end): block ib has ib + 1 */
inline long triangle_tiles(long ib_begin, long ib_end) { return (ib_end * (ib_end + 1) - ib_begin * (ib_begin + 1)) / 2; }
std::vector<int> band_edges(int ib_begin, int ib_end_all, size_t real_size, const GeometryOptions &o);

std::vector<WorkItem> xcd_lane_order(const std::vector<std::vector<WorkItem>> &by_chunk);
std::vector<WorkItem> band_items(int band_begin, int band_end, int jc_tiles, int num_jc, int order, bool pairs, int head_tiles = 0, int head_count = 0);

struct PairChunks {
    int tiles = 64, head_tiles = 0, head_count = 0;
};
PairChunks choose_pair_chunk(int ib_begin, int ib_end, int num_tiles, size_t real_size, const GeometryOptions &o, int slots);
PairChunks choose_pair_chunk_by_replay(int ib_begin, int ib_end, int num_tiles, size_t real_size, const GeometryOptions &o, int slots);

PairChunks shard_chunks(const GeometryOptions &o, int ib_begin, int ib_end, int num_tiles, size_t real_size, bool sym, bool split, bool pair, bool wide_nl, int slots);
int product_chunk_tiles(const GeometryOptions &o, bool rect, int num_ib, int num_jt);

}  // namespace lssvm
