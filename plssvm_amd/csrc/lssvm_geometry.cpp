/*
 * lssvm_geometry.cpp -- the work-item geometry (lssvm_geometry.hpp): host code only, its own unit like capi_io.cpp.
 */
#include "lssvm_geometry.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <map>
#include <mutex>
#include <thread>
#include <tuple>

namespace lssvm {

/* ------------------------------------------------------------------ the row blocks of a rank ------------------------------------------------------------------ */
/* first row block of rank r when the lower triangle is dealt by equal area: tiles * sqrt(r / world), rounded to an EVEN block index -- the
 * 256-row workgroups of lssvm_tile_f32_pair.hip.hpp work on the block pairs (2p, 2p + 1), which must not straddle two devices (every symmetric
 * partition follows the rule, whichever kernel runs: one partition per problem shape) */
int sym_block_boundary(int num_tiles, int r, int world, const std::vector<double> *weights) {
    if (r <= 0) return 0;
    if (r >= world) return num_tiles;
    // the share of the triangle's AREA in front of rank r: r / world, or -- shard weights (lssvm_mi355_set_shard_weights: devices of unequal pace) -- the ranks' weights in front of it
    double share = static_cast<double>(r) / static_cast<double>(world);
    if (weights != nullptr && static_cast<int>(weights->size()) == world) {
        double before = 0.0, all = 0.0;
        for (int k = 0; k < world; ++k) {
            all += (*weights)[static_cast<size_t>(k)];
            if (k < r) before += (*weights)[static_cast<size_t>(k)];
        }
        share = before / all;
    }
    const int b = 2 * static_cast<int>(std::llround(0.5 * static_cast<double>(num_tiles) * std::sqrt(share)));
    return std::min(std::max(b, 0), num_tiles);
}

/* the row blocks [begin, end) of rank `rank`: equal (or weighted) AREAS of the lower triangle (symmetric variant: block ib costs ib + 1 tiles),
 * equal contiguous runs otherwise (every row costs the same, and the all-gather of the full-square variant needs equal slices: no weights there) */
void shard_blocks(int num_tiles, int world, int rank, bool symmetric, int &begin, int &end, const std::vector<double> *weights) {
    if (symmetric) {
        begin = sym_block_boundary(num_tiles, rank, world, weights);
        end = std::max(begin, sym_block_boundary(num_tiles, rank + 1, world, weights));
    } else {
        const int per_rank = (num_tiles + world - 1) / world;
        begin = std::min(rank * per_rank, num_tiles);
        end = std::min(begin + per_rank, num_tiles);
    }
}

/* ------------------------------------------------------------------ work-item geometry of the symmetric variant ------------------------------------------------------------------ */
/* Row-block BANDS of equal triangle AREA whose column-sum records fit the slab budget (see Problem<T>::build_shard_lists). */
std::vector<int> band_edges(int ib_begin, int ib_end_all, size_t real_size, const GeometryOptions &o) {
    const double rec_bytes = static_cast<double>(TILE) * real_size;
    const double total_bytes = static_cast<double>(pairs_below(ib_end_all) - pairs_below(ib_begin)) * rec_bytes;
    const double band_bytes = static_cast<double>(std::min(std::max<int64_t>(o.colslab_band_mb, 1), o.colslab_limit_mb)) * 1048576.0;
    const int nbands = static_cast<int>(std::min<double>(std::max(1.0, std::ceil(total_bytes / band_bytes)), std::max(ib_end_all - ib_begin, 1)));
    // equal areas: band k of this device ends where the triangle area reaches (k + 1) / nbands of the device's share
    const double a0 = static_cast<double>(ib_begin) * ib_begin, a1 = static_cast<double>(ib_end_all) * ib_end_all;
    std::vector<int> edge(nbands + 1, ib_begin);
    for (int k = 1; k < nbands; ++k) {
        const int e = 2 * static_cast<int>(std::llround(0.5 * std::sqrt(a0 + (a1 - a0) * static_cast<double>(k) / nbands)));  // even: a block pair stays in one band
        edge[k] = std::min<int>(std::max(e, edge[k - 1]), ib_end_all);
    }
    edge[nbands] = ib_end_all;
    return edge;
}

/* The work items of a launch, given chunk by chunk, in XCD-LANE order: list position 8 k + x belongs to lane x (the persistent workgroups of XCD x draw from it first,
 * for_each_work_item; the hardware's own deal is round-robin too), and a lane works through one UNIT -- a run of items of ONE column chunk -- at a time, the units dealt
 * to the lanes as they run dry.  Round 6: a unit used to be a whole chunk.  A lane that found no chunk left gave its list positions to the others, which shifts every
 * later item to another lane: with FEWER CHUNKS THAN A FEW PER LANE the mapping was scrambled for most of the list -- predict_values at 200 000 x 50 000 has 7 chunks for
 * 8 lanes: L2 hit rate 0.19, 17 GB of fabric reads per 5 ms launch (profiles/r06_pmc_predict.txt); 50 000 x 128 training: 8 chunks of unequal length, 0.77.  Now a launch
 * of fewer than 64 chunks cuts its chunks into pieces (of at least 32 items: the CUs of one XCD) so that there are about 64 units: the lanes stay aligned until the last
 * unit of the list.  Launches of 64 chunks and more (1 000 000 x 128: 123 per band) are dealt as before. */
std::vector<WorkItem> xcd_lane_order(const std::vector<std::vector<WorkItem>> &by_chunk) {
    size_t total = 0;
    for (const auto &c : by_chunk) total += c.size();
    const size_t pieces = by_chunk.size() < 64 ? (64 + by_chunk.size() - 1) / std::max<size_t>(by_chunk.size(), 1) : 1;
    struct Unit {
        const WorkItem *begin;
        size_t count;
    };
    std::vector<Unit> units;
    for (const auto &c : by_chunk) {
        if (c.empty()) continue;
        const size_t n_pieces = std::max<size_t>(1, std::min(pieces, c.size() / 32));
        for (size_t k = 0; k < n_pieces; ++k) {
            const size_t lo = c.size() * k / n_pieces, hi = c.size() * (k + 1) / n_pieces;
            units.push_back({ c.data() + lo, hi - lo });
        }
    }
    std::vector<WorkItem> out;
    out.reserve(total);
    size_t next_unit = 0;
    std::vector<long> lane_unit(8, -1);  // -1: none yet, -2: the list of units is exhausted
    std::vector<size_t> lane_pos(8, 0);
    while (out.size() < total) {
        for (int x = 0; x < 8 && out.size() < total; ++x) {
            while (lane_unit[x] == -1 || (lane_unit[x] >= 0 && lane_pos[x] >= units[static_cast<size_t>(lane_unit[x])].count)) {
                if (next_unit >= units.size()) {
                    lane_unit[x] = -2;
                    break;
                }
                lane_unit[x] = static_cast<long>(next_unit++);
                lane_pos[x] = 0;
            }
            if (lane_unit[x] == -2) continue;  // (this lane has run out of units: its positions go to the others -- the last round of the list only)
            out.push_back(units[static_cast<size_t>(lane_unit[x])].begin[lane_pos[x]++]);
        }
    }
    return out;
}

/* The (row block, column chunk) work items of one band in DISPATCH order: column chunk major (concurrent workgroups share the chunk; the
   hardware dispatches workgroups in item order as CU slots free up).  order >= 1 (ITEM_ORDER): the items cut short by the diagonal go last in
   their band, longest first, so that the final dispatch round is made of the shortest items.  .x = absolute row block, .y = chunk. */
std::vector<WorkItem> band_items(int band_begin, int band_end, int jc_tiles, int num_jc, int order, bool pairs, int head_tiles, int head_count) {
    std::vector<WorkItem> full, cut;
    auto cbegin = [&](int jc) { return chunk_begin(jc, jc_tiles, head_tiles, head_count); };
    auto clen = [&](int jc) { return chunk_len(jc, jc_tiles, head_tiles, head_count); };
    const int rows = pairs ? 2 : 1;  // row blocks per work item: block pairs (2p, 2p + 1) for the 256-row workgroups (.x = the even block; the band edges are even)
    const int nrow_items = (band_end - band_begin + rows - 1) / rows;
    if (order >= 4) {
        // ROW-GROUP major, for the kernels that re-load their row panel at every tile (panels inside a tile): the 64 workgroups an XCD runs at a time
        // are the items of a GROUP of row blocks x their column chunks, so that the row panels they keep re-reading fit that XCD's L2 (with the
        // column-chunk major orders every concurrent workgroup has a row panel of its own: 60 000 x 640 rbf re-read 54 GB of row planes per matvec
        // from beyond L2) and a column tile is streamed for the whole group at once.  List position 8 k + x belongs to XCD x: runs of 64 consecutive items of the
        // sequence go to one lane.
        std::vector<WorkItem> seq;
        const int GROUP = order == 4 ? 4 : (order == 5 ? 2 : (order == 6 ? 8 : 1));  // (4 and 5 ship; 6, 7: development builds, item_order_dev)
        for (int g0 = 0; g0 < nrow_items; g0 += GROUP) {
            for (int jc = 0; jc < num_jc; ++jc) {
                for (int k = g0; k < std::min(g0 + GROUP, nrow_items); ++k) {
                    const int ib = band_begin + rows * k;
                    if (cbegin(jc) > ib + rows - 1) continue;
                    seq.push_back({ ib, jc });
                }
            }
        }
        std::vector<std::vector<WorkItem>> lane(8);
        for (size_t i = 0; i < seq.size(); ++i) lane[(i / 64) % 8].push_back(seq[i]);
        std::vector<WorkItem> out;
        out.reserve(seq.size());
        std::vector<size_t> pos(8, 0);
        while (out.size() < seq.size()) {
            for (int x = 0; x < 8; ++x) {
                if (pos[x] < lane[x].size()) out.push_back(lane[x][pos[x]++]);
            }
        }
        return out;
    }
    for (int jc = 0; jc < num_jc; ++jc) {
        for (int k = 0; k < nrow_items; ++k) {
            const int ib = band_begin + rows * (order == 2 ? nrow_items - 1 - k : k);
            const int last = ib + rows - 1;  // the item's tiles end at the diagonal of its LAST block
            if (cbegin(jc) > last) continue;
            const bool is_cut = cbegin(jc) + clen(jc) > last + 1 || clen(jc) < jc_tiles;  // fewer than jc_tiles tiles: cut by the diagonal, or a chunk of the short head
            (order >= 1 && is_cut ? cut : full).push_back({ ib, jc });
        }
    }
    auto item_tiles = [&](const WorkItem &it) { return std::min(cbegin(it.y) + clen(it.y), it.x + rows) - cbegin(it.y); };
    std::stable_sort(cut.begin(), cut.end(), [&](const WorkItem &x, const WorkItem &y) { return item_tiles(x) > item_tiles(y); });
    if (order == 3) {
        // XCD-aware: the hardware deals consecutive workgroups round-robin over the 8 XCDs (observed, a speed matter only), each with an L2 of its own.
        // In column-chunk major order the workgroups that stream one chunk are spread over all eight L2s, which each fetch it from the fabric; here list
        // position 8 k + x belongs to "lane" x, and a lane works through ONE column chunk at a time, so that an XCD's workgroups share their column
        // stream in ITS L2 (xcd_lane_order above).
        std::vector<std::vector<WorkItem>> by_chunk(static_cast<size_t>(num_jc));
        for (const WorkItem &it : full) by_chunk[static_cast<size_t>(it.y)].push_back(it);
        full = xcd_lane_order(by_chunk);
    }
    full.insert(full.end(), cut.begin(), cut.end());
    return full;
}

/* ------------------------------------------------------------------ column chunks ------------------------------------------------------------------ */
/* Chunk length of the 256-row workgroups (block pairs) when the launch is SMALL: one workgroup per CU means 256 slots, and a problem of 20 000
 * points has only ~6 000 pair-tiles -- whether the items come out as 0.9 or 1.6 or 8 rounds over the slots decides the launch time (measured at
 * 20 000 x 128: 0.186 ms with 3-tile items, 0.144 with 16, 0.136 with 32; 10 000 points: 0.070 / 0.049 with 2 / 8 tiles;
 * profiles/r04_chunk_sweep_pair.log).  The host therefore replays the hardware's dispatch (items in list order onto the slot that frees up
 * first) for a handful of candidate lengths with the cost model  item = tiles + 2.6  (the work-item prologue and tail in tile units, fitted to
 * that sweep) and takes the shortest makespan.  Large launches (more than 16 items per slot at the longest chunk) keep the longest chunk. */
int num_chunks(int num_tiles, int tiles, int head_tiles, int head_count) {
    const int head = head_count * head_tiles;
    return head_count + (std::max(num_tiles - head, 0) + tiles - 1) / tiles;
}
/* Round 5: the replay also tries a HEAD of short chunks -- the first `head_count` column chunks of every row pair have `head_tiles` tiles -- whose items are
 * dispatched last, longest first, together with the items cut short by the diagonal: long items for the bulk of a launch (fewer row-panel loads), short ones
 * to fill its end.  Searched where a launch is a few rounds long (at most 8 items per slot at the longest chunk: that is where the last round
 * decides; ADVICE r04: no long replays of large launches); a fixed head of two 16-tile chunks up to 32 items per slot, none beyond.
 * MEASURED, same box, against the replay's best uniform length (option j_chunk_head = 0):
 *   - with one workgroup per item, dealt by the hardware (profiles/r05_ab_chunk_head.log): -2.5 % at 40 000 points, -1 % at 70 000, but +2.5 % at 30 000 and +1 % at
 *     50 000 -- a wash: that deal is in order and static per XCD (tests/tools/item_trace.py: CUs wait 8 ... 40 us in front of the short items, and the launch ends
 *     with its slowest XCD whatever the items);
 *   - with the PERSISTENT launches that draw their items from per-XCD counters (pair_queue_fetch; profiles/r05_queue_chunk_sweep.log, r05_queue_head_large.log):
 *     -5.4 % at 20 000 points, -4.5 % at 30 000, -3.5 % at 40 000, -2.6 % at 50 000, -0.9 % at 70 000, -1.6 % at 100 000, -1.0 % at 150 000, nothing at 250 000.
 * So heads are the default since the launches are persistent. */
/* The replay is a pure function of the shard's shape and three options, and it costs 1.6 of the 4 ms a 50 000-point problem takes to set up: a process that creates
 * problems of one shape again and again (a parameter search over C and gamma, predict after train) replays once. */
PairChunks choose_pair_chunk(int ib_begin, int ib_end, int num_tiles, size_t real_size, const GeometryOptions &o, int slots) {
    using Key = std::tuple<int, int, int, size_t, int, int64_t, int64_t, int64_t>;
    static std::mutex cache_mutex;
    static std::map<Key, PairChunks> cache;
    const Key key{ ib_begin, ib_end, num_tiles, real_size, slots, o.j_chunk_head, o.colslab_band_mb, o.colslab_limit_mb };
    {
        const std::lock_guard<std::mutex> lock(cache_mutex);
        if (const auto it = cache.find(key); it != cache.end()) return it->second;
    }
    const PairChunks chosen = choose_pair_chunk_by_replay(ib_begin, ib_end, num_tiles, real_size, o, slots);
    const std::lock_guard<std::mutex> lock(cache_mutex);
    if (cache.size() >= 4096) cache.clear();  // (bounded: shapes, not problems)
    cache.emplace(key, chosen);
    return chosen;
}
PairChunks choose_pair_chunk_by_replay(int ib_begin, int ib_end, int num_tiles, size_t real_size, const GeometryOptions &o, int slots) {
    const int cap = 64;
    PairChunks best_c;
    const long area = triangle_tiles(ib_begin, ib_end) / 2;  // pair-tiles, about
    if (area / cap > 16L * slots) {  // (beyond ~16 dispatch rounds the last round no longer decides, and the replay itself costs: 16 of 27 ms of set-up at 250 000 points)
        if (o.j_chunk_head == 1 && area / cap <= 32L * slots && num_tiles > 2 * 16 + cap) {
            best_c.head_tiles = 16;
            best_c.head_count = 2;
        }
        return best_c;
    }
    const std::vector<int> edge = band_edges(ib_begin, ib_end, real_size, o);
    const bool few_rounds = area / cap <= 8L * slots && edge.size() == 2;
    const double item_cost = 2.6;  // (with the persistent launches a traced item costs 1.2 tiles beside its tiles -- tests/tools/item_trace.py --; replays with 1.2 and 0.6 choose within
                                   // 1 % of this one, 2.6 a little better from 70 000 points on: profiles/r05_queue_chunk_sweep.log)
    struct Candidate {
        int jc, head_tiles, head_count;
        double makespan;
    };
    auto replay = [&](Candidate &c) {  // (a pure function of the candidate: the replays run side by side below)
        const int num_jc = num_chunks(num_tiles, c.jc, c.head_tiles, c.head_count);
        double total = 0.0;
        for (size_t k = 0; k + 1 < edge.size(); ++k) {
            if (edge[k + 1] <= edge[k]) continue;
            std::vector<double> slot(static_cast<size_t>(slots), 0.0);  // a min-heap of the slots' finish times
            auto later = [](double x, double y) { return x > y; };
            for (const WorkItem &it : band_items(edge[k], edge[k + 1], c.jc, num_jc, ITEM_ORDER, true, c.head_tiles, c.head_count)) {
                const int b = chunk_begin(it.y, c.jc, c.head_tiles, c.head_count);
                const int tiles = std::min(std::min(b + chunk_len(it.y, c.jc, c.head_tiles, c.head_count), it.x + 2), num_tiles) - b;
                std::pop_heap(slot.begin(), slot.end(), later);
                slot.back() += static_cast<double>(std::max(tiles, 0)) + item_cost;
                std::push_heap(slot.begin(), slot.end(), later);
            }
            total += *std::max_element(slot.begin(), slot.end());
        }
        c.makespan = total;
    };
    std::vector<Candidate> cands;
    for (const int jc : { 2, 3, 4, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64 }) cands.push_back({ jc, 0, 0, 0.0 });
    if (!few_rounds && o.j_chunk_head == 1 && edge.size() == 2) {
        for (const int jc : { 48, 64 }) {
            if (2 * 16 + jc <= num_tiles) cands.push_back({ jc, 16, 2, 0.0 });
        }
    }
    if (few_rounds && o.j_chunk_head == 1) {
        for (const int jc : { 24, 32, 40, 48, 56, 64 }) {
            for (const int hc : { 1, 2, 3, 4, 6, 8 }) {
                for (const int ht : { 4, 8, 12, 16, 20, 24 }) {
                    if (ht >= jc || hc * ht + jc > num_tiles) continue;
                    cands.push_back({ jc, ht, hc, 0.0 });
                }
            }
        }
    }
    // some 230 replays of a thousand items each: 8 ms of the set-up of a 50 000-point problem on one thread (a problem that iterates in 0.7 ms), 1 ms on eight; the
    // choice -- the first candidate of the list with the shortest makespan -- does not depend on how the replays are spread
    const unsigned nthreads = cands.size() >= 32 ? std::min(8u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
    std::atomic<size_t> next{ 0 };
    auto worker = [&] {
        for (size_t k = next.fetch_add(1); k < cands.size(); k = next.fetch_add(1)) replay(cands[k]);
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nthreads; ++t) pool.emplace_back(worker);
    worker();
    for (std::thread &t : pool) t.join();
    const Candidate *best = &cands[0];
    for (const Candidate &c : cands) {
        if (c.makespan < best->makespan) best = &c;
    }
    best_c.tiles = best->jc;
    best_c.head_tiles = best->head_count > 0 ? best->head_tiles : 0;
    best_c.head_count = best->head_count;
    return best_c;
}

/* The column chunks of a training shard -- the row blocks [ib_begin, ib_end) of `num_tiles`, symmetric (`sym`) or full square: option j_chunk_tiles, or automatically
 * by the path (`split`: the fp32 split kernels, `pair`: 256-row workgroups on `slots` CUs, `wide_nl`: panels inside a tile); the head of the 256-row workgroups. */
PairChunks shard_chunks(const GeometryOptions &o, int ib_begin, int ib_end, int num_tiles, size_t real_size, bool sym, bool split, bool pair, bool wide_nl, int slots) {
    PairChunks c;
    if (o.j_chunk_tiles > 0) {
        c.tiles = static_cast<int>(o.j_chunk_tiles);
    } else {
        // automatic: long chunks amortise a work item's prologue (row panel load) and keep its row sums in registers, but the grid
        // must fill 256 CUs x 2 workgroups several times over.  Measured optimum (tests/tools/gpu_probe.py --small, 3 000 ... 50 000
        // points): about 4096 work items, between 2 and 16 tiles each.
        const long area = sym ? triangle_tiles(ib_begin, ib_end) : static_cast<long>(ib_end - ib_begin) * num_tiles;
        // the bf16x6 kernel has the costlier work-item prologue (three planes of the row panel) and the faster tiles: longer chunks
        // (measured 16 -> 64 tiles: +1.5 % at 100 000 points, +2 % at 300 000; the native kernels are flat or lose beyond 16)
        const long cap = split ? 64 : 16;
        c.tiles = static_cast<int>(std::min<long>(cap, std::max<long>(2, (area + 2048) / 4096)));
        if (pair) c = choose_pair_chunk(ib_begin, ib_end, num_tiles, real_size, o, slots);
        // panels inside a tile, symmetric variant: SHORT items in row-group major order (Problem<T>::wide_order_) -- the shorter the better at every shape
        // (12 > 8 > 4 > 2 tiles, profiles/r04_ab_wide_item_order_groups.log, r04_ab_wide_final.log); longer only where the partial slabs would grow
        // beyond 256 per row
        if (wide_nl && sym) c.tiles = static_cast<int>(std::min<long>(64, std::max<long>(2, (num_tiles + 255) / 256)));
    }
    if (pair && o.j_chunk_head >= 1024) {  // an explicit head (option j_chunk_head = 1024 count + tiles): tests, A/B runs
        c.head_count = static_cast<int>(o.j_chunk_head / 1024);
        c.head_tiles = static_cast<int>(o.j_chunk_head % 1024);
        if (c.head_count <= 0 || c.head_tiles <= 0 || c.head_count * c.head_tiles >= num_tiles) c.head_count = c.head_tiles = 0;
    }
    if (!pair) c.head_count = c.head_tiles = 0;
    return c;
}

/* column tiles per work item of a rectangular product of num_ib row blocks x num_jt column tiles: the option, or automatically about 4096 work items (as
 * shard_chunks); 256-row items (`rect`): about eight per CU, at most 64 tiles */
int product_chunk_tiles(const GeometryOptions &o, bool rect, int num_ib, int num_jt) {
    long tiles = static_cast<long>(o.j_chunk_tiles);
    if (tiles <= 0) {
        tiles = rect ? std::min<long>(64, std::max<long>(4, (static_cast<long>(num_ib / 2) * num_jt + 1024) / 2048))
                     : std::min<long>(16, std::max<long>(2, (static_cast<long>(num_ib) * num_jt + 2048) / 4096));
    }
    return static_cast<int>(tiles);
}

}  // namespace lssvm
