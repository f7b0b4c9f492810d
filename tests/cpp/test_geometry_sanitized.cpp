/*
 * test_geometry_sanitized.cpp -- the work-item geometry (plssvm_amd/csrc/lssvm_geometry.cpp) on the CPU, g++ -fsanitize=address,undefined: which tiles of the implicit
 * matrix are evaluated, by whom and in what order.  A mistake there is a silently wrong K*v -- a tile left out, a tile counted twice, a block pair split across two
 * bands or two ranks.  Two parts:
 *   - invariants over the argument domain the callers produce (jc_tiles >= 1; a head with head_count * head_tiles < num_tiles, or none; even band edges; slots >= 1):
 *     the chunks tile [0, num_tiles); the ranks partition the row blocks at even boundaries; the bands partition a rank's blocks at even edges; the items of a band
 *     cover every row's tiles [0, min(ib + rows, num_tiles)) exactly once in every order (the tile behind an odd last block is padding: the kernels cut at num_tiles);
 *     xcd_lane_order permutes; the replayed chunk choice is in range, fits and is what the cache returns;
 *   - a characterisation: `--dump` prints one line per case of a fixed table (inputs -> row blocks, band edges, chunk choice, item count, FNV-1a hash of the item
 *     list); the default mode compares it with tests/golden/geometry_cases.txt (`--golden PATH`), which was recorded from the functions as they stood inside
 *     lssvm_problem.hip / lssvm_predict.hip before they became a unit of their own.
 * The item checks dedupe bands by (begin, end) and take the shards of one world per tile count, 1 ... 16 in turn (the large tile counts: three ranks of sixteen, and
 * three bands of the whole triangle of 7813 blocks at the default budget; a head with block pairs, none without), so that the run stays at a few seconds under ASan.
 * Exit code 0 = every check held, the dump equals the golden file, and the sanitizers stayed silent.
 */
#include "../../plssvm_amd/csrc/lssvm_geometry.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

using namespace lssvm;

static int failures = 0;
#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond)) {                                                      \
            if (++failures <= 20) {                                         \
                std::fprintf(stderr, "FAILED %s (line %d): ", #cond, __LINE__); \
                std::fprintf(stderr, __VA_ARGS__);                          \
                std::fprintf(stderr, "\n");                                 \
            }                                                               \
        }                                                                   \
    } while (0)

static std::vector<int> tile_counts() {
    std::vector<int> v;
    for (int n = 1; n <= 200; ++n) v.push_back(n);
    for (const int n : { 391, 782, 1954, 7813 }) v.push_back(n);
    return v;
}
struct Head {
    int count, tiles;
};
static const Head HEADS[] = { { 0, 0 }, { 1, 4 }, { 2, 16 }, { 3, 8 }, { 4, 1 }, { 6, 12 }, { 8, 24 } };
static const int CHUNK_TILES[] = { 1, 2, 3, 4, 5, 7, 8, 12, 16, 24, 31, 32, 48, 63, 64 };
static bool head_fits(const Head &h, int num_tiles) { return h.count == 0 || h.count * h.tiles < num_tiles; }

/* weights of a world: mode 0 none, 1 equal, 2 unequal */
static std::vector<double> shard_weights(int world, int mode) {
    std::vector<double> w;
    for (int k = 0; mode != 0 && k < world; ++k) w.push_back(mode == 1 ? 2.5 : 1.0 + 0.25 * ((k * 7 + 3) % 5));
    return w;
}
static constexpr int64_t DEFAULT_BAND_MB = 2048, DEFAULT_LIMIT_MB = 98304;  // (Options' defaults)
static GeometryOptions geometry(int64_t band_mb, int64_t j_chunk_head = 1, int64_t j_chunk_tiles = 0) { return { j_chunk_tiles, j_chunk_head, band_mb, DEFAULT_LIMIT_MB }; }

/* ------------------------------------------------------------------ chunks ------------------------------------------------------------------ */
static void check_chunks() {
    for (const int nt : tile_counts()) {
        for (const int tiles : CHUNK_TILES) {
            for (const Head &h : HEADS) {
                if (!head_fits(h, nt)) continue;
                const int n = num_chunks(nt, tiles, h.tiles, h.count);
                int pos = 0;
                for (int jc = 0; jc < n; ++jc) {
                    const int b = chunk_begin(jc, tiles, h.tiles, h.count), len = chunk_len(jc, tiles, h.tiles, h.count);
                    CHECK(b == pos && len >= 1 && b < nt, "chunk %d of %d: begin %d (expected %d), length %d; %d tiles, chunks of %d, head %d x %d", jc, n, b, pos, len, nt, tiles, h.count, h.tiles);
                    pos = b + len;
                }
                CHECK(pos >= nt, "%d chunks end at %d of %d tiles; chunks of %d, head %d x %d", n, pos, nt, tiles, h.count, h.tiles);
            }
        }
    }
}

/* ------------------------------------------------------------------ shards ------------------------------------------------------------------ */
struct Range {
    int begin, end;
};
static std::vector<Range> shard_ranges(int nt, int world, bool sym, int wmode) {
    const std::vector<double> w = shard_weights(world, wmode);
    std::vector<Range> r(static_cast<size_t>(world));
    for (int k = 0; k < world; ++k) shard_blocks(nt, world, k, sym, r[static_cast<size_t>(k)].begin, r[static_cast<size_t>(k)].end, wmode != 0 ? &w : nullptr);
    return r;
}
static void check_shards() {
    for (const int nt : tile_counts()) {
        for (int world = 1; world <= 16; ++world) {
            for (int wmode = 0; wmode < 3; ++wmode) {
                for (const bool sym : { true, false }) {
                    const std::vector<Range> r = shard_ranges(nt, world, sym, wmode);
                    int pos = 0;
                    for (int k = 0; k < world; ++k) {
                        const Range &s = r[static_cast<size_t>(k)];
                        CHECK(s.begin == pos && s.end >= s.begin, "rank %d of %d: [%d, %d) after %d; %d tiles, symmetric %d, weights %d", k, world, s.begin, s.end, pos, nt, sym, wmode);
                        pos = s.end;
                        if (sym) {
                            CHECK(s.begin % 2 == 0 || s.begin == nt, "rank %d of %d begins at the odd block %d of %d, weights %d", k, world, s.begin, nt, wmode);
                        } else {
                            const int per_rank = (nt + world - 1) / world;  // the ceil-sized runs, whatever the weights
                            CHECK(s.begin == std::min(k * per_rank, nt) && s.end == std::min(s.begin + per_rank, nt), "rank %d of %d: [%d, %d), %d tiles", k, world, s.begin, s.end, nt);
                        }
                    }
                    CHECK(pos == nt, "the ranks of %d end at %d of %d; symmetric %d, weights %d", world, pos, nt, sym, wmode);
                    if (wmode == 1) {  // equal weights are no weights
                        const std::vector<Range> plain = shard_ranges(nt, world, sym, 0);
                        for (int k = 0; k < world; ++k) CHECK(plain[static_cast<size_t>(k)].begin == r[static_cast<size_t>(k)].begin, "rank %d of %d, %d tiles, symmetric %d", k, world, nt, sym);
                    }
                }
            }
        }
    }
}

/* ------------------------------------------------------------------ bands ------------------------------------------------------------------ */
static void check_band_edges(const std::vector<int> &edge, int ib_begin, int ib_end, size_t real_size, int64_t band_mb) {
    CHECK(edge.size() >= 2 && edge.front() == ib_begin && edge.back() == ib_end, "%zu edges from %d to %d for [%d, %d)", edge.size(), edge.empty() ? -1 : edge.front(), edge.empty() ? -1 : edge.back(), ib_begin, ib_end);
    for (size_t k = 1; k < edge.size(); ++k) {
        CHECK(edge[k] >= edge[k - 1], "edge %zu = %d after %d; [%d, %d), %zu bytes, %ld MiB", k, edge[k], edge[k - 1], ib_begin, ib_end, real_size, static_cast<long>(band_mb));
        if (k + 1 < edge.size()) CHECK(edge[k] % 2 == 0 || edge[k] == ib_end, "odd interior edge %d; [%d, %d), %zu bytes, %ld MiB", edge[k], ib_begin, ib_end, real_size, static_cast<long>(band_mb));
    }
    const double bytes = static_cast<double>(pairs_below(ib_end) - pairs_below(ib_begin)) * TILE * static_cast<double>(real_size);
    if (bytes <= static_cast<double>(band_mb) * 1048576.0) CHECK(edge.size() == 2, "%zu edges though the records fit; [%d, %d), %zu bytes, %ld MiB", edge.size(), ib_begin, ib_end, real_size, static_cast<long>(band_mb));
}
static const int64_t BAND_MB[] = { 1, 64, DEFAULT_BAND_MB };

/* ------------------------------------------------------------------ items ------------------------------------------------------------------ */
static const int ORDERS[] = { 0, 1, 2, 3, 4, 5 };
/* the items of the band [begin, end) in every order: each row's items are its chunks up to the diagonal, once each, and their tiles add up to the row's */
static long check_band_items(int begin, int end, int nt, int tiles, const Head &h, bool pairs) {
    const int rows = pairs ? 2 : 1, num_jc = num_chunks(nt, tiles, h.tiles, h.count), nrow = (end - begin + rows - 1) / rows;
    std::vector<unsigned char> seen;
    std::vector<int> covered;
    unsigned long long first_sum = 0;
    long visited = 0;
    for (const int order : ORDERS) {
        const std::vector<WorkItem> items = band_items(begin, end, tiles, num_jc, order, pairs, h.tiles, h.count);
        seen.assign(static_cast<size_t>(nrow) * num_jc, 0);
        covered.assign(static_cast<size_t>(nrow), 0);
        unsigned long long sum = 0;  // of a hash per item: the same set in every order
        bool ok = true;
        for (const WorkItem &it : items) {
            const int k = (it.x - begin) / rows;
            if (it.x < begin || it.x >= end || (it.x - begin) % rows != 0 || it.y < 0 || it.y >= num_jc) {
                ok = false;
                break;
            }
            const int b = chunk_begin(it.y, tiles, h.tiles, h.count), e = std::min(std::min(b + chunk_len(it.y, tiles, h.tiles, h.count), it.x + rows), nt);
            unsigned char &s = seen[static_cast<size_t>(k) * num_jc + it.y];
            if (e <= b || s != 0) {  // empty, or repeated
                ok = false;
                break;
            }
            s = 1;
            covered[static_cast<size_t>(k)] += e - b;
            sum += (static_cast<unsigned long long>(it.x) * 1000003ULL + static_cast<unsigned long long>(it.y) + 1ULL) * 0x9E3779B97F4A7C15ULL;
        }
        for (int k = 0; ok && k < nrow; ++k) ok = covered[static_cast<size_t>(k)] == std::min(begin + rows * k + rows, nt);  // distinct chunks, which tile in order: the union is [0, that)
        if (order == ORDERS[0]) first_sum = sum;
        CHECK(ok && sum == first_sum, "band [%d, %d) of %d tiles, chunks of %d, head %d x %d, pairs %d, order %d: %zu items", begin, end, nt, tiles, h.count, h.tiles, pairs, order, items.size());
        visited += static_cast<long>(items.size());
    }
    return visited;
}

static long check_bands_and_items() {
    long visited = 0;
    size_t hpick = 0;
    for (const int nt : tile_counts()) {
        const bool large = nt > 200;
        std::set<std::pair<int, int>> item_bands;  // the bands whose items are checked, each once
        for (int world = 1; world <= 16; ++world) {
            for (int wmode = 0; wmode < 3; ++wmode) {
                const std::vector<Range> ranks = shard_ranges(nt, world, true, wmode);
                for (int k = 0; k < world; ++k) {
                    const Range &s = ranks[static_cast<size_t>(k)];
                    const bool with_items = large ? (world == 16 && wmode == 2 && (k == 0 || k == 5 || k == 15)) : (world == nt % 16 + 1 && wmode == nt % 3);
                    for (const int64_t mb : BAND_MB) {
                        for (const size_t real_size : { sizeof(float), sizeof(double) }) {
                            const std::vector<int> edge = band_edges(s.begin, s.end, real_size, geometry(mb));
                            check_band_edges(edge, s.begin, s.end, real_size, mb);
                            for (size_t b = 0; with_items && b + 1 < edge.size(); ++b) item_bands.insert({ edge[b], edge[b + 1] });
                        }
                    }
                }
            }
        }
        if (nt == 7813) {  // the whole triangle of a million points at the default budget: the shipped multi-band case
            const std::vector<int> edge = band_edges(0, nt, sizeof(float), geometry(DEFAULT_BAND_MB));
            for (const size_t b : { size_t(0), edge.size() / 2, edge.size() - 2 }) item_bands.insert({ edge[b], edge[b + 1] });  // (its first, a middle and its last band)
        }
        const int tiles = large ? 64 : CHUNK_TILES[nt > 100 ? 6 + nt % 9 : nt % 15];  // (every chunk length up to 100 blocks, the lengths from 8 on beyond: the item count goes with blocks^2 / length)
        Head head = HEADS[1 + hpick++ % 6];
        if (!head_fits(head, nt)) head = nt > 4 ? HEADS[1] : Head{ 1, 1 };
        for (const auto &band : item_bands) {
            for (const bool pairs : { false, true }) {
                if (pairs && band.first % 2 != 0) continue;  // (an empty band at an odd end: nothing to evaluate)
                if (!large || !pairs) visited += check_band_items(band.first, band.second, nt, tiles, HEADS[0], pairs);
                if ((!large || pairs) && head_fits(head, nt)) visited += check_band_items(band.first, band.second, nt, tiles, head, pairs);
            }
        }
    }
    return visited;
}

static void check_xcd_lane_order() {
    for (const size_t nchunks : { 0u, 1u, 3u, 7u, 8u, 9u, 63u, 64u, 65u, 130u }) {
        for (const size_t modulus : { 1u, 20u, 100u, 500u }) {  // chunk lengths (37 c + nchunks) % modulus: all empty, shorter than 32, mixed with empty ones
            std::vector<std::vector<WorkItem>> by_chunk(nchunks);
            size_t total = 0;
            for (size_t c = 0; c < nchunks; ++c) {
                for (size_t i = 0; i < (37 * c + nchunks) % modulus; ++i) by_chunk[c].push_back({ static_cast<int>(i), static_cast<int>(c) });
                total += by_chunk[c].size();
            }
            const std::vector<WorkItem> out = xcd_lane_order(by_chunk);
            std::vector<std::vector<unsigned char>> seen(nchunks);
            for (size_t c = 0; c < nchunks; ++c) seen[c].assign(by_chunk[c].size(), 0);
            bool ok = out.size() == total;
            for (const WorkItem &it : out) {
                ok = ok && it.y >= 0 && static_cast<size_t>(it.y) < nchunks && it.x >= 0 && static_cast<size_t>(it.x) < seen[static_cast<size_t>(it.y)].size() && seen[static_cast<size_t>(it.y)][static_cast<size_t>(it.x)]++ == 0;
                if (!ok) break;
            }
            CHECK(ok, "xcd_lane_order of %zu chunks, lengths modulo %zu: %zu of %zu items", nchunks, modulus, out.size(), total);
        }
    }
}

/* ------------------------------------------------------------------ replay ------------------------------------------------------------------ */
static const int REPLAY_TILES[] = { 64, 65, 79, 157, 235, 391, 782, 1954 };
static void check_replay() {
    const int slots = 256;
    for (const int nt : REPLAY_TILES) {
        for (const int64_t head : { 0, 1 }) {
            const GeometryOptions o = geometry(DEFAULT_BAND_MB, head);
            const PairChunks replayed = choose_pair_chunk_by_replay(0, nt, nt, sizeof(float), o, slots), first = choose_pair_chunk(0, nt, nt, sizeof(float), o, slots),
                             cached = choose_pair_chunk(0, nt, nt, sizeof(float), o, slots);
            for (const PairChunks &c : { first, cached }) CHECK(c.tiles == replayed.tiles && c.head_tiles == replayed.head_tiles && c.head_count == replayed.head_count, "%d tiles, head %d", nt, static_cast<int>(head));
            CHECK(replayed.tiles >= 2 && replayed.tiles <= 64, "%d tiles, head %d: chunks of %d", nt, static_cast<int>(head), replayed.tiles);
            CHECK(replayed.head_count >= 0 && replayed.head_tiles >= 0 && (replayed.head_count == 0) == (replayed.head_tiles == 0) && (head == 1 || replayed.head_count == 0)
                      && (replayed.head_count == 0 || replayed.head_count * replayed.head_tiles + replayed.tiles <= nt),
                  "%d tiles, head %d: %d x %d in front of chunks of %d", nt, static_cast<int>(head), replayed.head_count, replayed.head_tiles, replayed.tiles);
        }
    }
    // beyond 16 rounds over the slots at the longest chunk: the fixed answers -- the fixed head up to 32 rounds where the option allows one, none beyond
    struct Fixed {
        int nt, slots;
        int64_t head;
        PairChunks want;
    };
    for (const Fixed &f : { Fixed{ 1954, 256, 1, { 64, 0, 0 } }, Fixed{ 1954, 256, 0, { 64, 0, 0 } }, Fixed{ 1200, 256, 1, { 64, 16, 2 } }, Fixed{ 1200, 256, 0, { 64, 0, 0 } },
                            Fixed{ 7813, 256, 1, { 64, 0, 0 } }, Fixed{ 200, 1, 1, { 64, 0, 0 } }, Fixed{ 100, 2, 1, { 64, 16, 2 } }, Fixed{ 96, 2, 1, { 64, 0, 0 } } }) {
        const PairChunks c = choose_pair_chunk_by_replay(0, f.nt, f.nt, sizeof(float), geometry(DEFAULT_BAND_MB, f.head), f.slots);
        CHECK(c.tiles == f.want.tiles && c.head_tiles == f.want.head_tiles && c.head_count == f.want.head_count, "%d tiles on %d slots, head %d: %d x %d in front of chunks of %d", f.nt, f.slots,
              static_cast<int>(f.head), c.head_count, c.head_tiles, c.tiles);
    }
}

/* ------------------------------------------------------------------ characterisation ------------------------------------------------------------------ */
static unsigned long long fnv1a(unsigned long long h, int v) {
    for (int b = 0; b < 4; ++b) {
        h ^= (static_cast<unsigned>(v) >> (8 * b)) & 0xFFu;
        h *= 0x100000001B3ULL;
    }
    return h;
}
static constexpr unsigned long long FNV_BASIS = 0xCBF29CE484222325ULL;
static void appendf(std::string &out, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    out += buf;
}

static std::string dump() {
    std::string out;
    // the symmetric shards: row blocks, band edges, the items of all bands
    const int nts[] = { 1, 2, 3, 7, 33, 64, 65, 79, 128, 157, 200, 391, 782, 1954, 7813 }, worlds[] = { 1, 2, 3, 4, 8, 16 }, jcs[] = { 1, 2, 3, 8, 16, 24, 48, 64 };
    for (int i = 0; i < 300; ++i) {
        const int nt = nts[i % 15];
        int world = worlds[(i / 15 + i) % 6];
        if (nt == 7813 && world < 8) world = 16;
        const int rank = (i * 7) % world, wmode = i % 3, order = i % 6, tiles = nt > 1000 ? 64 : jcs[(i / 5) % 8];
        const int64_t mb = BAND_MB[(i / 3) % 3];
        const size_t real_size = i % 2 != 0 ? 8 : 4;
        const bool pairs = (i / 2) % 2 != 0;
        Head h = i % 4 == 1 ? HEADS[1 + (i / 4) % 6] : HEADS[0];
        if (!head_fits(h, nt)) h = HEADS[0];
        const std::vector<double> w = shard_weights(world, wmode);
        int begin = 0, end = 0;
        shard_blocks(nt, world, rank, true, begin, end, wmode != 0 ? &w : nullptr);
        const std::vector<int> edge = band_edges(begin, end, real_size, geometry(mb));
        unsigned long long eh = FNV_BASIS, ih = FNV_BASIS;
        size_t count = 0;
        const int num_jc = num_chunks(nt, tiles, h.tiles, h.count);
        for (size_t b = 0; b < edge.size(); ++b) {
            eh = fnv1a(eh, edge[b]);
            if (b + 1 == edge.size()) break;
            for (const WorkItem &it : band_items(edge[b], edge[b + 1], tiles, num_jc, order, pairs, h.tiles, h.count)) {
                ih = fnv1a(fnv1a(ih, it.x), it.y);
                ++count;
            }
        }
        appendf(out, "shard tiles=%d world=%d rank=%d weights=%d band_mb=%ld real=%zu chunk=%d head=%dx%d order=%d pairs=%d -> blocks=[%d,%d) chunks=%d bands=%zu edges=", nt, world, rank, wmode,
                static_cast<long>(mb), real_size, tiles, h.count, h.tiles, order, pairs ? 1 : 0, begin, end, num_jc, edge.size() - 1);
        for (size_t b = 0; b < edge.size() && edge.size() <= 12; ++b) appendf(out, "%s%d", b == 0 ? "" : ",", edge[b]);
        appendf(out, "%s#%016llx items=%zu#%016llx\n", edge.size() <= 12 ? "" : "...", eh, count, ih);
    }
    // the full-square shards: the ceil-sized runs
    for (int i = 0; i < 20; ++i) {
        const int nt = nts[(i * 4) % 15], world = worlds[i % 6], rank = (i * 5) % world;
        int begin = 0, end = 0;
        shard_blocks(nt, world, rank, false, begin, end, nullptr);
        appendf(out, "full tiles=%d world=%d rank=%d -> blocks=[%d,%d)\n", nt, world, rank, begin, end);
    }
    // the replayed chunk choice
    for (const int slots : { 256, 64 }) {
        for (const int nt : { 64, 65, 79, 157, 235, 391, 782, 1200, 1954 }) {
            for (const int64_t head : { 0, 1 }) {
                const PairChunks c = choose_pair_chunk(0, nt, nt, sizeof(float), geometry(DEFAULT_BAND_MB, head), slots);
                appendf(out, "replay tiles=%d slots=%d head=%d -> chunk=%d head=%dx%d\n", nt, slots, static_cast<int>(head), c.tiles, c.head_count, c.head_tiles);
            }
        }
    }
    {  // a shard of several bands, rank 1 of 2: no head search
        int begin = 0, end = 0;
        shard_blocks(391, 2, 1, true, begin, end, nullptr);
        const PairChunks c = choose_pair_chunk(begin, end, 391, sizeof(float), geometry(1), 256);
        appendf(out, "replay tiles=391 blocks=[%d,%d) band_mb=1 slots=256 head=1 -> chunk=%d head=%dx%d\n", begin, end, c.tiles, c.head_count, c.head_tiles);
    }
    // the automatic chunk length of a training shard: flags sym | split | pair | wide_nl
    struct Flags {
        bool sym, split, pair, wide_nl;
    };
    const Flags flags[] = { { true, false, false, false }, { true, true, false, false }, { true, true, true, false }, { true, true, false, true }, { false, false, false, false },
                            { false, true, false, false }, { false, true, false, true } };
    int n = 0;
    for (const int nt : { 3, 24, 63, 64, 79, 157, 391, 782, 2344 }) {
        for (const Flags &f : flags) {
            if (f.pair && nt < 64) continue;
            ++n;
            const int world = n % 3 == 0 ? 2 : 1, rank = n % 2 != 0 ? 0 : world - 1;
            const int64_t j_chunk_tiles = n % 7 == 0 ? 5 : 0, j_chunk_head = n % 5 == 0 ? 2 * 1024 + 8 : (n % 5 == 1 ? 0 : 1);
            int begin = 0, end = 0;
            shard_blocks(nt, world, rank, f.sym, begin, end, nullptr);
            const PairChunks c = shard_chunks(geometry(DEFAULT_BAND_MB, j_chunk_head, j_chunk_tiles), begin, end, nt, sizeof(float), f.sym, f.split, f.pair, f.wide_nl, 256);
            appendf(out, "auto tiles=%d blocks=[%d,%d) sym=%d split=%d pair=%d wide_nl=%d j_chunk_tiles=%d j_chunk_head=%d -> chunk=%d head=%dx%d\n", nt, begin, end, f.sym, f.split, f.pair, f.wide_nl,
                    static_cast<int>(j_chunk_tiles), static_cast<int>(j_chunk_head), c.tiles, c.head_count, c.head_tiles);
        }
    }
    // ... and of a rectangular product
    for (const int num_ib : { 1, 2, 8, 63, 64, 157, 782, 1564 }) {
        for (const int num_jt : { 1, 3, 24, 79, 391 }) {
            for (const bool rect : { false, true }) {
                if (rect && (num_ib < 64 || num_ib % 2 != 0)) continue;
                const int64_t j_chunk_tiles = (num_ib + num_jt) % 9 == 0 ? 7 : 0;
                appendf(out, "product rows=%d cols=%d rect=%d j_chunk_tiles=%d -> chunk=%d\n", num_ib, num_jt, rect ? 1 : 0, static_cast<int>(j_chunk_tiles),
                        product_chunk_tiles(geometry(DEFAULT_BAND_MB, 1, j_chunk_tiles), rect, num_ib, num_jt));
            }
        }
    }
    return out;
}

int main(int argc, char **argv) {
    std::string golden = std::string(argv[0]);
    golden = golden.substr(0, golden.find_last_of('/') == std::string::npos ? 0 : golden.find_last_of('/') + 1) + "../golden/geometry_cases.txt";
    for (int a = 1; a < argc; ++a) {
        if (std::strcmp(argv[a], "--dump") == 0) {
            std::fputs(dump().c_str(), stdout);
            return 0;
        }
        if (std::strcmp(argv[a], "--golden") == 0 && a + 1 < argc) golden = argv[++a];
    }
    check_chunks();
    check_shards();
    const long visited = check_bands_and_items();
    check_xcd_lane_order();
    check_replay();
    std::ifstream in(golden);
    std::stringstream recorded;
    recorded << in.rdbuf();
    const std::string now = dump();
    if (!in || recorded.str() != now) {
        ++failures;
        std::istringstream a(recorded.str()), b(now);
        std::string la, lb;
        int line = 0, shown = 0;
        while (shown < 5) {
            const bool ha = static_cast<bool>(std::getline(a, la)), hb = static_cast<bool>(std::getline(b, lb));
            if (!ha && !hb) break;
            ++line;
            if (ha != hb || la != lb) {
                std::fprintf(stderr, "%s line %d\n  recorded: %s\n  now:      %s\n", golden.c_str(), line, ha ? la.c_str() : "(none)", hb ? lb.c_str() : "(none)");
                ++shown;
            }
        }
    }
    std::printf("%s: %ld work items visited, %d failures\n", failures == 0 ? "OK" : "FAILED", visited, failures);
    return failures == 0 ? 0 : 1;
}
