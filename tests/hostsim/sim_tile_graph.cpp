// gym_pcgrl_amd/csrc/tile_graph.h on the CPU lane-group simulator of sim_algos.cpp.  TEST ONLY.
//
// sim_tile_graph() does for one map what k_tile_graph (kernels_tile_graph.h) does for its lane group: the pass / source / reach planes
// from the tile bytes and three 32-bit tile sets, the two scalars by regions_and_longest_path, the label and distance planes by
// tile_graph.h, each row unpacked once.  Built as a shared library for tests/test_tile_graph_host.py and, with -DSIM_TILE_GRAPH_MAIN
// -fsanitize=address,undefined, as a stand-alone program that runs a few built-in levels through every (lane group, mask width) form.
#include "sim_algos.cpp"
#include "sim_forms.h"
#include "../../gym_pcgrl_amd/csrc/tile_graph.h"

// a map's [h, w] i16 output from its planes: row y by the words of lane y
template <int NP, int G, class T>
static void store_planes(int16_t* out, const SimVec<T, G>* p, const SimVec<T, G>& valid, int h, int w) {
    for (int y = 0; y < h; y++) {
        T words[NP];
        for (int k = 0; k < NP; k++) words[k] = p[k].v[y];
        for (int x = 0; x < w; x++) out[y * w + x] = (int16_t)tg_cell<NP>(words, valid.v[y], x);
    }
}

// source: -2 = the first cell of source_tiles, else the cell (-1, or outside the map: none).  Every output may be NULL.
// Returns 0, or -1 when the form does not hold the map; *status gets 4 for a byte >= 32 and 2 for a source cell outside the map.
template <int G, class T>
static int run_tile_graph(SimGroup<G, T> g, const uint8_t* map, int h, int w, uint32_t passable, uint32_t source_tiles, uint32_t reach_tiles, int source,
                          int32_t* regions_out, int32_t* longest_out, int16_t* labels_out, int16_t* dist_out, int32_t* reach_out,
                          int32_t* source_out, int32_t* status) {
    typedef SimVec<T, G> M;
    constexpr int NP = tg_planes(G, 8 * (int)sizeof(T));
    if (h > G || w > (int)(8 * sizeof(T))) return -1;
    M pass, srcs, goal;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const unsigned t = map[y * w + x];
            if (t >= 32) *status |= 4;
            const uint32_t bit = t < 32 ? 1u << t : 0u;
            pass.v[y] |= (T)((passable & bit) != 0) << x;
            srcs.v[y] |= (T)((source_tiles & bit) != 0) << x;
            goal.v[y] |= (T)((reach_tiles & bit) != 0) << x;
        }
    if (regions_out || longest_out) {
        int regions, path;
        regions_and_longest_path(g, pass, regions, path);
        if (regions_out) *regions_out = regions;
        if (longest_out) *longest_out = path;
    }
    if (labels_out) {
        M lp[NP];
        const int n = tg_labels<NP>(g, pass, lp);
        store_planes<NP>(labels_out, lp, pass, h, w);
        if (n >= (1 << NP)) abort();                // a label the planes do not hold
    }
    if (dist_out || reach_out || source_out) {
        M src;
        if (source != -2) {
            int c = source;
            if (c < -1 || c >= h * w) { *status |= 2; c = -1; }
            if (c >= 0) src.v[c / w] = (T)1 << (c % w);
        } else src = g.first_bit(srcs);
        if (source_out) {
            *source_out = -1;
            for (int y = 0; y < G; y++) if (src.v[y]) *source_out = y * w + __builtin_ctzll((unsigned long long)src.v[y]);
        }
        if (dist_out || reach_out) {
            M dp[NP], reached;
            tg_dist<NP>(g, src, pass, dp, reached);
            if (dist_out) store_planes<NP>(dist_out, dp, reached, h, w);
            if (reach_out) *reach_out = g.popcount_sum(goal & reached);
        }
    }
    return 0;
}

extern "C" {
// group = 16 or 64 lanes, mask_bits = 32 or 64; labels / dist [h][w].  -1: the form does not hold the map.
int sim_tile_graph(const uint8_t* map, int h, int w, int group, int mask_bits, uint32_t passable, uint32_t source_tiles, uint32_t reach_tiles,
                   int source, int32_t* regions_out, int32_t* longest_out, int16_t* labels_out, int16_t* dist_out, int32_t* reach_out,
                   int32_t* source_out, int32_t* status) {
    return sim_with_form(group, mask_bits, -1, [&](auto g) {
        return run_tile_graph(g, map, h, w, passable, source_tiles, reach_tiles, source, regions_out, longest_out, labels_out, dist_out, reach_out, source_out, status);
    });
}
}

#ifdef SIM_TILE_GRAPH_MAIN
static SimLcg lcg = {2024u};

// what the outputs must satisfy whatever the level: labels 1..regions exactly on the passable cells, each label 4-connected to
// nothing of another label; dist 0 exactly at a passable source, neighbours within 1, every reached cell but the source with a
// neighbour one nearer; reach counted over dist >= 0
static int check(const uint8_t* map, int h, int w, uint32_t passable, uint32_t reach_tiles, int regions, const int16_t* lab, const int16_t* dist,
                 int reach, int source) {
    int top = 0, cnt = 0;
    for (int c = 0; c < h * w; c++) {
        const bool p = map[c] < 32 && ((passable >> map[c]) & 1);
        if (p != (lab[c] > 0) || (!p && lab[c] != -1) || (!p && dist[c] != -1)) return 10;
        if (lab[c] > top) { if (lab[c] != top + 1) return 11; top = lab[c]; }          // numbered in the order of the first cells
        if (dist[c] >= 0 && map[c] < 32 && ((reach_tiles >> map[c]) & 1)) cnt++;
        if ((dist[c] == 0) != (c == source && p)) return 12;
        const int y = c / w, x = c % w;
        const int nb[4] = {x > 0 ? c - 1 : -1, x + 1 < w ? c + 1 : -1, y > 0 ? c - w : -1, y + 1 < h ? c + w : -1};
        bool nearer = false;
        for (int k = 0; k < 4; k++) {
            if (nb[k] < 0 || lab[nb[k]] < 0 || !p) continue;
            if (lab[nb[k]] != lab[c]) return 13;
            if ((dist[c] >= 0) != (dist[nb[k]] >= 0)) return 14;
            if (dist[c] >= 0 && (dist[c] - dist[nb[k]] > 1 || dist[nb[k]] - dist[c] > 1)) return 15;
            if (dist[c] > 0 && dist[nb[k]] == dist[c] - 1) nearer = true;
        }
        if (dist[c] > 0 && !nearer) return 16;
    }
    if (top != regions) return 17;
    if (cnt != reach) return 18;
    return 0;
}

int main() {
    const int sizes[7][2] = {{1, 1}, {3, 7}, {16, 32}, {16, 33}, {17, 9}, {9, 64}, {64, 64}};
    long levels = 0, reached = 0;
    for (int si = 0; si < 7; si++) {
        const int h = sizes[si][0], w = sizes[si][1];
        for (int rep = 0; rep < 8; rep++) {
            std::vector<uint8_t> map((size_t)h * w);
            for (int c = 0; c < h * w; c++) {
                const unsigned r = lcg() % 100;
                map[c] = rep == 6 ? (uint8_t)((c / w + c % w) & 1) : (rep == 7 ? (uint8_t)(30 + (r < 80)) : (r < 40 + 8 * rep ? 0 : (uint8_t)(1 + r % 7)));
            }
            if (rep == 5 && h * w > 1) map[1] = 200;                         // a byte no set can name
            const uint32_t passable = rep == 7 ? 0x80000000u : (rep & 1 ? 0x15u : 0x1u), source_tiles = rep == 7 ? 0x80000000u : 0x5u, reach_tiles = rep == 7 ? 0xC0000000u : 0x3u;
            const int source = rep == 2 ? (int)(lcg() % (unsigned)(h * w)) : (rep == 3 ? -1 : (rep == 4 ? h * w + 5 : -2));
            std::vector<int16_t> want_lab, want_dist;
            int32_t want[4] = {0, 0, 0, 0};
            bool have_want = false;
            for (int f = 0; f < 4; f++) {
                if (h > SIM_FORMS[f][0] || w > SIM_FORMS[f][1]) continue;
                std::vector<int16_t> lab((size_t)h * w + 2, 77), dist((size_t)h * w + 2, 77);      // a guard word at either end
                int32_t out[4] = {-9, -9, -9, -9}, status = 0;
                if (sim_tile_graph(map.data(), h, w, SIM_FORMS[f][0], SIM_FORMS[f][1], passable, source_tiles, reach_tiles, source, &out[0], &out[1],
                                   lab.data() + 1, dist.data() + 1, &out[2], &out[3], &status) != 0) return 2;
                if (lab[0] != 77 || lab[(size_t)h * w + 1] != 77 || dist[0] != 77 || dist[(size_t)h * w + 1] != 77) return 3;
                if (status != ((rep == 5 && h * w > 1) ? 4 : 0) + (rep == 4 ? 2 : 0)) return 4;
                if (const int rc = check(map.data(), h, w, passable, reach_tiles, out[0], lab.data() + 1, dist.data() + 1, out[2], out[3])) return rc;
                if (out[1] < 0 || out[1] >= h * w) return 5;
                // each output alone gives the same value
                int32_t alone = -9, st2 = 0;
                if (sim_tile_graph(map.data(), h, w, SIM_FORMS[f][0], SIM_FORMS[f][1], passable, source_tiles, reach_tiles, source, nullptr, nullptr, nullptr, nullptr,
                                   &alone, nullptr, &st2) != 0 || alone != out[2]) return 6;
                if (!have_want) { want_lab = lab; want_dist = dist; memcpy(want, out, sizeof(out)); have_want = true; }
                else if (want_lab != lab || want_dist != dist || memcmp(want, out, sizeof(out))) return 8;      // every form gives the same
                levels++;
                reached += out[2];
            }
        }
    }
    if (levels < 100 || reached < 1000) return 9;
    printf("levels %ld reached %ld\nok\n", levels, reached);
    return 0;
}
#endif
