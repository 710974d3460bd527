// gym_pcgrl_amd/csrc/path_trace.h on the CPU lane-group simulator of sim_algos.cpp.  TEST ONLY.
//
// sim_paths() does for one map what k_get_paths (kernels_paths.h) does for its lane group: the statistics row by the templates of
// pcgrl_algos.h, the legs by path_trace.h, the cells of each leg stored once and -1 from its end to the end of the row.  Built as a
// shared library for tests/test_paths_host.py and, with -DSIM_PATHS_MAIN -fsanitize=address,undefined, as a stand-alone program that
// runs a few built-in levels through every (lane group, mask width) form.
#include "sim_algos.cpp"
#include "sim_forms.h"
#include "../../gym_pcgrl_amd/csrc/path_trace.h"

// path_trace.h's Sink: the lane (row) that holds the bit stores y * W + x
template <int G, class T>
struct SimPathSink {
    int16_t* base;
    int16_t* row;
    int max_len, W;
    long puts;
    void leg(int l) { row = base + (size_t)l * max_len; }
    void put(const SimVec<T, G>& cur, int i) {
        int owners = 0;
        for (int y = 0; y < G; y++) {
            if (!cur.v[y]) continue;
            owners += __builtin_popcountll((unsigned long long)cur.v[y]);
            if (i < max_len) row[i] = (int16_t)(y * W + __builtin_ctzll((unsigned long long)cur.v[y]));
        }
        if (owners != 1) abort();                   // a walk-back that lost its cell, or holds two
        puts++;
    }
};

template <int G, class T>
static int run_paths(SimGroup<G, T> g, int prob, const uint8_t* map, int h, int w, int max_len, int16_t* cells, int32_t* length, int32_t* row8) {
    if (h > G || w > (int)(8 * sizeof(T))) return -1;
    SimVec<T, G> b0, b1, b2, valid;
    planes_of(map, h, w, b0, b1, b2);
    for (int y = 0; y < h; y++) valid.v[y] = (w >= (int)(8 * sizeof(T))) ? ~(T)0 : (((T)1 << w) - 1);
    PcgrlParams P; memset(&P, 0, sizeof(P));
    P.prob = prob; P.width = w; P.height = h; P.prob_width = w; P.prob_height = h;
    int32_t s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int legs = prob == PCGRL_PROB_BINARY ? 1 : 3;
    int len[3] = {-1, -1, -1};
    SimPathSink<G, T> sink = {cells, cells, max_len, w, 0};
    if (prob == PCGRL_PROB_BINARY) {
        int regions, path;
        regions_and_longest_path(g, ~b0 & valid, regions, path);
        s[0] = regions; s[1] = path;
        len[0] = binary_longest_leg(g, ~b0 & valid, path, sink);
    } else if (prob == PCGRL_PROB_ZELDA) {
        zelda_stats(g, P, b0, b1, b2, valid, s);
        zelda_legs(g, b0, b1, b2, valid, s, sink, len);
    } else return -1;
    for (int l = 0; l < legs; l++) {
        const int n = len[l] < 0 ? 0 : (len[l] + 1 < max_len ? len[l] + 1 : max_len);
        for (int i = n; i < max_len; i++) cells[(size_t)l * max_len + i] = -1;
        length[l] = len[l];
    }
    for (int k = 0; k < 8; k++) row8[k] = s[k];
    return 0;
}

extern "C" {
// group = 16 or 64 lanes, mask_bits = 32 or 64; cells [legs][max_len], length [legs], row8 [8].  -1: the form does not hold the map.
int sim_paths(int prob, const uint8_t* map, int h, int w, int group, int mask_bits, int max_len, int16_t* cells, int32_t* length, int32_t* row8) {
    return sim_with_form(group, mask_bits, -1, [&](auto g) { return run_paths(g, prob, map, h, w, max_len, cells, length, row8); });
}
}

#ifdef SIM_PATHS_MAIN
// the leg is a walk: in range, 4-adjacent, nothing repeated, length + 1 cells when the row holds them all
static bool walk_ok(const int16_t* c, int len, int max_len, int h, int w) {
    const int n = len < 0 ? 0 : (len + 1 < max_len ? len + 1 : max_len);
    for (int i = 0; i < max_len; i++) {
        if (i >= n) { if (c[i] != -1) return false; continue; }
        if (c[i] < 0 || c[i] >= h * w) return false;
        if (i > 0) {
            const int dy = c[i] / w - c[i - 1] / w, dx = c[i] % w - c[i - 1] % w;
            if (dy * dy + dx * dx != 1) return false;
        }
    }
    return true;
}
static SimLcg lcg = {2024u};

int main() {
    const int sizes[6][2] = {{1, 1}, {3, 7}, {16, 32}, {16, 33}, {17, 9}, {64, 64}};
    long legs_found = 0;
    for (int prob = 0; prob < 2; prob++) {
        for (int si = 0; si < 6; si++) {
            const int h = sizes[si][0], w = sizes[si][1];
            for (int rep = 0; rep < 6; rep++) {
                std::vector<uint8_t> map((size_t)h * w);
                for (auto& t : map) {
                    const unsigned r = lcg() % 100;
                    t = prob == 0 ? (r < 45 + 8 * rep ? 0 : 1) : (r < 60 ? 0 : (r < 85 ? 1 : (uint8_t)(2 + r % 6)));
                }
                if (prob == 1 && rep >= 2) {      // a playable level: one player, key and door, a few enemies, no walls
                    for (auto& t : map) t = 0;
                    map[0] = 2; map[(size_t)h * w - 1] = 3;
                    if (h * w > 4) { map[(size_t)h * w / 2] = 4; map[1] = rep == 5 ? 1 : 5; map[(size_t)h * w - 2] = 6; }
                }
                int32_t want_len[3] = {0, 0, 0}, want_row[8];
                std::vector<int16_t> want;
                bool have_want = false;
                for (int f = 0; f < 4; f++) {
                    if (h > SIM_FORMS[f][0] || w > SIM_FORMS[f][1]) continue;
                    for (int max_len : {1, 2, h * w, h * w + 3}) {
                        std::vector<int16_t> cells((size_t)3 * max_len + 2, 77);      // two guard words behind the rows
                        int32_t len[3] = {-9, -9, -9}, row[8];
                        if (sim_paths(prob, map.data(), h, w, SIM_FORMS[f][0], SIM_FORMS[f][1], max_len, cells.data(), len, row) != 0) return 2;
                        const int legs = prob == 0 ? 1 : 3;
                        if (cells[(size_t)legs * max_len] != 77 || cells[(size_t)3 * max_len + 1] != 77) return 3;
                        for (int l = 0; l < legs; l++) {
                            if (!walk_ok(cells.data() + (size_t)l * max_len, len[l], max_len, h, w)) return 4;
                            if (len[l] >= 0) legs_found++;
                        }
                        if (prob == 0 && len[0] >= 0 && len[0] != row[1]) return 5;
                        if (prob == 1 && len[0] >= 0 && len[0] + len[1] != row[6]) return 6;
                        if (prob == 1 && len[2] >= 0 && len[2] != row[5]) return 7;
                        if (max_len == h * w) {       // every form gives the same rows
                            if (!have_want) { want = cells; memcpy(want_len, len, sizeof(len)); memcpy(want_row, row, sizeof(row)); have_want = true; }
                            else if (want != cells || memcmp(want_len, len, sizeof(len)) || memcmp(want_row, row, sizeof(row))) return 8;
                        }
                    }
                }
            }
        }
    }
    if (legs_found < 100) return 9;
    printf("legs %ld\nok\n", legs_found);
    return 0;
}
#endif
