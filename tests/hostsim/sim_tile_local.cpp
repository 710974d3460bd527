// gym_pcgrl_amd/csrc/tile_local.h on the CPU.  TEST ONLY.
//
// sim_tile_local() does for one map what k_tile_local (kernels_tile_local.h) does for its lane group: the lanes run one after the other
// through tl_lane_cells / tl_lane_counts -- they share nothing but the bytes -- and their partial sums are added up where the kernel has
// its DPP reduction.  The forms: `lanes` 16 or 64 on a stage -- a copy of the map of exactly h * w bytes, checked for bytes >= 32 on the
// way like eval_stage_map -- or 64 lanes on the caller's bytes with the lanes' own check.  Built as a shared library for
// tests/test_tile_local_host.py and, with -DSIM_TILE_LOCAL_MAIN -fsanitize=address,undefined, as a stand-alone program that runs built-in
// levels through every form against a plain restatement of the rules, with guard elements around every output.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../gym_pcgrl_amd/csrc/tile_local.h"

// D: the descriptor of ONE map (count 1, maps ignored: `map` is read).  Returns 0, or -1 for a form that does not hold the map.
template <bool STAGED>
static int run_tile_local(const uint8_t* map, int h, int w, int lanes, const pcgrl_tile_local_desc& D, int32_t* status) {
    const int cells = h * w;
    std::vector<uint8_t> stage;
    const uint8_t* tiles = map;
    if (STAGED) {
        if (h > 64 || w > 64) return -1;
        stage.assign(map, map + cells);             // (exactly the map: a read beyond it is the sanitizer's)
        for (int c = 0; c < cells; c++) if (map[c] >= 32) *status |= 4;
        tiles = stage.data();
    }
    const TlWant want = tl_want(D);
    TlLane total = {0, 0, 0, 0, 0};
    long long even[16] = {0}, odd[16] = {0};
    for (int lane = 0; lane < lanes; lane++) {
        TlLane a = {0, 0, 0, 0, 0};
        if (want.floor || want.group || want.changes) tl_lane_cells<!STAGED>(tiles, D, want, w, h, lane, lanes, D.floor_map_out, D.group_map_out, a);
        if (want.counts) {
            uint32_t p[16];
            tl_lane_counts<!STAGED>(tiles, cells, lane, lanes, p, a);
            for (int k = 0; k < 16; k++) { even[k] += p[k] & 0xFFFFu; odd[k] += p[k] >> 16; }
        }
        total.floor_dist += a.floor_dist; total.grouping += a.grouping; total.changes_h += a.changes_h; total.changes_v += a.changes_v; total.bad |= a.bad;
    }
    if (!STAGED && total.bad) *status |= 4;
    if (D.floor_dist_out) *D.floor_dist_out = total.floor_dist;
    if (D.grouping_out) *D.grouping_out = total.grouping;
    if (D.changes_out) { D.changes_out[0] = total.changes_h; D.changes_out[1] = total.changes_v; }
    if (D.counts_out) for (int k = 0; k < 16; k++) { D.counts_out[2 * k] = (int32_t)even[k]; D.counts_out[2 * k + 1] = (int32_t)odd[k]; }
    return 0;
}

extern "C" {
int sim_tile_local(const uint8_t* map, int h, int w, int lanes, int staged, const pcgrl_tile_local_desc* D, int32_t* status) {
    if (lanes != 16 && lanes != 64) return -1;
    return staged ? run_tile_local<true>(map, h, w, lanes, *D, status) : run_tile_local<false>(map, h, w, lanes, *D, status);
}
int sim_tile_local_desc_bytes() { return (int)sizeof(pcgrl_tile_local_desc); }
}

#ifdef SIM_TILE_LOCAL_MAIN
static unsigned lcg_state = 2025u;
static unsigned lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }
static bool in_set(uint32_t set, unsigned t) { return t < 32 && ((set >> t) & 1); }

template <class T>
struct Guarded {                                    // n elements between two guards of 8
    std::vector<T> v;
    explicit Guarded(size_t n) : v(n + 16, (T)77) {}
    T* data() { return v.data() + 8; }
    bool intact() const { for (int i = 0; i < 8; i++) if (v[i] != (T)77 || v[v.size() - 1 - i] != (T)77) return false; return true; }
};

int main() {
    const int sizes[13][2] = {{40, 300}, {1, 1}, {1, 9}, {8, 1}, {3, 7}, {14, 14}, {9, 16}, {9, 17}, {64, 64}, {65, 2}, {64, 65}, {14, 114}, {255, 255}};
    const int forms[3][2] = {{16, 1}, {64, 1}, {64, 0}};
    long levels = 0, sum = 0;
    for (int si = 0; si < 13; si++) {
        const int h = sizes[si][0], w = sizes[si][1], cells = h * w;
        for (int rep = 0; rep < 6; rep++) {
            std::vector<uint8_t> map((size_t)cells);
            for (int c = 0; c < cells; c++) {
                const unsigned r = lcg() % 100;
                map[c] = rep == 4 ? (uint8_t)(30 + (r < 50)) : (rep == 5 ? (uint8_t)1 : (r < 30 + 10 * rep ? 0 : (uint8_t)(1 + r % 7)));
            }
            if (rep == 3 && cells > 1) map[cells - 1] = 200;                    // a byte no set can name
            pcgrl_tile_local_desc D;
            memset(&D, 0, sizeof(D));
            D.count = 1;
            D.from_tiles = rep == 4 ? 0x40000000u : 0x5u; D.floor_tiles = rep == 4 ? 0x80000000u : (rep == 2 ? 0u : 0x5Au);
            D.group_tiles = rep == 4 ? 0xC0000000u : 0x42u; D.group_min = 1; D.group_max = rep == 1 ? 0 : 9;
            const int8_t offs[16][2] = {{-1, 0}, {1, 0}, {0, -1}, {0, 1}, {0, 0}, {1, 0}, {-128, 0}, {127, 127}, {0, -128}, {-1, -1}, {1, 1}, {-1, 1}, {1, -1}, {2, 0}, {0, 2}, {-3, 3}};
            D.noffsets = rep == 2 ? 0 : (rep == 0 ? 2 : 16);
            memcpy(D.offsets, offs, sizeof(offs));
            // the rules, restated plainly
            std::vector<int> fmap(cells), gmap(cells), cnt(32, 0);
            int want[4] = {0, 0, 0, 0};
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    const int c = y * w + x;
                    int d = h - 1;
                    for (int dy = 0; y + dy < h; dy++) if (in_set(D.floor_tiles, map[c + dy * w])) { d = dy - 1; break; }
                    fmap[c] = d;
                    if (in_set(D.from_tiles, map[c])) want[0] += d;
                    int v = 0;
                    for (int k = 0; k < D.noffsets; k++) {
                        const int nx = x + D.offsets[k][0], ny = y + D.offsets[k][1];
                        if (nx >= 0 && ny >= 0 && nx < w && ny < h && in_set(D.group_tiles, map[ny * w + nx])) v++;
                    }
                    gmap[c] = v;
                    if (in_set(D.group_tiles, map[c]) && v >= D.group_min && v <= D.group_max) want[1]++;
                    if (x > 0 && map[c] != map[c - 1]) want[2]++;
                    if (y > 0 && map[c] != map[c - w]) want[3]++;
                    if (map[c] < 32) cnt[map[c]]++;
                }
            for (int f = 0; f < 3; f++) {
                if (forms[f][1] && (h > 64 || w > 64)) continue;
                for (int pick = 0; pick < 7; pick++) {                          // every output alone, then all of them
                    Guarded<int32_t> counts(32), fd(1), gr(1), ch(2);
                    Guarded<int16_t> fm((size_t)cells);
                    Guarded<int8_t> gm((size_t)cells);
                    pcgrl_tile_local_desc E = D;
                    const bool all = pick == 6;
                    if (all || pick == 0) E.counts_out = counts.data();
                    if (all || pick == 1) E.floor_dist_out = fd.data();
                    if (all || pick == 2) E.floor_map_out = fm.data();
                    if (all || pick == 3) E.grouping_out = gr.data();
                    if (all || pick == 4) E.group_map_out = gm.data();
                    if (all || pick == 5) E.changes_out = ch.data();
                    int32_t status = 0;
                    if (sim_tile_local(map.data(), h, w, forms[f][0], forms[f][1], &E, &status) != 0) return 2;
                    if (!counts.intact() || !fd.intact() || !gr.intact() || !ch.intact() || !fm.intact() || !gm.intact()) return 3;
                    if (status != ((rep == 3 && cells > 1) ? 4 : 0)) return 4;
                    if (E.counts_out) { for (int t = 0; t < 32; t++) if (counts.data()[t] != cnt[t]) return 5; }
                    else if (counts.data()[0] != 77) return 6;                  // not asked for: untouched
                    if (E.floor_dist_out ? fd.data()[0] != want[0] : fd.data()[0] != 77) return 7;
                    if (E.grouping_out ? gr.data()[0] != want[1] : gr.data()[0] != 77) return 8;
                    if (E.changes_out ? (ch.data()[0] != want[2] || ch.data()[1] != want[3]) : ch.data()[0] != 77) return 9;
                    for (int c = 0; c < cells; c++) {
                        if (E.floor_map_out ? fm.data()[c] != fmap[c] : fm.data()[c] != 77) return 10;
                        if (E.group_map_out ? gm.data()[c] != gmap[c] : gm.data()[c] != 77) return 11;
                    }
                    levels++;
                }
            }
            sum += want[0] + want[1] + want[2] + want[3];
        }
    }
    if (levels < 1000 || sum < 1000) return 12;
    printf("levels %ld sum %ld\nok\n", levels, sum);
    return 0;
}
#endif
