// The in-register edit of k_get_changes (gym_pcgrl_amd/csrc/kernels_changes.h) on the CPU lane-group simulator of sim_algos.cpp.  TEST ONLY.
//
// Only the edit is simulated: sim_changes() does for one level what a lane group of the kernel does per (cell, tile) -- the working
// planes taken from a kept copy (the kernel's copy is in LDS; here an array), the row that owns the cell edited by planes_set_cell
// (pcgrl_algos.h), the template the kernel instantiates -- and checks that the planes are those of the edited bytes, built here the way
// planes_from_tiles (reset_env.h, device only) builds them, that only the owning row changed, and that the working planes, which go on
// from entry to entry, are the level's again after each reload.  The kernel's own staging, LDS copy and reload are covered on the GPU,
// entry by entry against the oracle (tests/test_gpu_changes.py).  Built as a shared library for tests/test_changes_host.py and, with
// -DSIM_CHANGES_MAIN -fsanitize=address,undefined, as a stand-alone program that runs built-in levels of the GPU tests' shapes through
// every (lane group, mask width) form.
#include "sim_algos.cpp"
#include "sim_forms.h"

template <int G, class T>
static bool same(const SimVec<T, G>& a, const SimVec<T, G>& b) { return memcmp(a.v, b.v, sizeof(a.v)) == 0; }

// the number of (cell, tile) pairs checked, or -(entry + 1) of the first that fails; -1 000 000 000: the form does not hold the map
template <int G, class T>
static long run_changes(SimGroup<G, T>, const uint8_t* map, int h, int w, int ntiles) {
    typedef SimVec<T, G> M;
    if (h > G || w > (int)(8 * sizeof(T)) || ntiles > 8) return -1000000000L;
    M k0, k1, k2;                                                        // the kept copy: written once per level
    planes_of(map, h, w, k0, k1, k2);
    std::vector<uint8_t> edited(map, map + (size_t)h * w);
    long n = 0;
    M b0, b1, b2;                                                        // the working planes: edited in place, entry after entry
    for (int c = 0; c < h * w; c++) {
        for (int t = 0; t < ntiles; t++, n++) {
            b0 = k0; b1 = k1; b2 = k2;                                   // the restore: a reload of the kept copy
            {
                M l0, l1, l2;
                planes_of(map, h, w, l0, l1, l2);
                if (!same(b0, l0) || !same(b1, l1) || !same(b2, l2)) return -(n + 1);      // after the entry before: the level's again
            }
            const int y = c / w, x = c - y * w;
            planes_set_cell(b0.v[y], b1.v[y], b2.v[y], x, t);           // the lane that owns row y
            edited[c] = (uint8_t)t;
            M r0, r1, r2;
            planes_of(edited.data(), h, w, r0, r1, r2);
            edited[c] = map[c];
            if (!same(b0, r0) || !same(b1, r1) || !same(b2, r2)) return -(n + 1);
            for (int r = 0; r < G; r++)
                if (r != y && (b0.v[r] != k0.v[r] || b1.v[r] != k1.v[r] || b2.v[r] != k2.v[r])) return -(n + 1);
            if (t == map[c] && (!same(b0, k0) || !same(b1, k1) || !same(b2, k2))) return -(n + 1);      // the tile it holds: nothing changes
        }
    }
    return n;
}

extern "C" {
// group = 16 or 64 lanes, mask_bits = 32 or 64
long sim_changes(const uint8_t* map, int h, int w, int ntiles, int group, int mask_bits) {
    return sim_with_form(group, mask_bits, -1000000000L, [&](auto g) { return run_changes(g, map, h, w, ntiles); });
}
}

#ifdef SIM_CHANGES_MAIN
static SimLcg lcg = {2025u};

int main() {
    // (tiles, rows, columns): binary and zelda at the shapes of tests/test_gpu_changes.py
    const int shapes[9][3] = {{2, 1, 1}, {2, 3, 5}, {2, 16, 32}, {2, 16, 33}, {2, 17, 32}, {2, 17, 33}, {2, 64, 64}, {8, 7, 11}, {8, 17, 33}};
    long checked = 0;
    int forms_seen = 0;
    for (int si = 0; si < 9; si++) {
        const int nt = shapes[si][0], h = shapes[si][1], w = shapes[si][2];
        for (int rep = 0; rep < 3; rep++) {             // random, all of the first tile, all of the last
            std::vector<uint8_t> map((size_t)h * w);
            for (auto& t : map) t = rep == 0 ? (uint8_t)(lcg() % nt) : (rep == 1 ? 0 : (uint8_t)(nt - 1));
            for (int f = 0; f < 4; f++) {
                if (h > SIM_FORMS[f][0] || w > SIM_FORMS[f][1]) continue;
                const long n = sim_changes(map.data(), h, w, nt, SIM_FORMS[f][0], SIM_FORMS[f][1]);
                if (n != (long)h * w * nt) { printf("shape %d x %d form %d/%d: %ld\n", h, w, SIM_FORMS[f][0], SIM_FORMS[f][1], n); return 2; }
                checked += n;
                forms_seen |= 1 << f;
            }
        }
    }
    if (forms_seen != 15) return 3;
    printf("entries %ld\nok\n", checked);
    return 0;
}
#endif
