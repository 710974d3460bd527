// What the read-outs' simulators (sim_paths.cpp, sim_tile_graph.cpp, sim_changes.cpp) share.  TEST ONLY; included after sim_algos.cpp.
#pragma once

// the kernels' (lane group, mask width) forms: the table the stand-alone programs walk, and the form a (group, mask_bits) pair names --
// f(SimGroup<G, T>()), or `none` for a pair that names no form
static const int SIM_FORMS[4][2] = {{16, 32}, {16, 64}, {64, 32}, {64, 64}};
template <class R, class F>
static R sim_with_form(int group, int mask_bits, R none, F f) {
    if (group == 16 && mask_bits == 32) return f(SimGroup<16, uint32_t>());
    if (group == 16 && mask_bits == 64) return f(SimGroup<16, uint64_t>());
    if (group == 64 && mask_bits == 32) return f(SimGroup<64, uint32_t>());
    if (group == 64 && mask_bits == 64) return f(SimGroup<64, uint64_t>());
    return none;
}

// the generator behind the stand-alone programs' levels: `static SimLcg lcg = {seed};`, then lcg()
struct SimLcg {
    unsigned state;
    unsigned operator()() { state = state * 1664525u + 1013904223u; return state >> 8; }
};

// the three row planes of a byte map (planes_from_tiles, reset_env.h, is device only): bit x of lane y's word p = bit p of the tile at (y, x)
template <int G, class T>
static void planes_of(const uint8_t* map, int h, int w, SimVec<T, G>& b0, SimVec<T, G>& b1, SimVec<T, G>& b2) {
    b0 = SimVec<T, G>(); b1 = SimVec<T, G>(); b2 = SimVec<T, G>();
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const T t = map[y * w + x];
            b0.v[y] |= (t & 1) << x; b1.v[y] |= ((t >> 1) & 1) << x; b2.v[y] |= ((t >> 2) & 1) << x;
        }
}
