// CPU lane-group simulator for the touch -> resume route of the binary statistics (pcgrl_algos.h: binary_touch with a memo,
// rlp_resume).  TEST ONLY.  Built on the simulator backend of sim_algos.cpp (included as it is).
//
// sim_touch_resume walks a map through single-cell flips with the routing of the step kernels -- binary_incremental away from the
// champion, binary_touch in or next to it, rlp_resume with the touch's memo when it gives up, rlp_resume with an empty memo for want
// of a champion -- and checks the carried state by brute force after EVERY step:
//   * the champion is one whole component of the map and its double sweep equals the path, or it is empty and the path is the
//     closed-form value of the tiny components;
//   * ub2 is at least the double-sweep value of every other component.
// Regions and path of every step go back to the caller (tests/test_hostsim_touch_resume.py compares them with the oracle).
// The program's own main() runs the same walks against the plain recomputation: a stand-alone binary for the sanitizers.
#include "sim_algos.cpp"

// components of `pass` by a plain cell flood (no bitboard program involved)
template <int G, class T>
static void brute_components(const typename SimGroup<G, T>::mask_t& pass, int h, int w, std::vector<typename SimGroup<G, T>::mask_t>& out) {
    typedef typename SimGroup<G, T>::mask_t M;
    M seen;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            if (!((pass.v[y] >> x) & 1) || ((seen.v[y] >> x) & 1)) continue;
            M comp;
            std::vector<int> stack(1, y * w + x);
            comp.v[y] |= (T)1 << x;
            while (!stack.empty()) {
                const int c = stack.back(); stack.pop_back();
                const int cy = c / w, cx = c % w;
                const int dy[4] = {-1, 1, 0, 0}, dx[4] = {0, 0, -1, 1};
                for (int d = 0; d < 4; d++) {
                    const int ny = cy + dy[d], nx = cx + dx[d];
                    if (ny < 0 || ny >= h || nx < 0 || nx >= w) continue;
                    if (!((pass.v[ny] >> nx) & 1) || ((comp.v[ny] >> nx) & 1)) continue;
                    comp.v[ny] |= (T)1 << nx;
                    stack.push_back(ny * w + nx);
                }
            }
            for (int r = 0; r < G; r++) seen.v[r] |= comp.v[r];
            out.push_back(comp);
        }
}

// 0 = the state is sound; else which invariant broke (1: champion is no whole component, 2: its sweep is not the path, 3: no
// champion but the path is not the tiny components', 4: ub2 below another component's value, 5: ub2 above the path or unknown)
template <int G, class T>
static int check_state(const typename SimGroup<G, T>::mask_t& pass, int h, int w, int path, const typename SimGroup<G, T>::mask_t& champ, int ub2) {
    typedef SimGroup<G, T> Gp;
    typedef typename Gp::mask_t M;
    Gp g;
    const int spur = g_spurious; g_spurious = 0;
    std::vector<M> comps;
    brute_components<G, T>(pass, h, w, comps);
    int err = 0, champ_at = -1, best_small = 0;
    for (size_t i = 0; i < comps.size(); i++) {
        const int n = g.popcount_sum(comps[i]);
        if (n <= 3 && n - 1 > best_small) best_small = n - 1;
        if (g.any(champ & comps[i])) { if (g.any(champ ^ comps[i]) || champ_at >= 0) err = 1; champ_at = (int)i; }
    }
    if (!err && g.any(champ) && champ_at < 0) err = 1;
    if (!err && champ_at >= 0 && pcg_double_sweep(g, champ, -1) != path) err = 2;
    if (!err && champ_at < 0 && path != best_small) err = 3;
    if (!err && (ub2 < 0 || ub2 > path)) err = 5;
    for (size_t i = 0; i < comps.size() && !err; i++)
        if ((int)i != champ_at && pcg_double_sweep(g, comps[i], -1) > ub2) err = 4;
    g_spurious = spur;
    return err;
}

// counts: [0] incremental, [1] touches, [2] touches given up and resumed, [3] of those removals, [4] of those additions, [5] plain
// computations for want of a champion, [6] touches of the parent's route on the same walk, [7] of those given up.
// Returns 0, or (step + 1) * 8 + the broken invariant of check_state.
template <int G, class T>
static long run_touch_resume(const uint8_t* map0, int h, int w, const int* flips, int nflips, int32_t* out, long* counts) {
    typedef SimGroup<G, T> Gp;
    typedef typename Gp::mask_t M;
    Gp g;
    M pass;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) if (!(map0[y * w + x] & 1)) pass.v[y] |= (T)1 << x;
    int regions, path, ub2 = -1;
    M champ;
    regions_and_longest_path(g, pass, regions, path, champ, ub2);      // (a reset's statistics)
    // the parent's route next to it, with a state of its own: how often IT gives up on this walk
    int p_regions = regions, p_path = path, p_ub2 = ub2;
    M p_champ = champ;
    out[0] = regions; out[1] = path;
    for (int f = 0; f < nflips; f++) {
        const int y = flips[f] / w, x = flips[f] % w;
        M cbit; cbit.v[y] = (T)1 << x;
        const bool added = !(pass.v[y] >> x & 1);
        pass.v[y] ^= (T)1 << x;
        int r2, p2, u2; M c2;
        if (!g.any(champ) || ub2 < 0) {
            rlp_resume(g, pass, touch_memo_empty(g, pass), r2, p2, c2, u2);
            counts[5]++;
        } else if (g.any(pcg_expand(g, cbit) & champ)) {
            TouchMemo<M> memo;
            counts[1]++;
            if (!binary_touch(g, pass, cbit, added, regions, champ, ub2, r2, p2, c2, u2, memo)) {
                counts[2]++; counts[added ? 4 : 3]++;
                rlp_resume(g, pass, memo, r2, p2, c2, u2);
            }
        } else {
            binary_incremental(g, pass, cbit, added, regions, path, champ, ub2, r2, p2, c2, u2);
            counts[0]++;
        }
        regions = r2; path = p2; champ = c2; ub2 = u2;
        out[2 * (f + 1)] = regions; out[2 * (f + 1) + 1] = path;
        if (g.any(champ) || ub2 >= 0) {      // (no champion and no bound: nothing is carried, the next change computes in full)
            const int err = check_state<G, T>(pass, h, w, path, champ, ub2);
            if (err) return (long)(f + 1) * 8 + err;
        }
        {
            const int spur = g_spurious; g_spurious = 0;
            if (!g.any(p_champ) || p_ub2 < 0) regions_and_longest_path(g, pass, p_regions, p_path, p_champ, p_ub2);
            else if (g.any(pcg_expand(g, cbit) & p_champ)) {
                counts[6]++;
                if (binary_touch(g, pass, cbit, added, p_regions, p_champ, p_ub2, r2, p2, c2, u2)) { p_regions = r2; p_path = p2; p_champ = c2; p_ub2 = u2; }
                else { regions_and_longest_path(g, pass, p_regions, p_path, p_champ, p_ub2); counts[7]++; }
            } else {
                binary_incremental(g, pass, cbit, added, p_regions, p_path, p_champ, p_ub2, r2, p2, c2, u2);
                p_regions = r2; p_path = p2; p_champ = c2; p_ub2 = u2;
            }
            g_spurious = spur;
            if (p_regions != regions || p_path != path) return (long)(f + 1) * 8 + 6;      // 6: the two routes disagree
        }
    }
    return 0;
}

extern "C" long sim_touch_resume(const uint8_t* map0, int h, int w, const int* flips, int nflips, int32_t* out, long* counts) {
    if (w > 32) return run_touch_resume<16, uint64_t>(map0, h, w, flips, nflips, out, counts);
    return run_touch_resume<16, uint32_t>(map0, h, w, flips, nflips, out, counts);
}

// Stand-alone: the walks of the test (shapes, densities, spurious rounds) with a generator of its own; regions and path of every
// step against the plain recomputation of the map.
int main() {
    const int shapes[7][2] = {{14, 14}, {16, 11}, {5, 5}, {9, 32}, {3, 7}, {16, 40}, {1, 9}};
    const double dens[3] = {0.3, 0.5, 0.65};
    unsigned rng = 2463534242u;
    auto next = [&rng]() { rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5; return rng; };
    long counts[8] = {0, 0, 0, 0, 0, 0, 0, 0}, steps = 0;
    for (int s = 0; s < 7; s++)
        for (int d = 0; d < 3; d++) {
            const int h = shapes[s][0], w = shapes[s][1], T = (h == 14 && d == 1) ? 6000 : 400;
            std::vector<uint8_t> map(h * w);
            for (auto& c : map) c = (next() % 1000) < dens[d] * 1000 ? 1 : 0;
            std::vector<int> flips(T);
            for (auto& c : flips) c = (int)(next() % (unsigned)(h * w));
            std::vector<int32_t> out(2 * (T + 1));
            g_spurious = (int)(next() % 30);
            const long rc = sim_touch_resume(map.data(), h, w, flips.data(), T, out.data(), counts);
            g_spurious = 0;
            if (rc) { printf("FAIL %dx%d density %.2f: step %ld, invariant %ld\n", h, w, dens[d], rc / 8 - 1, rc % 8); return 1; }
            for (int t = 0; t <= T; t++) {
                if (t > 0) map[flips[t - 1]] ^= 1;
                int32_t ref[8]; int ns;
                if (w > 32) run<16, uint64_t>(PCGRL_PROB_BINARY, map.data(), h, w, w, h, ref, &ns);
                else run<16, uint32_t>(PCGRL_PROB_BINARY, map.data(), h, w, w, h, ref, &ns);
                if (ref[0] != out[2 * t] || ref[1] != out[2 * t + 1]) {
                    printf("FAIL %dx%d density %.2f: step %d gives (%d, %d), the recomputation (%d, %d)\n", h, w, dens[d], t - 1, out[2 * t], out[2 * t + 1], ref[0], ref[1]);
                    return 1;
                }
            }
            steps += T;
        }
    printf("ok: %ld steps; incremental %ld, touches %ld, resumed %ld (removals %ld, additions %ld), plain %ld; parent's route: touches %ld, given up %ld\n",
           steps, counts[0], counts[1], counts[2], counts[3], counts[4], counts[5], counts[6], counts[7]);
    return 0;
}
