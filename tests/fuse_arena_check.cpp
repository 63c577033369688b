// Host-only check of fuse_layout (stella_vslam_amd/csrc/fuse_layout.h): the smallest and the largest shape of tests/test_gpu_fuse_chain.py,
// stereo slots beside monocular ones, an empty target, the results as one range, the prefix invariant across the two passes (lists off, of
// capacity 1, of a capacity past 1 MiB), and the two sizing rules.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fuse_layout.h"
#include "layout_check.h"

static Rows rows_of(const FusePieces& Y, const FuseShape& S, bool lists, size_t cap) {
    const size_t slots = S.kf_n.size(), K = slots - 1, L = S.num_landmarks, E = S.num_entries, O = S.num_observers, l = lists ? cap : 0;
    size_t N = 0, NX = 0, NC = 0, nt_max = 0;
    for (size_t u = 0; u < slots; ++u) {
        N += (size_t)S.kf_n[u];
        if (S.kf_xright[u]) NX += (size_t)S.kf_n[u];
        NC += ((size_t)S.kf_cells[u] + 1 + 63) / 64 * 64;
        nt_max = std::max(nt_max, (size_t)S.kf_n[u]);
    }
    const size_t rows = std::max(S.n_fwd, S.n_bwd), n_out = K * S.n_fwd + S.n_bwd;
    return Rows{{Y.desc, N * 32}, {Y.xy, N * 8}, {Y.octave, N * 4}, {Y.xright, NX * 4}, {Y.kp_lm, N * 4}, {Y.kf_tab, slots * S.kf_rec},
                {Y.observer_rank, O * 4}, {Y.observer_kf, O * 4}, {Y.observer_twc, O * 24}, {Y.pos_w, L * 24}, {Y.ref_twc, L * 24}, {Y.ref_sf, L * 4},
                {Y.obs_off, L * 4}, {Y.obs_cap, L * 4}, {Y.alive, L}, {Y.lm_desc, L * 32}, {Y.mean_normal, L * 24}, {Y.min_d, L * 4}, {Y.max_d, L * 4},
                {Y.has_desc, L}, {Y.has_geom, L}, {Y.obs_cnt, L * 4}, {Y.replaced_by, L * 4}, {Y.obs_observer, E * 4}, {Y.obs_kp, E * 4},
                {Y.obs_desc, E * 32}, {Y.obs_weight, E * 4}, {Y.fwd_list, S.n_fwd * 4}, {Y.bwd_list, S.n_bwd * 4}, {Y.cell_of, N * 4}, {Y.cell_off, NC * 4},
                {Y.cell_items, N * 4}, {Y.visible, rows}, {Y.reproj, rows * 16}, {Y.x_right, rows * 4}, {Y.q_xy, rows * 8}, {Y.q_margin, rows * 4},
                {Y.q_min_level, rows * 4}, {Y.q_max_level, rows * 4}, {Y.cand_off, (rows + 1) * 4}, {Y.hit_lm, rows * 4}, {Y.owner, nt_max * 4},
                {Y.match, rows * 4}, {Y.touch, L * 4}, {Y.total0, (K + 1) * 4}, {Y.flag, 4}, {Y.best, n_out * 4}, {Y.event, n_out},
                {Y.num_fused, (K + 1) * 4}, {Y.cand_idx, l * 4}, {Y.dist, l * 4}};
}

static void check(const char* what, FuseShape S) {
    S.kf_rec = 48, S.grid_rec = 136;
    const size_t caps[3] = {0, 1, (size_t(1) << 18) + 1};
    std::vector<Rows> placed;
    for (const size_t cap : caps) {
        char name[160];
        std::snprintf(name, sizeof name, "%s lists %zu", what, cap);
        layout_check<FusePieces>(
            name, [&](Arena& A, FusePieces& Y) { fuse_layout(A, S, cap > 0, cap, Y); }, [&](const FusePieces& Y) { return rows_of(Y, S, cap > 0, cap); },
            [&](const FusePieces& Y, const char* base, size_t) {
                size_t first = 0, fx = 0, fc = 0;
                for (size_t u = 0; u < S.kf_n.size(); ++u) {  // a slot's arrays lie inside the concatenations in slot order; its counters start aligned
                    CHECK(Y.first[u] == first && Y.first_cell[u] == fc && fc % 64 == 0);
                    CHECK(S.kf_xright[u] ? Y.first_xr[u] == fx : Y.first_xr[u] == ~size_t(0));
                    first += (size_t)S.kf_n[u], fc += ((size_t)S.kf_cells[u] + 1 + 63) / 64 * 64;
                    if (S.kf_xright[u]) fx += (size_t)S.kf_n[u];
                }
                CHECK((const char*)Y.best.p + pad(Y.best.bytes()) == (const char*)Y.event.p);  // the results: one range
                CHECK((const char*)Y.event.p + pad(Y.event.bytes()) == (const char*)Y.num_fused.p);
                Rows rr = rows_of(Y, S, cap > 0, cap);
                for (Row& x : rr) x.p = x.p ? (const char*)(x.p - base) : nullptr;
                placed.push_back(rr);
            });
    }
    for (size_t v = 1; v < placed.size(); ++v) {  // the prefix invariant: the lists come last and move nothing
        const Rows &a = placed[0], &b = placed[v];
        CHECK(a.size() == b.size());
        for (size_t i = 0; i + 2 < a.size(); ++i) CHECK(a[i].p == b[i].p && a[i].touched == b[i].touched);
        const Row &ci = b[b.size() - 2], &di = b[b.size() - 1];
        for (size_t i = 0; i + 2 < b.size(); ++i)
            if (b[i].touched) CHECK(b[i].p + b[i].touched <= ci.p);
        CHECK(ci.p + ci.touched <= di.p);
    }
}

int main() {
    {  // smallest: one target
        FuseShape S;
        S.kf_n = {100, 100}, S.kf_xright = {0, 0}, S.kf_cells = {3072, 3072};
        S.num_observers = 4, S.num_landmarks = 90, S.num_entries = 90 * 12, S.n_fwd = 100, S.n_bwd = 30;
        check("single", S);
    }
    {  // stereo beside monocular slots, an empty target, a backward list longer than the forward list
        FuseShape S;
        S.kf_n = {100, 0, 164}, S.kf_xright = {1, 0, 1}, S.kf_cells = {3072, 3072, 12};
        S.num_observers = 5, S.num_landmarks = 93, S.num_entries = 1300, S.n_fwd = 100, S.n_bwd = 140;
        check("stereo with an empty target", S);
    }
    {  // largest: twelve targets
        FuseShape S;
        S.kf_n.assign(13, 64), S.kf_xright.assign(13, 0), S.kf_cells.assign(13, 3072);
        S.kf_n[0] = 8192;
        S.num_observers = 15, S.num_landmarks = 4000, S.num_entries = 4000 * 24, S.n_fwd = 8192, S.n_bwd = 700;
        check("twelve targets", S);
    }
    // the sizing rules
    const int32_t t0[4] = {10, 0, 300, 7};
    CHECK(fuse_cand_capacity(t0, 4) == FUSE_CAND_FACTOR * 300 + FUSE_CAND_SLACK);
    const int32_t none[2] = {0, 0};
    CHECK(fuse_cand_capacity(none, 2) == FUSE_CAND_SLACK && fuse_cand_capacity(none, 0) == FUSE_CAND_SLACK);
    CHECK(fuse_obs_capacity(3, 5) == 3 + 5 + FUSE_OBS_SLACK && fuse_obs_capacity(0, 1) <= FUSE_OBS_CAP_MAX);
    return layout_check_result("fuse arena ok");
}
