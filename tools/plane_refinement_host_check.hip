// Stand-alone host program over csrc/plane_refinement.hpp for a sanitizer build (no GPU, no Python): refinement() as the host build runs it, on
// heap buffers of exact size -- three lists of one plane (two of equal size, shared and erased members, an entry that names no landmark), a plane
// apart from them, an invalid row between them and a row that is not in the database; then the same map with lists that have no room for the
// merge (OVERFLOW: nothing of the merge is written), a single plane (TOO_FEW_PLANES: no table touched) and each stage alone.
//
//   hipcc -std=c++17 -O1 -g -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/plane_refinement_host_check.hip -o plane_refinement_host_check
//   ./plane_refinement_host_check           # prints one line per scene and "ok"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../structure-plp-slam_amd/csrc/plane_refinement.hpp"

using namespace plp;

namespace {
struct Lcg {                                          // a small generator of the program's own
    uint64_t s;
    double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
    double sym() { return 2.0 * next() - 1.0; }
};

struct Scene {
    int NP, n_cap, L;
    std::unique_ptr<uint8_t[]> state, erased, status, merged, planes, points, removed, update_status, lm_changed, mark_guard;
    std::unique_ptr<double[]> eq, best, pos, dist, err;
    std::unique_ptr<int32_t[]> count, lm, owner, num_merges, merges, num_updates;
    PlaneRefArgs A{};
};

// rows: 0 z = 1 (40 members), 1 invalid, 2 z = 1 (40, shares 5 with row 0), 3 x = 3 (40), 4 not in the database, 5 z = 1 (25, three erased)
std::unique_ptr<Scene> make_scene(int n_cap, int rows, int stages) {
    auto S = std::make_unique<Scene>();
    const int NP = rows, L = 200;
    S->NP = NP; S->n_cap = n_cap; S->L = L;
    S->state.reset(new uint8_t[NP]); S->eq.reset(new double[4 * (size_t)NP]); S->best.reset(new double[NP]); S->count.reset(new int32_t[NP]);
    S->lm.reset(new int32_t[(size_t)NP * n_cap]); S->pos.reset(new double[3 * (size_t)L]); S->erased.reset(new uint8_t[L]); S->owner.reset(new int32_t[L]);
    S->dist.reset(new double[1]{0.02}); S->err.reset(new double[1]{0.002});
    S->status.reset(new uint8_t[1]); S->merged.reset(new uint8_t[1]); S->planes.reset(new uint8_t[1]); S->points.reset(new uint8_t[1]);
    S->removed.reset(new uint8_t[NP]); S->num_merges.reset(new int32_t[1]); S->merges.reset(new int32_t[2 * 2]); S->num_updates.reset(new int32_t[1]);
    S->update_status.reset(new uint8_t[NP]); S->lm_changed.reset(new uint8_t[L]);
    Lcg g{91};
    for (int l = 0; l < L; ++l) { S->erased[l] = 0; S->owner[l] = -1; S->pos[3 * l] = S->pos[3 * l + 1] = S->pos[3 * l + 2] = 0.0; }
    for (size_t k = 0; k < (size_t)NP * n_cap; ++k) S->lm[k] = -9;
    const int first[6] = {0, 40, 60, 95, 135, 150}, members[6] = {40, 20, 40, 40, 15, 25};
    const uint8_t st[6] = {3, 1, 3, 3, 6, 3};
    for (int r = 0; r < NP; ++r) {
        const bool wall = r == 3;
        S->state[r] = st[r]; S->best[r] = 1.0; S->count[r] = members[r] < n_cap ? members[r] : n_cap;
        const double e[4] = {wall ? 1.0 : 0.0, 0.0, wall ? 0.0 : 1.0, wall ? -3.0 : -1.0};
        for (int i = 0; i < 4; ++i) S->eq[4 * r + i] = e[i];
        for (int s = 0; s < S->count[r]; ++s) {
            int l = first[r] + s;
            if (r == 2 && s < 5) l = 35 + s;              // shared with row 0
            S->lm[(size_t)r * n_cap + s] = l;
            if (r == 2 && s < 5) continue;
            const double a = 2.0 * g.sym(), b = 2.0 * g.sym(), h = 0.004 * g.sym();
            S->pos[3 * l] = wall ? 3.0 + h : a; S->pos[3 * l + 1] = b; S->pos[3 * l + 2] = wall ? a : 1.0 + h;
            S->owner[l] = r;
        }
    }
    if (NP > 5) {
        for (int s = 20; s < 23; ++s) S->erased[first[5] + s] = 1;
        S->lm[(size_t)5 * n_cap + 24] = 5000;             // names no landmark
    }
    PlaneRefArgs& A = S->A;
    A.G = 1; A.NP_cap = NP; A.n_cap = n_cap; A.L = L; A.merge_cap = 2; A.stages = stages; A.points_per_ransac = 18; A.iters = 8; A.offset_delta_factor = 6;
    A.dot_thr = 0.8; A.seed = 42;
    A.pl_state = S->state.get(); A.pl_equation = S->eq.get(); A.pl_best_error = S->best.get(); A.pl_count = S->count.get(); A.pl_lm = S->lm.get();
    A.pos_w = S->pos.get(); A.lm_erased = S->erased.get(); A.lm_owner = S->owner.get(); A.dist_thresh = S->dist.get(); A.error_thresh = S->err.get();
    A.out_status = S->status.get(); A.out_was_merged = S->merged.get(); A.out_planes_changed = S->planes.get(); A.out_points_changed = S->points.get();
    A.out_removed = S->removed.get(); A.out_num_merges = S->num_merges.get(); A.out_merges = S->merges.get(); A.out_num_updates = S->num_updates.get();
    A.out_update_status = S->update_status.get(); A.out_lm_changed = S->lm_changed.get();
    return S;
}

int run(Scene& S) {
    std::vector<uint8_t> mark((size_t)S.L, 0);
    plane_ref_model_problem(S.A, 0, mark);
    for (uint8_t m : mark)
        if (m) return -1;                                 // the marks are left as they were
    return S.status[0];
}
}  // namespace

int main() {
    bool good = true;
    {
        auto S = make_scene(128, 6, 7);
        const int st = run(*S);
        int in_db = 0, moved = 0;
        for (int r = 0; r < 6; ++r) in_db += S->state[r] & 1;
        for (int l = 0; l < S->L; ++l) moved += S->lm_changed[l];
        std::printf("refinement(): status %d, %d merges (%d listed: %d<-%d, %d<-%d), %d updates, %d rows left, %d landmarks moved\n", st, S->num_merges[0], 2,
                    S->merges[0], S->merges[1], S->merges[2], S->merges[3], S->num_updates[0], in_db, moved);
        good = good && st == PLP_PLANE_REFINEMENT_OK && S->merged[0] == 1 && S->num_merges[0] == 2 && S->merges[0] == 2 && S->merges[1] == 0 && S->merges[2] == 0 && S->merges[3] == 5 && S->removed[1] == 2 &&
               S->removed[4] == 0 && (S->state[4] == 6) && S->owner[150 + 20] == -1 && moved > 20;
    }
    {
        auto S = make_scene(41, 6, 7);
        const int st = run(*S);
        bool untouched = S->count[0] == 40 && S->count[2] == 40 && S->state[0] == 3 && S->state[2] == 3 && S->owner[0] == 0 && S->owner[60 + 5] == 2;
        std::printf("lists of 41 slots: status %d, the pair %s\n", st, untouched ? "as it was" : "WRITTEN");
        good = good && st == PLP_PLANE_REFINEMENT_OVERFLOW && untouched;
    }
    {
        auto S = make_scene(64, 1, 7);
        const int st = run(*S);
        std::printf("one plane: status %d\n", st);
        good = good && st == PLP_PLANE_REFINEMENT_TOO_FEW_PLANES && S->state[0] == 3 && S->count[0] == 40 && S->update_status[0] == kPlaneRefNoUpdate;
    }
    for (int stages : {1, 2, 4}) {
        auto S = make_scene(128, 6, stages);
        const int st = run(*S);
        std::printf("stages %d: status %d, merged %d, planes changed %d, points changed %d\n", stages, st, S->merged[0], S->planes[0], S->points[0]);
        good = good && st == PLP_PLANE_REFINEMENT_OK && (S->merged[0] != 0) == (stages == 1) && (S->points[0] != 0) == (stages == 4);
    }
    {   // the walk of the candidate loop against the loop as written, on every validity pattern of 10 entries
        int bad = 0;
        for (int pattern = 0; pattern < 1024; ++pattern) {
            bool tested[10] = {};
            for (int j = 0; j < 10; ++j) {                // planar_mapping_module.cc:826-835
                if (!((pattern >> j) & 1)) {
                    j++;
                    if (j >= 10) break;
                }
                tested[j] = true;
            }
            int before = 0;
            for (int j = 0; j < 10; ++j) {
                const bool valid = (pattern >> j) & 1;
                if (plane_candidate_tested(valid, before) != tested[j]) ++bad;
                before = valid ? 0 : before + 1;
            }
        }
        std::printf("candidate walk: %d differences\n", bad);
        good = good && bad == 0;
    }
    good = good && plane_pair_test(std::unique_ptr<double[]>(new double[4]{0, 0, 2, -2}).get(), std::unique_ptr<double[]>(new double[4]{0, 0, 1, -1.05}).get(), 0.12, 0.8) == kPlanePairMerge;
    std::printf("%s\n", good ? "ok" : "FAILED");
    return good ? 0 : 1;
}
