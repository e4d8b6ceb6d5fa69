// Stand-alone host program over csrc/covisibility.hpp for a sanitizer build (no GPU, no Python): a generated map of 90 key frames of up to 70
// slots and 1200 landmarks with erased rows, rows outside their tables, counts below and above the row width and a landmark in two slots; an
// owner list with a row outside the table and a repeat through cv_count and cv_apply, once with tables wide enough and once with both caps too
// short, then an erase of a dozen key frames through cv_erase, with a team of one lane, on heap buffers of exact size.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/covisibility_host_check.hip -o covisibility_host_check
//   ./covisibility_host_check        # prints the counts of every pass and "ok"
#include <cstdio>
#include <memory>
#include <vector>

#include "../structure-plp-slam_amd/csrc/covisibility.hpp"

using namespace plp;

static uint32_t rnd_state = 2323u;
static int rnd(int n) { rnd_state = rnd_state * 1664525u + 1013904223u; return (int)((rnd_state >> 8) % (uint32_t)n); }

template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) {     // a heap block of exactly the vector's size
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

// the rows of a state are well-formed: lengths within reason, C ascending and inside the table, O a permutation of a subset of C in descending key
static bool well_formed(const CvArgs& A, const uint8_t* touched, int* n_over) {
    bool good = true;
    for (int j = 0; j < A.F; ++j) {
        if (touched[j] == 2) { ++*n_over; continue; }
        const int nc = A.kf_n_conn[j], no = A.kf_n_covis[j];
        good = good && 0 <= nc && nc <= A.conn_cap && 0 <= no && no <= A.covis_cap && no <= nc;
        if (!good) return false;
        for (int i = 0; i < A.conn_cap; ++i) {
            const int r = A.kf_conn[(size_t)j * A.conn_cap + i];
            if (touched[j] == 0) continue;
            good = good && (i < nc ? (0 <= r && r < A.F && r != j && (i == 0 || A.kf_conn[(size_t)j * A.conn_cap + i - 1] < r)) : r == -1);
        }
        for (int i = 0; i + 1 < no; ++i) {
            const size_t at = (size_t)j * A.covis_cap + i;
            good = good && cv_key(A.kf_covis_w[at], A.kf_covis[at]) > cv_key(A.kf_covis_w[at + 1], A.kf_covis[at + 1]);
        }
        for (int i = 0; i < no; ++i) {
            const size_t at = (size_t)j * A.covis_cap + i;
            const int c = cv_find(A.kf_conn + (size_t)j * A.conn_cap, nc, A.kf_covis[at]);
            good = good && c >= 0 && A.kf_conn_w[(size_t)j * A.conn_cap + c] == A.kf_covis_w[at];
        }
    }
    return good;
}

int main() {
    const int F = 90, L = 1200, cap = 70;
    std::vector<int32_t> kf_lm((size_t)F * cap, -1), kf_counts(F), off(L + 1, 0), obs_kf;
    std::vector<uint32_t> kf_id(F);
    std::vector<uint8_t> lm_erased(L);
    std::vector<int> used(F, 0);
    for (int f = 0; f < F; ++f) kf_id[f] = f == 4 ? 0u : 20u + f;
    for (int l = 0; l < L; ++l) {
        lm_erased[l] = rnd(25) == 0;
        const int n = l % 200 == 9 ? 40 : rnd(9);
        for (int i = 0; i < n; ++i) {
            const int kf = (l / 14 + rnd(n == 40 ? F : 7)) % F;
            if (used[kf] >= cap - 2) continue;
            kf_lm[(size_t)kf * cap + used[kf]++] = l;
            obs_kf.push_back(rnd(70) == 0 ? F + 1 : rnd(70) == 0 ? -2 : kf);
        }
        off[l + 1] = (int32_t)obs_kf.size();
    }
    for (int f = 0; f < F; ++f) {
        kf_counts[f] = f == 3 ? cap + 4 : f == 6 ? -1 : f == 50 ? 0 : cap;
        kf_lm[(size_t)f * cap + used[f]] = rnd(2) ? L + 5 : -9;                        // a row outside the table behind the last landmark
        if (used[f] > 0) kf_lm[(size_t)f * cap + used[f] + 1] = kf_lm[(size_t)f * cap];   // a landmark in two slots
    }
    std::vector<int32_t> owners;
    for (int i = 0; i < F; ++i) owners.push_back((i * 37) % F);
    owners[10] = F; owners[20] = -1; owners[30] = owners[5];
    const int G = (int)owners.size();
    auto p_kl = exact(kf_lm); auto p_kc = exact(kf_counts); auto p_of = exact(off); auto p_ok = exact(obs_kf); auto p_le = exact(lm_erased);
    auto p_id = exact(kf_id); auto p_ow = exact(owners);
    auto sh = std::make_unique<CvShared>();
    LmTeamHost par;
    bool good = true;
    for (int pass = 0; pass < 2; ++pass) {
        const int conn_cap = pass == 0 ? F : 62, covis_cap = pass == 0 ? F : 5;
        auto conn = exact(std::vector<int32_t>((size_t)F * conn_cap, -1)); auto conn_w = exact(std::vector<int32_t>((size_t)F * conn_cap, 0));
        auto covis = exact(std::vector<int32_t>((size_t)F * covis_cap, -1)); auto covis_w = exact(std::vector<int32_t>((size_t)F * covis_cap, 0));
        auto n_conn = exact(std::vector<int32_t>(F, 0)); auto n_covis = exact(std::vector<int32_t>(F, 0));
        auto parent = exact(std::vector<int32_t>(F, -1)); auto unset = exact(std::vector<uint8_t>(F, 1));
        auto status = exact(std::vector<uint8_t>(G, 99)); auto nearest = exact(std::vector<int32_t>(G, -9)); auto maxw = exact(std::vector<int32_t>(G, -9));
        auto touched = exact(std::vector<uint8_t>(F, 99));
        auto ws = exact(std::vector<int32_t>(cv_scratch_words(F, G, conn_cap, covis_cap), -1));
        CvArgs A{};
        A.F = F; A.L = L; A.T = (int)obs_kf.size(); A.cap = cap; A.G = G; A.conn_cap = conn_cap; A.covis_cap = covis_cap;
        A.kf_lm = p_kl.get(); A.kf_counts = p_kc.get(); A.obs_offsets = p_of.get(); A.obs_kf = p_ok.get(); A.lm_erased = p_le.get(); A.kf_id = p_id.get();
        A.kf_conn = conn.get(); A.kf_conn_w = conn_w.get(); A.kf_n_conn = n_conn.get(); A.kf_covis = covis.get(); A.kf_covis_w = covis_w.get();
        A.kf_n_covis = n_covis.get(); A.kf_parent = parent.get(); A.kf_parent_unset = unset.get(); A.owners = p_ow.get();
        A.out_status = status.get(); A.out_nearest = nearest.get(); A.out_max_weight = maxw.get(); A.out_touched = touched.get();
        A.pos_of = ws.get();
        cv_scratch_split(A);
        for (int p = 0; p < G; ++p) cv_count(A, p, *sh, par);
        for (int j = 0; j < F; ++j) cv_apply(A, j, *sh, par);
        int seen = 0, n_over = 0, parents = 0;
        for (int p = 0; p < G; ++p) {
            seen |= 1 << status[p];
            const bool done = status[p] == PLP_COVIS_OK || status[p] == PLP_COVIS_OVERFLOW;
            good = good && status[p] <= PLP_COVIS_OVERFLOW && (done ? (0 <= nearest[p] && nearest[p] < F && maxw[p] > 0) : (nearest[p] == -1 && maxw[p] == 0));
            if (done) good = good && (kf_id[owners[p]] == 0u ? unset[owners[p]] == 1 : (unset[owners[p]] == 0 && parent[owners[p]] == nearest[p]));
        }
        for (int j = 0; j < F; ++j) { good = good && touched[j] <= 2; parents += parent[j] >= 0; }
        good = good && well_formed(A, touched.get(), &n_over);
        good = good && (pass == 0 ? (n_over == 0 && (seen & 0x0f) == 0x0f) : (0 < n_over && n_over < F && (seen & (1 << PLP_COVIS_OVERFLOW))));
        std::printf("update, caps %d / %d: statuses seen 0x%x, %d rows not valid, %d parents\n", conn_cap, covis_cap, seen, n_over, parents);
        if (pass == 1) continue;
        // erase_all_connections of a dozen key frames over the complete state
        std::vector<uint8_t> gone(F, 0);
        for (int i = 0; i < 12; ++i) gone[rnd(F)] = 1;
        auto p_go = exact(gone); auto est = exact(std::vector<uint8_t>(F, 99)); auto eto = exact(std::vector<uint8_t>(F, 99));
        A.erased = p_go.get(); A.out_status = est.get(); A.out_touched = eto.get();
        for (A.phase = 0; A.phase < 2; ++A.phase)
            for (int j = 0; j < F; ++j) cv_erase(A, j, *sh, par);
        int lost = 0, over = 0;
        for (int j = 0; j < F; ++j) {
            good = good && est[j] <= PLP_COVIS_OVERFLOW && eto[j] <= 2 && (!gone[j] || (n_conn[j] == 0 && n_covis[j] == 0 && eto[j] == 1));
            lost += !gone[j] && eto[j] != 0;
        }
        good = good && well_formed(A, eto.get(), &over) && lost > 0;
        std::printf("erase: %d surviving rows rewritten, %d lists outgrew their table\n", lost, over);
    }
    std::printf("%s\n", good ? "ok" : "FAILED");
    return good ? 0 : 1;
}
