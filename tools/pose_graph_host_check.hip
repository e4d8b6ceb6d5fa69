// Stand-alone host program over csrc/pose_graph.hpp for a sanitizer build (no GPU, no Python): a generated chain of 60 key frames with drift, band
// edges, an erased row, a parent outside the table, loop edges both ways, covisibility rows of every length up to the row width, per-problem lists
// with rows outside the table, three problems (free scale, fixed scale, a loop key frame that is erased) through pg_prepare, pg_solve and pg_finish
// with a team of one lane, then the landmark half, on heap buffers of exact size; once more with caps that are one too short.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/pose_graph_host_check.hip -o pose_graph_host_check
//   ./pose_graph_host_check          # prints every problem's status, edges, iterations and chi2 and "ok"
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "../structure-plp-slam_amd/csrc/pose_graph.hpp"

using namespace plp;

template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) {     // a heap block of exactly the vector's size
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

static void pose_of(double angle, double radius, double* p15) {
    const double c = std::cos(angle), s = std::sin(angle);
    const double R[9] = {c, s, 0.0, -s, c, 0.0, 0.0, 0.0, 1.0};                     // rot_cw of a camera turned by `angle` about z
    const double C[3] = {radius * c, radius * s, 0.1 * angle};
    for (int i = 0; i < 9; ++i) p15[i] = R[i];
    for (int i = 0; i < 3; ++i) p15[9 + i] = -((R[3 * i] * C[0] + R[3 * i + 1] * C[1]) + R[3 * i + 2] * C[2]);
    for (int i = 0; i < 3; ++i) p15[12 + i] = C[i];
}

static int run(int edge_cap, int env_cap, bool expect_ok) {
    const int F = 60, G = 3, cap = 6;
    std::vector<double> pose((size_t)F * 15);
    for (int f = 0; f < F; ++f) pose_of(0.1 * f * (1.0 + 0.002 * f), 5.0 * (1.0 + 0.001 * f), pose.data() + 15 * f);
    std::vector<uint8_t> erased(F, 0);
    erased[17] = 1;
    std::vector<int32_t> id(F), parent(F), conn((size_t)F * cap, -1), conn_w((size_t)F * cap, 0), n_conn(F, 0), covis((size_t)F * cap, -1), covis_w((size_t)F * cap, 0),
        n_covis(F, 0), loop_off(F + 1, 0), loop;
    for (int f = 0; f < F; ++f) {
        id[f] = 3 * f;
        parent[f] = f == 0 ? -1 : f == 30 ? F + 4 : f - 1;
        const int nb[6] = {f - 1, f + 1, f - 2, f + 2, f - 3, f + 3}, w[6] = {150, 150, 120, 120, 60, 60};
        int n = 0;
        for (int k = 0; k < (f % 7 == 3 ? 4 : 6); ++k)                               // every seventh row holds strong entries only
            if (nb[k] >= 0 && nb[k] < F) { covis[(size_t)f * cap + n] = nb[k]; covis_w[(size_t)f * cap + n] = w[k]; ++n; }
        n_covis[f] = f == 44 ? cap + 5 : n;                                          // a count above the row width is cut
        int m = 0;
        for (int c = f - 3; c <= f + 3; ++c)
            if (c != f && c >= 0 && c < F) { conn[(size_t)f * cap + m] = c; conn_w[(size_t)f * cap + m] = c == f - 1 || c == f + 1 ? 150 : c == f - 2 || c == f + 2 ? 120 : 60; ++m; }
        n_conn[f] = m;
    }
    for (int f = 0; f < F; ++f) {
        if (f == 50) { loop.push_back(4); loop.push_back(F + 9); }
        if (f == 4) loop.push_back(50);
        loop_off[f + 1] = (int)loop.size();
    }
    std::vector<int32_t> loop_kf = {0, 2, 17}, curr_kf = {F - 1, F - 1, F - 1};
    std::vector<uint8_t> fix_scale = {0, 1, 0};
    std::vector<int32_t> pre_off = {0, 2, 3, 3}, pre_row = {F - 1, F + 2, F - 1}, non_off = {0, 1, 2, 2}, non_row = {F - 1, F - 1};
    std::vector<double> pre_sim3(3 * 8), non_sim3(2 * 8);
    for (int i = 0; i < 3; ++i) {
        double p15[15];
        pose_of(0.1 * (F - 1), 5.0, p15);
        pg_sim3_from_pose(p15, pre_sim3.data() + 8 * i);
        if (i == 0) pre_sim3[7] = 1.04;
    }
    for (int i = 0; i < 2; ++i) pg_sim3_from_pose(pose.data() + 15 * (F - 1), non_sim3.data() + 8 * i);
    std::vector<int32_t> lc_off = {0, 4, 5, 5}, lc_owner = {F - 1, F - 1, -3, F - 2, F - 1}, lc_target = {0, F - 4, 2, 17, 2};

    auto p_pose = exact(pose); auto p_er = exact(erased); auto p_id = exact(id); auto p_par = exact(parent); auto p_conn = exact(conn); auto p_connw = exact(conn_w);
    auto p_nconn = exact(n_conn); auto p_cov = exact(covis); auto p_covw = exact(covis_w); auto p_ncov = exact(n_covis); auto p_loff = exact(loop_off); auto p_loop = exact(loop);
    auto p_lkf = exact(loop_kf); auto p_ckf = exact(curr_kf); auto p_fs = exact(fix_scale); auto p_po = exact(pre_off); auto p_pr = exact(pre_row); auto p_ps = exact(pre_sim3);
    auto p_no = exact(non_off); auto p_nr = exact(non_row); auto p_ns = exact(non_sim3); auto p_lo = exact(lc_off); auto p_lw = exact(lc_owner); auto p_lt = exact(lc_target);
    std::vector<uint8_t> status(G, 0xEE);
    std::vector<int32_t> num_edges(G, -1), edges((size_t)G * edge_cap * 3, -1), info((size_t)G * 4, -1);
    std::vector<double> cw((size_t)G * F * 8, 0.0), wc((size_t)G * F * 8, 0.0), out_pose((size_t)G * F * 15, 0.0), chi2((size_t)G * 2, 0.0);
    auto o_st = exact(status); auto o_ne = exact(num_edges); auto o_ed = exact(edges); auto o_in = exact(info); auto o_cw = exact(cw); auto o_wc = exact(wc);
    auto o_po = exact(out_pose); auto o_ch = exact(chi2);

    PgArgs A{};
    A.G = G; A.F = F; A.pose_stride = 15; A.conn_cap = cap; A.covis_cap = cap; A.edge_cap = edge_cap; A.env_cap = env_cap; A.max_iter = 8;
    A.pose = p_pose.get(); A.kf_erased = p_er.get(); A.kf_id = p_id.get(); A.kf_parent = p_par.get(); A.kf_conn = p_conn.get(); A.kf_conn_w = p_connw.get();
    A.kf_n_conn = p_nconn.get(); A.kf_covis = p_cov.get(); A.kf_covis_w = p_covw.get(); A.kf_n_covis = p_ncov.get(); A.kf_loop_offsets = p_loff.get(); A.kf_loop = p_loop.get();
    A.loop_kf = p_lkf.get(); A.curr_kf = p_ckf.get(); A.fix_scale = p_fs.get(); A.pre_offsets = p_po.get(); A.pre_row = p_pr.get(); A.pre_sim3 = p_ps.get();
    A.non_offsets = p_no.get(); A.non_row = p_nr.get(); A.non_sim3 = p_ns.get(); A.lc_offsets = p_lo.get(); A.lc_owner = p_lw.get(); A.lc_target = p_lt.get();
    A.out_status = o_st.get(); A.out_num_edges = o_ne.get(); A.out_edges = o_ed.get(); A.out_sim3_cw = o_cw.get(); A.out_corrected_wc = o_wc.get(); A.out_pose = o_po.get();
    A.out_info = o_in.get(); A.out_chi2 = o_ch.get();
    std::unique_ptr<double[]> d(new double[pg_doubles(F, edge_cap, env_cap)]());
    std::unique_ptr<int32_t[]> iv(new int32_t[pg_ints(F, edge_cap, env_cap)]());
    A.ctx_d = d.get(); A.ctx_i = iv.get();
    std::unique_ptr<PgShared> sh(new PgShared());
    PgTeamHost par;
    bool good = true;
    for (int g = 0; g < G; ++g) {
        A.ctx_base = g;
        pg_prepare(A, g, *sh, par);
        pg_solve(A, g, *sh, par);
        pg_finish(A, g, par);
        std::printf("caps %d %d problem %d: status %d, %d edges, %d vertices, %d iterations, %d rejected, end %d, chi2 %.6e\n", edge_cap, env_cap, g, (int)A.out_status[g],
                    A.out_num_edges[g], A.out_info[4 * g + 3], A.out_info[4 * g], A.out_info[4 * g + 1], A.out_info[4 * g + 2], A.out_chi2[2 * g]);
        const int want = g == 2 ? PLP_POSE_GRAPH_BAD_LOOP_KF : expect_ok ? PLP_POSE_GRAPH_OK : -1;
        good = good && (want < 0 ? (A.out_status[g] == PLP_POSE_GRAPH_TOO_MANY_EDGES || A.out_status[g] == PLP_POSE_GRAPH_ENVELOPE_TOO_LARGE) : A.out_status[g] == want);
        if (A.out_status[g] == PLP_POSE_GRAPH_OK)
            for (int f = 0; f < F; ++f)
                for (int i = 0; i < 15 && !erased[f]; ++i) good = good && std::isfinite(A.out_pose[((size_t)g * F + f) * 15 + i]);
    }
    if (!expect_ok) return good ? A.out_num_edges[0] : -1;
    // the landmark half over problem 0
    const int L = 300;
    std::vector<double> pos((size_t)L * 3);
    std::vector<int32_t> ref(L);
    std::vector<uint8_t> lm_er(L, 0), lm_st(L, 0xEE);
    for (int l = 0; l < L; ++l) {
        for (int i = 0; i < 3; ++i) pos[(size_t)3 * l + i] = 0.01 * ((l * 37 + i * 11) % 500) - 2.5;
        ref[l] = l % 23 == 0 ? F + 1 : l % 31 == 0 ? -2 : l % F;
        lm_er[l] = l % 13 == 0;
    }
    auto p_pos = exact(pos); auto p_ref = exact(ref); auto p_ler = exact(lm_er); auto p_lst = exact(lm_st);
    PgLmArgs M{};
    M.L = L; M.F = F; M.pos_w = p_pos.get(); M.lm_erased = p_ler.get(); M.ref_kf = p_ref.get(); M.kf_erased = p_er.get(); M.sim3_cw = o_cw.get(); M.corrected_wc = o_wc.get();
    M.out_pos_w = p_pos.get(); M.out_status = p_lst.get();
    int n_ok = 0;
    for (int l = 0; l < L; ++l) { pg_correct_landmark(M, l); n_ok += M.out_status[l] == PLP_CORRECT_LM_OK; }
    std::printf("landmarks: %d of %d corrected\n", n_ok, L);
    return good && n_ok > 200 && n_ok < L ? A.out_num_edges[0] : -1;
}

int main() {
    const int edges = run(256, 1024, true);
    if (edges < 0) { std::printf("FAILED\n"); return 1; }
    if (run(edges - 1, 1024, false) < 0 || run(256, 100, false) < 0) { std::printf("FAILED\n"); return 1; }
    std::printf("ok\n");
    return 0;
}
