// Host-only driver of build_pose_graph_edges (stella_vslam_amd/host/drop_in/graph_optimizer_hip.cc): built and run by
// tests/test_posegraph_problem_classes.py.  Reads one graph as whitespace-separated numbers from the file given as argv[1]:
//   n curr_id loop_id min_num_shared_lms
//   per keyframe: id erased parent_id(-1 none) has_non_corrected, 8 doubles sim3_cw, 8 doubles sim3_non_corrected,
//                 L then L loop-edge ids, C then C (id weight) covisibilities in descending weight
//   M, then per loop connection: key id, K, K ids
// and prints one line per edge: id1 id2 and the 8 doubles of Sim3_21 (%.17g).
#include <cstdio>
#include <fstream>
#include <vector>

#include "drop_in/graph_optimizer_hip.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int n;
    uint32_t curr, loop, min_shared;
    in >> n >> curr >> loop >> min_shared;
    std::vector<uint32_t> id(n), loop_id, covis_id, covis_w;
    std::vector<uint8_t> erased(n), has_non(n);
    std::vector<int64_t> parent(n);
    std::vector<int32_t> loop_off(1, 0), covis_off(1, 0);
    std::vector<double> cw(8 * n), non(8 * n);
    for (int k = 0; k < n; ++k) {
        int e, h, cnt;
        in >> id[k] >> e >> parent[k] >> h;
        erased[k] = (uint8_t)e, has_non[k] = (uint8_t)h;
        for (int j = 0; j < 8; ++j) in >> cw[8 * k + j];
        for (int j = 0; j < 8; ++j) in >> non[8 * k + j];
        in >> cnt;
        for (int j = 0; j < cnt; ++j) {
            uint32_t v;
            in >> v;
            loop_id.push_back(v);
        }
        loop_off.push_back((int32_t)loop_id.size());
        in >> cnt;
        for (int j = 0; j < cnt; ++j) {
            uint32_t v, w;
            in >> v >> w;
            covis_id.push_back(v);
            covis_w.push_back(w);
        }
        covis_off.push_back((int32_t)covis_id.size());
    }
    int m;
    in >> m;
    std::vector<uint32_t> key(m), conn_id;
    std::vector<int32_t> conn_off(1, 0);
    for (int c = 0; c < m; ++c) {
        int cnt;
        in >> key[c] >> cnt;
        for (int j = 0; j < cnt; ++j) {
            uint32_t v;
            in >> v;
            conn_id.push_back(v);
        }
        conn_off.push_back((int32_t)conn_id.size());
    }
    if (!in) return 3;
    loop_id.push_back(0), covis_id.push_back(0), covis_w.push_back(0), conn_id.push_back(0);  // never empty: .data() stays a valid pointer
    stella_vslam_amd::pose_graph_keyframes K;
    K.n = n, K.id = id.data(), K.will_be_erased = erased.data(), K.parent_id = parent.data(), K.loop_off = loop_off.data(), K.loop_id = loop_id.data();
    K.covis_off = covis_off.data(), K.covis_id = covis_id.data(), K.covis_weight = covis_w.data(), K.sim3_cw = cw.data();
    K.has_non_corrected = has_non.data(), K.sim3_non_corrected = non.data();
    stella_vslam_amd::pose_graph_loop_connections Cn;
    Cn.n = m, Cn.key = key.data(), Cn.off = conn_off.data(), Cn.id = conn_id.data();
    for (const auto& e : stella_vslam_amd::build_pose_graph_edges(K, Cn, curr, loop, min_shared)) {
        std::printf("%u %u", e.id1, e.id2);
        for (int j = 0; j < 8; ++j) std::printf(" %.17g", e.sim3_21[j]);
        std::printf("\n");
    }
    return 0;
}
