#include "drop_in/graph_optimizer_hip.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <unordered_set>
#include <set>
#include <stdexcept>
#include <unordered_map>
#include <utility>

#include "sv_sim3.h"

namespace stella_vslam_amd {

std::vector<pose_graph_edge> build_pose_graph_edges(const pose_graph_keyframes& K, const pose_graph_loop_connections& conns, uint32_t curr_id,
                                                    uint32_t loop_id, unsigned int min_num_shared_lms) {
    std::unordered_map<uint32_t, int> index;
    for (int k = 0; k < K.n; ++k) index[K.id[k]] = k;
    const auto cw = [&](uint32_t id) { return sv_sim3_load(K.sim3_cw + 8 * (size_t)index.at(id)); };
    // "use only non-modified poses in the covisibility information"
    const auto non_corrected = [&](uint32_t id) {
        const int k = index.at(id);
        return K.has_non_corrected[k] ? sv_sim3_load(K.sim3_non_corrected + 8 * (size_t)k) : sv_sim3_load(K.sim3_cw + 8 * (size_t)k);
    };
    // graph_node::get_num_shared_landmarks: the weight of the connection, 0 without one
    const auto num_shared = [&](int k, uint32_t other) -> unsigned int {
        for (int c = K.covis_off[k]; c < K.covis_off[k + 1]; ++c)
            if (K.covis_id[c] == other) return K.covis_weight[c];
        return 0;
    };
    std::vector<pose_graph_edge> edges;
    std::set<std::pair<uint32_t, uint32_t>> inserted_edge_pairs;
    const auto insert_edge = [&](uint32_t id1, uint32_t id2, const SvSim3& Sim3_21) {
        pose_graph_edge e;
        e.id1 = id1, e.id2 = id2;
        sv_sim3_store(e.sim3_21, Sim3_21);
        edges.push_back(e);
        inserted_edge_pairs.insert(std::make_pair(std::min(id1, id2), std::max(id1, id2)));
    };
    // loop edges only over the number of shared landmarks threshold (:127-153)
    for (int c = 0; c < conns.n; ++c) {
        const uint32_t id1 = conns.key[c];
        const int k1 = index.at(id1);
        const SvSim3 Sim3_w1 = sv_sim3_inv(cw(id1));
        for (int j = conns.off[c]; j < conns.off[c + 1]; ++j) {
            const uint32_t id2 = conns.id[j];
            if (!(id1 == curr_id && id2 == loop_id) && num_shared(k1, id2) < min_num_shared_lms) continue;
            insert_edge(id1, id2, sv_sim3_mul(cw(id2), Sim3_w1));
        }
    }
    // non-loop-connected edges (:155-250)
    for (int k = 0; k < K.n; ++k) {
        const uint32_t id1 = K.id[k];
        const SvSim3 Sim3_w1 = sv_sim3_inv(non_corrected(id1));
        const bool has_parent = K.parent_id[k] >= 0;
        if (has_parent) {
            const uint32_t id2 = (uint32_t)K.parent_id[k];
            if (!(id1 <= id2)) insert_edge(id1, id2, sv_sim3_mul(non_corrected(id2), Sim3_w1));
            // (the reference `continue`s here: a keyframe whose id is not above its parent's adds NO loop or covisibility edge either)
            else continue;
        }
        for (int j = K.loop_off[k]; j < K.loop_off[k + 1]; ++j) {
            const uint32_t id2 = K.loop_id[j];
            if (id1 <= id2) continue;
            insert_edge(id1, id2, sv_sim3_mul(non_corrected(id2), Sim3_w1));
        }
        for (int j = K.covis_off[k]; j < K.covis_off[k + 1]; ++j) {
            if (K.covis_weight[j] < min_num_shared_lms) break;  // ordered by descending weight: the prefix from the threshold on
            if (!has_parent) continue;
            const uint32_t id2 = K.covis_id[j];
            const int k2 = index.at(id2);
            // parent-child edges have been inserted already
            if (id2 == (uint32_t)K.parent_id[k] || (K.parent_id[k2] >= 0 && (uint32_t)K.parent_id[k2] == id1)) continue;
            // and so have the edges associated to the loop
            if (std::find(K.loop_id + K.loop_off[k], K.loop_id + K.loop_off[k + 1], id2) != K.loop_id + K.loop_off[k + 1]) continue;
            if (K.will_be_erased[k2]) continue;
            if (id1 <= id2) continue;
            if (inserted_edge_pairs.count(std::make_pair(std::min(id1, id2), std::max(id1, id2)))) continue;
            insert_edge(id1, id2, sv_sim3_mul(non_corrected(id2), Sim3_w1));
        }
    }
    return edges;
}

}  // namespace stella_vslam_amd

#ifndef SVGPU_POSE_GRAPH_EDGES_ONLY
namespace stella_vslam {
namespace optimize {
namespace hip {

namespace {
void put_sim3(double* p, const g2o::Sim3& S) {
#ifdef SVGPU_WITH_STELLA_VSLAM
    const auto& q = S.rotation();
    const auto& t = S.translation();
    p[0] = q.x(), p[1] = q.y(), p[2] = q.z(), p[3] = q.w(), p[4] = t(0), p[5] = t(1), p[6] = t(2), p[7] = S.scale();
#else
    for (int k = 0; k < 4; ++k) p[k] = S.q[k];
    for (int k = 0; k < 3; ++k) p[4 + k] = S.t[k];
    p[7] = S.s;
#endif
}
}  // namespace

graph_optimizer::graph_optimizer(const YAML::Node& yaml_node, const bool fix_scale)
    : fix_scale_(fix_scale), min_num_shared_lms_(yaml_node["min_num_shared_lms"].as<unsigned int>(100)) {}

void graph_optimizer::optimize(const std::shared_ptr<data::keyframe>& loop_keyfrm, const std::shared_ptr<data::keyframe>& curr_keyfrm,
                               const module::keyframe_Sim3_pairs_t& non_corrected_Sim3s, const module::keyframe_Sim3_pairs_t& pre_corrected_Sim3s,
                               const std::map<std::shared_ptr<data::keyframe>, std::set<std::shared_ptr<data::keyframe>>>& loop_connections,
                               std::unordered_map<unsigned int, unsigned int>& found_lm_to_ref_keyfrm_id) const {
    // 2. vertices (:45-106): every keyframe reachable from the root that is not about to be erased, and their landmarks
    const auto reachable = curr_keyfrm->graph_node_->get_keyframes_from_root();
    std::unordered_set<unsigned int> already_found_landmark_ids;
    std::vector<std::shared_ptr<data::landmark>> all_lms;
    for (const auto& keyfrm : reachable) {
        for (const auto& lm : keyfrm->get_landmarks()) {
            if (!lm || lm->will_be_erased() || already_found_landmark_ids.count(lm->id_)) continue;
            already_found_landmark_ids.insert(lm->id_);
            all_lms.push_back(lm);
        }
    }
    std::vector<std::shared_ptr<data::keyframe>> all_keyfrms;  // the vertices, in their order
    for (const auto& keyfrm : reachable)
        if (!keyfrm->will_be_erased()) all_keyfrms.push_back(keyfrm);
    const int n = (int)all_keyfrms.size();
    std::unordered_map<unsigned int, int> vertex_of;
    std::vector<uint32_t> id(n);
    std::vector<uint8_t> erased(n, 0), fixed(n, 0), has_non(n, 0);
    std::vector<int64_t> parent(n, -1);
    std::vector<double> sim3_cw(8 * (size_t)n), sim3_non(8 * (size_t)n, 0.0);
    std::vector<int32_t> loop_off(1, 0), covis_off(1, 0);
    std::vector<uint32_t> loop_id, covis_id, covis_w;
    for (int k = 0; k < n; ++k) {
        const auto& keyfrm = all_keyfrms[k];
        id[k] = keyfrm->id_;
        vertex_of[keyfrm->id_] = k;
        // BEFORE optimization, the already-modified pose where there is one, else the pose with scale 1
        const auto iter = pre_corrected_Sim3s.find(keyfrm);
        if (iter != pre_corrected_Sim3s.end()) put_sim3(&sim3_cw[8 * (size_t)k], iter->second);
        else {
            const Mat33_t rot_cw = keyfrm->get_rot_cw();
            const Vec3_t trans_cw = keyfrm->get_trans_cw();
            SvMat3 R{rot_cw(0, 0), rot_cw(0, 1), rot_cw(0, 2), rot_cw(1, 0), rot_cw(1, 1), rot_cw(1, 2), rot_cw(2, 0), rot_cw(2, 1), rot_cw(2, 2)};
            SvSim3 S;
            sv_rot_to_quat(R, S.qx, S.qy, S.qz, S.qw);
            const double nrm = std::sqrt(S.qx * S.qx + S.qy * S.qy + S.qz * S.qz + S.qw * S.qw);  // Sim3(R, t, s) normalises its quaternion
            S.qx /= nrm, S.qy /= nrm, S.qz /= nrm, S.qw /= nrm;
            S.t = sv3(trans_cw(0), trans_cw(1), trans_cw(2));
            S.s = 1.0;
            sv_sim3_store(&sim3_cw[8 * (size_t)k], S);
        }
        const auto non = non_corrected_Sim3s.find(keyfrm);
        if (non != non_corrected_Sim3s.end()) {
            has_non[k] = 1;
            put_sim3(&sim3_non[8 * (size_t)k], non->second);
        }
        // fix the loop keyframe, the current keyframe and the root (:96-98)
        fixed[k] = keyfrm->id_ == loop_keyfrm->id_ || keyfrm->id_ == curr_keyfrm->id_ || keyfrm->graph_node_->is_spanning_root();
        if (const auto p = keyfrm->graph_node_->get_spanning_parent()) parent[k] = p->id_;
        for (const auto& other : keyfrm->graph_node_->get_loop_edges()) loop_id.push_back(other->id_);
        loop_off.push_back((int32_t)loop_id.size());
        // every covisibility with its weight (get_num_shared_landmarks of the loop connections reads them too), strongest first
        for (const auto& other : keyfrm->graph_node_->get_covisibilities_over_min_num_shared_lms(0)) {
            if (!other) continue;
            covis_id.push_back(other->id_);
            covis_w.push_back(keyfrm->graph_node_->get_num_shared_landmarks(other));
        }
        covis_off.push_back((int32_t)covis_id.size());
    }
    // a neighbour that has no vertex (about to be erased, or outside the spanning tree) is marked erased for the edge builder
    std::vector<uint32_t> extra_id;
    const auto known = [&](uint32_t i) { return vertex_of.count(i) != 0; };
    for (uint32_t i : covis_id)
        if (!known(i) && std::find(extra_id.begin(), extra_id.end(), i) == extra_id.end()) extra_id.push_back(i);
    for (uint32_t i : extra_id) {
        id.push_back(i), erased.push_back(1), has_non.push_back(0), parent.push_back(-1);
        loop_off.push_back(loop_off.back()), covis_off.push_back(covis_off.back());
        sim3_cw.insert(sim3_cw.end(), {0, 0, 0, 1, 0, 0, 0, 1});
        sim3_non.insert(sim3_non.end(), 8, 0.0);
    }
    std::vector<uint32_t> conn_key, conn_id;
    std::vector<int32_t> conn_off(1, 0);
    for (const auto& loop_connection : loop_connections) {
        conn_key.push_back(loop_connection.first->id_);
        for (const auto& other : loop_connection.second) conn_id.push_back(other->id_);
        conn_off.push_back((int32_t)conn_id.size());
    }
    loop_id.push_back(0), covis_id.push_back(0), covis_w.push_back(0), conn_id.push_back(0), conn_key.push_back(0);  // .data() of an empty vector
    stella_vslam_amd::pose_graph_keyframes K;
    K.n = (int)id.size(), K.id = id.data(), K.will_be_erased = erased.data(), K.parent_id = parent.data(), K.loop_off = loop_off.data(), K.loop_id = loop_id.data();
    K.covis_off = covis_off.data(), K.covis_id = covis_id.data(), K.covis_weight = covis_w.data(), K.sim3_cw = sim3_cw.data();
    K.has_non_corrected = has_non.data(), K.sim3_non_corrected = sim3_non.data();
    stella_vslam_amd::pose_graph_loop_connections C;
    C.n = (int)conn_off.size() - 1, C.key = conn_key.data(), C.off = conn_off.data(), C.id = conn_id.data();
    // 3. edges (:108-250)
    const auto edges = stella_vslam_amd::build_pose_graph_edges(K, C, curr_keyfrm->id_, loop_keyfrm->id_, min_num_shared_lms_);
    std::vector<int32_t> e1(edges.size()), e2(edges.size());
    std::vector<double> meas(8 * edges.size());
    for (size_t e = 0; e < edges.size(); ++e) {
        e1[e] = vertex_of.at(edges[e].id1);  // (the reference's vertices.at)
        e2[e] = vertex_of.at(edges[e].id2);
        std::copy(edges[e].sim3_21, edges[e].sim3_21 + 8, &meas[8 * e]);
    }
    // 4. the optimisation (:252-257)
    std::vector<double> sim3_out(8 * (size_t)n), pose_out(12 * (size_t)n);
    svgpu_ctx* ctx = stella_vslam::hip::context();
    svgpu_pose_graph_options options{};
    options.solver = solver_;
    stella_vslam::hip::check(svgpu_pose_graph_optimize_ex(ctx, n, sim3_cw.data(), fixed.data(), (int)edges.size(), e1.data(), e2.data(), meas.data(), fix_scale_ ? 1 : 0,
                                                          50, 1e-3, sim3_out.data(), pose_out.data(), &last_stats_, &options, &last_solver_stats_),
                             "svgpu_pose_graph_optimize_ex");
    // 5. poses and point cloud (:259-302)
    std::vector<std::shared_ptr<data::landmark>> lms;
    std::vector<int32_t> ref;
    std::vector<double> pos;
    for (const auto& lm : all_lms) {
        if (lm->will_be_erased()) continue;
        const auto ref_id = found_lm_to_ref_keyfrm_id.count(lm->id_) ? found_lm_to_ref_keyfrm_id.at(lm->id_) : lm->get_ref_keyframe()->id_;
        lms.push_back(lm);
        ref.push_back(vertex_of.at(ref_id));
        const Vec3_t pos_w = lm->get_pos_in_world();
        pos.insert(pos.end(), {pos_w(0), pos_w(1), pos_w(2)});
    }
    std::vector<double> corrected(pos.size());
    stella_vslam::hip::check(svgpu_pose_graph_correct_landmarks(ctx, n, sim3_cw.data(), sim3_out.data(), (int)lms.size(), ref.data(), pos.data(), corrected.data()),
                             "svgpu_pose_graph_correct_landmarks");
    std::lock_guard<std::mutex> lock(data::map_database::mtx_database_);
    for (int k = 0; k < n; ++k) {
        Mat44_t cam_pose_cw = Mat44_t::Identity();
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) cam_pose_cw(i, j) = pose_out[12 * (size_t)k + 4 * i + j];
        all_keyfrms[k]->set_pose_cw(cam_pose_cw);
    }
    for (size_t l = 0; l < lms.size(); ++l) {
        Vec3_t p;
        p(0) = corrected[3 * l], p(1) = corrected[3 * l + 1], p(2) = corrected[3 * l + 2];
        lms[l]->set_pos_in_world(p);
        lms[l]->update_mean_normal_and_obs_scale_variance();
    }
}

}  // namespace hip
}  // namespace optimize
}  // namespace stella_vslam
#endif
