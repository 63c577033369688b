#include "landmark_fuser_hip.h"

#include <cstring>

#include "fuse_layout.h"

namespace stella_vslam {
namespace module {
namespace hip {

using lm_ptr = landmark_fuser::lm_ptr;
using kf_ptr = landmark_fuser::kf_ptr;

namespace {
// the landmarks of the targets, each once, in first appearance
std::vector<lm_ptr> backward_candidates(const std::vector<kf_ptr>& tgts, bool alive_only) {
    std::vector<lm_ptr> out;
    std::unordered_set<lm_ptr> seen;
    for (const auto& kf : tgts)
        for (const auto& lm : kf->get_landmarks()) {
            if (!lm || (alive_only && lm->will_be_erased())) continue;
            if (seen.insert(lm).second) out.push_back(lm);
        }
    return out;
}
// mapping_module.cc:436-467 / :504-535 behind one detect_duplication
void apply(const kf_ptr& keyfrm, std::unordered_map<lm_ptr, lm_ptr>& duplicated, std::unordered_map<unsigned int, lm_ptr>& new_connections,
           data::map_database* map_db, std::unordered_map<lm_ptr, lm_ptr>& replaced_lms) {
    for (const auto& lms_pair : duplicated) {
        auto lm_to_replace = lms_pair.first;
        auto lm_in_keyfrm = lms_pair.second;
        if (lm_to_replace->num_observations() < lm_in_keyfrm->num_observations()) std::swap(lm_to_replace, lm_in_keyfrm);
        if (lm_to_replace->id_ != lm_in_keyfrm->id_) {
            replaced_lms[lm_in_keyfrm] = lm_to_replace;
            lm_in_keyfrm->replace(lm_to_replace, map_db);
            if (!lm_to_replace->has_representative_descriptor()) lm_to_replace->compute_descriptor();
            if (!lm_to_replace->has_valid_prediction_parameters()) lm_to_replace->update_mean_normal_and_obs_scale_variance();
        }
    }
    for (const auto& best_idx_lm : new_connections) {
        auto lm = best_idx_lm.second;
        while (replaced_lms.count(lm)) lm = replaced_lms[lm];
        lm->connect_to_keyframe(keyfrm, best_idx_lm.first);
        lm->update_mean_normal_and_obs_scale_variance();
        lm->compute_descriptor();
    }
}
}  // namespace

void landmark_fuser::fuse_by_single_calls(const kf_ptr& cur, const std::vector<kf_ptr>& tgts, data::map_database* map_db,
                                          std::unordered_map<lm_ptr, lm_ptr>& replaced_lms) const {
    const match::hip::fuse fuse_matcher(0.6);
    const auto cur_landmarks = cur->get_landmarks();
    for (const auto& tgt : tgts) {
        std::unordered_map<lm_ptr, lm_ptr> duplicated;
        std::unordered_map<unsigned int, lm_ptr> new_connections;
        fuse_matcher.detect_duplication(tgt, tgt->get_rot_cw(), tgt->get_trans_cw(), cur_landmarks, margin_, duplicated, new_connections, do_reprojection_matching_);
        apply(tgt, duplicated, new_connections, map_db, replaced_lms);
    }
    const std::vector<lm_ptr> candidates = backward_candidates(tgts, true);
    std::unordered_map<lm_ptr, lm_ptr> duplicated;
    std::unordered_map<unsigned int, lm_ptr> new_connections;
    fuse_matcher.detect_duplication(cur, cur->get_rot_cw(), cur->get_trans_cw(), candidates, margin_, duplicated, new_connections, do_reprojection_matching_);
    apply(cur, duplicated, new_connections, map_db, replaced_lms);
}

void landmark_fuser::fuse(const kf_ptr& cur, const std::vector<kf_ptr>& tgts, data::map_database* map_db, std::unordered_map<lm_ptr, lm_ptr>& replaced_lms) const {
    last_took_batch_ = last_overflowed_ = false;
    last_stats_ = svgpu_call_stats{0, 0, 0};
    if (tgts.empty()) return;
    if (tgts.size() >= min_targets_for_batch_ && fuse_batch(cur, tgts, map_db, replaced_lms)) {
        last_took_batch_ = true;
        return;
    }
    fuse_by_single_calls(cur, tgts, map_db, replaced_lms);
}

// false: nothing was touched and the caller takes the single calls
bool landmark_fuser::fuse_batch(const kf_ptr& cur, const std::vector<kf_ptr>& tgts, data::map_database* map_db,
                                std::unordered_map<lm_ptr, lm_ptr>& replaced_lms) const {
    const int K = (int)tgts.size(), passes = K + 1;
    std::vector<kf_ptr> slots{cur};
    slots.insert(slots.end(), tgts.begin(), tgts.end());
    const auto* op = cur->orb_params_;
    // ---- the union of the landmarks, in first appearance; every keyframe that observes one of them is an observer
    std::vector<lm_ptr> lms;
    std::unordered_map<lm_ptr, int> slot_of;
    for (const auto& kf : slots) {
        if (kf->orb_params_ != op && kf->orb_params_->scale_factors_ != op->scale_factors_) return false;  // one set of ORB tables per call
        for (const auto& lm : kf->get_landmarks())
            if (lm && slot_of.emplace(lm, (int)lms.size()).second) lms.push_back(lm);
    }
    const int L = (int)lms.size();
    if (L == 0) return false;
    std::vector<kf_ptr> observers;
    std::unordered_map<kf_ptr, int> observer_of;
    auto observer = [&](const kf_ptr& kf) {
        const auto it = observer_of.emplace(kf, (int)observers.size());
        if (it.second) observers.push_back(kf);
        return it.first->second;
    };
    for (const auto& kf : slots) observer(kf);
    std::vector<double> pos_w((size_t)L * 3), ref_twc((size_t)L * 3), normal((size_t)L * 3);
    std::vector<float> ref_sf(L), min_d(L), max_d(L);
    std::vector<int32_t> obs_off(L), obs_cap(L), obs_cnt(L), replaced_by(L, -1), e_obs, e_kp, e_w;
    std::vector<uint8_t> alive(L), desc((size_t)L * 32, 0), has_desc(L), has_geom(L), e_desc;
    for (int l = 0; l < L; ++l) {
        const auto& lm = lms[l];
        const Vec3_t p = lm->get_pos_in_world(), n = lm->get_obs_mean_normal();
        for (int k = 0; k < 3; ++k) pos_w[3 * l + k] = p(k), normal[3 * l + k] = n(k);
        min_d[l] = lm->get_min_valid_distance(), max_d[l] = lm->get_max_valid_distance();
        alive[l] = lm->will_be_erased() ? 0 : 1;
        has_desc[l] = lm->has_representative_descriptor(), has_geom[l] = lm->has_valid_prediction_parameters();
        const cv::Mat d = lm->get_descriptor();
        if (alive[l] && (!has_desc[l] || !has_geom[l] || d.rows < 1)) return false;  // the getters assert the flags (data/landmark.cc:95-99, 193-197)
        if (d.rows >= 1) std::memcpy(&desc[(size_t)l * 32], d.ptr(0), 32);
        const auto observations = lm->get_observations();
        obs_off[l] = (int32_t)e_obs.size();
        obs_cnt[l] = (int32_t)observations.size();
        obs_cap[l] = std::max(0, fuse_obs_capacity(obs_cnt[l], passes) + obs_slack_);
        if (obs_cap[l] < obs_cnt[l] || obs_cap[l] > FUSE_OBS_CAP_MAX) return false;
        for (const auto& o : observations) {  // the map's own order: id_less
            const auto kf = o.first.lock();
            if (!kf || kf->will_be_erased()) return false;  // compute_descriptor leaves such an observer out (:217-219): not expressed in the table
            e_obs.push_back(observer(kf)), e_kp.push_back((int32_t)o.second);
            e_w.push_back((!kf->frm_obs_.stereo_x_right_.empty() && 0 <= kf->frm_obs_.stereo_x_right_.at(o.second)) ? 2 : 1);
            const uint8_t* row = kf->frm_obs_.descriptors_.ptr((int)o.second);
            e_desc.insert(e_desc.end(), row, row + 32);
        }
        for (int e = obs_cnt[l]; e < obs_cap[l]; ++e) e_obs.push_back(-1), e_kp.push_back(-1), e_w.push_back(0), e_desc.insert(e_desc.end(), 32, 0);
        if (alive[l]) {
            const auto ref = lm->get_ref_keyframe();
            const int idx = ref ? lm->get_index_in_keyframe(ref) : -1;
            if (idx < 0) return false;
            const Vec3_t c = ref->get_trans_wc();
            for (int k = 0; k < 3; ++k) ref_twc[3 * l + k] = c(k);
            ref_sf[l] = ref->orb_params_->scale_factors_.at(ref->frm_obs_.undist_keypts_.at(idx).octave);
        }
    }
    const int O = (int)observers.size();
    std::vector<int32_t> rank(O);
    std::vector<double> twc((size_t)O * 3);
    for (int o = 0; o < O; ++o) {
        rank[o] = (int32_t)observers[o]->id_;
        const Vec3_t c = observers[o]->get_trans_wc();
        for (int k = 0; k < 3; ++k) twc[3 * o + k] = c(k);
    }
    // ---- the keyframe slots
    struct side {
        svgpu_camera cam;
        double R[9], t[3];
        std::vector<uint8_t> desc;
        std::vector<float> xy;
        std::vector<int32_t> octave, kp_lm;
    };
    std::vector<side> sides(passes);
    std::vector<svgpu_fuse_keyframe> recs(passes);
    for (int u = 0; u < passes; ++u) {
        const auto& kf = slots[u];
        side& s = sides[u];
        s.cam = stella_vslam::hip::to_svgpu_camera(kf->camera_);
        const Mat33_t R = kf->get_rot_cw();
        const Vec3_t t = kf->get_trans_cw();
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) s.R[3 * i + j] = R(i, j);
            s.t[i] = t(i);
        }
        const auto& fo = kf->frm_obs_;
        const int n = (int)fo.undist_keypts_.size();
        s.desc.resize((size_t)n * 32), s.xy.resize((size_t)n * 2), s.octave.resize(n), s.kp_lm.assign(n, -1);
        const auto kf_lms = kf->get_landmarks();
        for (int i = 0; i < n; ++i) {
            std::memcpy(&s.desc[(size_t)i * 32], fo.descriptors_.ptr(i), 32);
            s.xy[2 * i] = fo.undist_keypts_[i].pt.x, s.xy[2 * i + 1] = fo.undist_keypts_[i].pt.y;
            s.octave[i] = fo.undist_keypts_[i].octave;
            if (kf_lms[i]) s.kp_lm[i] = slot_of.at(kf_lms[i]);
        }
        recs[u] = svgpu_fuse_keyframe{&s.cam, s.R, s.t, s.desc.data(), s.xy.data(), s.octave.data(), fo.stereo_x_right_.empty() ? nullptr : fo.stereo_x_right_.data(),
                                      s.kp_lm.data(), n, observer_of.at(kf), (int32_t)fo.num_grid_cols_, (int32_t)fo.num_grid_rows_};
    }
    const std::vector<int32_t> fwd = sides[0].kp_lm;  // cur_keyfrm_->get_landmarks() as copied before the loop (:426)
    std::vector<int32_t> bwd;
    for (const auto& lm : backward_candidates(tgts, false)) bwd.push_back(slot_of.at(lm));
    svgpu_fuse_table T{};
    T.num_landmarks = L, T.num_entries = (int32_t)e_obs.size();
    T.pos_w = pos_w.data(), T.ref_trans_wc = ref_twc.data(), T.ref_scale_factor = ref_sf.data(), T.obs_off = obs_off.data(), T.obs_cap = obs_cap.data();
    T.alive = alive.data(), T.descriptor = desc.data(), T.mean_normal = normal.data(), T.min_valid_dist = min_d.data(), T.max_valid_dist = max_d.data();
    T.has_descriptor = has_desc.data(), T.has_geometry = has_geom.data(), T.obs_cnt = obs_cnt.data(), T.obs_observer = e_obs.data(), T.obs_kp = e_kp.data();
    T.obs_desc = e_desc.data(), T.obs_weight = e_w.data(), T.replaced_by = replaced_by.data();
    const int n_fwd = (int)fwd.size(), n_bwd = (int)bwd.size();
    const size_t n_out = (size_t)K * n_fwd + n_bwd;
    std::vector<int32_t> best(n_out + 1, -1), num_fused(passes, 0);
    std::vector<uint8_t> event(n_out + 1, 0);
    const int rc = svgpu_fuse_landmarks_batch(stella_vslam::hip::context(), K, recs.data(), O, rank.data(), twc.data(), &T, n_fwd, fwd.data(), n_bwd, bwd.data(),
                                              (int)op->num_levels_, op->scale_factors_.data(), op->inv_level_sigma_sq_.data(), op->log_scale_factor_,
                                              op->inv_scale_factors_.at(op->num_levels_ - 1), margin_, do_reprojection_matching_ ? 1 : 0, best.data(), event.data(),
                                              num_fused.data(), &last_stats_);
    if (rc == SVGPU_FUSE_OVERFLOW) {
        last_overflowed_ = true;
        return false;
    }
    stella_vslam::hip::check(rc, "svgpu_fuse_landmarks_batch");
    // ---- replay on the object graph: per pass the duplicates in ascending list index, then the new connections
    std::vector<uint8_t> touched(L, 0);
    auto holder = [&](int u, int kp) { return slots[u]->get_landmark((unsigned)kp); };
    for (int p = 0; p < passes; ++p) {
        const int u = p < K ? p + 1 : 0, n = p < K ? n_fwd : n_bwd;
        const int32_t* list = p < K ? fwd.data() : bwd.data();
        const size_t o = p < K ? (size_t)p * n_fwd : (size_t)K * n_fwd;
        std::vector<lm_ptr> in_keyfrm(n);
        for (int i = 0; i < n; ++i)
            if (0 <= best[o + i]) in_keyfrm[i] = holder(u, best[o + i]);  // keyfrm->get_landmark(best_idx) at detection time (fuse.cc:136)
        for (int i = 0; i < n; ++i) {
            const uint8_t ev = event[o + i];
            if (ev != SVGPU_FUSE_DUP_SURVIVED && ev != SVGPU_FUSE_DUP_LOST) continue;
            const lm_ptr checked = lms[list[i]], other = in_keyfrm[i];
            const lm_ptr survivor = ev == SVGPU_FUSE_DUP_SURVIVED ? checked : other, loser = ev == SVGPU_FUSE_DUP_SURVIVED ? other : checked;
            replaced_lms[loser] = survivor;
            loser->replace(survivor, map_db);
            touched[slot_of.at(survivor)] = 1;
        }
        for (int i = 0; i < n; ++i) {
            if (event[o + i] != SVGPU_FUSE_NEW_CONNECTION) continue;
            lm_ptr lm = lms[list[i]];
            while (replaced_lms.count(lm)) lm = replaced_lms[lm];
            lm->connect_to_keyframe(slots[u], (unsigned)best[o + i]);
            touched[slot_of.at(lm)] = 1;
        }
    }
    // ---- what compute_descriptor / update_mean_normal_and_obs_scale_variance would have stored, from the table
    for (int l = 0; l < L; ++l) {
        if (!touched[l] || !alive[l]) continue;
        Vec3_t n;
        for (int k = 0; k < 3; ++k) n(k) = normal[3 * l + k];
        lms[l]->set_prediction_parameters(n, min_d[l], max_d[l]);
        lms[l]->set_representative_descriptor(&desc[(size_t)l * 32]);
    }
    return true;
}

}  // namespace hip
}  // namespace module
}  // namespace stella_vslam
