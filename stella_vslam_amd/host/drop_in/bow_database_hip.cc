#include "bow_database_hip.h"

#include <algorithm>

namespace stella_vslam {
namespace data {
namespace hip {

namespace {
// a std::map iterates in ascending word id: the order the C ABI asks for
void flatten(const bow_vector& bow_vec, std::vector<uint32_t>& words, std::vector<double>& weights) {
    words.clear(), weights.clear();
    words.reserve(bow_vec.size()), weights.reserve(bow_vec.size());
    for (const auto& word_and_weight : bow_vec) {
        words.push_back((uint32_t)word_and_weight.first);
        weights.push_back((double)word_and_weight.second);
    }
}
}  // namespace

bow_database::bow_database(bow_vocabulary* bow_vocab, int score_form) : bow_vocab_(bow_vocab) {
    stella_vslam::hip::check(svgpu_bowdb_create(stella_vslam::hip::context(), score_form, &db_), "svgpu_bowdb_create");
}

bow_database::~bow_database() { svgpu_bowdb_destroy(db_); }

void bow_database::add_keyframe(const std::shared_ptr<keyframe>& keyfrm) {
    std::lock_guard<std::mutex> lock(mtx_);
    if (slot_of_id_.count(keyfrm->id_)) return;  // (the reference would list it twice and count its words twice; nothing adds a keyframe twice)
    std::vector<uint32_t> words;
    std::vector<double> weights;
    flatten(keyfrm->bow_vec_, words, weights);
    int32_t slot = -1;
    stella_vslam::hip::check(svgpu_bowdb_add(stella_vslam::hip::context(), db_, (int)words.size(), words.data(), weights.data(), &slot), "svgpu_bowdb_add");
    slot_of_id_[keyfrm->id_] = slot;
    keyfrm_of_slot_[slot] = keyfrm;
}

void bow_database::add_keyframes(const std::vector<std::shared_ptr<keyframe>>& keyfrms) {
    std::lock_guard<std::mutex> lock(mtx_);
    std::vector<std::shared_ptr<keyframe>> fresh;
    std::vector<int32_t> off{0};
    std::vector<uint32_t> words;
    std::vector<double> weights;
    for (const auto& keyfrm : keyfrms) {
        if (slot_of_id_.count(keyfrm->id_) || std::any_of(fresh.begin(), fresh.end(), [&](const auto& k) { return k->id_ == keyfrm->id_; })) continue;
        fresh.push_back(keyfrm);
        for (const auto& word_and_weight : keyfrm->bow_vec_) {
            words.push_back((uint32_t)word_and_weight.first);
            weights.push_back((double)word_and_weight.second);
        }
        off.push_back((int32_t)words.size());
    }
    std::vector<int32_t> slots(fresh.size(), -1);
    stella_vslam::hip::check(svgpu_bowdb_add_batch(stella_vslam::hip::context(), db_, (int)fresh.size(), off.data(), words.data(), weights.data(), slots.data()),
                             "svgpu_bowdb_add_batch");
    for (size_t i = 0; i < fresh.size(); ++i) {
        slot_of_id_[fresh[i]->id_] = slots[i];
        keyfrm_of_slot_[slots[i]] = fresh[i];
    }
}

void bow_database::add_keyframes(const std::vector<std::shared_ptr<keyframe>>& keyfrms, const stella_vslam_hip::data::bow_vocabulary_hip& vocab, int levels_up) {
    std::lock_guard<std::mutex> lock(mtx_);
    std::vector<std::shared_ptr<keyframe>> fresh;
    std::vector<cv::Mat> descriptors;
    for (const auto& keyfrm : keyfrms) {
        if (slot_of_id_.count(keyfrm->id_) || std::any_of(fresh.begin(), fresh.end(), [&](const auto& k) { return k->id_ == keyfrm->id_; })) continue;
        fresh.push_back(keyfrm);
        descriptors.push_back(keyfrm->frm_obs_.descriptors_);
    }
    std::vector<bow_vector> bow_vecs;
    std::vector<bow_feature_vector> bow_feat_vecs;
    std::vector<int32_t> slots;
    vocab.compute_bow_batch(descriptors, bow_vecs, bow_feat_vecs, levels_up, db_, &slots);
    for (size_t i = 0; i < fresh.size(); ++i) {
        fresh[i]->bow_vec_.swap(bow_vecs[i]);
        fresh[i]->bow_feat_vec_.swap(bow_feat_vecs[i]);
        slot_of_id_[fresh[i]->id_] = slots[i];
        keyfrm_of_slot_[slots[i]] = fresh[i];
    }
}

void bow_database::erase_keyframe(const std::shared_ptr<keyframe>& keyfrm) {
    std::lock_guard<std::mutex> lock(mtx_);
    const auto it = slot_of_id_.find(keyfrm->id_);
    if (it == slot_of_id_.end()) return;
    stella_vslam::hip::check(svgpu_bowdb_erase(stella_vslam::hip::context(), db_, it->second), "svgpu_bowdb_erase");
    keyfrm_of_slot_.erase(it->second);
    slot_of_id_.erase(it);
}

void bow_database::clear() {
    std::lock_guard<std::mutex> lock(mtx_);
    stella_vslam::hip::check(svgpu_bowdb_clear(stella_vslam::hip::context(), db_), "svgpu_bowdb_clear");
    slot_of_id_.clear();
    keyfrm_of_slot_.clear();
}

std::vector<std::shared_ptr<keyframe>> bow_database::acquire_keyframes(const bow_vector& bow_vec, const float min_score,
                                                                       const float num_common_words_thr_ratio,
                                                                       const std::set<std::shared_ptr<keyframe>>& keyfrms_to_reject) {
    std::lock_guard<std::mutex> lock(mtx_);
    std::vector<uint32_t> words;
    std::vector<double> weights;
    flatten(bow_vec, words, weights);
    std::vector<int32_t> reject;
    for (const auto& keyfrm : keyfrms_to_reject) {
        const auto it = keyfrm ? slot_of_id_.find(keyfrm->id_) : slot_of_id_.end();
        if (it != slot_of_id_.end()) reject.push_back(it->second);
    }
    const int cap = (int)keyfrm_of_slot_.size();
    std::vector<int32_t> slots(cap);
    std::vector<uint32_t> common(cap);
    std::vector<float> score(cap);
    int32_t n = 0;
    stella_vslam::hip::check(svgpu_bowdb_acquire(stella_vslam::hip::context(), db_, (int)words.size(), words.data(), weights.data(), min_score,
                                                 num_common_words_thr_ratio, (int)reject.size(), reject.data(), cap, slots.data(), common.data(), score.data(),
                                                 &n, nullptr),
                             "svgpu_bowdb_acquire");
    std::vector<std::shared_ptr<keyframe>> candidates;
    last_num_common_words_.clear(), last_scores_.clear();
    for (int i = 0; i < n && i < cap; ++i) {
        candidates.push_back(keyfrm_of_slot_.at(slots[i]));
        last_num_common_words_.push_back(common[i]);
        last_scores_.push_back(score[i]);
    }
    return candidates;
}

std::vector<float> bow_database::score_keyframes(const bow_vector& bow_vec, const std::vector<std::shared_ptr<keyframe>>& keyfrms) {
    std::lock_guard<std::mutex> lock(mtx_);
    std::vector<uint32_t> words;
    std::vector<double> weights;
    flatten(bow_vec, words, weights);
    std::vector<int32_t> slots;
    for (const auto& keyfrm : keyfrms) {
        const auto it = keyfrm ? slot_of_id_.find(keyfrm->id_) : slot_of_id_.end();
        slots.push_back(it != slot_of_id_.end() ? it->second : -1);
    }
    std::vector<float> scores(slots.size(), -1.0f);
    stella_vslam::hip::check(svgpu_bowdb_score(stella_vslam::hip::context(), db_, (int)words.size(), words.data(), weights.data(), (int)slots.size(),
                                               slots.data(), scores.data()),
                             "svgpu_bowdb_score");
    return scores;
}

}  // namespace hip
}  // namespace data
}  // namespace stella_vslam
