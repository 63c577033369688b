// stella_vslam::data::hip::bow_database -- data/bow_database.h:20-100 with the reference's public signatures, backed by the
// device-resident database svgpu_bowdb_* (include/svgpu.h).  The host keeps the keyframe id -> slot map and the shared_ptrs; the
// reference's inverted index keyfrms_in_node_ has no counterpart (the device scans a forward index).  acquire_keyframes returns the
// candidates in ascending slot (= insertion) order; the reference's order is that of an unordered_set, i.e. unspecified.
#pragma once
#include <mutex>
#include <unordered_map>

#include "camera.h"
#include "hip_backend.h"

namespace stella_vslam {
namespace data {
#ifdef SVGPU_WITH_STELLA_VSLAM
class bow_vocabulary;
#else
using bow_vocabulary = void;  // only carried, as the reference's constructor takes it
#endif
namespace hip {

class bow_database {
public:
    //! score_form: SVGPU_BOW_SCORE_FBOW_L2 (the default build) or SVGPU_BOW_SCORE_DBOW2_L1 (USE_DBOW2)
    explicit bow_database(bow_vocabulary* bow_vocab, int score_form = SVGPU_BOW_SCORE_FBOW_L2);
    ~bow_database();
    bow_database(const bow_database&) = delete;
    bow_database& operator=(const bow_database&) = delete;

    void add_keyframe(const std::shared_ptr<keyframe>& keyfrm);
    //! add_keyframe for every keyframe of the list, in order, as ONE svgpu_bowdb_add_batch (map load: io/map_database_io_*.cc register
    //! every keyframe); keyframes the database already holds are passed over
    void add_keyframes(const std::vector<std::shared_ptr<keyframe>>& keyfrms);
    //! the same for keyframes that have descriptors but no BoW yet (data/keyframe.cc:244, data/map_database.cc:399): compute_bow of all
    //! of them in one svgpu_bow_compute_batch, which fills bow_vec_ / bow_feat_vec_ and appends the vectors to the database device to device
    void add_keyframes(const std::vector<std::shared_ptr<keyframe>>& keyfrms, const stella_vslam_hip::data::bow_vocabulary_hip& vocab, int levels_up = 4);
    void erase_keyframe(const std::shared_ptr<keyframe>& keyfrm);
    void clear();
    std::vector<std::shared_ptr<keyframe>> acquire_keyframes(const bow_vector& bow_vec, const float min_score = 0.0f,
                                                             const float num_common_words_thr_ratio = 0.8f,
                                                             const std::set<std::shared_ptr<keyframe>>& keyfrms_to_reject = {});
    //! bow_vocabulary_util::score(bow_vocab, bow_vec, keyfrm->bow_vec_) for each listed keyframe in one device call
    //! (loop_detector::compute_min_score_in_covisibilities, module/loop_detector.cc:278-297); -1 for a keyframe the database does not hold
    std::vector<float> score_keyframes(const bow_vector& bow_vec, const std::vector<std::shared_ptr<keyframe>>& keyfrms);
    //! shared-word count and score of every keyframe the last acquire_keyframes returned, in its order
    std::vector<unsigned int> last_num_common_words_;
    std::vector<float> last_scores_;

private:
    bow_vocabulary* bow_vocab_;
    svgpu_bowdb* db_ = nullptr;
    mutable std::mutex mtx_;
    std::unordered_map<unsigned int, int32_t> slot_of_id_;       // keyframe::id_ -> slot
    std::unordered_map<int32_t, std::shared_ptr<keyframe>> keyfrm_of_slot_;
};

}  // namespace hip
}  // namespace data
}  // namespace stella_vslam
