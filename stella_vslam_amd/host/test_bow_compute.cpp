// data::bow_vocabulary_hip::compute_bow_batch and data::hip::bow_database::add_keyframes (both overloads) over the stand-in data:: classes,
// against the loop of compute_bow plus add_keyframe on the same descriptors, for both forms: the maps entry for entry with the weights as
// raw bit patterns, and every later acquire_keyframes (keyframe ids, shared-word counts, scores as bits), also after erases.
//   test_bow_compute                      the checks
//   test_bow_compute --bench B N REPS     times of registering B keyframes of N descriptors against a vocabulary of about 10^5 words: the
//                                         loop and the one call, for tools/bench_bow_compute.py (outputs asserted equal first)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "drop_in/bow_database_hip.h"

using namespace stella_vslam;
using stella_vslam_hip::data::bow_vocabulary_hip;

namespace {
unsigned long long g_state = 88172645463325252ull;
unsigned long long rnd() {  // xorshift64
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return g_state;
}
int g_fail = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                  \
        }                                                              \
    } while (0)

using keyfrm_ptr = std::shared_ptr<data::keyframe>;

// a full tree of branching k and the given depth; word ids not contiguous, one leaf in seven a stop word
std::unique_ptr<bow_vocabulary_hip> make_vocabulary(int k, int depth, int fbow_k) {
    std::vector<int> child_off{0}, children, word_id;
    std::vector<float> weight;
    std::vector<int> level{0};
    int n = 1;
    for (int i = 0; i < n; ++i) {  // breadth first: node i's children are appended while the list grows
        if (level[(size_t)i] < depth)
            for (int c = 0; c < k; ++c) {
                children.push_back(n++);
                level.push_back(level[(size_t)i] + 1);
            }
        child_off.push_back((int)children.size());
    }
    cv::Mat desc(n, 32, CV_8U);
    for (int i = 0; i < n; ++i) {
        for (int b = 0; b < 32; ++b) desc.ptr(i)[b] = (unsigned char)(rnd() >> 24);
        const bool leaf = level[(size_t)i] == depth;
        word_id.push_back(leaf ? 7 + 13 * i : -1);
        weight.push_back(leaf ? (rnd() % 7 == 0 ? 0.f : 0.01f + (float)(rnd() % 4000) * 0.001f) : 0.f);
    }
    return std::make_unique<bow_vocabulary_hip>(stella_vslam::hip::context(), child_off, children, desc, weight, word_id, depth, fbow_k);
}

cv::Mat random_descriptors(int n) {
    cv::Mat d(n, 32, CV_8U);
    for (int i = 0; i < n; ++i)
        for (int b = 0; b < 32; ++b) d.ptr(i)[b] = (unsigned char)(rnd() >> 24);
    return d;
}

std::vector<keyfrm_ptr> make_keyframes(const std::vector<cv::Mat>& descs) {
    std::vector<keyfrm_ptr> kfs;
    for (size_t i = 0; i < descs.size(); ++i) {
        kfs.push_back(std::make_shared<data::keyframe>(10 + 3 * (unsigned int)i, nullptr, nullptr));
        kfs.back()->frm_obs_.descriptors_ = descs[i];
    }
    return kfs;
}

bool same_bits(const data::bow_vector& a, const data::bow_vector& b) {
    if (a.size() != b.size()) return false;
    for (auto i = a.begin(), j = b.begin(); i != a.end(); ++i, ++j)
        if (i->first != j->first || std::memcmp(&i->second, &j->second, 8) != 0) return false;
    return true;
}

// the same query on both databases: the same keyframes by id, the same counts, the same scores bit for bit
void same_answers(data::hip::bow_database& a, data::hip::bow_database& b, const data::bow_vector& q, float ratio, int& total) {
    const auto ra = a.acquire_keyframes(q, 0.0f, ratio);
    const auto rb = b.acquire_keyframes(q, 0.0f, ratio);
    CHECK(ra.size() == rb.size());
    for (size_t i = 0; i < ra.size() && i < rb.size(); ++i) {
        CHECK(ra[i]->id_ == rb[i]->id_ && a.last_num_common_words_[i] == b.last_num_common_words_[i]);
        CHECK(std::memcmp(&a.last_scores_[i], &b.last_scores_[i], 4) == 0);
    }
    total += (int)ra.size();
}

void run_form(int fbow_k) {
    const int form = fbow_k > 0 ? SVGPU_BOW_SCORE_FBOW_L2 : SVGPU_BOW_SCORE_DBOW2_L1;
    auto voc = make_vocabulary(4, 4, fbow_k);
    const int levels_up = 2;
    std::vector<cv::Mat> descs;
    for (int n : {0, 1, 65, 300, 12, 0, 257, 64, 40, 500, 7, 130, 0}) descs.push_back(random_descriptors(n));
    const size_t B = descs.size();
    // the loop that exists: compute_bow and add_keyframe per keyframe
    auto kf_loop = make_keyframes(descs);
    data::hip::bow_database db_loop(nullptr, form);
    for (auto& kf : kf_loop) {
        voc->compute_bow(kf->frm_obs_.descriptors_, kf->bow_vec_, kf->bow_feat_vec_, levels_up);
        db_loop.add_keyframe(kf);
    }
    // compute_bow_batch through the batch call and through its loop: the maps entry for entry
    for (int min_frames : {1, 1000}) {
        voc->min_frames_for_batch_ = min_frames;
        std::vector<data::bow_vector> bv;
        std::vector<data::bow_feature_vector> fv;
        voc->compute_bow_batch(descs, bv, fv, levels_up);
        CHECK(bv.size() == B && fv.size() == B);
        for (size_t f = 0; f < B && f < bv.size(); ++f) CHECK(same_bits(bv[f], kf_loop[f]->bow_vec_) && fv[f] == kf_loop[f]->bow_feat_vec_);
    }
    voc->min_frames_for_batch_ = 1;
    // add_keyframes of keyframes that hold their BoW, and of keyframes that hold descriptors only
    auto kf_add = make_keyframes(descs), kf_fused = make_keyframes(descs);
    for (size_t f = 0; f < B; ++f) kf_add[f]->bow_vec_ = kf_loop[f]->bow_vec_, kf_add[f]->bow_feat_vec_ = kf_loop[f]->bow_feat_vec_;
    data::hip::bow_database db_add(nullptr, form), db_fused(nullptr, form);
    db_add.add_keyframes(kf_add);
    db_add.add_keyframes({kf_add[2], kf_add[3]});  // held already: passed over
    db_fused.add_keyframes(kf_fused, *voc, levels_up);
    size_t words = 0;
    for (size_t f = 0; f < B; ++f) {
        CHECK(same_bits(kf_fused[f]->bow_vec_, kf_loop[f]->bow_vec_) && kf_fused[f]->bow_feat_vec_ == kf_loop[f]->bow_feat_vec_);
        words += kf_loop[f]->bow_vec_.size();
    }
    CHECK(words > 500);
    int total = 0;
    auto all_queries = [&]() {
        for (size_t f : {size_t(2), size_t(3), size_t(6), size_t(9), size_t(0)})
            for (float ratio : {0.0f, 0.3f, 0.8f}) {
                same_answers(db_loop, db_add, kf_loop[f]->bow_vec_, ratio, total);
                same_answers(db_loop, db_fused, kf_loop[f]->bow_vec_, ratio, total);
            }
    };
    all_queries();
    for (size_t f : {size_t(3), size_t(9), size_t(6)}) {  // the long ones: about half of what the pools hold
        db_loop.erase_keyframe(kf_loop[f]);
        db_add.erase_keyframe(kf_add[f]);
        db_fused.erase_keyframe(kf_fused[f]);
    }
    all_queries();
    // a second batch behind the erases
    std::vector<cv::Mat> more;
    for (int n : {90, 0, 33}) more.push_back(random_descriptors(n));
    auto m_loop = make_keyframes(more), m_fused = make_keyframes(more);
    for (size_t f = 0; f < more.size(); ++f) {
        m_loop[f]->id_ += 1000, m_fused[f]->id_ += 1000;
        voc->compute_bow(more[f], m_loop[f]->bow_vec_, m_loop[f]->bow_feat_vec_, levels_up);
        db_loop.add_keyframe(m_loop[f]);
    }
    auto m_add = make_keyframes(more);
    for (size_t f = 0; f < more.size(); ++f) m_add[f]->id_ += 1000, m_add[f]->bow_vec_ = m_loop[f]->bow_vec_;
    db_add.add_keyframes(m_add);
    db_fused.add_keyframes(m_fused, *voc, levels_up);
    all_queries();
    same_answers(db_loop, db_fused, m_loop[0]->bow_vec_, 0.0f, total);
    same_answers(db_loop, db_add, m_loop[0]->bow_vec_, 0.0f, total);
    CHECK(total > 100);
    std::printf("%s: %zu keyframes, %zu words, %d candidates compared\n", fbow_k > 0 ? "fbow" : "dbow2", B, words, total);
}

struct Spread {
    double p10, median, p90;
};
Spread spread(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return {v[v.size() / 10], v[v.size() / 2], v[v.size() * 9 / 10]};
}

int bench(int B, int N, int reps) {
    auto voc = make_vocabulary(10, 5, 10);  // 10^5 words, the default (FBoW) form
    std::vector<cv::Mat> descs;
    for (int f = 0; f < B; ++f) descs.push_back(random_descriptors(N));
    auto kf_loop = make_keyframes(descs), kf_batch = make_keyframes(descs);
    data::hip::bow_database db_loop(nullptr, SVGPU_BOW_SCORE_FBOW_L2), db_batch(nullptr, SVGPU_BOW_SCORE_FBOW_L2);
    auto loop = [&]() {
        db_loop.clear();
        for (auto& kf : kf_loop) {
            voc->compute_bow(kf->frm_obs_.descriptors_, kf->bow_vec_, kf->bow_feat_vec_, 4);
            db_loop.add_keyframe(kf);
        }
    };
    auto batch = [&]() {
        db_batch.clear();
        db_batch.add_keyframes(kf_batch, *voc, 4);
    };
    loop(), batch();  // equal first
    for (int f = 0; f < B; ++f)
        if (!same_bits(kf_loop[(size_t)f]->bow_vec_, kf_batch[(size_t)f]->bow_vec_) || kf_loop[(size_t)f]->bow_feat_vec_ != kf_batch[(size_t)f]->bow_feat_vec_) return 1;
    int total = 0;
    same_answers(db_loop, db_batch, kf_loop[0]->bow_vec_, 0.0f, total);
    if (g_fail) return 1;
    const int warm = std::max(2, reps / 10);
    std::vector<double> tl, tb;
    for (int r = 0; r < reps + warm; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        loop();
        const auto t1 = std::chrono::steady_clock::now();
        batch();
        const auto t2 = std::chrono::steady_clock::now();
        if (r >= warm) tl.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()), tb.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    // per kernel class, HIP events, in a run of their own
    svgpu_ctx* ctx = stella_vslam::hip::context();
    const int prof_reps = std::max(3, std::min(20, reps / 3));
    svgpu_profile_select(ctx, "*");
    for (int r = 0; r < prof_reps; ++r) batch();
    const char* classes[4] = {"k_fbow_descend", "k_bowc_sort", "k_bowc_emit", nullptr};
    double us[3] = {0, 0, 0};
    for (int c = 0; classes[c]; ++c) {
        double ms = 0;
        long long launches = 0;
        svgpu_profile_read_class(ctx, classes[c], &ms, &launches);
        us[c] = 1000.0 * ms / prof_reps;
    }
    svgpu_profile_select(ctx, nullptr);
    const Spread l = spread(tl), b = spread(tb);
    std::printf("{\"frames\": %d, \"descriptors\": %d, \"calls\": %d, \"batch_ms\": [%.4f, %.4f, %.4f], \"loop_ms\": [%.4f, %.4f, %.4f], "
                "\"descend_us\": %.1f, \"sort_us\": %.1f, \"emit_us\": %.1f}\n",
                B, N, reps, b.p10, b.median, b.p90, l.p10, l.median, l.p90, us[0], us[1], us[2]);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    try {
        if (argc == 5 && !std::strcmp(argv[1], "--bench")) return bench(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
        run_form(4);
        run_form(0);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("bow compute drop-in ok\n");
    return 0;
}
