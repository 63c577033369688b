// data::hip::bow_database on stand-in keyframes against a host transcription of the reference's algorithm (data/bow_database.cc:58-159:
// an inverted index word -> list of keyframes, shared words counted in a second hash map, the survivors scored one by one), over the same
// objects, for both score forms: candidate sets equal, scores bit-equal.
//   test_bow_database                         the checks
//   test_bow_database --bench KF WORDS REPS   median times of one query: the host transcription and the device call, for tools/bench_extra.py
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <memory>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "drop_in/bow_database_hip.h"

using namespace stella_vslam;

namespace {
unsigned long long g_state = 88172645463325252ull;
double uni() {  // xorshift64, [0, 1)
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return (double)(g_state >> 11) / 9007199254740992.0;
}
int g_fail = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                           \
        }                                                       \
    } while (0)

using keyfrm_ptr = std::shared_ptr<data::keyframe>;

// score of two BoW vectors by the sequential merge of the two libraries (restated from their published sources: parity unpinned)
float host_score(int form, const data::bow_vector& v1, const data::bow_vector& v2) {
    auto i1 = v1.begin(), i2 = v2.begin();
    double s = 0.0;
    while (i1 != v1.end() && i2 != v2.end()) {
        if (i1->first == i2->first) {
            if (form == SVGPU_BOW_SCORE_FBOW_L2) {
                const float vi = (float)i1->second, wi = (float)i2->second;
                s += (double)(vi * wi);
            }
            else {
                const double vi = i1->second, wi = i2->second;
                s += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
            }
            ++i1, ++i2;
        }
        else if (i1->first < i2->first) ++i1;
        else ++i2;
    }
    if (form == SVGPU_BOW_SCORE_FBOW_L2) return (float)(s >= 1.0 ? 1.0 : 1.0 - std::sqrt(1.0 - s));
    return (float)(-s / 2.0);
}

// the reference's database on the host
struct host_database {
    int form;
    std::unordered_map<unsigned int, std::list<keyfrm_ptr>> keyfrms_in_node;
    void add(const keyfrm_ptr& kf) {
        for (const auto& w : kf->bow_vec_) keyfrms_in_node[w.first].push_back(kf);
    }
    void erase(const keyfrm_ptr& kf) {
        for (const auto& w : kf->bow_vec_) {
            auto it = keyfrms_in_node.find(w.first);
            if (it == keyfrms_in_node.end()) continue;
            for (auto k = it->second.begin(); k != it->second.end(); ++k)
                if ((*k)->id_ == kf->id_) {
                    it->second.erase(k);
                    break;
                }
        }
    }
    std::unordered_map<keyfrm_ptr, float> acquire(const data::bow_vector& q, float min_score, float ratio, const std::set<keyfrm_ptr>& reject) const {
        std::unordered_map<keyfrm_ptr, unsigned int> num_common;
        for (const auto& w : q) {
            const auto it = keyfrms_in_node.find(w.first);
            if (it == keyfrms_in_node.end()) continue;
            for (const auto& kf : it->second)
                if (!reject.count(kf)) ++num_common[kf];
        }
        std::unordered_map<keyfrm_ptr, float> kept;
        if (num_common.empty()) return kept;
        unsigned int max_common = 0;
        for (const auto& kc : num_common) max_common = std::max(max_common, kc.second);
        const auto thr = static_cast<unsigned int>(ratio * max_common);
        for (const auto& kc : num_common) {
            if (!(thr < kc.second)) continue;
            const float score = host_score(form, q, kc.first->bow_vec_);
            if (min_score > score) continue;
            kept[kc.first] = score;
        }
        return kept;
    }
};

data::bow_vector random_vector(int n, unsigned int vocab, int form) {
    data::bow_vector v;
    while ((int)v.size() < n) v[(unsigned int)(uni() * vocab)] = 0.05 + uni();
    double norm = 0.0;
    for (const auto& w : v) norm += form == SVGPU_BOW_SCORE_FBOW_L2 ? w.second * w.second : std::fabs(w.second);
    if (form == SVGPU_BOW_SCORE_FBOW_L2) norm = std::sqrt(norm);
    for (auto& w : v) w.second /= norm;
    return v;
}
// `keep` of the words of `src` (with fresh weights), filled up to n with random ones
data::bow_vector near_copy(const data::bow_vector& src, double keep, int n, unsigned int vocab, int form) {
    data::bow_vector v;
    for (const auto& w : src)
        if (uni() < keep) v[w.first] = 0.05 + uni();
    data::bow_vector fill = random_vector(std::max(n - (int)v.size(), 1), vocab, form);
    for (const auto& w : fill) v.emplace(w.first, w.second);
    double norm = 0.0;
    for (const auto& w : v) norm += form == SVGPU_BOW_SCORE_FBOW_L2 ? w.second * w.second : std::fabs(w.second);
    if (form == SVGPU_BOW_SCORE_FBOW_L2) norm = std::sqrt(norm);
    for (auto& w : v) w.second /= norm;
    return v;
}

void compare(data::hip::bow_database& dev, const host_database& host, const data::bow_vector& q, float min_score, float ratio,
             const std::set<keyfrm_ptr>& reject, int& total) {
    const auto got = dev.acquire_keyframes(q, min_score, ratio, reject);
    const auto exp = host.acquire(q, min_score, ratio, reject);
    CHECK(got.size() == exp.size());
    for (size_t i = 0; i < got.size(); ++i) {
        const auto it = exp.find(got[i]);
        CHECK(it != exp.end());
        if (it != exp.end()) CHECK(std::memcmp(&it->second, &dev.last_scores_[i], 4) == 0);
        if (i) CHECK(got[i - 1]->id_ < got[i]->id_);  // insertion order = id order here
    }
    total += (int)got.size();
}

int run_form(int form) {
    const unsigned int vocab = 5000;
    const int n_kf = 200, n_words = 180;
    host_database host{form, {}};
    data::hip::bow_database dev(nullptr, form);
    std::vector<keyfrm_ptr> kfs;
    const data::bow_vector q = random_vector(n_words, vocab, form);
    for (int i = 0; i < n_kf; ++i) {
        auto kf = std::make_shared<data::keyframe>(10 + 3 * i, nullptr, nullptr);
        kf->bow_vec_ = i % 20 == 5 ? near_copy(q, 0.5 + 0.45 * uni(), n_words, vocab, form) : random_vector(n_words / 2 + (int)(uni() * n_words), vocab, form);
        kfs.push_back(kf);
        host.add(kf);
        dev.add_keyframe(kf);
    }
    int total = 0;
    compare(dev, host, q, 0.0f, 0.8f, {}, total);
    compare(dev, host, q, 0.0f, 0.0f, {}, total);
    compare(dev, host, q, 0.05f, 0.3f, {kfs[5], kfs[25]}, total);
    CHECK(total > 10);
    // a score of a kept keyframe as the gate: it stays; the reference's own keyframe set, rejected altogether: nothing
    const auto kept = host.acquire(q, 0.0f, 0.5f, {});
    CHECK(!kept.empty());
    if (!kept.empty()) compare(dev, host, q, kept.begin()->second, 0.5f, {}, total);
    compare(dev, host, q, 0.0f, 0.8f, std::set<keyfrm_ptr>(kfs.begin(), kfs.end()), total);
    // listed scores (the loop detector's covisibilities), one of them not in the database
    auto stranger = std::make_shared<data::keyframe>(7, nullptr, nullptr);
    const auto sc = dev.score_keyframes(q, {kfs[5], stranger, kfs[0], kfs[45]});
    CHECK(sc.size() == 4 && sc[1] == -1.0f);
    for (int j : {0, 2, 3}) {
        const float e = host_score(form, q, kfs[j == 0 ? 5 : j == 2 ? 0 : 45]->bow_vec_);
        CHECK(std::memcmp(&e, &sc[j], 4) == 0);
    }
    // erase (the best ones, and one twice), then clear and reuse
    for (int i : {5, 25, 45, 5}) {
        host.erase(kfs[i]);
        dev.erase_keyframe(kfs[i]);
    }
    compare(dev, host, q, 0.0f, 0.8f, {}, total);
    compare(dev, host, kfs[65]->bow_vec_, 0.0f, 0.8f, {kfs[65]}, total);
    dev.clear();
    host.keyfrms_in_node.clear();
    compare(dev, host, q, 0.0f, 0.8f, {}, total);
    for (int i = 100; i < 140; ++i) host.add(kfs[i]), dev.add_keyframe(kfs[i]);
    compare(dev, host, q, 0.0f, 0.0f, {}, total);
    std::printf("%s: %d candidates compared\n", form == SVGPU_BOW_SCORE_FBOW_L2 ? "fbow L2" : "dbow2 L1", total);
    return total;
}

double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int bench(int n_kf, int n_words, int reps) {
    const int form = SVGPU_BOW_SCORE_FBOW_L2;
    const unsigned int vocab = 100000;
    host_database host{form, {}};
    data::hip::bow_database dev(nullptr, form);
    const data::bow_vector q = random_vector(n_words, vocab, form);
    for (int i = 0; i < n_kf; ++i) {
        auto kf = std::make_shared<data::keyframe>(i, nullptr, nullptr);
        kf->bow_vec_ = i % 100 == 5 ? near_copy(q, 0.8, n_words, vocab, form) : random_vector(n_words, vocab, form);
        host.add(kf);
        dev.add_keyframe(kf);
    }
    std::vector<double> th, td;
    size_t nh = 0, nd = 0;
    for (int r = 0; r < reps + 3; ++r) {
        auto t0 = std::chrono::steady_clock::now();
        nh = host.acquire(q, 0.0f, 0.8f, {}).size();
        auto t1 = std::chrono::steady_clock::now();
        nd = dev.acquire_keyframes(q, 0.0f, 0.8f, {}).size();
        auto t2 = std::chrono::steady_clock::now();
        if (r >= 3) th.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()), td.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    std::printf("{\"keyframes\": %d, \"words\": %d, \"candidates\": %zu, \"host_transcription_ms\": %.4f, \"drop_in_ms\": %.4f}\n", n_kf, n_words, nd, median(th),
                median(td));
    return nh == nd ? 0 : 1;
}
}  // namespace

int main(int argc, char** argv) {
    try {
        if (argc == 5 && !std::strcmp(argv[1], "--bench")) return bench(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
        run_form(SVGPU_BOW_SCORE_FBOW_L2);
        run_form(SVGPU_BOW_SCORE_DBOW2_L1);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("bow_database ok\n");
    return 0;
}
