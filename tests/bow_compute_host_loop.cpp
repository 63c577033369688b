// The host accumulation of data::bow_vocabulary_hip::compute_bow (stella_vslam_amd/host/camera.cpp) compiled alone: the same std::map
// loops over descent arrays read from a file, the two maps written out flat.  tests/test_bow_compute_problem_classes.py compares the
// step-by-step restatement of tests/bow_compute_problems.py with it, bit for bit.  Build with -ffp-contract=off, as the library is.
//   in:  int32 form (0 dbow2, 1 fbow), int32 n, int32 word[n], float weight[n], uint32 node[n]
//   out: int32 nv, int32 nf, uint32 vec_word[nv], double vec_weight[nv], uint32 feat_key[nf], int32 feat_index[nf]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t form = 0, n = 0;
    if (std::fread(&form, 4, 1, in) != 1 || std::fread(&n, 4, 1, in) != 1 || n < 0) return 2;
    std::vector<int32_t> word((size_t)n);
    std::vector<float> weight((size_t)n);
    std::vector<uint32_t> node((size_t)n);
    if (n && (std::fread(word.data(), 4, (size_t)n, in) != (size_t)n || std::fread(weight.data(), 4, (size_t)n, in) != (size_t)n
              || std::fread(node.data(), 4, (size_t)n, in) != (size_t)n))
        return 2;
    std::fclose(in);

    std::map<unsigned int, double> bow_vec;
    std::map<unsigned int, std::vector<unsigned int>> bow_feat_vec;
    if (form == 1) {
        for (int i = 0; i < n; ++i) {
            bow_vec[(unsigned int)word[(size_t)i]] += (double)weight[(size_t)i];
            bow_feat_vec[node[(size_t)i]].push_back((unsigned int)i);
        }
        double norm = 0.0;
        for (const auto& kv : bow_vec) norm += kv.second * kv.second;
        if (norm > 0.0)
            for (auto& kv : bow_vec) kv.second *= 1.0 / std::sqrt(norm);
    }
    else {
        for (int i = 0; i < n; ++i)
            if (weight[(size_t)i] > 0.f) {
                bow_vec[(unsigned int)word[(size_t)i]] += (double)weight[(size_t)i];
                bow_feat_vec[node[(size_t)i]].push_back((unsigned int)i);
            }
        double norm = 0.0;
        for (const auto& kv : bow_vec) norm += std::fabs(kv.second);
        if (norm > 0.0)
            for (auto& kv : bow_vec) kv.second /= norm;
    }

    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    int32_t nv = (int32_t)bow_vec.size(), nf = 0;
    for (const auto& kv : bow_feat_vec) nf += (int32_t)kv.second.size();
    std::fwrite(&nv, 4, 1, out), std::fwrite(&nf, 4, 1, out);
    for (const auto& kv : bow_vec) std::fwrite(&kv.first, 4, 1, out);
    for (const auto& kv : bow_vec) std::fwrite(&kv.second, 8, 1, out);
    for (const auto& kv : bow_feat_vec)
        for (size_t j = 0; j < kv.second.size(); ++j) std::fwrite(&kv.first, 4, 1, out);
    for (const auto& kv : bow_feat_vec)
        for (unsigned int i : kv.second) std::fwrite(&i, 4, 1, out);
    std::fclose(out);
    std::printf("bow compute host loop ok\n");
    return 0;
}
