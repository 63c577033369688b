// compute_bow on the device (data/bow_vocabulary.cc:18-24; host/camera.cpp bow_vocabulary_hip::compute_bow) for many descriptor sets:
// behind the tree descent of bow_kernels.hip, the two sparse maps of every frame -- bow_vec (word -> summed weight, normalised) and
// bow_feat_vec (node key -> feature indices) -- as flat arrays in the iteration order of the reference's std::map.  DESIGN section 21.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>

#include "svgpu_internal.h"
#include "bow_compute_layout.h"

#define SV_BOWC_DROPPED (~0ull)  // the composite key of a feature that takes no part (DBoW2 form: weight not > 0); sorts behind every other

struct BowComputeProblem {
    int num_frames, total;  // B, N
    int dbow2;              // 1: stop words dropped, L1 norm; 0: FBoW form, every feature, L2 norm
    const int32_t* d_off;   // B + 1
    int32_t* frame;         // N
    const int32_t* word;
    const float* weight;
    const int32_t* node;
    unsigned long long *vkey, *fkey;
    int32_t *head, *kept;
    int32_t *vec_off, *feat_off;
    uint32_t *vec_word, *feat_key;
    double* vec_weight;
    int32_t* feat_index;
};

// bow_kernels.hip: the descent kernels of svgpu_bow_transform / svgpu_fbow_transform over n descriptors that lie on the device
// (fbow_k == 0: DBoW2 form with `level` = node_level; else FBoW form with `level` = store_level)
int sv_vocabulary_device(const svgpu_vocabulary* vocab);
void sv_launch_bow_descend(hipStream_t s, const svgpu_vocabulary* vocab, const uint32_t* desc, int n, int level, int fbow_k, int32_t* word, float* weight,
                           int32_t* node);

void sv_launch_bowc_owner(hipStream_t s, const BowComputeProblem& P);
// one workgroup per frame of at most SV_BOWC_LDS_MAX descriptors; `max_lds_frame`: the longest of them
void sv_launch_bowc_sort_lds(hipStream_t s, const BowComputeProblem& P, int max_lds_frame);
// a longer frame through sv_sort_pairs: keys and payload of pass `which` (0: words, 1: node keys) of the frame at `first` with n descriptors
void sv_launch_bowc_big_init(hipStream_t s, const BowComputeProblem& P, int first, int n, int which, unsigned* keys, unsigned long long* vals);
void sv_launch_bowc_big_pack(hipStream_t s, const BowComputeProblem& P, int first, int n, int which, const unsigned* keys, const unsigned long long* vals);
void sv_launch_bowc_heads(hipStream_t s, const BowComputeProblem& P);
void sv_launch_bowc_emit(hipStream_t s, const BowComputeProblem& P);
void sv_launch_bowc_normalise(hipStream_t s, const BowComputeProblem& P);

// svgpu_bowdb.hip: B vectors appended to a database's pools as one submission, from host arrays or from device arrays on ctx's stream.
// begin() takes the database's mutex, makes the one growth check and enqueues the copies; the caller synchronises the stream; commit()
// then makes the slots known to the host side.  The mutex is held until the object goes (a call that fails in between changes nothing
// the database's host side knows of).
struct SvBowdbAppendState;  // the held mutex and the new slot records (svgpu_bowdb.hip)
struct SvBowdbAppend {
    svgpu_bowdb* db = nullptr;
    std::unique_ptr<SvBowdbAppendState> state;
    int copies = 0, syncs = 0;  // what begin() issued
    int begin(svgpu_ctx* ctx, svgpu_bowdb* db_, int num, const int32_t* off, const uint32_t* words, const double* weights, bool on_device);
    void commit(int32_t* slots);
    ~SvBowdbAppend();  // (out of line: where the state's type is complete)
    SvBowdbAppend();
    SvBowdbAppend(const SvBowdbAppend&) = delete;
    SvBowdbAppend& operator=(const SvBowdbAppend&) = delete;
};
int sv_bowdb_device(const svgpu_bowdb* db);
