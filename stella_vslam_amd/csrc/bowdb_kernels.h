// Keyframe BoW database (data/bow_database.cc:58-159, data/bow_vocabulary.cc:9-16): a forward index on the device -- one pool of word ids, one
// of weights, a slot table -- scanned by two passes: shared-word counts (k_bowdb_count), then an ordered score per survivor (k_bowdb_score)
// and the compaction of the kept keyframes in ascending slot order (k_bowdb_emit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svgpu_internal.h"

#define SV_BOWDB_STAGE 4096   // query word ids a workgroup stages in LDS at a time (16 KB); a longer query is processed in chunks
#define SV_BOWDB_THREADS 256  // 4 waves: a wave owns a keyframe
#define SV_BOWDB_MAX_GRID 1024

struct BowSlot {  // one keyframe: its span of the pools
    uint32_t off, len;
    uint32_t live, pad;
};

struct BowdbProblem {
    // the database
    const uint32_t* pool_ids;
    const double* pool_w;
    const BowSlot* slots;
    int num_slots;
    int score_form;  // SVGPU_BOW_SCORE_*
    // Q queries in CSR form
    int num_queries;
    const int32_t* q_off;
    const uint32_t* q_ids;
    const double* q_w;
    const float* min_score;  // per query
    float ratio;
    const uint8_t* reject;   // num_slots bytes
    uint32_t* common;        // Q x num_slots
    uint32_t* max_common;    // Q (zeroed before the count pass)
    double* sum;             // Q x num_items: the running sum of a survivor between two chunks of a long query
    float* score;            // Q x num_items
    uint8_t* keep;           // Q x num_items
    // listed-slot form (svgpu_bowdb_score): items are list entries, every live one is scored; null: items are the slots, gated by common
    const int32_t* list;
    int num_list;
    // compacted output
    int cap;
    int32_t* out_slots;      // Q x cap
    uint32_t* out_common;
    float* out_score;
    uint32_t* n_out;         // Q
};

void sv_launch_bowdb_reject(hipStream_t s, const int32_t* reject_slots, int n, uint8_t* reject, int num_slots);
void sv_launch_bowdb_count(hipStream_t s, const BowdbProblem& P);
void sv_launch_bowdb_score(hipStream_t s, const BowdbProblem& P);
void sv_launch_bowdb_emit(hipStream_t s, const BowdbProblem& P);
// compaction of the pools: move m spans (src offset, dst offset, length) from the old pools into the new ones
void sv_launch_bowdb_move(hipStream_t s, const uint32_t* ids_old, const double* w_old, uint32_t* ids_new, double* w_new, const uint32_t* moves, int m);
