// The host side of optimize::graph_optimizer on the device (svgpu_pose_graph_optimize, include/svgpu.h): the edge list of
// optimize/graph_optimizer.cc:127-250 as a PURE function over flat arrays, testable without a device or a map.
// and stella_vslam::optimize::hip::graph_optimizer, optimize/graph_optimizer.h:19-50 with the reference's constructor and `optimize`
// signature: it gathers the arrays below from the keyframes, calls build_pose_graph_edges, svgpu_pose_graph_optimize and
// svgpu_pose_graph_correct_landmarks and writes poses and landmarks back.  With SVGPU_POSE_GRAPH_EDGES_ONLY only the pure function is
// declared (the host-only test compiles it without the library).
#pragma once
#include <cstdint>
#include <vector>

namespace stella_vslam_amd {

// keyframe k of all_keyfrms (= get_keyframes_from_root(), in that order); ids are keyframe::id_
struct pose_graph_keyframes {
    int n = 0;
    const uint32_t* id = nullptr;
    const uint8_t* will_be_erased = nullptr;
    const int64_t* parent_id = nullptr;       // spanning parent's id, -1 = none
    const int32_t* loop_off = nullptr;        // n + 1: graph_node::get_loop_edges() as ids ...
    const uint32_t* loop_id = nullptr;
    const int32_t* covis_off = nullptr;       // n + 1: ordered covisibilities (descending weight) as ids and weights ...
    const uint32_t* covis_id = nullptr;
    const uint32_t* covis_weight = nullptr;
    const double* sim3_cw = nullptr;          // n x 8: Sim3s_cw of step 2 (the pre-corrected Sim3 where there is one, else the pose with scale 1)
    const uint8_t* has_non_corrected = nullptr;  // n: the keyframe is in non_corrected_Sim3s ...
    const double* sim3_non_corrected = nullptr;  // n x 8 (rows without the flag are not read)
};
// loop_connections in the order the caller iterates its map: entry c is keyframe conn_key[c] with the ids conn_id[conn_off[c] .. conn_off[c + 1])
struct pose_graph_loop_connections {
    int n = 0;
    const uint32_t* key = nullptr;
    const int32_t* off = nullptr;
    const uint32_t* id = nullptr;
};
struct pose_graph_edge {
    uint32_t id1, id2;
    double sim3_21[8];
};

// The four edge loops of graph_optimizer.cc:127-250 in their order: loop connections (the curr -> loop pair whatever its weight, the others
// from min_num_shared_lms shared landmarks on, measured from Sim3s_cw), then per keyframe the spanning parent, the loop edges and the
// covisibilities (id1 <= id2 skipped; parent, children, loop edges, erased neighbours and pairs already inserted excluded), measured from
// the NON-corrected Sim3 of both ends where there is one.  Throws std::out_of_range for an id that is not among the keyframes, as the
// reference's .at() does.
std::vector<pose_graph_edge> build_pose_graph_edges(const pose_graph_keyframes& kfs, const pose_graph_loop_connections& conns, uint32_t curr_id,
                                                    uint32_t loop_id, unsigned int min_num_shared_lms);

}  // namespace stella_vslam_amd

#ifndef SVGPU_POSE_GRAPH_EDGES_ONLY
#include <map>
#include <memory>
#include <unordered_map>

#include "hip_backend.h"

namespace stella_vslam {
namespace optimize {
namespace hip {

class graph_optimizer {
public:
    //! Constructor (optimize/graph_optimizer.cc:22-24: min_num_shared_lms defaults to 100)
    explicit graph_optimizer(const YAML::Node& yaml_node, const bool fix_scale);
    virtual ~graph_optimizer() = default;

    //! Perform pose graph optimization (optimize/graph_optimizer.cc:26-303), one svgpu_pose_graph_optimize call
    void optimize(const std::shared_ptr<data::keyframe>& loop_keyfrm, const std::shared_ptr<data::keyframe>& curr_keyfrm,
                  const module::keyframe_Sim3_pairs_t& non_corrected_Sim3s, const module::keyframe_Sim3_pairs_t& pre_corrected_Sim3s,
                  const std::map<std::shared_ptr<data::keyframe>, std::set<std::shared_ptr<data::keyframe>>>& loop_connections,
                  std::unordered_map<unsigned int, unsigned int>& found_lm_to_ref_keyfrm_id) const;

    //! Linear solver of the damped systems (svgpu_pose_graph_optimize_ex); the default is the PCG of svgpu_pose_graph_optimize
    void set_linear_solver(svgpu_pose_graph_solver solver) { solver_ = solver; }

    //! what the last call's device run reported
    mutable svgpu_pose_graph_stats last_stats_{};
    mutable svgpu_pose_graph_solver_stats last_solver_stats_{};

private:
    const bool fix_scale_;
    const unsigned int min_num_shared_lms_;
    svgpu_pose_graph_solver solver_ = SVGPU_PG_SOLVER_PCG;
};

}  // namespace hip
}  // namespace optimize
}  // namespace stella_vslam
#endif
