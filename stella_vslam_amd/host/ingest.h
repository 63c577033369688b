// Drop-in C++ adaptors for what system::create_*_frame does to an image before the extractor sees it (reference:
// src/stella_vslam/util/image_converter.cc:8-43, util/stereo_rectifier.cc:62-66), on top of the C ABI (include/svgpu.h, "image ingest").
//
//     util::convert_to_grayscale(img, color_order)       -> stella_vslam_hip::util::convert_to_grayscale(ctx, img, color_order)
//     util::convert_to_true_depth(img, depthmap_factor)  -> stella_vslam_hip::util::convert_to_true_depth(ctx, img, depthmap_factor)
//     util::stereo_rectifier::rectify(l, r, out_l, out_r)-> stella_vslam_hip::util::hip::stereo_rectifier::rectify (built from its four maps)
// The rectifier hands out GREY rectified images: it is fused with the conversion that follows it in the reference (remap per channel, then
// grey -- the reference's order and bits); convert_to_grayscale of a 1-channel image is the reference's no-op.
// A caller that tracks through tracked_frame_chain does not call these per frame at all: tracked_frame_chain::set_ingest() moves them into
// the tracked frame's own submission.
#pragma once
#include <stdexcept>

#ifdef SVGPU_WITH_OPENCV
#include <opencv2/core/mat.hpp>
#else
#include "standin/cv_standin.h"
#endif

#include "svgpu.h"

namespace stella_vslam_hip {
namespace util {

enum class color_order_t { Gray = 0, RGB = 1, BGR = 2 };  // camera/base.h:33-37

//! util::convert_to_grayscale: 8U images of 3 or 4 channels become CV_8UC1 in place; 1 channel passes through.
//! color_order_t::Gray with 3 or 4 channels throws (the reference would hand the colour image to the extractor).
void convert_to_grayscale(svgpu_ctx* ctx, cv::Mat& img, color_order_t in_color_order);
//! util::convert_to_true_depth: CV_16U / CV_32F, one channel -> CV_32F metres in place
void convert_to_true_depth(svgpu_ctx* ctx, cv::Mat& img, double depthmap_factor);

namespace hip {
class stereo_rectifier {
public:
    //! the four CV_32FC1 maps of the reference's class (undist_map_x_l_, undist_map_y_l_, undist_map_x_r_, undist_map_y_r_) and the cameras' raw format
    stereo_rectifier(svgpu_ctx* ctx, const cv::Mat& map_x_l, const cv::Mat& map_y_l, const cv::Mat& map_x_r, const cv::Mat& map_y_r, int channels,
                     color_order_t color_order);
    ~stereo_rectifier();
    stereo_rectifier(const stereo_rectifier&) = delete;
    stereo_rectifier& operator=(const stereo_rectifier&) = delete;
    //! util/stereo_rectifier.cc:62-66 (+ the grey conversion that follows it in system::feed_stereo_frame)
    void rectify(const cv::Mat& in_img_l, const cv::Mat& in_img_r, cv::Mat& out_img_l, cv::Mat& out_img_r) const;
    //! for tracked_frame_chain::set_ingest
    const svgpu_ingest* left() const { return left_; }
    const svgpu_ingest* right() const { return right_; }

private:
    svgpu_ctx* ctx_;
    svgpu_ingest *left_ = nullptr, *right_ = nullptr;
    int channels_;
};
}  // namespace hip

}  // namespace util
}  // namespace stella_vslam_hip
