#include "ingest.h"

#include <string>

namespace stella_vslam_hip {
namespace util {

namespace {
void check(svgpu_ctx* ctx, int rc, const char* where) {
    if (rc != SVGPU_OK) throw std::runtime_error(std::string(where) + ": " + svgpu_status_string(rc) + " (" + svgpu_last_error(ctx) + ")");
}
svgpu_ingest* make_ingest(svgpu_ctx* ctx, int cols, int rows, int channels, color_order_t order, const cv::Mat* mx, const cv::Mat* my) {
    svgpu_ingest* g = nullptr;
    if (mx && (mx->type() != CV_32F || my->type() != CV_32F || mx->rows != my->rows || mx->cols != my->cols || mx->step != my->step))
        throw std::runtime_error("stereo_rectifier: the maps must be CV_32FC1 of one size");
    check(ctx, svgpu_ingest_create(ctx, cols, rows, channels, (int)order, mx ? reinterpret_cast<const float*>(mx->ptr(0)) : nullptr,
                                   my ? reinterpret_cast<const float*>(my->ptr(0)) : nullptr, mx ? (int)mx->step : 0, &g),
          "svgpu_ingest_create");
    return g;
}
void run_gray(svgpu_ctx* ctx, const svgpu_ingest* g, const cv::Mat& in, cv::Mat& out) {
    cv::Mat dst(in.rows, in.cols, CV_8UC1);  // (a fresh matrix: `out` may be `in`)
    check(ctx, svgpu_ingest_gray(ctx, g, in.ptr(0), (int)in.step, dst.ptr(0), (int)dst.step), "svgpu_ingest_gray");
    out = dst;
}
}  // namespace

void convert_to_grayscale(svgpu_ctx* ctx, cv::Mat& img, const color_order_t in_color_order) {
    if (img.empty() || img.depth() != CV_8U) throw std::runtime_error("convert_to_grayscale: 8-bit images only");
    if (img.channels() == 1) return;  // image_converter.cc:9,24: neither branch
    svgpu_ingest* g = make_ingest(ctx, img.cols, img.rows, img.channels(), in_color_order, nullptr, nullptr);
    try {
        run_gray(ctx, g, img, img);
    } catch (...) {
        svgpu_ingest_destroy(g);
        throw;
    }
    svgpu_ingest_destroy(g);
}

void convert_to_true_depth(svgpu_ctx* ctx, cv::Mat& img, const double depthmap_factor) {
    if (img.empty() || img.channels() != 1 || (img.depth() != CV_16U && img.depth() != CV_32F)) throw std::runtime_error("convert_to_true_depth: CV_16UC1 or CV_32FC1");
    cv::Mat dst(img.rows, img.cols, CV_32F);
    check(ctx, svgpu_ingest_depth(ctx, img.ptr(0), img.depth() == CV_16U ? SVGPU_DEPTH_U16 : SVGPU_DEPTH_F32, (int)img.step, img.cols, img.rows, depthmap_factor,
                                  reinterpret_cast<float*>(dst.ptr(0)), (int)dst.step),
          "svgpu_ingest_depth");
    img = dst;
}

namespace hip {

stereo_rectifier::stereo_rectifier(svgpu_ctx* ctx, const cv::Mat& map_x_l, const cv::Mat& map_y_l, const cv::Mat& map_x_r, const cv::Mat& map_y_r, int channels,
                                   color_order_t color_order)
    : ctx_(ctx), channels_(channels) {
    left_ = make_ingest(ctx, map_x_l.cols, map_x_l.rows, channels, color_order, &map_x_l, &map_y_l);
    try {
        right_ = make_ingest(ctx, map_x_r.cols, map_x_r.rows, channels, color_order, &map_x_r, &map_y_r);
    } catch (...) {
        svgpu_ingest_destroy(left_);
        throw;
    }
}

stereo_rectifier::~stereo_rectifier() {
    svgpu_ingest_destroy(left_);
    svgpu_ingest_destroy(right_);
}

void stereo_rectifier::rectify(const cv::Mat& in_img_l, const cv::Mat& in_img_r, cv::Mat& out_img_l, cv::Mat& out_img_r) const {
    for (const cv::Mat* m : {&in_img_l, &in_img_r})
        if (m->empty() || m->depth() != CV_8U || m->channels() != channels_) throw std::runtime_error("stereo_rectifier::rectify: not the rectifier's image format");
    run_gray(ctx_, left_, in_img_l, out_img_l);
    run_gray(ctx_, right_, in_img_r, out_img_r);
}

}  // namespace hip
}  // namespace util
}  // namespace stella_vslam_hip
