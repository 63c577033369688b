// util::convert_to_grayscale / convert_to_true_depth / util::hip::stereo_rectifier on stand-in matrices against the arithmetic written out
// here (OpenCV's 8-bit fixed point as tests/ingest_problems.py states it): every byte equal.
#include <cmath>
#include <cstdio>
#include <vector>

#include "ingest.h"

using namespace stella_vslam_hip;

namespace {
unsigned long long g_state = 88172645463325252ull;
unsigned rnd() {  // xorshift64
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return (unsigned)(g_state >> 33);
}
int g_fail = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                           \
        }                                                       \
    } while (0)

int grey_of(int r, int g, int b) { return (r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15; }

// remap per channel, then grey
std::vector<uint8_t> expect(const cv::Mat& img, bool bgr, const cv::Mat* mx, const cv::Mat* my) {
    const int w = img.cols, h = img.rows, ch = img.channels();
    std::vector<uint8_t> out((size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int c[4] = {0, 0, 0, 0};
            if (!mx) {
                for (int k = 0; k < ch; ++k) c[k] = img.ptr(y)[x * ch + k];
            } else {
                const float vx = std::nearbyint(reinterpret_cast<const float*>(mx->ptr(y))[x] * 32.0f), vy = std::nearbyint(reinterpret_cast<const float*>(my->ptr(y))[x] * 32.0f);
                if (std::fabs(vx) < 1073741824.0f && std::fabs(vy) < 1073741824.0f) {
                    const int sx = (int)vx, sy = (int)vy, ix = sx >> 5, iy = sy >> 5, fx = sx & 31, fy = sy & 31;
                    const int wt[4] = {(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32};
                    for (int k = 0; k < ch; ++k) {
                        long long acc = 0;
                        for (int t = 0; t < 4; ++t) {
                            const int xx = ix + (t & 1), yy = iy + (t >> 1);
                            if (xx >= 0 && xx < w && yy >= 0 && yy < h) acc += (long long)wt[t] * img.ptr(yy)[xx * ch + k];
                        }
                        c[k] = (int)((acc + (1 << 14)) >> 15);
                    }
                }
            }
            out[(size_t)y * w + x] = (uint8_t)(ch == 1 ? c[0] : bgr ? grey_of(c[2], c[1], c[0]) : grey_of(c[0], c[1], c[2]));
        }
    return out;
}

bool same(const cv::Mat& m, const std::vector<uint8_t>& e) {
    if (m.type() != CV_8UC1 || (size_t)m.rows * m.cols != e.size()) return false;
    for (int y = 0; y < m.rows; ++y)
        for (int x = 0; x < m.cols; ++x)
            if (m.ptr(y)[x] != e[(size_t)y * m.cols + x]) return false;
    return true;
}

cv::Mat noise(int w, int h, int type) {
    cv::Mat m(h, w, type);
    for (size_t i = 0; i < (size_t)h * m.step; ++i) m.data[i] = (uint8_t)rnd();
    return m;
}
}  // namespace

int main() {
    svgpu_ctx* ctx = nullptr;
    if (svgpu_create(0, &ctx) != SVGPU_OK) {
        std::printf("no device\n");
        return 2;
    }
    const int w = 203, h = 157;
    // convert_to_grayscale
    for (int type : {CV_8UC3, CV_8UC4})
        for (util::color_order_t order : {util::color_order_t::RGB, util::color_order_t::BGR}) {
            cv::Mat img = noise(w, h, type);
            const auto e = expect(img, order == util::color_order_t::BGR, nullptr, nullptr);
            util::convert_to_grayscale(ctx, img, order);
            CHECK(same(img, e));
        }
    {
        cv::Mat g = noise(w, h, CV_8UC1);
        const uint8_t* before = g.data;
        util::convert_to_grayscale(ctx, g, util::color_order_t::Gray);
        CHECK(g.data == before && g.type() == CV_8UC1);
        cv::Mat c3 = noise(w, h, CV_8UC3);
        bool threw = false;
        try {
            util::convert_to_grayscale(ctx, c3, util::color_order_t::Gray);
        } catch (const std::runtime_error&) {
            threw = true;
        }
        CHECK(threw && c3.type() == CV_8UC3);
    }
    // convert_to_true_depth
    {
        cv::Mat d(h, w, CV_16U);
        uint16_t* p = reinterpret_cast<uint16_t*>(d.data);
        for (int i = 0; i < w * h; ++i) p[i] = (uint16_t)rnd();
        p[0] = 0, p[1] = 65535, p[2] = 5000;
        std::vector<uint16_t> keep(p, p + w * h);
        util::convert_to_true_depth(ctx, d, 5000.0);
        CHECK(d.type() == CV_32F && d.cols == w && d.rows == h);
        const float s = (float)(1.0 / 5000.0), *f = reinterpret_cast<const float*>(d.data);
        bool ok = true;
        for (int i = 0; i < w * h; ++i) ok = ok && f[i] == (float)keep[i] * s;
        CHECK(ok && f[2] == 1.0f && f[0] == 0.0f);
        util::convert_to_true_depth(ctx, d, 2.0);
        CHECK(reinterpret_cast<const float*>(d.data)[2] == 0.5f);
    }
    // stereo_rectifier: two different map pairs (a shear and a shift, some entries outside, one non-finite)
    {
        cv::Mat mxl(h, w, CV_32F), myl(h, w, CV_32F), mxr(h, w, CV_32F), myr(h, w, CV_32F);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                reinterpret_cast<float*>(mxl.ptr(y))[x] = (float)(x + 0.013 * y - 1.3);
                reinterpret_cast<float*>(myl.ptr(y))[x] = (float)(y - 0.009 * x + 0.7);
                reinterpret_cast<float*>(mxr.ptr(y))[x] = (float)(x * 1.01 + 2.515625);
                reinterpret_cast<float*>(myr.ptr(y))[x] = (float)(y * 0.99 - 0.5);
            }
        reinterpret_cast<float*>(mxr.ptr(3))[5] = NAN;
        reinterpret_cast<float*>(myl.ptr(4))[6] = 1e9f;
        util::hip::stereo_rectifier rect(ctx, mxl, myl, mxr, myr, 3, util::color_order_t::BGR);
        cv::Mat l = noise(w, h, CV_8UC3), r = noise(w, h, CV_8UC3), ol, orr;
        rect.rectify(l, r, ol, orr);
        CHECK(same(ol, expect(l, true, &mxl, &myl)));
        CHECK(same(orr, expect(r, true, &mxr, &myr)));
        CHECK(orr.ptr(3)[5] == 0 && ol.ptr(4)[6] == 0);
        CHECK(rect.left() && rect.right() && rect.left() != rect.right());
    }
    svgpu_destroy(ctx);
    if (g_fail) return 1;
    std::printf("ingest ok\n");
    return 0;
}
