// Sim3 arithmetic of the pose-graph optimizer, as g2o's types/sim3/sim3.h states it: a unit quaternion, a translation and a scale, with
// product, inverse, map and Strasdat's closed-form exp / log.  fp64, no contraction (the library is built with -ffp-contract=off).  The
// same header compiles on the host (host/drop_in/graph_optimizer_hip.cc, the host test programs): SV_HD is empty there.
//
// The small-value branches are written from the closed form and its limits, at g2o's threshold 1e-5: exp() branches on |sigma| and on
// the rotation angle theta, log() on |sigma| and on d = cos(theta) > 1 - 1e-5.  g2o's own text was not at hand when this was written, so
// the thresholds are NOT pinned against it.  Every non-loop edge of a pose graph starts with an error of zero, and
// the numeric Jacobian perturbs by 1e-9: the small branches are the normal case.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SV_HD __host__ __device__ inline
#else
#define SV_HD inline
#endif

struct SvVec3 {
    double x, y, z;
};
struct SvMat3 {  // row-major
    double a00, a01, a02, a10, a11, a12, a20, a21, a22;
};
struct SvSim3 {
    double qx, qy, qz, qw;
    SvVec3 t;
    double s;
};
struct SvVec7 {  // omega (3), upsilon (3), sigma
    double w0, w1, w2, u0, u1, u2, sg;
};

#define SV_SIM3_EPS 0.00001

SV_HD SvVec3 sv3(double x, double y, double z) { return SvVec3{x, y, z}; }
SV_HD SvVec3 sv3_add(SvVec3 a, SvVec3 b) { return sv3(a.x + b.x, a.y + b.y, a.z + b.z); }
SV_HD SvVec3 sv3_scale(double k, SvVec3 a) { return sv3(k * a.x, k * a.y, k * a.z); }
SV_HD SvVec3 sv3_cross(SvVec3 a, SvVec3 b) { return sv3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
SV_HD SvVec3 sv_m3_mul(const SvMat3& M, SvVec3 v) {
    return sv3(M.a00 * v.x + M.a01 * v.y + M.a02 * v.z, M.a10 * v.x + M.a11 * v.y + M.a12 * v.z, M.a20 * v.x + M.a21 * v.y + M.a22 * v.z);
}

// Eigen's QuaternionBase::_transformVector: v + w * (2 q x v) + q x (2 q x v)
SV_HD SvVec3 sv_quat_rotate(double qx, double qy, double qz, double qw, SvVec3 v) {
    const SvVec3 q = sv3(qx, qy, qz);
    SvVec3 uv = sv3_cross(q, v);
    uv = sv3_add(uv, uv);
    return sv3_add(sv3_add(v, sv3_scale(qw, uv)), sv3_cross(q, uv));
}

// Eigen's QuaternionBase::toRotationMatrix
SV_HD SvMat3 sv_quat_to_rot(double qx, double qy, double qz, double qw) {
    const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw;
    const double txx = tx * qx, txy = ty * qx, txz = tz * qx;
    const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    SvMat3 R;
    R.a00 = 1.0 - (tyy + tzz), R.a01 = txy - twz, R.a02 = txz + twy;
    R.a10 = txy + twz, R.a11 = 1.0 - (txx + tzz), R.a12 = tyz - twx;
    R.a20 = txz - twy, R.a21 = tyz + twx, R.a22 = 1.0 - (txx + tyy);
    return R;
}

// Eigen's quaternion from a rotation matrix (trace branch, else the largest diagonal element)
SV_HD void sv_rot_to_quat(const SvMat3& R, double& qx, double& qy, double& qz, double& qw) {
    double t = R.a00 + R.a11 + R.a22;
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        qw = 0.5 * t;
        t = 0.5 / t;
        qx = (R.a21 - R.a12) * t, qy = (R.a02 - R.a20) * t, qz = (R.a10 - R.a01) * t;
    }
    else if (R.a00 >= R.a11 && R.a00 >= R.a22) {  // i = 0, j = 1, k = 2
        t = sqrt(R.a00 - R.a11 - R.a22 + 1.0);
        qx = 0.5 * t;
        t = 0.5 / t;
        qw = (R.a21 - R.a12) * t, qy = (R.a10 + R.a01) * t, qz = (R.a20 + R.a02) * t;
    }
    else if (R.a11 >= R.a22) {  // i = 1, j = 2, k = 0
        t = sqrt(R.a11 - R.a22 - R.a00 + 1.0);
        qy = 0.5 * t;
        t = 0.5 / t;
        qw = (R.a02 - R.a20) * t, qz = (R.a21 + R.a12) * t, qx = (R.a01 + R.a10) * t;
    }
    else {  // i = 2, j = 0, k = 1
        t = sqrt(R.a22 - R.a00 - R.a11 + 1.0);
        qz = 0.5 * t;
        t = 0.5 / t;
        qw = (R.a10 - R.a01) * t, qx = (R.a02 + R.a20) * t, qy = (R.a12 + R.a21) * t;
    }
}

// Sim3 operator*: r = r1 r2, t = s1 (r1 t2) + t1, s = s1 s2 (no renormalisation, as in g2o)
SV_HD SvSim3 sv_sim3_mul(const SvSim3& a, const SvSim3& b) {
    SvSim3 o;
    o.qw = a.qw * b.qw - a.qx * b.qx - a.qy * b.qy - a.qz * b.qz;
    o.qx = a.qw * b.qx + a.qx * b.qw + a.qy * b.qz - a.qz * b.qy;
    o.qy = a.qw * b.qy + a.qy * b.qw + a.qz * b.qx - a.qx * b.qz;
    o.qz = a.qw * b.qz + a.qz * b.qw + a.qx * b.qy - a.qy * b.qx;
    o.t = sv3_add(sv3_scale(a.s, sv_quat_rotate(a.qx, a.qy, a.qz, a.qw, b.t)), a.t);
    o.s = a.s * b.s;
    return o;
}

// Sim3::inverse: (r^*, r^* t * (-1 / s), 1 / s)
SV_HD SvSim3 sv_sim3_inv(const SvSim3& a) {
    SvSim3 o;
    o.qx = -a.qx, o.qy = -a.qy, o.qz = -a.qz, o.qw = a.qw;
    o.t = sv3_scale(-1.0 / a.s, sv_quat_rotate(o.qx, o.qy, o.qz, o.qw, a.t));
    o.s = 1.0 / a.s;
    return o;
}

// Sim3::map: s (r x) + t
SV_HD SvVec3 sv_sim3_map(const SvSim3& a, SvVec3 p) { return sv3_add(sv3_scale(a.s, sv_quat_rotate(a.qx, a.qy, a.qz, a.qw, p)), a.t); }

// the coefficients of W = A Omega + B Omega^2 + C I shared by exp and log; `small_rot` is the caller's small-angle decision
SV_HD void sv_sim3_abc(double sigma, double s, double theta, bool small_rot, double& A, double& B, double& C) {
    if (fabs(sigma) < SV_SIM3_EPS) {
        C = 1.0;
        if (small_rot) {
            A = 1.0 / 2.0;
            B = 1.0 / 6.0;
        }
        else {
            const double theta2 = theta * theta;
            A = (1.0 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    }
    else {
        C = (s - 1.0) / sigma;
        const double sigma2 = sigma * sigma;
        if (small_rot) {
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1.0) * s - 1.0) / (sigma2 * sigma);
        }
        else {
            const double a = s * sin(theta), b = s * cos(theta);
            const double theta2 = theta * theta;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / theta2;
        }
    }
}

// W = A skew(w) + B skew(w)^2 + C I
SV_HD SvMat3 sv_sim3_W(SvVec3 w, double A, double B, double C) {
    // skew(w)^2 = w w^T - |w|^2 I
    const double xx = w.x * w.x, yy = w.y * w.y, zz = w.z * w.z, xy = w.x * w.y, xz = w.x * w.z, yz = w.y * w.z;
    SvMat3 W;
    W.a00 = B * (-(yy + zz)) + C, W.a01 = A * (-w.z) + B * xy, W.a02 = A * w.y + B * xz;
    W.a10 = A * w.z + B * xy, W.a11 = B * (-(xx + zz)) + C, W.a12 = A * (-w.x) + B * yz;
    W.a20 = A * (-w.y) + B * xz, W.a21 = A * w.x + B * yz, W.a22 = B * (-(xx + yy)) + C;
    return W;
}

// Sim3(update): the exponential map
SV_HD SvSim3 sv_sim3_exp(const SvVec7& u) {
    const SvVec3 w = sv3(u.w0, u.w1, u.w2);
    const double sigma = u.sg;
    const double theta = sqrt(w.x * w.x + w.y * w.y + w.z * w.z);
    const double s = exp(sigma);
    const bool small_rot = theta < SV_SIM3_EPS;
    // R = I + k1 Omega + k2 Omega^2
    double k1, k2;
    if (small_rot) {
        k1 = 1.0;
        k2 = 0.5;
    }
    else {
        k1 = sin(theta) / theta;
        k2 = (1.0 - cos(theta)) / (theta * theta);
    }
    const SvMat3 R = sv_sim3_W(w, k1, k2, 1.0);
    double A, B, C;
    sv_sim3_abc(sigma, s, theta, small_rot, A, B, C);
    SvSim3 o;
    sv_rot_to_quat(R, o.qx, o.qy, o.qz, o.qw);
    o.t = sv_m3_mul(sv_sim3_W(w, A, B, C), sv3(u.u0, u.u1, u.u2));
    o.s = s;
    return o;
}

// W^-1 t by the adjugate (g2o takes W.lu().solve(t); W = C I + ... is far from singular wherever the optimizer goes)
SV_HD SvVec3 sv_m3_solve(const SvMat3& W, SvVec3 t) {
    const double c00 = W.a11 * W.a22 - W.a12 * W.a21, c01 = W.a12 * W.a20 - W.a10 * W.a22, c02 = W.a10 * W.a21 - W.a11 * W.a20;
    const double c10 = W.a02 * W.a21 - W.a01 * W.a22, c11 = W.a00 * W.a22 - W.a02 * W.a20, c12 = W.a01 * W.a20 - W.a00 * W.a21;
    const double c20 = W.a01 * W.a12 - W.a02 * W.a11, c21 = W.a02 * W.a10 - W.a00 * W.a12, c22 = W.a00 * W.a11 - W.a01 * W.a10;
    const double det = W.a00 * c00 + W.a01 * c01 + W.a02 * c02;
    const double inv = 1.0 / det;
    return sv3((c00 * t.x + c10 * t.y + c20 * t.z) * inv, (c01 * t.x + c11 * t.y + c21 * t.z) * inv, (c02 * t.x + c12 * t.y + c22 * t.z) * inv);
}

// Sim3::log
SV_HD SvVec7 sv_sim3_log(const SvSim3& a) {
    const double sigma = log(a.s);
    const SvMat3 R = sv_quat_to_rot(a.qx, a.qy, a.qz, a.qw);
    const double d = 0.5 * (R.a00 + R.a11 + R.a22 - 1.0);
    const SvVec3 dR = sv3(R.a21 - R.a12, R.a02 - R.a20, R.a10 - R.a01);  // deltaR
    const bool small_rot = d > 1.0 - SV_SIM3_EPS;
    double theta = 0.0;
    SvVec3 w;
    if (small_rot) w = sv3_scale(0.5, dR);
    else {
        theta = acos(d);
        w = sv3_scale(theta / (2.0 * sqrt(1.0 - d * d)), dR);
    }
    double A, B, C;
    sv_sim3_abc(sigma, a.s, theta, small_rot, A, B, C);
    const SvVec3 up = sv_m3_solve(sv_sim3_W(w, A, B, C), a.t);
    return SvVec7{w.x, w.y, w.z, up.x, up.y, up.z, sigma};
}

// the [R | t / s] pose graph_optimizer.cc:272-278 writes back: `const float s = corrected_Sim3_cw.scale()` rounds the scale to a float
SV_HD void sv_sim3_to_pose(const SvSim3& a, double* pose12) {
    const SvMat3 R = sv_quat_to_rot(a.qx, a.qy, a.qz, a.qw);
    const double s = (double)(float)a.s;
    pose12[0] = R.a00, pose12[1] = R.a01, pose12[2] = R.a02, pose12[3] = a.t.x / s;
    pose12[4] = R.a10, pose12[5] = R.a11, pose12[6] = R.a12, pose12[7] = a.t.y / s;
    pose12[8] = R.a20, pose12[9] = R.a21, pose12[10] = R.a22, pose12[11] = a.t.z / s;
}

// the update that moves one coordinate by v (g2o's numeric Jacobian perturbs one coordinate at a time)
SV_HD SvVec7 sv_sim3_unit_update(int coord, double v) {
    SvVec7 u;
    u.w0 = coord == 0 ? v : 0.0, u.w1 = coord == 1 ? v : 0.0, u.w2 = coord == 2 ? v : 0.0;
    u.u0 = coord == 3 ? v : 0.0, u.u1 = coord == 4 ? v : 0.0, u.u2 = coord == 5 ? v : 0.0;
    u.sg = coord == 6 ? v : 0.0;
    return u;
}

SV_HD SvSim3 sv_sim3_load(const double* p) { return SvSim3{p[0], p[1], p[2], p[3], SvVec3{p[4], p[5], p[6]}, p[7]}; }
SV_HD void sv_sim3_store(double* p, const SvSim3& a) {
    p[0] = a.qx, p[1] = a.qy, p[2] = a.qz, p[3] = a.qw, p[4] = a.t.x, p[5] = a.t.y, p[6] = a.t.z, p[7] = a.s;
}
