// Observation staging of bundle adjustment (local_ba_impl in svgpu_ba.hip): everything the host does to bring the caller's observations
// into the page-locked image of ba_layout.h -- the scan of the index arrays, the landmark offsets, the stable sort of observations that do
// not arrive grouped by landmark, and, at global-BA sizes, the team of host threads that stages the measurements beside the device's
// structure work and uploads them.  Plain C++17 with no HIP include and no read of the environment: the device copy is a callable of the
// caller's.  tests/ba_stage_check.cpp runs this header alone against a single-thread restatement, also under the thread sanitizer.
#pragma once
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "ba_layout.h"  // BaIn, Piece
#include "ba_plan.h"    // svgpu.h: svgpu_ba_problem

#define BA_STAGE_MAX_THREADS 16  // ba_plan_host_threads never asks for more
#define BA_STAGE_ERR_RANGE 1     // an upload past the end of its device piece (hipErrorInvalidValue: svgpu_ba.hip asserts they agree)

// how the workers cut their shares
struct BaStageTuning {
    size_t obs_chunk;     // observations staged between two looks at `go`
    size_t lm_chunk;      // landmark positions likewise
    size_t chunked_from;  // observations from which every worker uploads its own chunks as they are staged
};
// 2.6 MB of measurements and 6 MB of positions per chunk.  Every device copy holds the runtime's lock for ~15 us, and the caller's launches
// queue behind it: below 4 M observations the worker that finishes LAST uploads the whole image in four copies
constexpr BaStageTuning BA_STAGE_TUNING{(size_t)128 << 10, (size_t)256 << 10, (size_t)4 << 20};

// the CPUs this process may run on: the affinity mask, which is what a container's cpuset leaves, not the machine's core count (0: not known)
inline unsigned ba_stage_usable_cpus() {
    unsigned hw = std::thread::hardware_concurrency();
    cpu_set_t cpus;
    if (sched_getaffinity(0, sizeof(cpus), &cpus) == 0 && CPU_COUNT(&cpus) > 0) hw = hw == 0 ? (unsigned)CPU_COUNT(&cpus) : std::min(hw, (unsigned)CPU_COUNT(&cpus));
    return hw;
}

struct BaStageResult {
    bool no_threads = false;         // the system refused a thread of the team: nothing was scanned
    bool bad_index = false;          // an observation names a pose or a landmark out of range: nothing else below is valid
    bool lm_major = true;            // the observations arrived grouped by landmark (the order local_bundle_adjuster_g2o.cc:168-227 and
                                     // global_bundle_adjuster.cc:66-118 create their edges in)
    std::vector<int> perm;           // else: sorted position -> caller's observation index (empty = identity)
    std::vector<uint8_t> pose_seen;  // a pose with an observation (the pose half of the first stage's activity pass)
};

// measurements [a, b) of the caller's order into the image
inline void ba_stage_measurements(const svgpu_ba_problem& pr, const BaIn& h, size_t a, size_t b) {
    memcpy(h.e_uvr + 3 * a, pr.obs_uvr + 3 * a, 12 * (b - a));
    memcpy(h.e_w + a, pr.obs_inv_sigma_sq + a, 4 * (b - a));
    if (pr.obs_huber_delta) memcpy(h.e_hub + a, pr.obs_huber_delta + a, 4 * (b - a));
    else memset(h.e_hub + a, 0, 4 * (b - a));
}

// observations that do not arrive grouped by landmark: offsets by counting, a stable order, all five arrays written through it
inline void ba_stage_sorted(const svgpu_ba_problem& pr, const BaIn& h, std::vector<int>& perm) {
    const int L = pr.num_points, E = pr.num_obs;
    int* const lm_off = h.lm_off;
    for (int l = 0; l <= L; ++l) lm_off[l] = 0;
    for (int e = 0; e < E; ++e) lm_off[pr.obs_point[e] + 1]++;
    for (int l = 0; l < L; ++l) lm_off[l + 1] += lm_off[l];
    perm.resize(E);
    std::vector<int> fill(lm_off, lm_off + L);
    for (int e = 0; e < E; ++e) perm[fill[pr.obs_point[e]]++] = e;
    for (int k = 0; k < E; ++k) {
        const int e = perm[k];
        h.e_pose[k] = pr.obs_pose[e];
        h.e_point[k] = pr.obs_point[e];
        h.e_uvr[3 * k] = pr.obs_uvr[3 * e];
        h.e_uvr[3 * k + 1] = pr.obs_uvr[3 * e + 1];
        h.e_uvr[3 * k + 2] = pr.obs_uvr[3 * e + 2];
        h.e_w[k] = pr.obs_inv_sigma_sq[e];
        h.e_hub[k] = pr.obs_huber_delta ? pr.obs_huber_delta[e] : 0.f;
    }
}

// The host team of one call: nth threads (the caller's included) scan the observation indices -- range check, "already grouped by
// landmark?" and, valid in that case, the landmark offsets -- and stage the two index arrays; the nth - 1 workers then go on staging the
// measurements, the landmark positions and the caller's points_out (which starts as its input) while the caller runs the device's
// structure work, and upload what they staged once the caller says where to (release).  One spawn per call; the phases of the scan are
// separated by spin barriers (a few microseconds each).  With nth == 1 there are no workers: scan() stages everything itself, except
// points_out.
// Upload: `int begin()`, once on every worker (the device is a per-thread setting), and `int operator()(Piece<T> dev, Piece<T> host,
// size_t first, size_t count)`: elements [first, first + count) of a staged piece to the same elements of its device piece; 0 or an error
// code, of which join() returns the first.
template <class Upload>
class BaStageTeam {
public:
    BaStageTeam(const svgpu_ba_problem& problem, const BaIn& host_image, double* points_out_, int threads, const BaStageTuning& tuning, Upload upload)
        : pr(problem), hin(host_image), points_out(points_out_), nth(std::max(1, std::min(threads, BA_STAGE_MAX_THREADS))), tune(tuning), up(upload), P(problem.num_poses),
          L(problem.num_points), E(problem.num_obs) {}
    BaStageTeam(const BaStageTeam&) = delete;
    BaStageTeam& operator=(const BaStageTeam&) = delete;
    ~BaStageTeam() {
        abandon();
        join();
    }

    // Starts the workers and scans.  Returns behind the last barrier, the whole scan done, and with the team running only if the
    // observations are valid and grouped by landmark: otherwise it is abandoned and joined, and the caller's thread has staged whatever
    // the image needs.
    BaStageResult scan() {
        BaStageResult R;
        if (nth > 1) {
            // (the workers wait at a gate until the whole team exists: a thread the system refuses to create must not leave the others at a
            //  barrier that counts nth arrivals)
            bool spawned = true;
            try {
                th.reserve(nth - 1);
                for (int q = 1; q < nth; ++q)
                    th.emplace_back([this, q] {
                        for (int spins = 0; gate.load() == 0; ++spins)
                            if (spins > 2000) std::this_thread::yield();
                        if (gate.load() != 1) return;
                        scan_share(q);
                        stage_share(q);
                    });
            } catch (...) {
                spawned = false;
            }
            gate.store(spawned ? 1 : 2);
            if (!spawned) {
                join();
                R.no_threads = true;
                return R;
            }
            is_running = true;
        }
        scan_share(0);
        int any_unsorted = 0;
        for (int q = 0; q < nth; ++q) R.bad_index |= bad[q] != 0, any_unsorted |= unsorted[q];
        R.lm_major = !any_unsorted;
        if (R.bad_index || !R.lm_major) {  // (unsorted is rare at this size: the permuted copy writes the whole staging image itself)
            abandon();
            join();
        }
        if (R.bad_index) return R;
        R.pose_seen = std::move(seen[0]);
        for (int q = 1; q < nth; ++q)
            for (int p = 0; p < P; ++p) R.pose_seen[p] |= seen[q][p];
        if (!is_running) memcpy(hin.points, pr.points, hin.points.bytes());
        if (!R.lm_major) ba_stage_sorted(pr, hin, R.perm);
        return R;
    }
    bool running() const { return is_running; }  // workers were started and have not been joined
    // the device arena is known: the workers upload what they staged to these pieces
    void release(const BaIn& device_image) {
        din = device_image;
        int z = 0;
        go.compare_exchange_strong(z, 1);
    }
    // the caller returns early or stages the observations itself: the workers upload nothing (no effect once released)
    void abandon() {
        int z = 0;
        go.compare_exchange_strong(z, 2);
    }
    // waits for the workers; the first error of their uploads, or 0
    int join() {
        for (auto& t : th)
            if (t.joinable()) t.join();
        th.clear();
        is_running = false;
        for (int q = 0; q < nth; ++q)
            if (err[q]) return err[q];
        return 0;
    }

private:
    void barrier(int k) {  // the k-th barrier of the call (k = 1, 2, ...): every thread of the team arrives once
        arrived.fetch_add(1);
        for (int spins = 0; arrived.load() < k * nth; ++spins)
            if (spins > 4000) std::this_thread::yield();
    }
    // Phase 1 of thread q: straight-line passes over its range (flag reductions the compiler vectorises), the landmark offsets as "end of
    // landmark l = index behind its last observation", stored where a landmark's run ends and closed over the empty landmarks by a running
    // maximum (shares of the offsets array, seeded by a backward look at the shares before)
    void scan_share(int q) {
        const int32_t* const op = pr.obs_pose;
        const int32_t* const ol = pr.obs_point;
        int* const lm_off = hin.lm_off;
        const size_t e0 = (size_t)E * q / nth, end = (size_t)E * (q + 1) / nth;
        const size_t k0 = ((size_t)L + 1) * q / nth, k1 = ((size_t)L + 1) * (q + 1) / nth;
        unsigned bd = 0, un = 0;
        for (size_t e = e0; e < end; ++e) bd |= (unsigned)((unsigned)op[e] >= (unsigned)P) | (unsigned)((unsigned)ol[e] >= (unsigned)L);
        for (size_t e = std::max<size_t>(e0, 1); e < end; ++e) un |= (unsigned)(ol[e] < ol[e - 1]);
        bad[q] = bd != 0, unsorted[q] = un != 0;
        if (!bd) {
            seen[q].assign(P, 0);
            uint8_t* const sn = seen[q].data();
            for (size_t e = e0; e < end; ++e) sn[op[e]] = 1;
            memcpy(hin.e_pose + e0, op + e0, 4 * (end - e0));
            memcpy(hin.e_point + e0, ol + e0, 4 * (end - e0));
            if (nth == 1) ba_stage_measurements(pr, hin, e0, end);  // (a team's follow in its second phase)
        }
        for (size_t k = k0; k < k1; ++k) lm_off[k] = 0;
        if (nth > 1) barrier(1);
        int any_bad = 0, any_un = 0;
        for (int t = 0; t < nth; ++t) any_bad |= bad[t], any_un |= unsorted[t];
        const bool ok = !any_bad && !any_un;
        if (ok && nth == 1)  // (one thread: stored unconditionally, the last observation of a landmark wins -- no branch to mispredict)
            for (size_t e = e0; e < end; ++e) lm_off[ol[e] + 1] = (int)(e + 1);
        else if (ok)
            for (size_t e = e0; e < end; ++e) {
                const int l = ol[e], nxt = e + 1 < (size_t)E ? ol[e + 1] : -1;
                if (nxt != l) lm_off[l + 1] = (int)(e + 1);
            }
        if (nth > 1) barrier(2);
        int v = 0;
        if (ok)
            for (size_t k = k0; k-- > 0;)
                if (lm_off[k]) {
                    v = lm_off[k];
                    break;
                }
        if (nth > 1) barrier(3);
        if (ok)
            for (size_t k = k0; k < k1; ++k) {
                v = std::max(v, lm_off[k]);
                lm_off[k] = v;
            }
        if (nth > 1) barrier(4);
    }
    // Phase 2 of worker q (1 .. nth - 1): its share of the measurements and of the landmark positions into the staging image, chunk by
    // chunk; a staged chunk is uploaded as soon as `go` says where to
    void stage_share(int q) {
        const int W = nth - 1, w = q - 1;
        const size_t e0 = (size_t)E * w / W, e1 = (size_t)E * (w + 1) / W, l0 = (size_t)L * w / W, l1 = (size_t)L * (w + 1) / W;
        memcpy(points_out + 3 * l0, pr.points + 3 * l0, 24 * (l1 - l0));  // (the caller's output starts as its input)
        int he = up.begin();
        size_t e_up = e0, l_up = l0;  // uploaded so far
        const bool chunked = (size_t)E >= tune.chunked_from;
        auto upload = [&](auto dev, auto host, size_t first, size_t count) {  // (dev: placed before `go` said 1)
            if (first + count > dev.n) he = BA_STAGE_ERR_RANGE;
            if (count && he == 0) he = up(dev, host, first, count);
        };
        auto flush = [&](size_t e_staged, size_t l_staged) {
            if (!chunked || go.load() != 1 || he != 0) return;
            if (e_staged > e_up) {
                upload(din.e_uvr, hin.e_uvr, 3 * e_up, 3 * (e_staged - e_up));
                upload(din.e_w, hin.e_w, e_up, e_staged - e_up);
                upload(din.e_hub, hin.e_hub, e_up, e_staged - e_up);
                e_up = e_staged;
            }
            if (l_staged > l_up) {
                upload(din.points, hin.points, 3 * l_up, 3 * (l_staged - l_up));
                l_up = l_staged;
            }
        };
        for (size_t a = e0; a < e1 && go.load() != 2; a += tune.obs_chunk) {
            const size_t b = std::min(e1, a + tune.obs_chunk);
            ba_stage_measurements(pr, hin, a, b);
            flush(b, l0);
        }
        for (size_t a = l0; a < l1 && go.load() != 2; a += tune.lm_chunk) {
            const size_t b = std::min(l1, a + tune.lm_chunk);
            memcpy(hin.points + 3 * a, pr.points + 3 * a, 24 * (b - a));
            flush(e1, b);
        }
        const bool last = staged.fetch_add(1) + 1 == W;
        for (int spins = 0; go.load() == 0; ++spins)
            if (spins > 2000) std::this_thread::yield();
        if (go.load() == 1) {
            if (chunked) flush(e1, l1);
            else if (last) {  // (every share is staged: fetch_add orders the others' writes before this thread's reads)
                upload(din.e_uvr, hin.e_uvr, 0, din.e_uvr.n), upload(din.e_w, hin.e_w, 0, din.e_w.n), upload(din.e_hub, hin.e_hub, 0, din.e_hub.n);
                upload(din.points, hin.points, 0, din.points.n);
            }
        }
        err[q] = he;
    }

    const svgpu_ba_problem& pr;
    const BaIn hin;  // placed over the host image
    BaIn din;        // placed over the device arena: written by release() before `go` says 1
    double* const points_out;
    const int nth;
    const BaStageTuning tune;
    Upload up;
    const int P, L, E;
    std::vector<std::thread> th;
    std::atomic<int> arrived{0};
    std::atomic<int> gate{0};    // 0: the team is being created, 1: run, 2: creation failed, leave
    std::atomic<int> staged{0};  // workers whose share of the measurements is in the staging image
    std::atomic<int> go{0};      // 0: the arena is not known yet, 1: upload, 2: abandoned
    int err[BA_STAGE_MAX_THREADS] = {0}, bad[BA_STAGE_MAX_THREADS] = {0}, unsorted[BA_STAGE_MAX_THREADS] = {0};
    std::vector<uint8_t> seen[BA_STAGE_MAX_THREADS];  // per thread: the poses its share observes
    bool is_running = false;
};
