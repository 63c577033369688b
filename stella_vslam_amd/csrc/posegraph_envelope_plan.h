// Host planner of the pose graph's direct solver (posegraph_envelope.hip): the block envelope ("skyline") of the damped system
// (H + lambda I) over the free vertices, 7x7 blocks.  Plain C++ (no HIP): tests/posegraph_envelope_check.cpp compiles this header alone.
//
// Input: nfree and, per edge, the free slots of its two ends (-1: the end is fixed -- such an edge touches a diagonal block only).
//   pairs      the distinct unordered free-free pairs (lo < hi slot) in ascending (lo, hi) order, each with a CSR list of its edges in
//              ascending edge order.  Edge (i, j) contributes Ji^T Jj to block (slot i, slot j): the entry's flag says that the edge
//              runs hi -> lo, i.e. that it contributes the TRANSPOSE to the pair's block (rows lo, columns hi).  Duplicate edges and edges
//              given in both orientations land in the same block.
//   ordering   three elimination orders are tried -- natural, interleaved from both ends (0, last, 1, last - 1, ...) and reverse
//              Cuthill-McKee -- and the smallest lower envelope in blocks wins; ties go to the earlier one.  Deterministic.
//   envelope   in the chosen order: first[row] = first column position of the row's envelope, rowoff = row offsets in blocks (block (i, k)
//              = rowoff[i] + k - first[i], the diagonal block last), and the same envelope by columns for the right-looking kernel:
//              coloff / colrows (rows i > j with first[i] <= j, ascending) / colbase (rowoff[i] - first[i]).  The update of column j
//              touches blocks (ip, iq) with first[ip] <= j < iq only, which lie in row ip's envelope: fill never leaves the envelope and
//              the one-workgroup kernel needs no monotone first[] (a window-in-LDS kernel would; `monotone` says whether it holds).
//   blk_src    per envelope block what the assembly writes: -1 zero, p < nfree the diagonal of position p, nfree + k pair k
//   pair_blk / pair_flag   per pair its envelope block and whether the block (rows lo, columns hi) is stored transposed
// pg_env_host_factor / pg_env_host_solve: plain fp64 elimination on a plan's value array, for the CPU check only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

enum { PG_ENV_ORDER_NATURAL = 0, PG_ENV_ORDER_INTERLEAVED = 1, PG_ENV_ORDER_RCM = 2 };

struct PgEnvPlan {
    int nfree = 0, num_pairs = 0, ordering = 0, max_column_rows = 0, monotone = 1;
    bool fits = true;      // false: the value count 49 * nblocks is beyond 32-bit indexing (only nblocks is set then)
    int64_t nblocks = 0;   // blocks of the lower envelope, diagonal included
    std::vector<int32_t> order, pos;                         // position -> slot, slot -> position
    std::vector<int32_t> first, rowoff;                      // nfree, nfree + 1
    std::vector<int32_t> coloff, colrows, colbase;           // nfree + 1, nblocks - nfree each
    std::vector<int32_t> blk_src;                            // nblocks
    std::vector<int32_t> pair_a, pair_b, pair_off, pair_ent; // lo, hi slot; CSR of edge << 1 | transposed
    std::vector<int32_t> pair_blk, pair_flag;
};

namespace pg_env_detail {

// blocks of the lower envelope of the pair graph under `order`
inline int64_t envelope_blocks(int n, const std::vector<int32_t>& order, const std::vector<int32_t>& pa, const std::vector<int32_t>& pb,
                               std::vector<int32_t>& pos, std::vector<int32_t>& first) {
    pos.assign((size_t)n, 0);
    first.resize((size_t)n);
    for (int p = 0; p < n; ++p) pos[(size_t)order[(size_t)p]] = p, first[(size_t)p] = p;
    for (size_t k = 0; k < pa.size(); ++k) {
        const int a = pos[(size_t)pa[k]], b = pos[(size_t)pb[k]];
        const int lo = std::min(a, b), hi = std::max(a, b);
        first[(size_t)hi] = std::min(first[(size_t)hi], lo);
    }
    int64_t total = 0;
    for (int p = 0; p < n; ++p) total += p - first[(size_t)p] + 1;
    return total;
}

// reverse Cuthill-McKee: every component starts at its vertex of lowest degree (lowest slot on a tie), neighbours are visited in
// ascending (degree, slot) order, the whole sequence is reversed
inline std::vector<int32_t> rcm(int n, const std::vector<int32_t>& pa, const std::vector<int32_t>& pb) {
    std::vector<int32_t> off((size_t)n + 1, 0), adj(2 * pa.size());
    for (size_t k = 0; k < pa.size(); ++k) ++off[(size_t)pa[k] + 1], ++off[(size_t)pb[k] + 1];
    for (int v = 0; v < n; ++v) off[(size_t)v + 1] += off[(size_t)v];
    std::vector<int32_t> fill(off.begin(), off.end() - 1);
    for (size_t k = 0; k < pa.size(); ++k) {
        adj[(size_t)fill[(size_t)pa[k]]++] = pb[k];
        adj[(size_t)fill[(size_t)pb[k]]++] = pa[k];
    }
    const auto deg = [&](int v) { return off[(size_t)v + 1] - off[(size_t)v]; };
    const auto less = [&](int a, int b) { return deg(a) != deg(b) ? deg(a) < deg(b) : a < b; };
    for (int v = 0; v < n; ++v) std::sort(adj.begin() + off[(size_t)v], adj.begin() + off[(size_t)v + 1], less);
    std::vector<int32_t> starts((size_t)n), out;
    for (int v = 0; v < n; ++v) starts[(size_t)v] = v;
    std::sort(starts.begin(), starts.end(), less);
    std::vector<char> seen((size_t)n, 0);
    out.reserve((size_t)n);
    for (int s : starts) {
        if (seen[(size_t)s]) continue;
        seen[(size_t)s] = 1;
        size_t head = out.size();
        out.push_back(s);
        while (head < out.size()) {
            const int v = out[head++];
            for (int k = off[(size_t)v]; k < off[(size_t)v + 1]; ++k) {
                const int w = adj[(size_t)k];
                if (!seen[(size_t)w]) seen[(size_t)w] = 1, out.push_back(w);
            }
        }
    }
    std::reverse(out.begin(), out.end());
    return out;
}

}  // namespace pg_env_detail

// sa / sb: per edge the free slot of vertex 0 / vertex 1 of the edge, or -1
inline void pg_env_plan(int nfree, int num_edges, const int32_t* sa, const int32_t* sb, PgEnvPlan& P) {
    using namespace pg_env_detail;
    P = PgEnvPlan{};
    P.nfree = nfree;
    const size_t n = (size_t)nfree;
    // ---- pairs
    struct Ent {
        int32_t lo, hi, e;
    };
    std::vector<Ent> ents;
    for (int e = 0; e < num_edges; ++e) {
        const int a = sa[e], b = sb[e];
        if (a < 0 || b < 0 || a == b) continue;
        ents.push_back({std::min(a, b), std::max(a, b), e});
    }
    std::stable_sort(ents.begin(), ents.end(), [](const Ent& x, const Ent& y) { return x.lo != y.lo ? x.lo < y.lo : x.hi < y.hi; });
    P.pair_off.push_back(0);
    for (size_t k = 0; k < ents.size(); ++k) {
        if (k == 0 || ents[k].lo != ents[k - 1].lo || ents[k].hi != ents[k - 1].hi) {
            if (k) P.pair_off.push_back((int32_t)k);
            P.pair_a.push_back(ents[k].lo);
            P.pair_b.push_back(ents[k].hi);
        }
        P.pair_ent.push_back(ents[k].e << 1 | (sa[ents[k].e] == ents[k].hi ? 1 : 0));
    }
    if (!ents.empty()) P.pair_off.push_back((int32_t)ents.size());
    P.num_pairs = (int)P.pair_a.size();
    // ---- ordering
    std::vector<int32_t> cand[3], pos, first;
    cand[0].resize(n), cand[1].resize(n);
    for (int p = 0; p < nfree; ++p) {
        cand[0][(size_t)p] = p;
        cand[1][(size_t)p] = (p & 1) ? nfree - 1 - p / 2 : p / 2;
    }
    cand[2] = rcm(nfree, P.pair_a, P.pair_b);
    int64_t best = -1;
    for (int o = 0; o < 3; ++o) {
        const int64_t size = envelope_blocks(nfree, cand[o], P.pair_a, P.pair_b, pos, first);
        if (best < 0 || size < best) best = size, P.ordering = o;
    }
    P.order = cand[P.ordering];
    P.nblocks = envelope_blocks(nfree, P.order, P.pair_a, P.pair_b, P.pos, P.first);
    if (P.nblocks * 49 > (int64_t)INT32_MAX) {
        P.fits = false;
        return;
    }
    // ---- the envelope by rows and by columns
    P.rowoff.assign(n + 1, 0);
    P.coloff.assign(n + 1, 0);
    for (int i = 0; i < nfree; ++i) {
        P.rowoff[(size_t)i + 1] = P.rowoff[(size_t)i] + (i - P.first[(size_t)i] + 1);
        for (int j = P.first[(size_t)i]; j < i; ++j) ++P.coloff[(size_t)j + 1];
        if (i > 0 && P.first[(size_t)i] < P.first[(size_t)i - 1]) P.monotone = 0;
    }
    for (int j = 0; j < nfree; ++j) {
        P.max_column_rows = std::max(P.max_column_rows, (int)P.coloff[(size_t)j + 1]);
        P.coloff[(size_t)j + 1] += P.coloff[(size_t)j];
    }
    P.colrows.resize((size_t)P.coloff[n]);
    P.colbase.resize((size_t)P.coloff[n]);
    std::vector<int32_t> fill(P.coloff.begin(), P.coloff.end() - 1);
    for (int i = 0; i < nfree; ++i)  // ascending i: every column's rows come out ascending
        for (int j = P.first[(size_t)i]; j < i; ++j) {
            P.colrows[(size_t)fill[(size_t)j]] = i;
            P.colbase[(size_t)fill[(size_t)j]++] = P.rowoff[(size_t)i] - P.first[(size_t)i];
        }
    // ---- what the assembly writes
    P.blk_src.assign((size_t)P.nblocks, -1);
    for (int i = 0; i < nfree; ++i) P.blk_src[(size_t)P.rowoff[(size_t)i + 1] - 1] = i;
    P.pair_blk.resize((size_t)P.num_pairs);
    P.pair_flag.resize((size_t)P.num_pairs);
    for (int k = 0; k < P.num_pairs; ++k) {
        const int plo = P.pos[(size_t)P.pair_a[(size_t)k]], phi = P.pos[(size_t)P.pair_b[(size_t)k]];
        const int row = std::max(plo, phi), col = std::min(plo, phi);
        const int blk = P.rowoff[(size_t)row] + col - P.first[(size_t)row];
        P.pair_blk[(size_t)k] = blk;
        P.pair_flag[(size_t)k] = plo > phi ? 0 : 1;  // stored block = rows of the later position: (lo, hi) as it is when lo comes later
        P.blk_src[(size_t)blk] = nfree + k;
    }
}

// ---- plain fp64 elimination on a plan (val: nblocks x 49 row-major blocks, the lower triangle of a diagonal block is what counts)
namespace pg_env_detail {
inline double& at(const PgEnvPlan& P, double* val, int r, int c) {  // scalar entry (r, c), c <= r, inside the envelope
    const int i = r / 7, a = r % 7, k = c / 7, b = c % 7;
    return val[((size_t)P.rowoff[(size_t)i] + (size_t)(k - P.first[(size_t)i])) * 49 + (size_t)(a * 7 + b)];
}
}  // namespace pg_env_detail

// L L^T in place, row by row inside the envelope; false on a pivot that is not positive and finite
inline bool pg_env_host_factor(const PgEnvPlan& P, double* val) {
    using pg_env_detail::at;
    const int n = 7 * P.nfree;
    for (int r = 0; r < n; ++r) {
        const int fr = 7 * P.first[(size_t)(r / 7)];
        for (int c = fr; c <= r; ++c) {
            const int fc = 7 * P.first[(size_t)(c / 7)];
            double s = at(P, val, r, c);
            for (int k = std::max(fr, fc); k < c; ++k) s -= at(P, val, r, k) * at(P, val, c, k);
            if (c < r) at(P, val, r, c) = s / at(P, val, c, c);
            else {
                if (!(s > 0.0) || !std::isfinite(s)) return false;
                at(P, val, r, r) = std::sqrt(s);
            }
        }
    }
    return true;
}

// L z = y forward, L^T x = z backward, in place; y is in plan order (7 per position)
inline void pg_env_host_solve(const PgEnvPlan& P, double* val, double* y) {
    using pg_env_detail::at;
    const int n = 7 * P.nfree;
    for (int r = 0; r < n; ++r) {
        double s = y[r];
        for (int k = 7 * P.first[(size_t)(r / 7)]; k < r; ++k) s -= at(P, val, r, k) * y[k];
        y[r] = s / at(P, val, r, r);
    }
    for (int r = n - 1; r >= 0; --r) {
        const double x = y[r] / at(P, val, r, r);
        y[r] = x;
        for (int k = 7 * P.first[(size_t)(r / 7)]; k < r; ++k) y[k] -= at(P, val, r, k) * x;
    }
}
