// The buffers of bundle adjustment (local_ba_impl in svgpu_ba.hip: local, global and both sharded forms), described once as functions of
// an arena: the device arena is input block | output block | work pieces, the page-locked host image input block | output block |
// structure block.  The two input blocks are the same function run on two arenas, so one copy carries the block and "device piece +
// element index" is where a host element goes.  Plain C++ (no HIP): tests/ba_arena_check.cpp compiles this header with sv_arena.h alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "sv_arena.h"

#define BA_LAYOUT_CTL 184  // sizeof(BaCtl) of ba_kernels.h (svgpu_ba.hip asserts they agree)

// stand-ins for HIP's int2 / int4 in the pieces that hold them (svgpu_ba.hip asserts size and alignment agree and casts at the boundary)
struct alignas(8) BaInt2 {
    int x, y;
};
struct alignas(16) BaInt4 {
    int x, y, z, w;
};

enum { BA_DBG_OFF = 0, BA_DBG_PER_LANDMARK = 1, BA_DBG_SCHUR = 2 };  // SVGPU_BA_DBG: no stamps | 8 per landmark-side workgroup | 8 per Schur unit

// everything the layouts depend on
struct BaSizes {
    int P, L, E, world;
    size_t pair_cap;        // worst-case pair storage: sum over the landmarks of k^2 (k observations; k(k+1)/2 pairs + duplicates never exceed it)
    size_t nb_cap;          // upper blocks of the reduced system when every one is kept
    size_t sc_part_blocks;  // NB * nshare <= pairs / 64 + NB (a share holds at least 64 pairs: one trip of a wave)
    size_t xch_doubles, nparts_max;
    int nb_lm, nb_pose;     // workgroups of k_ba_update / k_ba_chi2 (8 lanes per landmark) and of the pose-sized kernels
    size_t pair_scratch;    // bytes: the largest of the sv_ba_*_scratch_bytes of the .hip files, set by the driver
    bool want_dense;        // the dense matrix of the tiled LL^T (ba_dense_tiled.hip)
    bool renumber;          // the solve's own landmark numbering (ba_pairs.hip)
    bool chunk_units;       // chunk-major units of the Schur kernel (ba_pairs.hip); only under `renumber`
    int dbg;                // BA_DBG_*
    size_t unit_cap() const { return chunk_units ? sc_part_blocks : 0; }
};

// lm_off: the L + 1 landmark offsets of the observations, or null while they are not known -- the sizes that depend on them stay 0 then,
// which is enough for the host image (its blocks depend on P, L and E alone; the offsets are written INTO it).
// units_wanted: chunk-major units are not switched off; they are taken under `renumber` while the pairs can be counted in 31 bits.
inline BaSizes ba_sizes(int P, int L, int E, int world, const int* lm_off, bool want_dense, bool renumber, bool units_wanted, int dbg) {
    BaSizes Z{};
    Z.P = P, Z.L = L, Z.E = E, Z.world = world;
    Z.nb_lm = (8 * L + 255) / 256;
    Z.nb_pose = (P + 255) / 256;
    Z.nb_cap = (size_t)P * (P + 1) / 2;
    if (lm_off)
        for (int l = 0; l < L; ++l) {
            const size_t k = lm_off[l + 1] - lm_off[l];
            Z.pair_cap += k * k;
        }
    Z.sc_part_blocks = Z.pair_cap / 64 + Z.nb_cap + 16;
    Z.xch_doubles = std::max(std::max((size_t)P, 4 * (size_t)L), Z.nb_cap) + 8;
    Z.nparts_max = (size_t)(P + 3) / 4 + 1;
    Z.want_dense = want_dense;
    Z.renumber = renumber;
    Z.chunk_units = renumber && units_wanted && Z.pair_cap < ((size_t)1 << 31);
    Z.dbg = dbg;
    return Z;
}

// input block: what the caller passes, observations sorted by landmark; pe_* = pose -> edge lists (built on the device)
struct BaIn {
    Piece<double> pose, points, intr;  // 12 per pose | 3 per landmark | 5 per pose
    Piece<int> e_pose, e_point;
    Piece<float> e_uvr, e_w, e_hub;    // 3 per observation | 1 | 1
    Piece<uint8_t> e_robust;
    Piece<int> lm_off, pe_off, pe_idx;
};
template <class A>
void ba_in_layout(A& arena, const BaSizes& Z, BaIn& Y) {
    const size_t P = Z.P, L = Z.L, E = Z.E;
    Y.pose = arena.template piece<double>(12 * P);
    Y.points = arena.template piece<double>(3 * L);
    Y.intr = arena.template piece<double>(5 * P);
    Y.e_pose = arena.template piece<int>(E);
    Y.e_point = arena.template piece<int>(E);
    Y.e_uvr = arena.template piece<float>(3 * E);
    Y.e_w = arena.template piece<float>(E);
    Y.e_hub = arena.template piece<float>(E);
    Y.e_robust = arena.template piece<uint8_t>(E);
    Y.lm_off = arena.template piece<int>(L + 1);
    Y.pe_off = arena.template piece<int>(P + 1);
    Y.pe_idx = arena.template piece<int>(E);
}

// output block: control block | state = poses (12 each), points (3 each) | outlier flags.  Adjacent up to padding and read back in ONE copy.
struct BaOut {
    Piece<char> ctl;
    Piece<double> state;
    Piece<uint8_t> outlier;
};
template <class A>
void ba_out_layout(A& arena, const BaSizes& Z, BaOut& Y) {
    Y.ctl = arena.template piece<char>(BA_LAYOUT_CTL);
    Y.state = arena.template piece<double>(12 * (size_t)Z.P + 3 * (size_t)Z.L);
    Y.outlier = arena.template piece<uint8_t>((size_t)Z.E + 1);
}
inline Piece<double> ba_out_poses(const BaOut& Y, size_t P) { return {Y.state.p, 12 * P}; }
inline Piece<double> ba_out_points(const BaOut& Y, size_t P) { return {Y.state.p ? Y.state.p + 12 * P : nullptr, Y.state.n - 12 * P}; }
// bytes of the one-copy read-back, from the control block on: through `state` (a caller that takes no outlier flags) or through `outlier`
inline size_t ba_out_bytes(const BaOut& Y, bool with_flags) {
    return (size_t)((const char*)Y.outlier.p - Y.ctl.p) + (with_flags ? pad(Y.outlier.bytes()) : 0);
}
// bytes of the input block in front of an output block placed behind it (what one copy of the whole block moves)
inline size_t ba_in_bytes(const BaIn& in, const BaOut& out) { return (size_t)(out.ctl.p - (const char*)in.pose.p); }

// device-only pieces.  The conditional ones are empty when not taken: S (want_dense), dbg, the unit pieces (chunk_units), rn_* (renumber).
struct BaWork {
    Piece<double> pose1, pt1;  // the second state buffer (the first is the input block's pose | points)
    Piece<uint8_t> e_level;
    Piece<double> e_chi;
    Piece<int> pose_slot;
    Piece<uint8_t> pt_free;
    Piece<int> slot_pose;
    Piece<double> W, lp_part, sc_part, rhs_part, Hll, bl, Hpp, bp, Sblk;
    Piece<double> S;           // (+ the inverted diagonal tiles of ba_dense_tiled.hip)
    Piece<double> dp, red, lm_max;
    Piece<unsigned long long> dbg;
    Piece<double> HB_full;     // sharded: Hpp | bp summed over ranks | one slot per rank: its landmarks' largest diagonal (computeLambdaInit)
    Piece<double> sc;          // sharded: [0..3] per-trial sums, [8..8+world) lambda-init slots
    Piece<double> xch;         // sharded: pose-activity / block-presence / point exchange
    Piece<int> prow_off;
    Piece<BaInt2> prow_ent;
    Piece<int> diag_blk;
    Piece<double> pcg_Minv, pcg_rws, pcg_own, pcg_parts, pcg_scal;
    Piece<int> pm_point;
    Piece<float> pm_uvr, pm_w, pm_hub;
    Piece<BaInt2> blk_pairs;
    Piece<int> blk_pair_l;
    Piece<BaInt2> blk_ab;
    Piece<int> blk_off;
    Piece<char> pair_scratch;
    Piece<int> xs_idx;         // keyframe-segment exchange: block / slot lists
    Piece<uint8_t> lam_slot;   // ... and the damping owners
    Piece<uint8_t> any_owner;  // sharded: the landmark has observations on some rank
    Piece<BaInt4> unit_rec;
    Piece<int> blk_unit_off;
    Piece<double> rhs_unit;
    // renumbered solve: the uploaded arrays (caller's order) are the sources, these the arrays the kernels read
    Piece<int> rn_e_pose, rn_e_point, rn_src;
    Piece<float> rn_uvr, rn_w, rn_hub;
    Piece<int> rn_lm_off, rn_order;
    Piece<double> rn_pts;
    Piece<uint8_t> rn_pt_free_in;
};
template <class A>
void ba_work_layout(A& arena, const BaSizes& Z, BaWork& Y) {
    const size_t P = Z.P, L = Z.L, E = Z.E, nmax = 6 * P, world = Z.world;
    Y.pose1 = arena.template piece<double>(12 * P);
    Y.pt1 = arena.template piece<double>(3 * L);
    Y.e_level = arena.template piece<uint8_t>(E);
    Y.e_chi = arena.template piece<double>(E);
    Y.pose_slot = arena.template piece<int>(P);
    Y.pt_free = arena.template piece<uint8_t>(L);
    Y.slot_pose = arena.template piece<int>(P);
    Y.W = arena.template piece<double>(18 * E);
    Y.lp_part = arena.template piece<double>(27 * 16 * P);
    Y.sc_part = arena.template piece<double>(36 * Z.sc_part_blocks);
    Y.rhs_part = arena.template piece<double>(6 * 16 * P);
    Y.Hll = arena.template piece<double>(6 * L);
    Y.bl = arena.template piece<double>(3 * L);
    Y.Hpp = arena.template piece<double>(36 * P);
    Y.bp = arena.template piece<double>(6 * P);
    Y.Sblk = arena.template piece<double>(36 * Z.nb_cap + 6 * P + 8);
    Y.S = optional_piece<double>(arena, Z.want_dense, (nmax + 1) * nmax + (nmax / 48 + 1) * 48 * 48);
    Y.dp = arena.template piece<double>(nmax);
    Y.red = arena.template piece<double>((size_t)Z.nb_lm + Z.nb_lm + Z.nb_pose + 8);  // chi2 parts | step-scale parts (landmarks, poses) | flags
    Y.lm_max = arena.template piece<double>(Z.nb_lm);
    Y.dbg = optional_piece<unsigned long long>(arena, Z.dbg != BA_DBG_OFF, 8 * (Z.dbg == BA_DBG_SCHUR ? Z.sc_part_blocks + 64 : (size_t)Z.nb_lm));
    Y.HB_full = arena.template piece<double>(42 * P + std::max<size_t>(64, world));
    Y.sc = arena.template piece<double>(64 + world);
    Y.xch = arena.template piece<double>(Z.xch_doubles);
    Y.prow_off = arena.template piece<int>(P + 1);
    Y.prow_ent = arena.template piece<BaInt2>(2 * (Z.nb_cap + 1));
    Y.diag_blk = arena.template piece<int>(P);
    Y.pcg_Minv = arena.template piece<double>(36 * P);
    Y.pcg_rws = arena.template piece<double>(6 * nmax + 8);
    Y.pcg_own = arena.template piece<double>(2 * nmax + 8);
    Y.pcg_parts = arena.template piece<double>(2 * 4 * Z.nparts_max);
    Y.pcg_scal = arena.template piece<double>(8);
    Y.pm_point = arena.template piece<int>(E);
    Y.pm_uvr = arena.template piece<float>(3 * E);
    Y.pm_w = arena.template piece<float>(E);
    Y.pm_hub = arena.template piece<float>(E);
    Y.blk_pairs = arena.template piece<BaInt2>(Z.pair_cap);
    Y.blk_pair_l = arena.template piece<int>(Z.pair_cap);
    Y.blk_ab = arena.template piece<BaInt2>(Z.nb_cap);
    Y.blk_off = arena.template piece<int>(Z.nb_cap + 1);
    Y.pair_scratch = arena.template piece<char>(Z.pair_scratch);
    Y.xs_idx = arena.template piece<int>(Z.nb_cap + P);
    Y.lam_slot = arena.template piece<uint8_t>(P);
    Y.any_owner = arena.template piece<uint8_t>(L);
    Y.unit_rec = optional_piece<BaInt4>(arena, Z.chunk_units, Z.unit_cap());
    Y.blk_unit_off = optional_piece<int>(arena, Z.chunk_units, Z.nb_cap + 2);
    Y.rhs_unit = optional_piece<double>(arena, Z.chunk_units, 6 * Z.unit_cap());
    Y.rn_e_pose = optional_piece<int>(arena, Z.renumber, E);
    Y.rn_e_point = optional_piece<int>(arena, Z.renumber, E);
    Y.rn_src = optional_piece<int>(arena, Z.renumber, E);
    Y.rn_uvr = optional_piece<float>(arena, Z.renumber, 3 * E);
    Y.rn_w = optional_piece<float>(arena, Z.renumber, E);
    Y.rn_hub = optional_piece<float>(arena, Z.renumber, E);
    Y.rn_lm_off = optional_piece<int>(arena, Z.renumber, L + 1);
    Y.rn_order = optional_piece<int>(arena, Z.renumber, L);
    Y.rn_pts = optional_piece<double>(arena, Z.renumber, 3 * L);
    Y.rn_pt_free_in = optional_piece<uint8_t>(arena, Z.renumber, L);
}

// structure block (host image only; every piece is the source of one upload to the work piece of the same name)
struct BaStructure {
    Piece<uint8_t> pt_free;
    Piece<int> pose_slot, slot_pose;
    Piece<BaInt2> blk_ab;
    Piece<int> prow_off, diag;
    Piece<BaInt2> prow_ent;
    Piece<int> xs_idx;  // keyframe-segment exchange
    Piece<uint8_t> lam;
};
template <class A>
void ba_structure_layout(A& arena, const BaSizes& Z, BaStructure& Y) {
    const size_t P = Z.P;
    Y.pt_free = arena.template piece<uint8_t>(Z.L);
    Y.pose_slot = arena.template piece<int>(P);
    Y.slot_pose = arena.template piece<int>(P);
    Y.blk_ab = arena.template piece<BaInt2>(Z.nb_cap);
    Y.prow_off = arena.template piece<int>(P + 1);
    Y.diag = arena.template piece<int>(P);
    Y.prow_ent = arena.template piece<BaInt2>(2 * (Z.nb_cap + 1));
    Y.xs_idx = arena.template piece<int>(Z.nb_cap + P);
    Y.lam = arena.template piece<uint8_t>(P);
}

template <class A>
void ba_device_layout(A& arena, const BaSizes& Z, BaIn& in, BaOut& out, BaWork& work) {
    ba_in_layout(arena, Z, in);
    ba_out_layout(arena, Z, out);
    ba_work_layout(arena, Z, work);
}
template <class A>
void ba_host_layout(A& arena, const BaSizes& Z, BaIn& in, BaOut& out, BaStructure& st) {
    ba_in_layout(arena, Z, in);
    ba_out_layout(arena, Z, out);
    ba_structure_layout(arena, Z, st);
}

// Block rows of the kept upper blocks blk_ab[0 .. NB) (sorted by (a, b), every diagonal block among them) of an nP x nP block matrix, for
// the PCG: row a lists its own blocks (a, b) as (k, b) and, transposed, the blocks (c, a) as (k | 1 << 30, c), sorted by column;
// prow_off[a] .. prow_off[a + 1] are row a's entries in prow_ent, diag[a] is the index of block (a, a).
inline void ba_block_rows(const BaInt2* blk_ab, int NB, int nP, int* prow_off, int* diag, BaInt2* prow_ent) {
    for (int a = 0; a <= nP; ++a) prow_off[a] = 0;
    for (int k = 0; k < NB; ++k) {
        const BaInt2 ab = blk_ab[k];
        prow_off[ab.x + 1]++;
        if (ab.x != ab.y) prow_off[ab.y + 1]++;
        else diag[ab.x] = k;
    }
    for (int a = 0; a < nP; ++a) prow_off[a + 1] += prow_off[a];
    // blk_ab is sorted by (a, b): filling row a with its transposed blocks (c, a), c < a, first (they arrive in c order) and its own
    // blocks (a, b), b >= a, afterwards leaves every row sorted by column
    std::vector<int> fill(prow_off, prow_off + nP);
    for (int k = 0; k < NB; ++k) {
        const BaInt2 ab = blk_ab[k];
        if (ab.x != ab.y) prow_ent[fill[ab.y]++] = BaInt2{k | (1 << 30), ab.x};
    }
    for (int k = 0; k < NB; ++k) prow_ent[fill[blk_ab[k].x]++] = BaInt2{k, blk_ab[k].y};
}
