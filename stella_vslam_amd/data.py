"""Python mirror of the flat part of stella_vslam::data (frame_observation) over the C ABI.

`frame_observation` is built the way system::create_*_frame builds it (system.cc:384-395): undistort the extractor's
keypoints, convert them to bearings and bin them into the matcher grid -- one device call, no host arithmetic.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import camera as _camera
from ._lib import lib, ptr as _p
from .feature import Context


class frame_observation:
    """data/frame_observation.h:12-38.  `keypt_indices_in_cells_` is kept as CSR (cell = col * num_grid_rows_ + row):
    `cell_off_` (num_grid_cols_ * num_grid_rows_ + 1) and `cell_items_`; `indices_in_cell(col, row)` returns the
    reference's vector for one cell."""

    def __init__(self, camera: _camera.base, keypts, descriptors, num_grid_cols: int = 64, num_grid_rows: int = 48,
                 stereo_x_right=None, depths=None):
        self.num_grid_cols_, self.num_grid_rows_ = int(num_grid_cols), int(num_grid_rows)
        self.descriptors_ = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        und, brg, off, items = camera._observe(keypts, grid=(self.num_grid_cols_, self.num_grid_rows_))
        self.undist_keypts_, self.bearings_, self.cell_off_, self.cell_items_ = und, brg, off, items
        self.stereo_x_right_ = None if stereo_x_right is None else np.ascontiguousarray(stereo_x_right, np.float32)
        self.depths_ = None if depths is None else np.ascontiguousarray(depths, np.float32)

    def indices_in_cell(self, col: int, row: int) -> np.ndarray:
        c = col * self.num_grid_rows_ + row
        return self.cell_items_[self.cell_off_[c]:self.cell_off_[c + 1]]


class resident_frame:
    """A data::frame_observation kept on the device (include/svgpu.h svgpu_frame_*): descriptors, undistorted keypoints, stereo
    x_right, bearings and the keypoint grid.  `adopt_extraction` builds it from what the extractor's last extract() left on the
    device (system.cc:384-395 without the upload), `upload` from host arrays (keyframes); `bind(ctx)` makes the NEXT
    projection-family matcher call of `ctx` read its keypoint side from it."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._h = C.c_void_p()
        ctx.check(lib().svgpu_frame_create(ctx.handle, C.byref(self._h)), "svgpu_frame_create")

    def adopt_extraction(self, camera: _camera.base, num_grid_cols: int = 64, num_grid_rows: int = 48, extractor_ctx: Context | None = None):
        """-> (undist_keypts, bearings) as data::frame_observation holds them on the host"""
        from .feature import KEYPOINT_DTYPE as KP_DTYPE
        ectx = extractor_ctx or self.ctx
        n_max = lib().svgpu_orb_max_keypoints(ectx.handle)
        und = np.zeros(max(n_max, 1), KP_DTYPE)
        brg = np.zeros((max(n_max, 1), 3), np.float64)
        ectx.check(lib().svgpu_frame_adopt_extraction(ectx.handle, self._h, C.byref(camera.c_), num_grid_cols, num_grid_rows, _p(und), _p(brg)),
                   "svgpu_frame_adopt_extraction")
        n = self.size
        return und[:n].copy(), brg[:n].copy()

    def upload(self, camera: _camera.base, undist_keypts, descriptors, stereo_x_right=None, num_grid_cols: int = 64, num_grid_rows: int = 48):
        from .feature import KEYPOINT_DTYPE as KP_DTYPE
        k = np.ascontiguousarray(undist_keypts, KP_DTYPE)
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        xr = None if stereo_x_right is None else np.ascontiguousarray(stereo_x_right, np.float32)
        self.ctx.check(lib().svgpu_frame_upload(self.ctx.handle, self._h, C.byref(camera.c_), _p(k), _p(d), _p(xr), len(k), num_grid_cols, num_grid_rows),
                       "svgpu_frame_upload")
        return self

    def set_stereo(self, stereo_x_right):
        xr = None if stereo_x_right is None else np.ascontiguousarray(stereo_x_right, np.float32)
        self.ctx.check(lib().svgpu_frame_set_stereo(self.ctx.handle, self._h, _p(xr)), "svgpu_frame_set_stereo")
        return self

    @property
    def size(self) -> int:
        return int(lib().svgpu_frame_size(self._h))

    def bind(self, ctx: Context | None = None):
        c = ctx or self.ctx
        c.check(lib().svgpu_frame_bind(c.handle, self._h), "svgpu_frame_bind")
        return self

    def close(self):
        if self._h:
            lib().svgpu_frame_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def landmarks_compute_descriptor(ctx: Context, obs_off, obs_desc):
    """data::landmark::compute_descriptor (data/landmark.cc:199-254) for every CSR row of observations at once:
    returns (best_obs, descriptors) -- the index inside each landmark's list and the n x 32 representative descriptors."""
    off = np.ascontiguousarray(obs_off, np.int32)
    d = np.ascontiguousarray(obs_desc, np.uint8).reshape(-1, 32)
    n = len(off) - 1
    best, out = np.zeros(n, np.int32), np.zeros((n, 32), np.uint8)
    ctx.check(lib().svgpu_landmarks_compute_descriptor(ctx.handle, n, _p(off), _p(d), _p(best), _p(out)), "svgpu_landmarks_compute_descriptor")
    return best, out


def landmarks_update_mean_normal_and_obs_scale_variance(ctx: Context, obs_off, obs_trans_wc, pos_w, ref_trans_wc, ref_scale_factor,
                                                        inv_scale_factor_last):
    """data::landmark::update_mean_normal_and_obs_scale_variance (data/landmark.cc:285-318) for every landmark at once:
    returns (mean_normal n x 3, max_valid_dist, min_valid_dist)."""
    off = np.ascontiguousarray(obs_off, np.int32)
    c = np.ascontiguousarray(obs_trans_wc, np.float64).reshape(-1, 3)
    p = np.ascontiguousarray(pos_w, np.float64).reshape(-1, 3)
    r = np.ascontiguousarray(ref_trans_wc, np.float64).reshape(-1, 3)
    sfr = np.ascontiguousarray(ref_scale_factor, np.float32)
    n = len(off) - 1
    mnrm, mx, mn = np.zeros((n, 3), np.float64), np.zeros(n, np.float32), np.zeros(n, np.float32)
    ctx.check(lib().svgpu_landmarks_update_geometry(ctx.handle, n, _p(off), _p(c), _p(p), _p(r), _p(sfr), inv_scale_factor_last,
                                                    _p(mnrm), _p(mx), _p(mn)), "svgpu_landmarks_update_geometry")
    return mnrm, mx, mn


class bow_vocabulary:
    """data/bow_vocabulary.h on a flat tree (node 0 = root; `child_off` / `children` CSR; `node_desc` n x 32; `node_weight`,
    `word_id` per node; `depth` = L).  transform() is compute_bow (data/bow_vocabulary.cc:18-24): the tree descent runs on the
    device, the two sparse maps are assembled here.  Two frameworks, as in the reference's build switch (USE_DBOW2):
      framework = "fbow"   the DEFAULT build: fbow::Vocabulary::transform(descriptors, 4, bow_vec, bow_feat_vec) -- the store level counts
                           DOWN from the root, bow_feat_vec is keyed by FBoW's path code of the node, every word's weight is summed (no
                           stop-word skip) and the vector is normalised (`norm`: "L2" as upstream FBoW's transform does, or "L1")
      framework = "dbow2"  USE_DBOW2: TemplatedVocabulary::transform(features, bow_vec, bow_feat_vec, 4) -- levels UP from the leaves,
                           node index keys, zero-weight words skipped, L1 normalisation
    Both are restated from the libraries' published sources (neither is in the reference checkout): parity unpinned."""

    def __init__(self, ctx: Context, child_off, children, node_desc, node_weight, word_id, depth: int, framework: str = "dbow2", k: int | None = None,
                 norm: str | None = None):
        self.ctx = ctx
        self.depth_ = int(depth)
        if framework not in ("dbow2", "fbow"):
            raise ValueError(f"unknown BoW framework {framework!r}")
        self.framework_ = framework
        off, ch = np.ascontiguousarray(child_off, np.int32), np.ascontiguousarray(children, np.int32)
        self.k_ = int(k) if k is not None else int(np.diff(off).max(initial=2))
        self.norm_ = norm or ("L2" if framework == "fbow" else "L1")
        nd = np.ascontiguousarray(node_desc, np.uint8).reshape(-1, 32)
        nw, wi = np.ascontiguousarray(node_weight, np.float32), np.ascontiguousarray(word_id, np.int32)
        self._h = C.c_void_p()
        ctx.check(lib().svgpu_bow_vocabulary_upload(ctx.handle, len(off) - 1, _p(off), _p(ch), _p(nd), _p(nw), _p(wi), C.byref(self._h)),
                  "svgpu_bow_vocabulary_upload")

    @classmethod
    def load_fbow(cls, ctx: Context, path: str) -> "bow_vocabulary":
        """bow_vocabulary_util::load (data/bow_vocabulary.cc:26-47) for an .fbow file; see read_fbow for what is unverified."""
        t = read_fbow(path)
        return cls(ctx, t["child_off"], t["children"], t["node_desc"], t["node_weight"], t["word_id"], t["depth"], framework="fbow", k=t.get("k"))

    def descend(self, descriptors, levels_up: int = 4):
        """DBoW2 form: (word, weight, node index at depth L - levels_up).  FBoW form: use descend_fbow."""
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        n = len(d)
        word, weight, node = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        level = max(self.depth_ - levels_up, 0)
        self.ctx.check(lib().svgpu_bow_transform(self.ctx.handle, self._h, _p(d), n, level, _p(word), _p(weight), _p(node)),
                       "svgpu_bow_transform")
        return word, weight, node

    def descend_fbow(self, descriptors, store_level: int = 4):
        """fbow::Vocabulary::transform's descent: (word, weight, bow_feat_vec key = path code at `store_level` from the root)."""
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        n = len(d)
        word, weight, code = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
        self.ctx.check(lib().svgpu_fbow_transform(self.ctx.handle, self._h, _p(d), n, int(store_level), self.k_, _p(word), _p(weight), _p(code)),
                       "svgpu_fbow_transform")
        return word, weight, code

    def transform(self, descriptors, levels_up: int = 4):
        """-> (bow_vec: {word_id: weight}, bow_feat_vec: {node key: [feature indices]}); `levels_up` is the literal 4 compute_bow passes."""
        bow_vec, feat = {}, {}
        if self.framework_ == "fbow":
            word, weight, node = self.descend_fbow(descriptors, levels_up)
            for i in range(len(word)):
                bow_vec[int(word[i])] = bow_vec.get(int(word[i]), 0.0) + float(weight[i])
                feat.setdefault(int(node[i]), []).append(i)
        else:
            word, weight, node = self.descend(descriptors, levels_up)
            for i in range(len(word)):
                if weight[i] > 0:  # DBoW2 skips zero-weight words (stop words)
                    bow_vec[int(word[i])] = bow_vec.get(int(word[i]), 0.0) + float(weight[i])
                    feat.setdefault(int(node[i]), []).append(i)
        if self.norm_ == "L2":
            norm = float(np.sqrt(sum(v * v for _, v in sorted(bow_vec.items()))))
        else:
            norm = sum(abs(v) for _, v in sorted(bow_vec.items()))
        if norm > 0.0:
            bow_vec = {k: v / norm for k, v in bow_vec.items()}
        return dict(sorted(bow_vec.items())), dict(sorted(feat.items()))

    def compute_bow_batch(self, descriptor_sets, levels_up: int = 4, db: "bow_database | None" = None) -> dict:
        """svgpu_bow_compute_batch: compute_bow of every descriptor set in ONE device call, the two maps built on the device.  -> the flat
        arrays of include/svgpu.h: d_off, word, weight, node (per descriptor), vec_off / vec_word / vec_weight, feat_off / feat_key /
        feat_index, `stats` (launches, copies, synchronisations) and, with `db`, the `slots` the vectors were registered under.
        The arithmetic is that of the C++ class data::bow_vocabulary_hip::compute_bow: the FBoW form multiplies by 1.0 / sqrt(norm), where
        transform() divides by sqrt(norm) -- the two may differ in the last bit."""
        sets = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in descriptor_sets]
        b = len(sets)
        off = np.zeros(b + 1, np.int32)
        off[1:] = np.cumsum([len(d) for d in sets])
        n = int(off[-1])
        desc = np.ascontiguousarray(np.concatenate(sets)) if n else np.zeros((0, 32), np.uint8)
        fbow = self.framework_ == "fbow"
        level = int(levels_up) if fbow else max(self.depth_ - int(levels_up), 0)
        out = dict(d_off=off, word=np.zeros(n, np.int32), weight=np.zeros(n, np.float32), node=np.zeros(n, np.uint32),
                   vec_off=np.zeros(b + 1, np.int32), vec_word=np.zeros(n, np.uint32), vec_weight=np.zeros(n, np.float64),
                   feat_off=np.zeros(b + 1, np.int32), feat_key=np.zeros(n, np.uint32), feat_index=np.zeros(n, np.int32))
        slots = np.full(b, -1, np.int32) if db is not None else None
        stats = np.zeros(3, np.int32)
        self.ctx.check(lib().svgpu_bow_compute_batch(self.ctx.handle, self._h, 1 if fbow else 0, level, self.k_, b, _p(off), _p(desc), _p(out["word"]),
                                                     _p(out["weight"]), _p(out["node"]), _p(out["vec_off"]), _p(out["vec_word"]), _p(out["vec_weight"]),
                                                     _p(out["feat_off"]), _p(out["feat_key"]), _p(out["feat_index"]),
                                                     db._h if db is not None else None, _p(slots) if db is not None else None, _p(stats)),
                       "svgpu_bow_compute_batch")
        nv, nf = int(out["vec_off"][-1]), int(out["feat_off"][-1])
        for key in ("vec_word", "vec_weight"):
            out[key] = out[key][:nv]
        for key in ("feat_key", "feat_index"):
            out[key] = out[key][:nf]
        out["stats"] = dict(launches=int(stats[0]), copies=int(stats[1]), synchronisations=int(stats[2]))
        if db is not None:
            out["slots"] = slots
        return out

    def transform_batch(self, descriptor_sets, levels_up: int = 4, db: "bow_database | None" = None):
        """compute_bow for a list of descriptor arrays in one device call -> a list of (bow_vec, bow_feat_vec) as transform() returns them
        (see compute_bow_batch for the one difference in the FBoW form's last bit).  With `db` the vectors are registered in the database on
        the way, device to device: -> (that list, slots)."""
        r = self.compute_bow_batch(descriptor_sets, levels_up, db)
        res = []
        for f in range(len(r["d_off"]) - 1):
            v0, v1, f0, f1 = r["vec_off"][f], r["vec_off"][f + 1], r["feat_off"][f], r["feat_off"][f + 1]
            bow_vec = {int(w): float(x) for w, x in zip(r["vec_word"][v0:v1], r["vec_weight"][v0:v1])}
            feat = {}
            for key, i in zip(r["feat_key"][f0:f1], r["feat_index"][f0:f1]):
                feat.setdefault(int(key), []).append(int(i))
            res.append((bow_vec, feat))
        return (res, [int(s) for s in r["slots"]]) if db is not None else res

    def close(self):
        if self._h:
            lib().svgpu_bow_vocabulary_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bowdb_query_stage_capacity() -> int:
    """Word ids of a query that k_bowdb_count / k_bowdb_score hold in LDS at a time (a longer query is walked in chunks)."""
    return int(lib().svgpu_bowdb_query_stage_capacity())


def _bow_arrays(bow_vec):
    """{word: weight} (or a (words, weights) pair) -> ascending uint32 ids and float64 weights, the order of the reference's std::map"""
    if isinstance(bow_vec, dict):
        items = sorted(bow_vec.items())
        return np.array([k for k, _ in items], np.uint32), np.array([v for _, v in items], np.float64)
    w, v = bow_vec
    return np.ascontiguousarray(w, np.uint32), np.ascontiguousarray(v, np.float64)


class bow_database:
    """data/bow_database.h on the device (include/svgpu.h svgpu_bowdb_*): keyframes are known by the slot number add_keyframe returns
    (increasing, not reused before clear).  `framework` selects the score like bow_vocabulary's: "fbow" = fbow::BoWVector::score
    (the default build), "dbow2" = DBoW2's L1 score (USE_DBOW2); both restated from the published sources: parity unpinned.
    BoW vectors are the {word: weight} dicts bow_vocabulary.transform returns."""

    def __init__(self, ctx: Context, framework: str = "fbow"):
        if framework not in ("dbow2", "fbow"):
            raise ValueError(f"unknown BoW framework {framework!r}")
        self.ctx, self.framework_ = ctx, framework
        self._h = C.c_void_p()
        ctx.check(lib().svgpu_bowdb_create(ctx.handle, 0 if framework == "fbow" else 1, C.byref(self._h)), "svgpu_bowdb_create")

    def add_keyframe(self, bow_vec) -> int:
        w, v = _bow_arrays(bow_vec)
        slot = C.c_int32(-1)
        self.ctx.check(lib().svgpu_bowdb_add(self.ctx.handle, self._h, len(w), _p(w), _p(v), C.byref(slot)), "svgpu_bowdb_add")
        return slot.value

    def add_keyframes(self, bow_vecs) -> list:
        """svgpu_bowdb_add_batch: every vector of the list registered in one submission -> their slots, in order.  The database ends as
        after add_keyframe on each; if any vector's ids do not ascend strictly nothing is added."""
        arrs = [_bow_arrays(b) for b in bow_vecs]
        b = len(arrs)
        if b == 0:
            return []
        off = np.zeros(b + 1, np.int32)
        off[1:] = np.cumsum([len(w) for w, _ in arrs])
        w = np.ascontiguousarray(np.concatenate([a for a, _ in arrs]), np.uint32)
        v = np.ascontiguousarray(np.concatenate([a for _, a in arrs]), np.float64)
        slots = np.full(b, -1, np.int32)
        self.ctx.check(lib().svgpu_bowdb_add_batch(self.ctx.handle, self._h, b, _p(off), _p(w), _p(v), _p(slots)), "svgpu_bowdb_add_batch")
        return [int(s) for s in slots]

    def erase_keyframe(self, slot: int):
        self.ctx.check(lib().svgpu_bowdb_erase(self.ctx.handle, self._h, int(slot)), "svgpu_bowdb_erase")

    def clear(self):
        self.ctx.check(lib().svgpu_bowdb_clear(self.ctx.handle, self._h), "svgpu_bowdb_clear")

    def size(self):
        """-> (live keyframes, live entries)"""
        k, e = C.c_int(0), C.c_longlong(0)
        lib().svgpu_bowdb_size(self._h, C.byref(k), C.byref(e))
        return k.value, e.value

    def diagnostics(self) -> dict:
        v = [C.c_longlong(0) for _ in range(5)]
        lib().svgpu_bowdb_diagnostics(self._h, *[C.byref(x) for x in v])
        return dict(zip(("num_slots", "pool_capacity", "pool_used", "num_growths", "num_compactions"), (x.value for x in v)))

    def acquire_keyframes(self, bow_vec, min_score: float = 0.0, num_common_words_thr_ratio: float = 0.8, reject=(), cap: int | None = None,
                          full: bool = False):
        """-> (slots, common, score) of the candidates in ascending slot order; `cap` limits what is written (default: every slot).
        full=True: -> (slots, common, score, n_out, max_common), n_out counting the candidates beyond `cap` as well."""
        w, v = _bow_arrays(bow_vec)
        rej = np.ascontiguousarray(list(reject), np.int32)
        cap = self.diagnostics()["num_slots"] if cap is None else int(cap)
        slots, common, score = np.zeros(cap, np.int32), np.zeros(cap, np.uint32), np.zeros(cap, np.float32)
        n, mc = C.c_int32(0), C.c_uint32(0)
        self.ctx.check(lib().svgpu_bowdb_acquire(self.ctx.handle, self._h, len(w), _p(w), _p(v), min_score, num_common_words_thr_ratio,
                                                 len(rej), _p(rej), cap, _p(slots), _p(common), _p(score), C.byref(n), C.byref(mc)), "svgpu_bowdb_acquire")
        k = min(n.value, cap)
        r = (slots[:k], common[:k], score[:k])
        return r + (n.value, mc.value) if full else r

    def acquire_keyframes_batch(self, bow_vecs, min_scores=0.0, num_common_words_thr_ratio: float = 0.8, reject=(), cap: int | None = None):
        """One submission for len(bow_vecs) queries -> a list of (slots, common, score, n_out, max_common), one per query."""
        arrs = [_bow_arrays(b) for b in bow_vecs]
        q = len(arrs)
        if q == 0:
            return []
        off = np.zeros(q + 1, np.int32)
        off[1:] = np.cumsum([len(w) for w, _ in arrs])
        w = np.ascontiguousarray(np.concatenate([a for a, _ in arrs]), np.uint32)
        v = np.ascontiguousarray(np.concatenate([a for _, a in arrs]), np.float64)
        ms = np.ascontiguousarray(np.broadcast_to(np.asarray(min_scores, np.float32), (q,)))
        rej = np.ascontiguousarray(list(reject), np.int32)
        cap = self.diagnostics()["num_slots"] if cap is None else int(cap)
        slots, common, score = np.zeros((q, cap), np.int32), np.zeros((q, cap), np.uint32), np.zeros((q, cap), np.float32)
        n, mc = np.zeros(q, np.int32), np.zeros(q, np.uint32)
        self.ctx.check(lib().svgpu_bowdb_acquire_batch(self.ctx.handle, self._h, q, _p(off), _p(w), _p(v), _p(ms), num_common_words_thr_ratio,
                                                       len(rej), _p(rej), cap, _p(slots), _p(common), _p(score), _p(n), _p(mc)), "svgpu_bowdb_acquire_batch")
        return [(slots[i, :min(n[i], cap)], common[i, :min(n[i], cap)], score[i, :min(n[i], cap)], int(n[i]), int(mc[i])) for i in range(q)]

    def score(self, bow_vec, slots) -> np.ndarray:
        """bow_vocabulary_util::score of the query against each listed slot (-1 for an erased or unknown one)."""
        w, v = _bow_arrays(bow_vec)
        sl = np.ascontiguousarray(slots, np.int32)
        out = np.zeros(len(sl), np.float32)
        self.ctx.check(lib().svgpu_bowdb_score(self.ctx.handle, self._h, len(w), _p(w), _p(v), len(sl), _p(sl), _p(out)), "svgpu_bowdb_score")
        return out

    def close(self):
        if self._h:
            lib().svgpu_bowdb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------- .fbow vocabulary files
# data::bow_vocabulary_util::load (data/bow_vocabulary.cc:26-47) hands the path to fbow::Vocabulary::readFromFile in the default
# (FBoW) build.  FBoW is an un-vendored submodule (3rd/FBoW is empty in the checkout studied; the reference pins stella-cv/FBoW),
# so the layout below restates the published fbow/vocabulary.h and has NOT been checked against a real orb_vocab.fbow here
# (none is available offline): treat it as unverified until a real file has been read with it.
#   uint64 magic 55824124 | struct params (120 bytes) | _total_size bytes of blocks
#   params: char desc_name[50]; u32 alignment, nblocks; u64 desc_size_wp, block_size_wp, feature_off, child_off, total_size;
#           i32 desc_type, desc_size; u32 k                                   (natural C alignment, little endian)
#   block:  u16 N | u16 is_leaf | u32 parent | pad | N descriptors (desc_size_wp apart, from feature_off) |
#           N x {u32 id_or_childblock (MSB = leaf), f32 weight} from child_off
FBOW_MAGIC = 55824124
_FBOW_PARAMS = np.dtype([("desc_name", "S50"), ("_pad0", "V2"), ("alignment", "<u4"), ("nblocks", "<u4"), ("_pad1", "V4"), ("desc_size_wp", "<u8"),
                         ("block_size_wp", "<u8"), ("feature_off", "<u8"), ("child_off", "<u8"), ("total_size", "<u8"), ("desc_type", "<i4"),
                         ("desc_size", "<i4"), ("k", "<u4"), ("_pad2", "V4")])
assert _FBOW_PARAMS.itemsize == 120


def read_fbow(path: str) -> dict:
    """-> the flat tree svgpu_bow_vocabulary_upload takes (node 0 = a virtual root whose children are block 0's nodes; nodes in
    breadth-first order with siblings in block order, so that node ids at one depth sort like fbow's path-bit node ids)."""
    raw = np.fromfile(path, np.uint8)
    if len(raw) < 128 or int(raw[:8].view("<u8")[0]) != FBOW_MAGIC:
        raise ValueError(f"{path}: not an fbow vocabulary (bad signature)")
    P = raw[8:128].view(_FBOW_PARAMS)[0]
    if int(P["desc_size"]) != 32 or int(P["desc_type"]) != 0:
        raise ValueError(f"{path}: only 32-byte CV_8UC1 (ORB) vocabularies are supported (desc_size {P['desc_size']}, type {P['desc_type']})")
    bs, fo, co, dw, nb = (int(P[k]) for k in ("block_size_wp", "feature_off", "child_off", "desc_size_wp", "nblocks"))
    data = raw[128:128 + int(P["total_size"])]
    if len(data) != int(P["total_size"]) or nb * bs > len(data):
        raise ValueError(f"{path}: truncated")
    desc, weight, word, kids = [np.zeros(32, np.uint8)], [0.0], [-1], [[]]
    queue, depth, seen = [(0, 0, 0)], 0, set()      # (block, parent node, depth of the block's nodes - 1)
    while queue:
        blk, parent, d = queue.pop(0)
        if blk >= nb or blk in seen:
            raise ValueError(f"{path}: corrupt block graph at block {blk}")
        seen.add(blk)
        b = data[blk * bs:(blk + 1) * bs]
        n = int(b[:2].view("<u2")[0])
        info = b[co:co + 8 * n].view(np.dtype([("id", "<u4"), ("w", "<f4")]))
        depth = max(depth, d + 1)
        for i in range(n):
            node = len(desc)
            kids[parent].append(node)
            desc.append(b[fo + i * dw:fo + i * dw + 32].copy())
            kids.append([])
            if int(info["id"][i]) & 0x80000000:
                weight.append(float(info["w"][i]))
                word.append(int(info["id"][i]) & 0x7FFFFFFF)
            else:
                weight.append(0.0)
                word.append(-1)
                queue.append((int(info["id"][i]) & 0x7FFFFFFF, node, d + 1))
    off = np.zeros(len(desc) + 1, np.int32)
    off[1:] = np.cumsum([len(k) for k in kids])
    return dict(child_off=off, children=np.array([c for k in kids for c in k], np.int32), node_desc=np.stack(desc), node_weight=np.array(weight, np.float32),
                word_id=np.array(word, np.int32), depth=depth, k=int(P["k"]), desc_name=bytes(P["desc_name"]).split(b"\0")[0].decode())


def write_fbow(path: str, child_off, children, node_desc, node_weight, word_id, k: int, alignment: int = 8, desc_name: str = "orb") -> None:
    """Inverse of read_fbow (fixtures / converting a flat tree to a file the reference build can load)."""
    up = lambda v: (v + alignment - 1) // alignment * alignment
    dw, fo = up(32), up(8)
    co = fo + k * dw
    bs = up(co + 8 * k)
    blocks, queue = [], [(0, 0)]   # (node whose children form the block, parent block)
    index = {0: 0}
    while queue:
        node, parent = queue.pop(0)
        ch = [int(c) for c in children[child_off[node]:child_off[node + 1]]]
        assert 0 < len(ch) <= k
        b = np.zeros(bs, np.uint8)
        b[:2] = np.array([len(ch)], "<u2").view(np.uint8)
        leaf = all(child_off[c] == child_off[c + 1] for c in ch)
        b[2:4] = np.array([1 if leaf else 0], "<u2").view(np.uint8)
        b[4:8] = np.array([parent], "<u4").view(np.uint8)
        me = len(blocks)
        blocks.append(b)
        for i, c in enumerate(ch):
            b[fo + i * dw:fo + i * dw + 32] = node_desc[c]
            if child_off[c] == child_off[c + 1]:
                ident, w = 0x80000000 | int(word_id[c]), float(node_weight[c])
            else:
                index[c] = len(blocks) + len(queue)
                queue.append((c, me))
                ident, w = index[c], 0.0
            b[co + 8 * i:co + 8 * i + 4] = np.array([ident], "<u4").view(np.uint8)
            b[co + 8 * i + 4:co + 8 * i + 8] = np.array([w], "<f4").view(np.uint8)
    P = np.zeros(1, _FBOW_PARAMS)
    P["desc_name"], P["alignment"], P["nblocks"], P["desc_size_wp"], P["block_size_wp"] = desc_name.encode(), alignment, len(blocks), dw, bs
    P["feature_off"], P["child_off"], P["total_size"], P["desc_type"], P["desc_size"], P["k"] = fo, co, bs * len(blocks), 0, 32, k
    with open(path, "wb") as f:
        f.write(np.array([FBOW_MAGIC], "<u8").tobytes())
        f.write(P.tobytes())
        f.write(np.concatenate(blocks).tobytes())
