"""Image ingest on the device (svgpu_ingest_*, svgpu_tracker_set_ingest) against the numpy restatement of tests/ingest_problems.py.
Every comparison is byte equality."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

from tests import ingest_problems as IP
from tests import orb_images

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
FORMATS = list(IP.FORMATS)
KP_FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd import feature
    c = feature.Context()
    yield c
    c.close()


def _odd(n):
    """the next row stride >= n + 1 that is not a multiple of 4"""
    n += 1
    return n if n % 4 else n + 1


def _image(cls, w, h, channels, seed):
    if cls == "noise_rgb":
        return IP.noise_image(w, h, channels, seed)
    return IP.colour_image(orb_images.make(cls, w, h, seed), channels, seed)


def _check_single(ctx, fmt, w, h, map_kind, img_cls, seed, odd_strides):
    from stella_vslam_amd import ingest
    ch, order = IP.FORMATS[fmt]
    raw = _image(img_cls, w, h, ch, seed)
    mx, my = IP.make_maps(map_kind, w, h, seed) if map_kind else (None, None)
    exp = IP.ingest(raw, order, mx, my)
    ing = ingest.Ingest(ctx, w, h, ch, order, mx, my)
    src = IP.strided(raw, _odd(w * ch + 4)) if odd_strides else raw
    ds = _odd(w + 2) if odd_strides else w
    buf = np.full(h * ds, 0xA5, np.uint8)
    out = np.lib.stride_tricks.as_strided(buf, shape=(h, w), strides=(ds, 1))
    ing.gray(src, out=out)
    ing.close()
    assert np.array_equal(out, exp), (fmt, w, h, map_kind, img_cls, int((out != exp).sum()))
    pad = np.ones(buf.size, bool)      # nothing written between the rows
    for y in range(h):
        pad[y * ds: y * ds + w] = False
    assert (buf[pad] == 0xA5).all()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", IP.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gray_every_format_and_size(ctx, fmt, size):
    """formats x sizes, each without maps and with one map class (all five classes occur), image classes rotating, strides not multiples of 4"""
    w, h = size
    k = FORMATS.index(fmt) + IP.SIZES.index(size)
    classes = list(orb_images.CLASSES) + ["noise_rgb"]
    _check_single(ctx, fmt, w, h, None, classes[k % len(classes)], 10 + k, odd_strides=True)
    _check_single(ctx, fmt, w, h, IP.MAP_CLASSES[k % len(IP.MAP_CLASSES)], classes[(k + 3) % len(classes)], 20 + k, odd_strides=(k % 2 == 0))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("map_kind", IP.MAP_CLASSES)
def test_gray_every_format_and_map_class(ctx, fmt, map_kind):
    for (w, h), odd in (((203, 157), True), ((640, 480), False)):
        _check_single(ctx, fmt, w, h, map_kind, "noise_rgb", 5, odd)


@pytest.mark.parametrize("img_cls", list(orb_images.CLASSES) + ["noise_rgb"])
def test_gray_every_image_class(ctx, img_cls):
    _check_single(ctx, "RGB", 640, 480, None, img_cls, 3, False)
    _check_single(ctx, "BGRA", 640, 480, "plumb_bob", img_cls, 3, True)


def _batch(ctx, ing, frames, src_row, dst_row, src_gap, dst_gap, offset):
    """frames: list of raw (h, w[, c]) arrays -> (B, h, w) grey through svgpu_ingest_gray_batch_device on buffers with the given row strides,
    `gap` extra bytes between frames and `offset` bytes in front."""
    import torch
    B, h, w = len(frames), ing.height, ing.width
    rowb = w * ing.channels
    sfs, dfs = src_row * h + src_gap, dst_row * h + dst_gap
    host = np.full(offset + B * sfs, 0x5A, np.uint8)
    for b, f in enumerate(frames):
        v = np.lib.stride_tricks.as_strided(host[offset + b * sfs:], shape=(h, rowb), strides=(src_row, 1))
        v[...] = np.ascontiguousarray(f).reshape(h, rowb)
    src = torch.from_numpy(host).cuda()
    dst = torch.full((offset + B * dfs,), 0xC3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ing.gray_batch_device(src.data_ptr() + offset, B, sfs, src_row, dst.data_ptr() + offset, dfs, dst_row, ctx=ctx)
    ctx.synchronize()
    d = dst.cpu().numpy()
    out = np.stack([np.lib.stride_tricks.as_strided(d[offset + b * dfs:], shape=(h, w), strides=(dst_row, 1)).copy() for b in range(B)])
    written = np.zeros(d.size, bool)
    for b in range(B):
        for y in range(h):
            o = offset + b * dfs + y * dst_row
            written[o:o + w] = True
    assert (d[~written] == 0xC3).all()      # nothing outside the rows
    return out


def _distinct_frames(w, h, ch, B, seed):
    base = _image("noise_rgb" if seed % 2 else "spots", w, h, ch, seed)
    return [np.roll(base, (b, 2 * b), (0, 1)) ^ np.uint8(b & 0xFF) for b in range(B)]


@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("fmt,map_kind", [("RGB", None), ("RGB", "plumb_bob"), ("GRAY", None), ("BGRA", "quarter_outside")])
def test_batch_equals_single_calls(ctx, B, fmt, map_kind):
    from stella_vslam_amd import ingest
    w, h = 640, 480
    ch, order = IP.FORMATS[fmt]
    mx, my = IP.make_maps(map_kind, w, h, 7) if map_kind else (None, None)
    ing = ingest.Ingest(ctx, w, h, ch, order, mx, my)
    frames = _distinct_frames(w, h, ch, B, 31 + B)
    single = np.stack([ing.gray(f) for f in frames])
    assert np.array_equal(single[0], IP.ingest(frames[0], order, mx, my))
    if B > 1:
        assert not np.array_equal(single[0], single[1])
    aligned = _batch(ctx, ing, frames, w * ch, w, 0, 0, 0)                                   # dense, 16-byte aligned: the wide path
    assert np.array_equal(aligned, single)
    odd = _batch(ctx, ing, frames, _odd(w * ch + 8), _odd(w + 4), 3, 5, 1)                   # nothing aligned
    assert np.array_equal(odd, single)
    ing.close()


def test_batch_slices_with_a_partial_last_one(ctx):
    """70 frames of 1241 x 376: the rectifying kernel's blocks walk 8 frames each, the last slice holds 6"""
    from stella_vslam_amd import ingest
    w, h, B = 1241, 376, 70
    mx, my = IP.make_maps("plumb_bob", w, h, 9)
    ing = ingest.Ingest(ctx, w, h, 1, IP.GRAY, mx, my)
    frames = _distinct_frames(w, h, 1, B, 4)
    got = _batch(ctx, ing, frames, w + 3, w + 3, 0, 0, 0)
    for b in (0, 1, 7, 8, 63, 64, 69):
        assert np.array_equal(got[b], IP.ingest(frames[b], IP.GRAY, mx, my)), b
    single = np.stack([ing.gray(f) for f in frames])
    assert np.array_equal(got, single)
    ing.close()


def test_batch_output_feeds_the_extractor(ctx):
    """raw frames -> svgpu_ingest_gray_batch_device -> svgpu_orb_extract_batch_device, no host image in between: keypoints and descriptors of the
    same grey frames uploaded from the restatement"""
    import torch
    from stella_vslam_amd import feature, ingest
    from stella_vslam_amd._lib import lib
    L = lib()
    w, h, B = 640, 480, 3
    p = feature.orb_params()
    ext = feature.orb_extractor(p, ctx=ctx, max_batch=B)
    ext._configure(w, h)
    cap = ext.max_keypoints()
    mx, my = IP.make_maps("plumb_bob", w, h, 2)
    ing = ingest.Ingest(ctx, w, h, 3, IP.BGR, mx, my)
    from stella_vslam_amd import synthetic
    frames = [IP.colour_image(g, 3, 40 + i) for i, g in enumerate(synthetic.frame_sequence(B, w, h, seed=5))]
    pitch = 656
    grey_ref = np.zeros((B, h, pitch), np.uint8)
    for b in range(B):
        grey_ref[b, :, :w] = IP.ingest(frames[b], IP.BGR, mx, my)

    def extract(img_dev):
        kps = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda")
        desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(B * (1 + p.num_levels_), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.check(L.svgpu_orb_extract_batch_device(ctx.handle, C.c_void_p(img_dev.data_ptr()), B, C.c_size_t(h * pitch), pitch, None, C.c_size_t(0), 0,
                                                   C.c_void_p(kps.data_ptr()), C.c_void_p(desc.data_ptr()), cap, C.c_void_p(counts.data_ptr()), None), "extract")
        ctx.synchronize()
        return kps.cpu().numpy(), desc.cpu().numpy(), counts.cpu().numpy()

    raw = torch.from_numpy(np.stack(frames)).cuda()
    grey_dev = torch.zeros(B * h * pitch, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ing.gray_batch_device(raw.data_ptr(), B, h * w * 3, w * 3, grey_dev.data_ptr(), h * pitch, pitch, ctx=ctx)
    got = extract(grey_dev)                              # (same stream: ordered behind the ingest)
    assert np.array_equal(grey_dev.cpu().numpy().reshape(B, h, pitch), grey_ref)
    exp = extract(torch.from_numpy(grey_ref.reshape(-1)).cuda())
    n = exp[2].reshape(B, -1)[:, 0]
    assert (n > 500).all()
    for a, b in zip(got, exp):
        assert np.array_equal(a, b)
    ing.close()


def test_depth_equals_one_fp32_product(ctx):
    from stella_vslam_amd import ingest
    rng = np.random.default_rng(8)
    for (w, h) in ((640, 480), (203, 157)):
        d16 = rng.integers(0, 65536, (h, w), dtype=np.uint16)
        d16[0, :4] = (0, 65535, 5000, 1)
        for factor in (5000.0, 1000.0, 1.0, 3.7):
            got = ingest.depth(ctx, d16, factor)
            assert np.array_equal(got.view(np.uint32), IP.true_depth(d16, factor).view(np.uint32)), factor
        assert ingest.depth(ctx, d16, 5000.0)[0, 2] == np.float32(1.0)
        d32 = (rng.random((h, w)) * 40 - 2).astype(np.float32)
        d32[0, :3] = (0.0, -1.0, 65535.0)
        for factor in (1.0, 5000.0, 0.001):
            got = ingest.depth(ctx, d32, factor)
            assert np.array_equal(got.view(np.uint32), IP.true_depth(d32, factor).view(np.uint32)), factor
        # padded rows on both sides
        buf = np.zeros((h, w + 3), np.uint16)
        buf[:, :w] = d16
        assert np.array_equal(ingest.depth(ctx, buf[:, :w], 5000.0).view(np.uint32), IP.true_depth(d16, 5000.0).view(np.uint32))


def test_depth_device_form(ctx):
    import torch
    from stella_vslam_amd import ingest
    w, h = 321, 77
    d16 = np.random.default_rng(3).integers(0, 65536, (h, w + 1), dtype=np.uint16)
    src = torch.from_numpy(d16.view(np.int16)).cuda()
    dst = torch.full((h, w + 2), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ingest.depth_device(ctx, src.data_ptr(), ingest.DEPTH_U16, (w + 1) * 2, w, h, 5000.0, dst.data_ptr(), (w + 2) * 4)
    ctx.synchronize()
    got = dst.cpu().numpy()
    assert np.array_equal(got[:, :w].view(np.uint32), IP.true_depth(d16[:, :w], 5000.0).view(np.uint32)) and (got[:, w:] == -7.0).all()


# ---------------------------------------------------------------------------------------------------------------- the tracker
def _pose12(R, t):
    return np.concatenate([R, t.reshape(3, 1)], 1).reshape(12)


def _same_run(a, b, stereo):
    assert a["result"]["n_keypoints"] == b["result"]["n_keypoints"] > 1000
    for f in KP_FIELDS:
        assert np.array_equal(a["keypts"][f], b["keypts"][f]), f
        assert np.array_equal(a["undist_keypts"][f], b["undist_keypts"][f]), f
    assert a["descriptors"].tobytes() == b["descriptors"].tobytes() and a["bearings"].tobytes() == b["bearings"].tobytes()
    assert a["match_last"].tobytes() == b["match_last"].tobytes() and a["outlier"].tobytes() == b["outlier"].tobytes()
    assert a["result"]["pose_cw"].tobytes() == b["result"]["pose_cw"].tobytes()
    assert a["result"]["num_matches"] == b["result"]["num_matches"] and a["result"]["num_valid"] == b["result"]["num_valid"]
    if stereo:
        assert a["stereo_x_right"].tobytes() == b["stereo_x_right"].tobytes() and a["depths"].tobytes() == b["depths"].tobytes()


def _scene(kind):
    """-> everything one tracked frame of `kind` (mono | stereo | rgbd) needs: raw inputs, the restatement's grey / float images, ingests' arguments"""
    from stella_vslam_amd import synthetic
    if kind == "stereo":
        w, h, disp = 752, 480, 14
        big = synthetic.frame_sequence(2, w + 64, h, seed=23)
        left = [np.ascontiguousarray(b[:, 8:8 + w]) for b in big]
        right = [np.ascontiguousarray(b[:, 8 + disp:8 + disp + w]) for b in big]
        raw_l = [IP.colour_image(g, 3, 50 + i) for i, g in enumerate(left)]
        raw_r = [IP.colour_image(g, 4, 60 + i) for i, g in enumerate(right)]
        # two DIFFERENT map pairs: the same gentle lens, the right camera turned a little further about y
        gentle = (-0.012, 0.004, 0.0001, -0.0001, 0.0)
        maps_l = IP.plumb_bob_maps(w, h, seed=1, rot=(0.0008, -0.0015, 0.0005), dist=gentle)
        maps_r = IP.plumb_bob_maps(w, h, seed=1, rot=(0.0008, 0.0020, 0.0005), dist=gentle)
        assert not np.array_equal(maps_l[0], maps_r[0])
        grey_l = [IP.ingest(r, IP.RGB, *maps_l) for r in raw_l]
        grey_r = [IP.ingest(r, IP.BGR, *maps_r) for r in raw_r]
        return dict(w=w, h=h, raw_l=raw_l, raw_r=raw_r, grey_l=grey_l, grey_r=grey_r, fmt_l=(3, IP.RGB, maps_l), fmt_r=(4, IP.BGR, maps_r))
    w, h = 640, 480
    imgs = synthetic.frame_sequence(2, w, h, seed=11 if kind == "mono" else 31)
    raw = [IP.colour_image(g, 3, 70 + i) for i, g in enumerate(imgs)]
    grey = [IP.ingest(r, IP.RGB) for r in raw]
    sc = dict(w=w, h=h, raw_l=raw, grey_l=grey, fmt_l=(3, IP.RGB, (None, None)))
    if kind == "rgbd":
        yy, xx = np.mgrid[0:h, 0:w]
        metres = 4.0 + 1.5 * np.sin(xx / 70.0) + 0.8 * np.cos(yy / 55.0)
        d16 = np.clip(np.rint(metres * 5000.0), 0, 65535).astype(np.uint16)
        d16[(xx // 40 + yy // 40) % 7 == 0] = 0          # holes of the sensor
        sc.update(depth_raw=d16, depth_m=IP.true_depth(d16, 5000.0), factor=5000.0)
    return sc


@pytest.mark.parametrize("kind", ["mono", "stereo", "rgbd"])
def test_tracker_on_raw_frames_equals_tracker_on_restated_images(kind):
    """svgpu_tracker_set_ingest + raw frames against a second tracker fed the restatement's grey (and float depth) images: observation, matches,
    outlier flags and pose bytes are equal, so are the host synchronisations; one more launch per ingested image and one for the depth."""
    from stella_vslam_amd import camera, data, feature, ingest, match, tracking
    from stella_vslam_amd import synthetic
    sc = _scene(kind)
    w, h = sc["w"], sc["h"]
    stereo, rgbd = kind == "stereo", kind == "rgbd"
    ext = feature.orb_extractor(feature.orb_params())
    ext_r = feature.orb_extractor(feature.orb_params()) if stereo else None
    ctx = ext.ctx
    fx = fy = 458.654
    cx, cy = w / 2 - 8.5, h / 2 + 8.375
    bl = 0.11
    fxb = 0.0 if kind == "mono" else fx * bl
    dist = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0) if kind == "mono" else (0, 0, 0, 0, 0)
    setup = {"mono": "Monocular", "stereo": "Stereo", "rgbd": "RGBD"}[kind]
    cam = camera.perspective("t", setup, "RGB", w, h, 30.0, fx, fy, cx, cy, *dist, focal_x_baseline=fxb, ctx=ctx)
    T = synthetic.orb_tables(1.2, 8)
    # the last frame and the map, the usual way, from the restatement's images
    k0, d0 = ext.extract(sc["grey_l"][0])
    rf_last = data.resident_frame(ctx)
    und0, _ = rf_last.adopt_extraction(cam, 64, 48)
    if stereo:
        k0r, d0r = ext_r.extract(sc["grey_r"][0])
        xr0, dp0 = match.stereo(ext, ext_r, k0, k0r, d0, d0r, fxb, bl).compute()
        rf_last.set_stereo(xr0)
        assert (xr0 >= 0).sum() > 300
    elif rgbd:
        dp0 = sc["depth_m"][k0["y"].astype(np.int32), k0["x"].astype(np.int32)]
        dp0 = np.where(dp0 > 0, dp0, np.float32(-1))
        xr0 = np.where(dp0 > 0, (und0["x"].astype(np.float64) - fxb / np.where(dp0 > 0, dp0, 1).astype(np.float64)).astype(np.float32), np.float32(-1)).astype(np.float32)
        rf_last.set_stereo(xr0)
    else:
        dp0 = np.full(len(und0), 5.0, np.float32)
    Z = np.where(dp0 > 0, dp0, 5.0).astype(np.float64)
    pos = np.stack([(und0["x"] - cx) / fx * Z, (und0["y"] - cy) / fy * Z, Z], 1)
    dist0 = np.linalg.norm(pos, axis=1)
    nrm = pos / dist0[:, None]
    maxd = (dist0 * T["scale_factors"][und0["octave"]]).astype(np.float32)
    mind = (maxd * T["inv_scale_factors"][7]).astype(np.float32)
    ids = np.where(dp0 > 0, np.arange(len(und0)) * 2 + 1, -1).astype(np.int32)
    have = ids >= 0
    table = tracking.landmark_table(ctx).upsert(ids[have], tracking.landmark_records(pos[have], nrm[have], mind[have], maxd[have], d0[have]))
    mk = lambda: tracking.tracker(ctx, table, cam, T["scale_factors"], T["inv_level_sigma_sq"], T["log_scale_factor"], is_monocular=(kind == "mono"),
                                  true_baseline=0.0 if kind == "mono" else bl)
    trk_raw, trk_ref = mk(), mk()
    zbar = float(np.median(Z[have]))
    pose_last = _pose12(np.eye(3), np.zeros(3))
    guess = _pose12(np.eye(3), np.array([-3.0 * zbar / fx, -1.0 * zbar / fy, 0.0]))
    ing_l = ingest.Ingest(ctx, w, h, sc["fmt_l"][0], sc["fmt_l"][1], *sc["fmt_l"][2])
    ing_r = ingest.Ingest(ctx, w, h, sc["fmt_r"][0], sc["fmt_r"][1], *sc["fmt_r"][2]) if stereo else None
    trk_raw.set_ingest(ing_l, ing_r, ingest.DEPTH_U16 if rgbd else 0, sc.get("factor", 1.0))

    def run(trk, left, right=None, depth=None):
        cur = data.resident_frame(ctx)
        l0, s0 = trk.counters()
        if stereo:
            r = trk.track_motion_stereo(cur, rf_last, ids, guess, pose_last, 15.0, left, right, ext_r.ctx)
        elif rgbd:
            r = trk.track_motion_rgbd(cur, rf_last, ids, guess, pose_last, 15.0, left, depth)
        else:
            r = trk.track_motion(cur, rf_last, ids, guess, pose_last, 20.0, img=left)
        l1, s1 = trk.counters()
        return r, l1 - l0, s1 - s0

    # the reference tracker first: it leaves both contexts configured and warm
    ref, l_ref, s_ref = run(trk_ref, sc["grey_l"][1], sc["grey_r"][1] if stereo else None, sc.get("depth_m"))
    got, l_raw, s_raw = run(trk_raw, sc["raw_l"][1], sc["raw_r"][1] if stereo else None, sc.get("depth_raw"))
    _same_run(got, ref, stereo or rgbd)
    assert got["result"]["num_matches"] > 300 and got["result"]["num_valid"] > 150
    assert s_raw == s_ref == 1
    extra = {"mono": 1, "stereo": 2, "rgbd": 2}[kind]
    assert l_ref < l_raw <= l_ref + extra, (l_ref, l_raw)
    # padded raw rows give the same frame
    if kind == "mono":
        padded = IP.strided(sc["raw_l"][1], _odd(w * 3 + 8))
        again, _, _ = run(trk_raw, padded)
        _same_run(again, ref, False)
    # switched off again, the tracker reads grey as before -- and a tracker that never heard of ingest did so all along (trk_ref)
    trk_raw.set_ingest(None, None, 0, 1.0)
    back, l_back, s_back = run(trk_raw, sc["grey_l"][1], sc["grey_r"][1] if stereo else None, sc.get("depth_m"))
    _same_run(back, ref, stereo or rgbd)
    assert l_back == l_ref and s_back == 1


def test_refusals_launch_nothing(ctx):
    """geometry that does not match the configured extractor, channels outside {1, 3, 4}, Gray with colour channels, one map without the other, a
    stride below a row, a stereo pair of different geometry: status 1, and neither the profiler nor the tracker counts a launch"""
    from stella_vslam_amd import camera, data, feature, ingest, synthetic, tracking
    from stella_vslam_amd._lib import lib
    L = lib()
    w, h = 640, 480
    assert L.svgpu_profile_select(ctx.handle, b"k_ingest_gray") == 0
    hnd = C.c_void_p()
    mx, my = IP.make_maps("identity", w, h)
    pmx = C.c_void_p(mx.ctypes.data)
    for args in ((w, h, 2, IP.RGB, None, None, 0), (w, h, 5, IP.RGB, None, None, 0), (w, h, 0, IP.GRAY, None, None, 0), (w, h, 3, IP.GRAY, None, None, 0),
                 (w, h, 4, IP.GRAY, None, None, 0), (w, h, 3, 3, None, None, 0), (0, h, 1, IP.GRAY, None, None, 0), (w, h, 3, IP.RGB, pmx, None, w * 4),
                 (w, h, 3, IP.RGB, None, pmx, w * 4), (w, h, 3, IP.RGB, pmx, pmx, w * 4 - 4)):
        assert L.svgpu_ingest_create(ctx.handle, *args, C.byref(hnd)) == 1 and not hnd.value, args
    ing = ingest.Ingest(ctx, w, h, 3, IP.RGB, mx, my)
    raw = IP.noise_image(w, h, 3, 1)
    out = np.zeros((h, w), np.uint8)
    p_raw, p_out = C.c_void_p(raw.ctypes.data), C.c_void_p(out.ctypes.data)
    assert L.svgpu_ingest_gray(ctx.handle, ing._h, p_raw, w * 3 - 1, p_out, w) == 1
    assert L.svgpu_ingest_gray(ctx.handle, ing._h, p_raw, w * 3, p_out, w - 1) == 1
    assert L.svgpu_ingest_gray(ctx.handle, ing._h, None, w * 3, p_out, w) == 1
    assert L.svgpu_ingest_gray(ctx.handle, None, p_raw, w * 3, p_out, w) == 1
    assert L.svgpu_ingest_gray_batch_device(ctx.handle, ing._h, p_raw, 2, h * w * 3, w * 3 - 1, p_out, h * w, w, None) == 1
    assert L.svgpu_ingest_gray_batch_device(ctx.handle, ing._h, p_raw, 2, h * w * 3, w * 3, p_out, h * w, w - 1, None) == 1
    assert L.svgpu_ingest_gray_batch_device(ctx.handle, ing._h, p_raw, 2, h * w * 3 - 7, w * 3, p_out, h * w, w, None) == 1
    assert L.svgpu_ingest_gray_batch_device(ctx.handle, ing._h, p_raw, -1, h * w * 3, w * 3, p_out, h * w, w, None) == 1
    f32 = np.zeros((h, w), np.float32)
    pf = C.c_void_p(f32.ctypes.data)
    for args in ((pf, 3, w * 4, w, h, 5000.0, pf, w * 4), (pf, IP.DEPTH_U16, w * 2 - 2, w, h, 5000.0, pf, w * 4), (pf, IP.DEPTH_F32, w * 4, w, h, 5000.0, pf, w * 4 - 4),
                 (pf, IP.DEPTH_U16, w * 2, w, h, 0.0, pf, w * 4), (pf, IP.DEPTH_U16, w * 2, w, h, float("nan"), pf, w * 4), (None, IP.DEPTH_U16, w * 2, w, h, 1.0, pf, w * 4)):
        assert L.svgpu_ingest_depth(ctx.handle, *args) == 1, args
    assert not out.any() and not f32.any()
    ms, n = C.c_double(0), C.c_longlong(0)
    assert L.svgpu_profile_read(ctx.handle, C.byref(ms), C.byref(n)) == 0 and n.value == 0
    ing.gray(raw)                                          # (the counter does count: one launch)
    assert L.svgpu_profile_read(ctx.handle, C.byref(ms), C.byref(n)) == 0 and n.value == 1
    assert L.svgpu_profile_select(ctx.handle, None) == 0

    # the tracker: an ingest of another geometry, a pair that disagrees, a raw stride below a row
    ext = feature.orb_extractor(feature.orb_params())
    tctx = ext.ctx
    imgs = synthetic.frame_sequence(1, w, h, seed=2)
    k0, d0 = ext.extract(imgs[0])
    cam = camera.perspective("t", "Monocular", "RGB", w, h, 30.0, 450.0, 450.0, 320.0, 240.0, 0, 0, 0, 0, 0, ctx=tctx)
    T = synthetic.orb_tables(1.2, 8)
    rf_last = data.resident_frame(tctx)
    und0, _ = rf_last.adopt_extraction(cam, 64, 48)
    pos = np.stack([(und0["x"] - 320.0) / 450.0 * 5, (und0["y"] - 240.0) / 450.0 * 5, np.full(len(und0), 5.0)], 1).astype(np.float64)
    nrm = pos / np.linalg.norm(pos, axis=1, keepdims=True)
    maxd = (np.linalg.norm(pos, axis=1) * T["scale_factors"][und0["octave"]]).astype(np.float32)
    ids = np.arange(len(und0), dtype=np.int32)
    table = tracking.landmark_table(tctx).upsert(ids, tracking.landmark_records(pos, nrm, (maxd * T["inv_scale_factors"][7]).astype(np.float32), maxd, d0))
    trk = tracking.tracker(tctx, table, cam, T["scale_factors"], T["inv_level_sigma_sq"], T["log_scale_factor"])
    small = ingest.Ingest(tctx, 320, 240, 3, IP.RGB)
    good = ingest.Ingest(tctx, w, h, 3, IP.RGB)
    base = trk.counters()
    assert L.svgpu_tracker_set_ingest(trk._h, small._h, None, 0, 1.0) == 1          # not the configured extractor's geometry
    assert L.svgpu_tracker_set_ingest(trk._h, good._h, small._h, 0, 1.0) == 1       # a pair with different output geometry
    assert L.svgpu_tracker_set_ingest(trk._h, good._h, None, 3, 1.0) == 1           # unknown depth type
    assert L.svgpu_tracker_set_ingest(trk._h, good._h, None, IP.DEPTH_U16, 0.0) == 1
    trk.set_ingest(good)
    pose = _pose12(np.eye(3), np.zeros(3))
    cur = data.resident_frame(tctx)
    match, outl = np.full(len(ids), -1, np.int32), np.zeros(ext.max_keypoints(), np.uint8)
    res = tracking._TrackResult()
    vp = lambda a: C.c_void_p(a.ctypes.data)
    rc = lib().svgpu_track_motion(trk._h, cur._h, vp(raw), w * 3 - 1, rf_last._h, vp(ids), vp(pose), vp(pose), C.c_float(20.0), 1, None, None, None, None,
                                  len(outl), vp(match), vp(outl), C.byref(res))
    assert rc == 1 and trk.counters() == base
    # an extractor reconfigured to another geometry behind the tracker's back is caught per call
    ext._configure(752, 480)
    rc = lib().svgpu_track_motion(trk._h, cur._h, vp(raw), w * 3, rf_last._h, vp(ids), vp(pose), vp(pose), C.c_float(20.0), 1, None, None, None, None,
                                  len(outl), vp(match), vp(outl), C.byref(res))
    assert rc == 1 and trk.counters() == base


def test_host_adaptor_program():
    exe = ROOT / "stella_vslam_amd" / "host" / "test_ingest"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(exe.parent)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ingest ok" in out.stdout
