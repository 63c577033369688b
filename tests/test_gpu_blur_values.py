"""Value range and tap placement of the blur's horizontal pass (blur_hpair: byte dot products of the 12-byte window with shifted taps).

tests/test_gpu_blur_bands.py and tests/test_gpu_orb*.py cover the geometry of the blur kernels on natural-looking frames.  This file paints
the images the horizontal pass can get wrong without those noticing: saturated sums (all 255 -> 65 280 in a 16-bit half), hard edges,
stripes, and single impulses, whose response is the tap table itself -- at the image's left and right borders (reflect-101), around a
320-pixel segment boundary and around a 48-row band boundary.  Every case runs through the streaming kernel (max_batch = 1) and the band
kernel (max_batch = BLUR_SMALL_BATCH + 1) and is compared level by level with oracle.gaussian_blur7 of the device's own pyramid: level 0
is the painted image, the higher levels are whatever the pyramid makes of it.

The CPU tests restate the horizontal pass in numpy from the ten tap dwords and compare it with the seven-tap sum.
"""
import numpy as np
import pytest

from oracle import oracle as O

TAPS = (18, 34, 48, 56, 48, 34, 18)
BLUR_SMALL_BATCH = 4  # stella_vslam_amd/csrc/orb_plan.h (tests/test_gpu_blur_bands.py checks the mirror against the header)
SIZES = [(96, 64), (331, 250)]  # one band, one segment; all four w % 4 classes over the levels, a segment boundary at 320, a ragged last band

# The one place the tap dwords live on the Python side: TAP_DWORDS[j] = (x w0, x w1, x w2) for owned pixel j of the window w0 | w1 | w2, where
# byte k of a word sits at bits 8 k and w0 holds pixels x0 - 4 .. x0 - 1.  Written out, so that they pin what blur_tap_word() derives in
# stella_vslam_amd/csrc/orb_kernels.hip; two of the twelve are empty, ten dot products remain.
TAP_DWORDS = (
    (0x30221200, 0x12223038, 0x00000000),
    (0x22120000, 0x22303830, 0x00000012),
    (0x12000000, 0x30383022, 0x00001222),
    (0x00000000, 0x38302212, 0x00122230),
)


# ------------------------------------------------------------------------------------------------ CPU: the tap table
def _dot4(word, taps):
    """v_dot4_u32_u8: the four bytes of `word` (array of u32) times the four bytes of `taps`, summed."""
    word = word.astype(np.uint64)
    return sum(((word >> (8 * k)) & 255) * ((taps >> (8 * k)) & 255) for k in range(4))


def _hsums_by_dwords(row):
    """The horizontal pass as the kernels do it: for every aligned group x0 of an (already bordered) row, the sums of pixels x0 .. x0 + 3
    from the three window words.  `row` holds pixels -4 .. n + 3 of a row of n pixels, n a multiple of 4.  Returns the n sums."""
    words = np.ascontiguousarray(row, np.uint8).view("<u4")  # word i = pixels 4 i - 4 .. 4 i - 1
    w0, w1, w2 = words[:-2], words[1:-1], words[2:]
    out = np.zeros((len(w0), 4), np.uint64)
    for j in range(4):
        t0, t1, t2 = TAP_DWORDS[j]
        out[:, j] = _dot4(w0, t0) + _dot4(w1, t1) + _dot4(w2, t2)
    return out.reshape(-1)


def _hsums_by_taps(row):
    r = row.astype(np.uint64)
    n = len(row) - 8
    return sum(TAPS[t] * r[1 + t: 1 + t + n] for t in range(7))  # pixel x is row[4 + x]; taps over x - 3 .. x + 3


def test_ten_tap_dwords_follow_from_the_taps():
    """Byte i of the window is pixel x0 - 4 + i and tap t of owned pixel j multiplies pixel x0 + j - 3 + t: byte i carries tap i - j - 1."""
    nonzero = 0
    for j in range(4):
        for word in range(3):
            want = 0
            for k in range(4):
                t = 4 * word + k - j - 1
                if 0 <= t < 7:
                    want |= TAPS[t] << (8 * k)
            assert TAP_DWORDS[j][word] == want, (j, word, hex(want))
            nonzero += want != 0
    assert nonzero == 10 and sum(TAPS) == 256


@pytest.mark.parametrize("what", ["random", "all255", "impulse"])
def test_dword_restatement_equals_the_seven_tap_sum(what):
    n = 64
    if what == "random":
        row = np.random.default_rng(7).integers(0, 256, n + 8, dtype=np.uint8)
    elif what == "all255":
        row = np.full(n + 8, 255, np.uint8)
    else:
        row = np.zeros(n + 8, np.uint8)
        row[4 + 29] = 255  # pixel 29: every owned column j = 0 .. 3 of the groups around it sees it at another window byte
    got, want = _hsums_by_dwords(row), _hsums_by_taps(row)
    assert np.array_equal(got, want)
    assert int(want.max()) <= 65280
    if what == "all255":
        assert np.all(got == 65280)  # the largest value a 16-bit half carries
    if what == "impulse":
        assert [int(v) for v in got[26:33]] == [255 * t for t in TAPS] and got[:26].sum() == 0 and got[33:].sum() == 0


# ------------------------------------------------------------------------------------------------ GPU: painted images
@pytest.fixture(scope="module")
def extractors():
    """One extractor per kernel: the streaming kernel (contexts of at most BLUR_SMALL_BATCH frames) and the band kernel."""
    from stella_vslam_amd import feature as F
    return {"stream": F.orb_extractor(F.orb_params(), max_batch=1), "band": F.orb_extractor(F.orb_params(), max_batch=BLUR_SMALL_BATCH + 1)}


def _check(extractors, kernel, img, what):
    ext = extractors[kernel]
    ext.extract(img)
    pyr = ext.image_pyramid_
    assert np.array_equal(pyr[0], img), f"{what}: level 0 is the painted image"
    for l, a in enumerate(ext.blurred_pyramid()):
        want = O.gaussian_blur7(pyr[l])
        if not np.array_equal(a, want):
            ys, xs = np.nonzero(a != want)
            raise AssertionError(f"{kernel} {what}: blurred level {l} ({a.shape[1]}x{a.shape[0]}): {len(ys)} bytes differ, first at x={xs[0]} y={ys[0]}: "
                                 f"{a[ys[0], xs[0]]} != {want[ys[0], xs[0]]}")


def _extremes(w, h):
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    return {"all255": np.full((h, w), 255, np.uint8), "all0": np.zeros((h, w), np.uint8),
            "left0_right255": np.where(x < w // 2, 0, 255).astype(np.uint8), "top0_bottom255": np.where(y < h // 2, 0, 255).astype(np.uint8)}


def _stripes(w, h):
    """Period 2: 0, 255, 0, 255, ...  Period 7 (the length of the filter): four columns of 255, three of 0."""
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    return {"columns_period2": np.where(x % 2 == 1, 255, 0).astype(np.uint8), "columns_period7": np.where(x % 7 < 4, 255, 0).astype(np.uint8),
            "rows_period2": np.where(y % 2 == 1, 255, 0).astype(np.uint8), "rows_period7": np.where(y % 7 < 4, 255, 0).astype(np.uint8)}


def _impulse_positions(w, h):
    xs = list(range(8)) + list(range(w - 4, w)) + [x for x in (319, 320, 321) if x < w]
    ys = [0, 3, 47, 48, h - 1]
    return [(x, y) for x in xs for y in ys]


def _impulse_images(w, h, background, value):
    """Every impulse of _impulse_positions once; impulses share an image only when they are more than 7 px apart in x AND in y."""
    images = []  # (positions, image)
    for x, y in _impulse_positions(w, h):
        for pos, img in images:
            if all(abs(x - px) > 7 and abs(y - py) > 7 for px, py in pos):
                break
        else:
            pos, img = [], np.full((h, w), background, np.uint8)
            images.append((pos, img))
        pos.append((x, y))
        img[y, x] = value
    return images


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["stream", "band"])
@pytest.mark.parametrize("w,h", SIZES)
def test_extremes(extractors, kernel, w, h):
    for name, img in _extremes(w, h).items():
        _check(extractors, kernel, img, f"{w}x{h} {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["stream", "band"])
@pytest.mark.parametrize("w,h", SIZES)
def test_stripes(extractors, kernel, w, h):
    for name, img in _stripes(w, h).items():
        _check(extractors, kernel, img, f"{w}x{h} {name}")


def test_impulse_images_hold_every_position_once():
    for w, h in SIZES:
        images = _impulse_images(w, h, 0, 255)
        placed = sorted(p for pos, _ in images for p in pos)
        assert placed == sorted(_impulse_positions(w, h)) and len(set(placed)) == len(placed)
        assert sum(int((img == 255).sum()) for _, img in images) == len(placed)
        assert (319, 47) in placed if w > 321 else all(x < 8 or x >= w - 4 for x, _ in placed)


@pytest.mark.gpu
@pytest.mark.parametrize("background,value", [(0, 255), (255, 0)], ids=["255_on_black", "0_on_white"])
@pytest.mark.parametrize("kernel", ["stream", "band"])
@pytest.mark.parametrize("w,h", SIZES)
def test_impulses(extractors, kernel, w, h, background, value):
    for pos, img in _impulse_images(w, h, background, value):
        _check(extractors, kernel, img, f"{w}x{h} impulses {value} on {background} at {pos}")


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["stream", "band"])
@pytest.mark.parametrize("w,h", SIZES)
def test_random_image(extractors, kernel, w, h):
    img = np.random.default_rng(1000 * w + h).integers(0, 256, (h, w), dtype=np.uint8)
    _check(extractors, kernel, img, f"{w}x{h} random")
