"""The staged call (csrc/sv_staged_call.h) owns the regrowth of the scratch arena and of its page-locked mirror.  On ONE context two cheap
entry points are called small -> large -> small, the large call past the 1 MiB scratch granule and the first stage buffer, so both buffers
are replaced between calls; every output has to be bit-equal to the same call made on a fresh context.  Then the zero-filled mirror
path of svgpu_match_bruteforce (no angle arrays: the rows are written in the mirror, not uploaded) against the oracle."""
import numpy as np
import pytest

from tests import pnp_problems as PNP
from tests import posegraph_problems as PG

pytestmark = pytest.mark.gpu


def _context():
    from stella_vslam_amd.feature import Context
    return Context()


def _same_on_fresh_contexts(call, problems):
    shared = _context()
    for k, p in enumerate(problems):
        got, exp = call(shared, p), call(_context(), p)
        for g, e in zip(got, exp):
            assert g.shape == e.shape and g.tobytes() == e.tobytes(), f"call {k}"


def test_landmark_correction_small_large_small():
    from stella_vslam_amd import optimize
    before = np.stack([PG.make_sim3([0.1, -0.2, 0.3], [1.0, 2.0, 3.0], 1.0), PG.make_sim3([-0.3, 0.1, 0.2], [-2.0, 0.5, 1.0], 1.5)])
    after = np.stack([before[0], PG.make_sim3([-0.25, 0.15, 0.2], [-2.1, 0.4, 1.2], 1.4)])

    def problem(L):  # about 52 bytes of arena per landmark: 40 000 of them take some 2 MB
        rng = np.random.default_rng(L)
        return rng.integers(0, 2, size=L).astype(np.int32), rng.normal(size=(L, 3)) * 10.0

    def call(ctx, p):
        return (optimize.correct_landmarks(ctx, before, after, p[0], p[1]),)

    problems = [problem(1), problem(40000), problem(1)]
    _same_on_fresh_contexts(call, problems)
    ref, pos = problems[1]  # and the large call computes what numpy computes
    out = call(_context(), problems[1])[0]
    exp = PG.correct_landmarks(before.astype(np.longdouble), after.astype(np.longdouble), ref, pos.astype(np.longdouble))
    assert float((np.abs(out - exp).max(1) / np.maximum(1.0, np.abs(exp).max(1))).max()) <= 1e-12


def test_pnp_pose_small_large_small():
    from stella_vslam_amd import solve
    one = [PNP.planted(7, 4, "pinhole")]
    many = [PNP.planted(100 + s, 12, PNP.KINDS[s % 4], noise=1e-3) for s in range(2000)]

    def call(ctx, sets):
        off, brg, pw, _ = PNP.concatenate(sets)
        return solve.compute_pose(ctx, brg, pw, off)

    _same_on_fresh_contexts(call, [one, many, one])


def test_bruteforce_without_angle_arrays_against_the_oracle():
    from oracle import oracle as O
    from stella_vslam_amd import match
    rng = np.random.default_rng(5)
    n = 64
    d1 = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    d2 = d1[rng.permutation(n)].copy()
    flips = rng.integers(0, 256, size=(n, 3))  # three flipped bits per descriptor: unambiguous nearest neighbours
    for i in range(n):
        for b in flips[i]:
            d2[i, b // 8] ^= np.uint8(1 << (b % 8))
    pairs, out = match.robust(0.8, False, _context()).brute_force_match(d1, None, d2, None)
    zeros = np.zeros(n, np.float32)
    exp = O.brute_force_match(d1, zeros, d2, zeros, None, 0.8, False)
    assert np.array_equal(out, exp)
    assert len(pairs) == int((exp >= 0).sum()) > n // 2
