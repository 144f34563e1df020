"""Host side of the rescale: rescale_taps against the independent weight matrices of rescale_ref, the reference's own
properties (pool2 at step 2, identity, constants, the 32-bit bound, flips, scipy's zoom where installed), the slabs of
rescale_chunks, and the argument checks of volume_rescale that are made before any GPU work.  No GPU is needed."""
from fractions import Fraction

import numpy as np
import pytest

import rescale_ref as R
from transfer_em_amd.utils import (HIST_CHUNK_BYTES, rescale_chunks, rescale_shape, rescale_step, rescale_taps,
                                   volume_rescale)

AREA = [(1, 1), (2, 1), (3, 2), (5, 4), (7, 3), (8, 1), (64, 63)]
LINEAR = [(1, 2), (2, 3), (1, 5), (1, 8), (63, 64)]
EXTENTS = (1, 2, 7, 64, 65)
ids = lambda steps: [f"{p}_{q}" for p, q in steps]


def _matrix(taps, n):
    M = np.zeros((len(taps), n), np.int64)
    for j, (first, w, W) in enumerate(taps):
        assert 0 <= first and first + len(w) <= n and W == sum(w) and all(v > 0 for v in w), (j, first, w, W)
        M[j, first:first + len(w)] = w
    return M


# --------------------------------------------------------------------------------------------------------- rescale_taps
@pytest.mark.parametrize("p,q", AREA + LINEAR, ids=ids(AREA + LINEAR))
def test_taps_are_the_reference_matrix(p, q):
    for n in EXTENTS:
        taps = rescale_taps(n, p, q)
        M, W = R.axis_matrix(n, p, q)
        assert len(taps) == R.grid(n, p, q) == -(-n * q // p)
        assert np.array_equal(_matrix(taps, n), M), n
        assert [t[2] for t in taps] == list(W), n


@pytest.mark.parametrize("p,q", AREA, ids=ids(AREA))
def test_area_weights_are_a_partition_of_unity(p, q):
    for n in EXTENTS:
        taps = rescale_taps(n, p, q)
        M = _matrix(taps, n)                                             # asserts positive weights inside [0, n)
        assert (M.sum(axis=0) == q).all()                                # every source voxel is spent exactly once
        assert all(len(w) <= -(-p // q) + 1 for _, w, _ in taps)
        full = [W == p for _, _, W in taps]
        assert all(full[:-1]) and (full[-1] or (n * q) % p)              # a reduced denominator only at the far face
        assert taps[-1][2] == (n * q - 1) % p + 1


@pytest.mark.parametrize("p,q", LINEAR, ids=ids(LINEAR))
def test_linear_weights_sum_to_2q_with_clamped_indices(p, q):
    for n in EXTENTS:
        taps = rescale_taps(n, p, q)
        _matrix(taps, n)                                                 # asserts indices inside [0, n)
        assert all(W == 2 * q and sum(w) == 2 * q and len(w) <= 2 for _, w, W in taps)
        assert taps[0][0] == 0 and taps[-1][0] + len(taps[-1][1]) == n   # both faces are reached
        assert taps[0][1] == (2 * q,) and (n > 1 or taps[-1][1] == (2 * q,))     # clamped onto the first voxel


def test_taps_refuse_what_the_kernel_refuses():
    for n, p, q in ((0, 2, 1), (5, 0, 1), (5, 1, 0), (5, 65, 64), (5, 9, 1), (5, 1, 9), (5, 4, 2), (5, -2, 1)):
        with pytest.raises(ValueError):
            rescale_taps(n, p, q)


# -------------------------------------------------------------------------------------------- the reference's properties
def _vol(shape, seed=90):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def test_reference_step_2_is_pool2_and_step_1_the_identity():
    for shape in ((5, 7, 9), (4, 6, 8), (1, 1, 1), (3, 8, 5)):
        v = _vol(shape)
        assert np.array_equal(R.reference(v, ((2, 1),) * 3), R.pool2(v)), shape
        assert np.array_equal(R.reference(v, ((1, 1),) * 3), v), shape


def test_reference_integer_factors_are_rounded_block_means():
    v = _vol((6, 9, 8))
    got = R.reference(v, ((3, 1), (3, 1), (4, 1)))
    mean = v.reshape(2, 3, 3, 3, 2, 4).astype(np.float64).mean(axis=(1, 3, 5))
    assert np.array_equal(got, np.floor(mean + 0.5).astype(np.uint8))


@pytest.mark.parametrize("p,q", [(63, 64), (64, 63), (8, 1), (1, 8), (7, 3)], ids=ids([(63, 64), (64, 63), (8, 1), (1, 8), (7, 3)]))
def test_reference_keeps_a_constant_and_stays_below_2_31(p, q):
    for value in (255, 1, 0):
        v = np.full((3, 3, 70), value, np.uint8)
        S, den = R.sums(v, ((p, q),) * 3)
        assert (2 * S + den).max() < 2 ** 31 and den.max() <= 128 ** 3
        assert (R.reference(v, ((p, q),) * 3) == value).all()
    if (p, q) == (63, 64):
        assert (2 * S + den).max() == 128 ** 3                           # value 0: Den alone; 255: 511 x 128^3
        S, den = R.sums(np.full((3, 3, 70), 255, np.uint8), ((p, q),) * 3)
        assert (2 * S + den).max() == 511 * 128 ** 3 == 1071644672


def test_reference_commutes_with_flips():
    """Where the step divides the extent (n q a multiple of p) the grid is symmetric, and so is the rule."""
    steps, shape = ((2, 1), (3, 2), (2, 3)), (8, 9, 6)
    v = _vol(shape)
    want = R.reference(v, steps)
    assert want.shape == (4, 6, 9)
    for ax in range(3):
        assert np.array_equal(R.reference(np.flip(v, ax), steps), np.flip(want, ax)), ax


@pytest.mark.parametrize("p,q", [(1, 2), (1, 3), (1, 5), (2, 3)], ids=ids([(1, 2), (1, 3), (1, 5), (2, 3)]))
def test_reference_growing_is_scipy_zoom_before_rounding(p, q):
    """The bar is half a grey level, the rounding, plus 1e-9 for zoom's float64 weights."""
    ndimage = pytest.importorskip("scipy.ndimage")
    v = _vol((4, 6, 8), 91)
    z = ndimage.zoom(v.astype(np.float64), q / p, order=1, mode="nearest", grid_mode=True)
    got = R.reference(v, ((p, q),) * 3)
    assert got.shape == z.shape
    assert np.abs(got.astype(np.float64) - z).max() <= 0.5 + 1e-9
    S, den = R.sums(v, ((p, q),) * 3)
    assert np.abs(S / den - z).max() <= 1e-9                             # before rounding: the same number


# -------------------------------------------------------------------------------------------------------- rescale_chunks
VOL = (40, 50, 60)
STEPS = [(2, 2, 2), (Fraction(3, 2),) * 3, (2, 2, Fraction(1, 5)), (Fraction(1, 2), (7, 3), 1), ((1, 8), 8, (64, 63))]


def _pq(step):
    return tuple((Fraction(*s) if isinstance(s, tuple) else Fraction(s)) for s in reversed(step))     # (z, y, x)


def _check_slabs(chunks, box, vol, step, budget):
    """Disjoint cover, tight hulls with every tap inside, the budget; returns (z-cut slabs, y-cut slabs)."""
    fz, fy, fx = _pq(step)
    seen = np.zeros(tuple(hi for _, hi in box), np.int32)
    ycut = 0
    for out, read in chunks:
        (z0, z1), (y0, y1), (x0, x1) = out
        assert (x0, x1) == box[2] and read[2] == (0, vol[2])             # x is never cut; the read has the whole row
        seen[z0:z1, y0:y1, x0:x1] += 1
        assert read[0] == R.hull(z0, z1, vol[0], fz.numerator, fz.denominator)       # tight on both ends
        assert read[1] == R.hull(y0, y1, vol[1], fy.numerator, fy.denominator)
        nbytes = [int(np.prod([hi - lo for lo, hi in b])) for b in (out, read)]
        one_row = z1 - z0 == 1 and y1 - y0 == 1
        assert max(nbytes) <= budget or one_row, (out, read, nbytes)
        if (y0, y1) != box[1]:
            assert z1 - z0 == 1
            ycut += 1
    inside = seen[tuple(slice(lo, hi) for lo, hi in box)]
    assert (inside == 1).all() and seen.sum() == inside.size             # disjoint, and their union is the box
    return len(chunks) - ycut, ycut


@pytest.mark.parametrize("step", STEPS, ids=[str(i) for i in range(len(STEPS))])
def test_chunks_cover_the_box_with_tight_hulls(step):
    grid = rescale_shape(VOL, step)
    whole = tuple((0, n) for n in grid)
    inner = tuple((n // 4, n - n // 5) for n in grid)
    plane = max(grid[1] * grid[2], VOL[1] * VOL[2])
    for box in (whole, inner):
        assert len(rescale_chunks(box, VOL, step)) == 1                  # the default budget holds it all
        for budget, cuts_y in ((9 * plane + 7, False), (plane // 3, True), (7, True)):
            chunks = rescale_chunks(box, VOL, step, budget)
            zcut, ycut = _check_slabs(chunks, box, VOL, step, budget)
            assert (ycut > 0) == cuts_y and (cuts_y or zcut > 1), (box, budget, zcut, ycut)
            if budget == 7:                                              # under a row's bytes: one row per slab
                assert len(chunks) == (box[0][1] - box[0][0]) * (box[1][1] - box[1][0])
            parts = [rescale_chunks(box, VOL, step, budget, r, 3) for r in range(3)]
            assert [c for k in range(len(chunks)) for c in parts[k % 3][k // 3:k // 3 + 1]] == chunks   # round-robin


def test_chunks_refuse_bad_arguments():
    box = ((0, 20), (0, 25), (0, 30))
    assert rescale_chunks(((3, 3), (0, 25), (0, 30)), VOL, 2) == []
    assert rescale_chunks(box, VOL, 2, None) == rescale_chunks(box, VOL, (2, 2, 2), HIST_CHUNK_BYTES)
    for kw in (dict(chunk_bytes=0), dict(rank=2, world_size=2), dict(rank=-1)):
        with pytest.raises(ValueError):
            rescale_chunks(box, VOL, 2, **kw)
    with pytest.raises(ValueError, match="outside the output grid"):
        rescale_chunks(((0, 21), (0, 25), (0, 30)), VOL, 2)
    with pytest.raises(ValueError):
        rescale_chunks(box, VOL, (2, 2))


# ------------------------------------------------------------------------------------------------- steps, shapes, checks
def test_rescale_step_and_shape():
    assert rescale_step((4, 4, 40), (8, 8, 8)) == (2, 2, Fraction(1, 5))
    assert all(isinstance(f, Fraction) for f in rescale_step((4, 4, 40), (8, 8, 8)))
    assert rescale_step((8, 8), (12, 4)) == (Fraction(3, 2), Fraction(1, 2))
    assert rescale_step((Fraction(7, 2), 4, 4), (4, 4, 4)) == (Fraction(8, 7), 1, 1)
    for src, dst in (((4, 4, 40), (8, 8)), ((4, 4, 100), (8, 8, 8)), ((0, 4, 4), (8, 8, 8)), ((4, 4, 4), (8, 8, 0)),
                     ((4,), (8,)), ((127, 1, 1), (128, 1, 1))):
        with pytest.raises(ValueError):
            rescale_step(src, dst)
    assert rescale_shape((40, 50, 60), (2, 2, Fraction(1, 5))) == (200, 25, 30)
    assert rescale_shape((40, 51, 61), ((3, 2), 2, 1)) == (40, 26, 41)   # step in (x, y, z), shape in [z, y, x]
    assert rescale_shape((51, 61), ((3, 2), 2)) == (26, 41)
    assert rescale_shape((5, 6, 7), 2) == (3, 3, 4) and rescale_shape((5, 6, 7), Fraction(1, 2)) == (10, 12, 14)


BAD_STEPS = [(2, 2), (2, 2, 2, 2), (2, 2, 0), (2, 2, -1), (2, 2, 9), (2, 2, Fraction(1, 9)), (2, 2, (65, 64)), (2, 2, 1.5),
             (2, 2, (1, 0)), (2, 2, (1, 2, 3)), (2, 2, "2"), (2, 2, None), None, "2", 1.5, (2, 2, True)]


def test_volume_rescale_checks_come_before_the_gpu(monkeypatch):
    """Every ValueError is raised before H.require_gpu(), which is made to fail loudly here."""
    from transfer_em_amd import hip_ops

    def no_gpu():
        raise AssertionError("require_gpu was reached")
    monkeypatch.setattr(hip_ops, "require_gpu", no_gpu)
    v = np.zeros((8, 9, 10), np.uint8)
    for bad in (v.astype(np.float32), v.astype(np.int8), v.astype(np.uint16)):
        with pytest.raises(ValueError, match="uint8"):
            volume_rescale(bad, 2)
    for step in BAD_STEPS:
        with pytest.raises(ValueError):
            volume_rescale(v, step)
    with pytest.raises(ValueError):
        volume_rescale(v[0], (2, 2, 2))                                  # one image takes a 2-element step
    with pytest.raises(ValueError):
        volume_rescale(np.zeros((2, 3, 4, 5), np.uint8), 2)
    # the grid of v at step 2 is (4, 5, 5); start / size are (x, y, z)
    for start, size in (((0, 0, 0), (6, 5, 4)), ((0, 0, 1), (5, 5, 4)), ((-1, 0, 0), (2, 2, 2)), ((0, 0), (2, 2)),
                        ((0, 0, 0), (5, -1, 4)), ((0, 0, 0), (10, 9, 8))):
        with pytest.raises(ValueError, match="output grid"):
            volume_rescale(v, 2, start=start, size=size)
    for out in (np.zeros((4, 5, 6), np.uint8), np.zeros((5, 5), np.uint8), np.zeros((4, 5, 5), np.float32),
                np.zeros((8, 9, 10), np.uint8)):
        with pytest.raises(ValueError, match="out must be uint8"):
            volume_rescale(v, 2, out=out)
    with pytest.raises(ValueError, match="out must be uint8"):
        volume_rescale(v, 2, out=np.zeros((4, 5, 5), np.uint8), start=(1, 0, 0), size=(4, 5, 4))
    with pytest.raises(ValueError):
        volume_rescale(v, 2, chunk_bytes=0)
    with pytest.raises(ValueError):
        volume_rescale(v, 2, rank=1, world_size=1)
    with pytest.raises(AssertionError, match="require_gpu was reached"):  # a good call gets as far as the GPU
        volume_rescale(v, (2, (3, 2), Fraction(1, 2)))
