"""The host side of the affine alignment of sections, without a GPU: shift_subpixel, fit_section_maps, section_maps,
quantize_maps, the slab plan warp_chunks, the numpy reference warp_ref against volume_shift, every ValueError, and the
numbers of the fixture of rotated sections from the reference alone."""
import functools
import inspect

import numpy as np
import pytest

import warp_ref as WR
import zshift_ref as SR
from transfer_em_amd.utils import (HIST_CHUNK_BYTES, SectionFits, SubShifts, fit_section_maps, quantize_maps,
                                   section_maps, section_shifts, shift_counts, shift_positions, shift_scores,
                                   shift_subpixel, volume_shift, volume_warp, warp_chunks)

I23 = WR.IDENTITY
ONE, DEV = 1 << 16, 1 << 13


# --------------------------------------------------------------------------------------------------- shift_subpixel
def _sums_with_scores(c, count=100):
    """Sums q [Z, gy, gx, R, R, 5] and counts n whose shift_scores are `c` [Z - 1, gy, gx, R, R], for scores that are
    multiples of 1 / count: n = 1, S1 = T1 = 0, S2 = T2 = count, P = c count."""
    q = np.zeros((c.shape[0] + 1,) + c.shape[1:] + (5,), np.int64)
    q[:-1, ..., 1] = q[:-1, ..., 3] = count
    q[:-1, ..., 4] = np.rint(c * count).astype(np.int64)
    return q, np.ones(c.shape[1:], np.int64)


def test_subpixel_on_a_parabola_a_rim_peak_and_an_undecided_tile():
    r = 3
    dy, dx = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij")
    c = np.zeros((1, 1, 4, 7, 7))
    c[0, 0, 0] = 0.9 - 0.05 * (dy - 1) ** 2 - 0.02 * (dx + 2) ** 2 + 0.05 * (dy - 1) - 0.01 * (dx + 2)   # vertex (1.5, -2.25)
    c[0, 0, 1] = 0.9 - 0.05 * (dy - 3) ** 2 - 0.02 * dx ** 2                     # the maximum on the rim: undecided
    c[0, 0, 2] = 0.05 - 0.01 * (dy - 1) ** 2 - 0.01 * dx ** 2                    # below min_corr: undecided
    c[0, 0, 3] = np.where((dy == 2) & (dx == 0), 0.5, 0.2)                       # a lone peak: both neighbours equal
    q, n = _sums_with_scores(c)
    assert np.allclose(shift_scores(q, n), c, atol=1e-12)
    sub, s = shift_subpixel(q, n), section_shifts(q, n)
    assert isinstance(sub, SubShifts) and sub.offsets.dtype == np.float64 and sub.offsets.shape == (1, 1, 4, 2)
    assert np.array_equal(sub.decided, s.decided) and np.array_equal(sub.peak, s.peak)
    assert sub.decided[0, 0].tolist() == [True, False, False, True]
    assert s.tiles[0, 0, 0].tolist() == [1, -2]
    assert np.allclose(sub.offsets[0, 0, 0], [1.5, -2.25], atol=1e-9)           # a parabola's vertex, exactly
    assert sub.offsets[0, 0, 1].tolist() == s.tiles[0, 0, 1].tolist() == [3, 0]  # kept as integers
    assert sub.offsets[0, 0, 2].tolist() == s.tiles[0, 0, 2].tolist()
    assert sub.offsets[0, 0, 3].tolist() == [2.0, 0.0]                           # m == p: delta 0
    c[0, 0, 0] = np.where((dy == 0) & (dx == 0), 0.9, np.where((dy == 1) & (dx == 0), 0.9 - 1e-9, 0.0))
    q, n = _sums_with_scores(c, 10 ** 9)
    got = shift_subpixel(q, n).offsets[0, 0, 0]
    assert 0.499 < got[0] <= 0.5 and got[1] == 0.0                               # the vertex never leaves the half pixel
    with pytest.raises(ValueError):
        shift_subpixel(q, n, min_corr=1.5)
    with pytest.raises(ValueError):
        shift_subpixel(q[..., :4], n)


# ------------------------------------------------------------------------------------------------- fit_section_maps
SHAPE, TILE = (3, 90, 120), 32                       # 3 x 4 tiles, the last row and column partial


def _points(shape=SHAPE, tile=TILE):
    Y, X = shape[1:]
    c = lambda n: np.array([(k * tile + min((k + 1) * tile, n) - 1) / 2 for k in range(-(-n // tile))])
    return np.stack(np.meshgrid(c(Y), c(X), indexing="ij"), axis=-1)


def _offsets(maps):
    pts = _points()
    return np.stack([WR.apply(m, pts) - pts for m in maps])


MAPS = np.array([[[1.01, -0.02, 1.25], [0.015, 0.99, -2.5]], [[0.999, 0.03, -0.75], [-0.03, 1.002, 0.5]]])


def test_fit_recovers_exact_affine_offsets():
    assert _points()[2, 3].tolist() == [(64 + 90 - 1) / 2, (96 + 120 - 1) / 2]   # partial tiles: the voxels that exist
    off, dec = _offsets(MAPS), np.ones((2, 3, 4), bool)
    fit = fit_section_maps(SubShifts(off, dec, np.ones((2, 3, 4))), TILE, SHAPE)
    assert isinstance(fit, SectionFits) and fit.maps.shape == (2, 2, 3) and fit.maps.dtype == np.float64
    assert np.abs(fit.maps - MAPS).max() < 1e-9 and fit.kept.all() and fit.residual.max() < 1e-9 and fit.unresolved == []
    tr = fit_section_maps((off, dec), TILE, SHAPE, model="translation", max_residual=100.0)
    assert np.array_equal(tr.maps[:, :, :2], np.tile(np.eye(2), (2, 1, 1))) and tr.kept.all()
    assert np.allclose(tr.maps[:, :, 2], off.reshape(2, -1, 2).mean(axis=1), atol=1e-12)
    assert 1.0 < tr.residual.min() and tr.residual.max() < 3.0
    assert not fit_section_maps((off, dec), TILE, SHAPE, model="translation").kept.all()   # it does not explain them


def test_fit_drops_one_tile_of_nonsense_and_the_map_does_not_move():
    off, dec = _offsets(MAPS), np.ones((2, 3, 4), bool)
    off[0, 1, 2] += (3.0, -3.0)
    off[1, 0, 0] += (0.0, 2.5)
    fit = fit_section_maps((off, dec), TILE, SHAPE)
    want = np.ones((2, 3, 4), bool)
    want[0, 1, 2] = want[1, 0, 0] = False
    assert np.array_equal(fit.kept, want) and np.abs(fit.maps - MAPS).max() < 1e-9 and fit.residual.max() < 1e-9
    loose = fit_section_maps((off, dec), TILE, SHAPE, max_residual=10.0)           # nothing exceeds it: nothing is dropped
    assert loose.kept.all() and np.abs(loose.maps - MAPS).max() > 1e-3
    noise = np.random.default_rng(3).uniform(-4, 4, (1, 3, 4, 2))                  # stops when half are gone
    half = fit_section_maps((noise, dec[:1]), TILE, SHAPE, max_residual=1e-6)
    assert half.kept.sum() == 6 and half.residual[0] > 1e-6
    tie = np.zeros((1, 3, 4, 2))                                                   # equal residuals: the lowest index goes
    tie[0, 0, 0], tie[0, 0, 3], tie[0, 2, 0], tie[0, 2, 3] = (2, 2), (2, -2), (-2, 2), (-2, -2)
    t = fit_section_maps((tie, dec[:1]), TILE, SHAPE, model="translation", max_residual=1.9)
    assert not t.kept[0, 0, 0] and t.kept.sum() < 12


def test_fit_falls_back_to_a_translation_for_collinear_tiles_and_names_unresolved_pairs():
    off = _offsets(MAPS)
    dec = np.zeros((2, 3, 4), bool)
    dec[0, 1, :] = True                                                            # one row of tiles: rank 2
    fit = fit_section_maps((off, dec), TILE, SHAPE, max_residual=50.0)
    assert np.array_equal(fit.maps[0, :, :2], np.eye(2)) and fit.kept[0, 1].all()
    assert np.allclose(fit.maps[0, :, 2], off[0, 1].mean(axis=0), atol=1e-12)
    assert fit.unresolved == [1] and np.array_equal(fit.maps[1], I23) and fit.residual[1] == 0 and not fit.kept[1].any()
    dec[1, 2, 3] = True                                                            # a single tile: its own offset
    one = fit_section_maps((off, dec), TILE, SHAPE, max_residual=50.0)
    assert one.unresolved == [] and np.allclose(one.maps[1, :, 2], off[1, 2, 3]) and one.kept[1].sum() == 1
    assert np.array_equal(one.maps[1, :, :2], np.eye(2))
    two = np.zeros((2, 3, 4), bool)
    two[:, 0, 0] = two[:, 1, 1] = True                                             # two tiles on a diagonal
    assert np.array_equal(fit_section_maps((off, two), TILE, SHAPE, max_residual=50.0).maps[:, :, :2],
                          np.tile(np.eye(2), (2, 1, 1)))


def test_fit_refuses_bad_arguments():
    off, dec = _offsets(MAPS), np.ones((2, 3, 4), bool)
    for a, kw in ((((off[:, :2], dec), TILE, SHAPE), {}), (((off, dec[:, :2]), TILE, SHAPE), {}),
                  (((off, dec.astype(np.int8)), TILE, SHAPE), {}), (((off[..., :1], dec), TILE, SHAPE), {}),
                  (((off, dec), 16, SHAPE), {}), (((off, dec), 0, SHAPE), {}), (((off, dec), TILE, (90,)), {}),
                  (((off, dec), TILE, SHAPE), dict(model="rigid")), (((off, dec), TILE, SHAPE), dict(max_residual=0)),
                  (((off, dec), TILE, SHAPE), dict(max_residual=float("nan"))),
                  (((off, dec), TILE, SHAPE), dict(max_residual=None)), (((off.astype(str), dec), TILE, SHAPE), {})):
        with pytest.raises(ValueError):
            fit_section_maps(*a, **kw)


# ----------------------------------------------------------------------------------------------------- section_maps
def test_section_maps_compose_the_pairs():
    rng = np.random.default_rng(5)
    T = np.tile(I23, (6, 1, 1)) + rng.uniform(-0.05, 0.05, (6, 2, 3)) * [1, 1, 40]
    B = section_maps(T)
    assert B.shape == (7, 2, 3) and np.array_equal(B[0], I23)
    p = rng.uniform(0, 100, (5, 2))
    for z in range(6):
        assert np.allclose(WR.apply(B[z + 1], p), WR.apply(T[z], WR.apply(B[z], p)), atol=1e-9)      # B_{z + 1} = T_z o B_z
        assert np.allclose(B[z + 1], WR.compose(T[z], B[z]), atol=1e-12)
    W = section_maps(T, window=3)
    for z in range(7):
        run = np.sort(B[max(z - 1, 0):z + 2].reshape(-1, 6), axis=0)
        trend = run[(run.shape[0] - 1) // 2].reshape(2, 3)
        assert np.allclose(W[z], WR.compose(B[z], WR.invert(trend)), atol=1e-9)
    assert section_maps(np.zeros((0, 2, 3))).shape == (1, 2, 3)


@pytest.mark.parametrize("window", [None, 3, 5, 9])
def test_section_maps_equal_shift_positions_for_integer_translations(window):
    pairs = np.random.default_rng(9).integers(-4, 5, (11, 2)).astype(np.int64)
    T = np.tile(I23, (11, 1, 1))
    T[:, :, 2] = pairs
    B, P = section_maps(T, window), shift_positions(pairs, window)
    assert np.array_equal(B[:, :, :2], np.tile(np.eye(2), (12, 1, 1))) and np.array_equal(B[:, :, 2], P)   # exactly


def test_section_maps_refuse_bad_arguments():
    T = np.tile(I23, (3, 1, 1))
    for a, kw in (((T[0],), {}), ((T[:, :, :2],), {}), ((T.astype(np.int64),), {}), ((T,), dict(window=2)),
                  ((T,), dict(window=1)), ((T,), dict(window=3.0)), ((T * np.nan,), {}), ((T * 0,), dict(window=3))):
        with pytest.raises(ValueError):
            section_maps(*a, **kw)


# ---------------------------------------------------------------------------------------------------- quantize_maps
def test_quantize_maps_at_and_just_past_each_limit():
    q = quantize_maps(MAPS)
    assert q.dtype == np.int64 and q.shape == (2, 6) and np.array_equal(q, WR.quantize(MAPS))
    assert q[0].tolist() == [round(1.01 * ONE), round(-0.02 * ONE), round(1.25 * ONE), round(0.015 * ONE),
                             round(0.99 * ONE), round(-2.5 * ONE)]
    assert quantize_maps(I23[None]).tolist() == [[ONE, 0, 0, 0, ONE, 0]]
    assert quantize_maps(I23[None] + 0.49 / ONE).tolist() == [[ONE, 0, 0, 0, ONE, 0]]       # rint
    for (r, c) in ((0, 0), (0, 1), (1, 0), (1, 1)):
        for sign in (1, -1):
            m = I23[None].copy()
            m[0, r, c] += sign * 0.125
            assert quantize_maps(m)[0, 3 * r + c] == (ONE if r == c else 0) + sign * DEV     # at the limit
            m[0, r, c] += sign * 1.0 / ONE
            with pytest.raises(ValueError):
                quantize_maps(m)                                                             # one unit past it
    for r in (0, 1):
        for sign in (1, -1):
            m = I23[None].copy()
            m[0, r, 2] = sign * (2.0 ** 31 - 1.0 / ONE)
            assert quantize_maps(m)[0, 3 * r + 2] == sign * (2 ** 47 - 1)
            m[0, r, 2] = sign * 2.0 ** 31
            with pytest.raises(ValueError):
                quantize_maps(m)
            m[0, r, 2] = sign * 1e300
            with pytest.raises(ValueError):
                quantize_maps(m)
    for bad in (I23, I23[None, :, :2], np.tile(I23, (2, 1, 1)).astype(np.int64), I23[None] * np.nan,
                np.where(I23[None] == 0, np.inf, 1.0)):
        with pytest.raises(ValueError):
            quantize_maps(bad)


# ------------------------------------------------------------------------- the reference against volume_shift, exactly
@pytest.mark.parametrize("fill", [0, 7])
def test_the_reference_with_integer_maps_equals_volume_shift(fill):
    v = SR.jitter_volume()[:6]
    P = np.array([[0, 0], [3, -2], [-5, 7], [89, 0], [0, -120], [-90, 1]], np.int64)   # inside, to the last voxel, gone
    T = np.tile(I23, (6, 1, 1))
    T[:, :, 2] = P
    M = quantize_maps(T)
    want = volume_shift(v, P, fill=fill)
    assert WR.warp(v, M, fill=fill).tobytes() == want.tobytes()
    assert WR.warp(v, M, fill=fill, nearest=True).tobytes() == want.tobytes()
    assert (want[3, 1:] == fill).all() and (want[3, 0] == v[3, 89]).all() and (want[5] == fill).all()
    box = ((1, 4), (10, 47), (3, 100))
    assert np.array_equal(WR.warp(v, M, box, fill), want[1:4, 10:47, 3:100])
    half = T.copy()
    half[:, 0, 2] += 0.5                                                              # half a pixel: between two rows
    got = WR.warp(v, quantize_maps(half), fill=fill)[1, :80].astype(np.int64)
    a, b = want[1, :80].astype(np.int64), volume_shift(v, P + [1, 0], fill=fill)[1, :80].astype(np.int64)
    assert np.array_equal(got, (a + b + 1) >> 1)                                       # rounded half up, once


# ------------------------------------------------------------------------------------------------------ warp_chunks
def _size(box):
    return int(np.prod([hi - lo for lo, hi in box]))


def _table(Z, kind, shape):
    rng = np.random.default_rng(Z + len(kind))
    T = np.tile(I23, (Z, 1, 1))
    if kind == "rotations":
        for z in range(Z):
            T[z] = WR._rigid(rng.uniform(-0.1, 0.1), rng.uniform(-6, 6, 2), np.array(shape[1:]) / 2)
    elif kind == "limits":
        T[:, :, :2] += rng.choice([-0.125, 0.125], (Z, 2, 2))
        T[:, :, 2] = rng.uniform(-9, 9, (Z, 2))
    elif kind == "outside":
        T[:, 0, 2] = np.where(np.arange(Z) % 2 == 0, 10.0 * shape[1], -10.0 * shape[1])
    return quantize_maps(T)


@pytest.mark.parametrize("kind", ["identity", "rotations", "limits", "outside"])
def test_chunks_partition_the_box_and_hold_every_tap_within_the_budget(kind):
    shape = (5, 23, 17)
    Z, Y, X = shape
    M = _table(Z, kind, shape)
    for box in (((0, Z), (0, Y), (0, X)), ((1, 4), (3, 20), (2, 11))):
        for budget in (None, Z * Y * X, 2 * Y * X, Y * X, Y * X - 1, 12 * X, 6 * X, 2 * X, X, 1):
            chunks = warp_chunks(box, shape, M, budget)
            seen = np.zeros(shape, np.int32)
            b = HIST_CHUNK_BYTES if budget is None else budget
            for (oz, oy, ox), (rz, ry, rx) in chunks:
                seen[oz[0]:oz[1], oy[0]:oy[1], ox[0]:ox[1]] += 1
                assert oz[0] < oz[1] and oy[0] < oy[1] and ox == box[2] and rx == (0, X) and rz == oz
                assert oy == box[1] or oz[1] - oz[0] == 1                           # whole sections, or rows of one
                assert 0 <= ry[0] < ry[1] <= Y
                assert (_size((oz, oy, ox)) <= b and _size((rz, ry, rx)) <= b) or oy[1] - oy[0] == 1
                for z in range(*oz):
                    rows = WR.tap_rows(M[z], (oy, ox), (Y, X))
                    assert rows.size == 0 or (ry[0] <= rows[0] and rows[-1] < ry[1])   # every tap of weight above 0
                    near = WR.tap_rows(M[z], (oy, ox), (Y, X), nearest=True)
                    assert near.size == 0 or (ry[0] <= near[0] and near[-1] < ry[1])
            assert (seen[box[0][0]:box[0][1], box[1][0]:box[1][1], box[2][0]:box[2][1]] == 1).all() and seen.sum() == _size(box)
            order = [(c[0][0], c[1][0]) for c, _ in chunks]
            assert order == sorted(order)
            if budget == 1:
                assert len(chunks) == (box[0][1] - box[0][0]) * (box[1][1] - box[1][0])   # down to one row


def test_chunks_are_tight_take_what_fits_and_go_round_robin():
    shape = (6, 40, 30)
    Z, Y, X = shape
    whole = ((0, Z), (0, Y), (0, X))
    ident = _table(Z, "identity", shape)
    assert warp_chunks(whole, shape, ident) == [(whole, whole)]
    assert [o[0] for o, _ in warp_chunks(whole, shape, ident, 4 * Y * X)] == [(0, 4), (4, 6)]
    rows = warp_chunks(whole, shape, ident, 10 * X)                                # 9 rows read 10: one tap row more
    assert rows[0] == (((0, 1), (0, 9), (0, X)), ((0, 1), (0, 10), (0, X))) and rows[4][0][1] == (36, 40)
    assert rows[4][1][1] == (36, 40)                                               # clipped at the section's end
    # tightness: with every corner inside, the hull's first row is the least iy of the slab and its last row the
    # largest iy + 1 -- both are taps of a corner voxel
    T = np.tile(I23, (Z, 1, 1))
    for z in range(Z):
        T[z] = WR._rigid(0.03 * (z - 2.5), np.array([0.3 * z, -0.2 * z]), np.array([20.0, 15.0]))
    M = quantize_maps(T)
    box = ((0, Z), (8, 30), (6, 22))
    for budget in (None, 2 * Y * X, 7 * X):
        for (oz, oy, ox), (rz, ry, rx) in warp_chunks(box, shape, M, budget):
            iy = np.concatenate([(WR.positions(M[z], (oy, ox), (Y, X))[0] >> 8).reshape(-1) for z in range(*oz)])
            assert all(WR.positions(M[z], (oy, ox), (Y, X))[2].all() for z in range(*oz))
            assert ry == (iy.min(), iy.max() + 2)
    out = _table(Z, "outside", shape)                                               # wholly outside: one row is read
    assert [r[1] for _, r in warp_chunks(whole, shape, out, Y * X)] == [(Y - 1, Y), (0, 1)] * 3
    assert WR.warp(np.ones(shape, np.uint8), out, fill=9).min() == 9
    both = [warp_chunks(whole, shape, M, 2 * Y * X, rank=r, world_size=2) for r in (0, 1)]
    allc = warp_chunks(whole, shape, M, 2 * Y * X)
    assert both[0] == allc[0::2] and both[1] == allc[1::2] and len(allc) >= 3
    assert warp_chunks(((2, 2), (0, Y), (0, X)), shape, M) == []


def test_chunks_refuse_bad_arguments():
    shape = (4, 6, 8)
    M = _table(4, "identity", shape)
    whole = ((0, 4), (0, 6), (0, 8))
    bad = M.copy()
    bad[2, 1] = DEV + 1
    for a, kw in (((whole, shape, M), dict(chunk_bytes=0)), ((whole, shape, M), dict(rank=1)),
                  ((whole, shape, M), dict(rank=0, world_size=0)), ((whole, (6, 8), M), {}), ((whole, shape, M[:3]), {}),
                  ((whole, shape, M.astype(np.float64)), {}), ((whole, shape, M.astype(np.int32)), {}),
                  ((whole, shape, bad), {}), ((((0, 5), (0, 6), (0, 8)), shape, M), {}),
                  ((((0, 4), (-1, 6), (0, 8)), shape, M), {}), ((((0, 4), (0, 6), (0, 9)), shape, M), {})):
        with pytest.raises(ValueError):
            warp_chunks(*a, **kw)


# ------------------------------------------------------------------------------ volume_warp: refused before any GPU work
def test_volume_warp_refuses_bad_arguments_on_the_host(monkeypatch):
    from transfer_em_amd import hip_ops

    def no_gpu():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(hip_ops, "require_gpu", no_gpu)
    v = np.zeros((4, 6, 8), np.uint8)
    T = np.tile(I23, (4, 1, 1))
    far = T.copy()
    far[1, 0, 1] = 0.126
    for a, kw in (((v.astype(np.int16), T), {}), ((v[0, 0], T), {}), ((v[None], T), {}), ((v, T[:3]), {}), ((v, T[0]), {}),
                  ((v, T.astype(np.int64)), {}), ((v, quantize_maps(T).astype(np.int32)), {}), ((v, far), {}),
                  ((v, T * np.nan), {}), ((v, quantize_maps(T)[:, :5]), {}), ((v, T), dict(fill=256)),
                  ((v, T), dict(fill=-1)), ((v, T), dict(fill=1.5)), ((v, T), dict(fill=True)),
                  ((v, T), dict(start=(0, 0, 0), size=(9, 6, 4))), ((v, T), dict(start=(0, 0), size=(8, 6))),
                  ((v, T), dict(out=np.zeros((4, 6, 8), np.int8))), ((v, T), dict(out=np.zeros((4, 6, 9), np.uint8))),
                  ((v, T), dict(start=(1, 1, 1), size=(2, 2, 2), out=v)), ((v, T), dict(chunk_bytes=0)),
                  ((v, T), dict(rank=2, world_size=2)), ((v[0], T), {}), ((v[0], T[0]), dict(start=(0, 0, 0), size=(8, 6, 1)))):
        with pytest.raises(ValueError):
            volume_warp(*a, **kw)
    with pytest.raises(AssertionError, match="the GPU was asked for"):                 # and a good call gets that far
        volume_warp(v, T)
    with pytest.raises(AssertionError, match="the GPU was asked for"):
        volume_warp(v[0], quantize_maps(T)[0], nearest=True, fill=255)


def test_signatures_and_the_reference_alias():
    import transfer_em.utils as alias
    from transfer_em_amd import _lib, utils
    for name in ("shift_subpixel", "fit_section_maps", "section_maps", "quantize_maps", "warp_chunks", "volume_warp",
                 "SubShifts", "SectionFits"):
        assert getattr(alias, name) is getattr(utils, name)
    sig = lambda f: list(inspect.signature(f).parameters)
    dflt = lambda f, p: inspect.signature(f).parameters[p].default
    assert sig(shift_subpixel) == ["q", "n", "min_corr"] and dflt(shift_subpixel, "min_corr") == 0.1
    assert sig(fit_section_maps) == ["sub", "tile", "vol_shape", "model", "max_residual"]
    assert dflt(fit_section_maps, "model") == "affine" and dflt(fit_section_maps, "max_residual") == 1.0
    assert sig(section_maps) == ["pair_maps", "window"] and sig(quantize_maps) == ["maps"]
    assert sig(warp_chunks) == ["out_box", "vol_shape", "M", "chunk_bytes", "rank", "world_size"]
    assert sig(volume_warp) == ["volume", "maps", "out", "start", "size", "fill", "nearest", "chunk_bytes", "rank",
                                "world_size", "device", "stats"]
    assert dflt(volume_warp, "fill") == 0 and dflt(volume_warp, "nearest") is False
    assert SubShifts._fields == ("offsets", "decided", "peak")
    assert SectionFits._fields == ("maps", "kept", "residual", "unresolved")
    assert len(_lib._SIGS["tem_u8_warp_affine"]) == 17
    assert "volume_warp" in inspect.getdoc(volume_shift)


# ------------------------------------------------------------------------- the fixture's own numbers, reference only
@functools.lru_cache(maxsize=None)
def _fixture_fit():
    v = WR.rotated_volume()
    tile = (WR.FIX_TILE, WR.FIX_TILE)
    q = SR.volume_sums(v, tile, WR.FIX_RADIUS)
    n = shift_counts(v.shape, tile, WR.FIX_RADIUS)
    sub = shift_subpixel(q, n)
    return v, q, n, sub, fit_section_maps(sub, WR.FIX_TILE, v.shape)


def test_the_fixture_is_what_it_says():
    v = WR.rotated_volume()
    assert v.shape == WR.FIX_SHAPE == (16, 96, 128) and v.dtype == np.uint8
    T, B = WR.true_pair_maps(), WR.true_section_maps()
    assert T.shape == (15, 2, 3) and B.shape == (16, 2, 3) and np.array_equal(B[0], I23)
    for z in range(15):
        assert np.allclose(B[z + 1], WR.compose(T[z], B[z]), atol=1e-9)
        assert np.allclose(T[z][:, :2] @ T[z][:, :2].T, np.eye(2), atol=1e-12)         # a rotation
        step = abs(np.arctan2(T[z][1, 0], T[z][0, 0]))
        assert abs(step - WR.FIX_PLANTED[z]) < 1e-12 if z in WR.FIX_PLANTED else step <= WR.FIX_ROT
    quantize_maps(B)                                                                   # well inside the limits


def test_every_tile_of_the_fixture_decides_and_every_pair_is_fitted_within_half_a_pixel():
    """Half a voxel is the error that an integer shift cannot get under.  The committed fixture gives: smallest peak
    0.855, tile offsets within 0.43 px of the truth at the tiles' points, pair maps within 0.275 px of the true maps
    at the section's four corners."""
    v, q, n, sub, fit = _fixture_fit()
    Z, Y, X = v.shape
    assert sub.decided.all() and fit.unresolved == []
    print("smallest peak", sub.peak.min())
    corners = np.array([[0, 0], [0, X - 1], [Y - 1, 0], [Y - 1, X - 1]], np.float64)
    T = WR.true_pair_maps()
    pts = _points(v.shape, WR.FIX_TILE)
    tile_err = max(np.abs(WR.apply(T[z], pts) - pts - sub.offsets[z]).max() for z in range(Z - 1))
    err = [np.abs(WR.apply(fit.maps[z], corners) - WR.apply(T[z], corners)).max() for z in range(Z - 1)]
    print("tile offsets within", tile_err, "pair maps at the corners within", max(err), "residual", fit.residual.max())
    assert max(err) < 0.5, err
    assert fit.kept.all() and fit.residual.max() <= 1.0


def _interior(vol, n):
    """The mean correlation at offset (0, 0) and the measured offsets of the interior tiles (row 1, columns 1 and 2 of
    the 3 x 4 grid), from the reference sums."""
    tile, r = (WR.FIX_TILE, WR.FIX_TILE), WR.FIX_RADIUS
    q = SR.volume_sums(vol, tile, r)
    return shift_scores(q, n)[:, 1, 1:3, r, r].mean(), section_shifts(q, n).tiles[:, 1, 1:3]


def test_the_reference_warp_aligns_the_fixture_better_than_the_integer_shift():
    """The committed fixture gives 0.853 raw, 0.918 after volume_shift by the integer medians, 0.941 after the warp."""
    v, q, n, sub, fit = _fixture_fit()
    warped = WR.warp(v, quantize_maps(section_maps(fit.maps)))
    shifted = volume_shift(v, shift_positions(section_shifts(q, n).pairs))
    (c_raw, _), (c_shift, t_shift), (c_warp, t_warp) = _interior(v, n), _interior(shifted, n), _interior(warped, n)
    print("interior tiles' mean correlation: raw", c_raw, "shifted", c_shift, "warped", c_warp)
    assert not t_warp.any()                                                            # every interior tile re-measures (0, 0)
    assert t_shift.any()                                                               # after the integer shift not all do
    assert c_warp > c_shift > c_raw
