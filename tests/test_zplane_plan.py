"""The host side of the in-plane measurement: the planner plane_lag_chunks, the counts, the scores, the sharpness,
find_blurred, join_defects, plane_curve, z_pitch and pitch_step, every ValueError, and the conditions on the shared
fixture (zplane_ref) -- checked here on the CPU, from the reference alone, before any GPU test relies on them."""
from fractions import Fraction

import numpy as np
import pytest

import zplane_ref as PR
import zspace_ref as ZS
from transfer_em_amd import utils as U

TILE = (PR.FIX_TILE, PR.FIX_TILE)


def _bytes(box):
    return int(np.prod([hi - lo for lo, hi in box]))


# -------------------------------------------------------------------------------------------------------- the fixture
def test_the_fixture_meets_its_conditions():
    """Every planted section and tile is found and nothing else; the largest planted relative g is at most the ratio and
    the smallest clean one at least; find_defects' score of the planted tiles stays above its 0.5; the pitch is within
    5 % of the planted 2.0.  The values are the docstring's; the margin is recorded, not fixed."""
    planted_max, clean_min, zrel, px, per, pc = PR.check_fixture()
    print("relative g: planted at most", planted_max, "clean at least", clean_min, "margin", clean_min - planted_max)
    print("find_defects' relative score of the planted tiles at least", zrel, "pitch", px, per)
    assert planted_max <= 0.65 <= clean_min
    assert (round(planted_max, 4), round(clean_min, 4), round(zrel, 4)) == (0.5799, 0.8611, 0.8229)
    assert [round(float(v), 4) for v in pc] == [1.0, 0.8856, 0.629, 0.352, 0.1508, 0.0486, 0.0043, -0.0082]
    assert [round(float(v), 4) for v in PR.fixture_zcurve()] == [1.0, 0.6277, 0.1654, 0.0102]
    assert abs(px - 2.0) <= 0.05 * 2.0 and round(px, 4) == 1.9637
    assert [(k, round(v, 4)) for k, v in per] == [(1, 2.0048), (2, 1.9637), (3, 1.9557)]


def test_find_defects_sees_none_of_the_planted_blur():
    fx = PR.fixture()
    d = U.find_defects(ZS.volume_lag_sums(fx.volume, TILE, 1)[..., [0, 1, 3, 2]])   # section_sums' column order
    assert not set(d.sections) & set(PR.FIX_SECTIONS) and not (d.tiles & fx.planted).any() and not d.undecided.any()
    assert d.sections == [] and not d.tiles.any()


def test_the_host_functions_equal_the_reference_on_the_fixture():
    fx, s, n = PR.fixture(), PR.fixture_sums(), PR.fixture_counts()
    assert np.array_equal(U.plane_lag_counts(PR.FIX_SHAPE, TILE, PR.FIX_LAGS), n)
    assert np.array_equal(U.plane_scores(s, n), PR.scores(s, n))
    assert np.array_equal(U.section_sharpness(s, n), PR.sharpness(s, n))
    d = U.find_blurred(s, n)
    sections, tiles, undecided, g = PR.blurred(s, n)
    assert d.sections == sections == list(PR.FIX_SECTIONS) and np.array_equal(d.tiles, tiles)
    assert np.array_equal(d.undecided, undecided) and np.array_equal(d.scores, g)
    assert np.array_equal(d.tiles | np.isin(np.arange(24), d.sections)[:, None, None], fx.planted)
    pc = U.plane_curve(s, n, skip=d.sections)
    assert np.array_equal(pc, PR.curve(s, n, skip=sections)) and pc.size == 8
    zc = U.section_spacing(ZS.volume_lag_sums(fx.volume, TILE, PR.FIX_ZLAGS), skip=d.sections).curve
    assert np.array_equal(zc, PR.fixture_zcurve())
    zp = U.z_pitch(zc, pc)
    px, per = PR.pitch(zc, pc)
    assert zp.pixels == px and zp.used.all() and zp.per_lag.tolist() == [v for _, v in per]
    assert abs(zp.pixels - PR.FIX_PITCH) <= 0.05 * PR.FIX_PITCH
    assert U.pitch_step(zp.pixels) == (1, 1, PR.step(px)) == (1, 1, Fraction(28, 55))
    # other thresholds: the reference follows
    for kw in ({"ratio": 0.9}, {"ratio": 0.3}, {"section_fraction": 1.0}, {"min_corr": 0.9}):
        d, want = U.find_blurred(s, n, **kw), PR.blurred(s, n, **kw)
        assert d.sections == want[0] and np.array_equal(d.tiles, want[1]) and np.array_equal(d.undecided, want[2])
    assert U.find_blurred(s, n, min_corr=0.9).undecided.all()


def test_the_fast_reference_of_the_plane_sums_equals_the_loops():
    """The GPU tests of grids of many small tiles use plane_tile_sums_fast; here it is held to the loops: blocks at
    the section's top, middle and last rows, cores of rows inside the block, more lags than rows or columns."""
    rng = np.random.default_rng(2)
    for (D, H, W), (th, tw), (y_org, Y) in (((2, 33, 70), (3, 5), (4, 37)), ((2, 33, 70), (32, 32), (42, 75)),
                                            ((3, 5, 7), (1, 1), (0, 5)), ((1, 5, 7), (2048, 2048), (0, 5)),
                                            ((2, 20, 30), (7, 9), (9, 29)), ((2, 20, 30), (7, 9), (9, 60))):
        block = rng.integers(0, 256, (D, H, W), dtype=np.uint8)
        gy, gx = -(-Y // th) + 1, -(-W // tw) + 1
        for nlag in (1, 5, 8):
            last = y_org + H == Y                                                   # the block holds the section's last rows
            top = H if last else max(H - nlag, 0)                                   # else its last rows are halo only
            for (c0, c1), (r0, r1) in (((0, D), (0, top)), ((0, D), (0, max(H - nlag, 0))),
                                       ((D - 1, D), (top // 2, top)), ((0, 0), (0, top)), ((0, D), (2, 2))):
                a = PR.plane_tile_sums(block, c0, c1, r0, r1, y_org, Y, th, tw, gy, gx, nlag)
                b = PR.plane_tile_sums_fast(block, c0, c1, r0, r1, y_org, Y, th, tw, gy, gx, nlag)
                assert a.shape == b.shape and np.array_equal(a, b)
                assert int(a[..., 2].sum()) == (c1 - c0) * (r1 - r0) * W
                assert not a[..., 3 + min(nlag, Y):3 + nlag].any() and not a[..., 3 + nlag + min(nlag, W):].any()


def test_the_sums_by_their_definition_on_a_tiny_block():
    """One tile of 2 x 3 voxels, written out: the column order and the rule that the partner may lie outside the tile
    but not outside the section."""
    b = np.array([[[1, 4, 9, 0], [2, 2, 2, 7]]], np.uint8)                            # one plane of 2 rows x 4 columns
    s = PR.plane_tile_sums(b, 0, 1, 0, 2, 0, 2, 2, 3, 1, 2, 2)
    assert s[0, 0, 0].tolist() == [20, 110, 6, 1 + 4 + 49, 0, 9 + 25 + 81 + 25, 64 + 16 + 25]   # x lag 1 reaches column 3
    assert s[0, 0, 1].tolist() == [7, 49, 2, 49, 0, 0, 0]
    assert U.plane_lag_counts((2, 4), (2, 3), 2).tolist() == [[[[3, 0], [6, 4]], [[1, 0], [0, 0]]]]


# --------------------------------------------------------------------------------------------------- plane_lag_chunks
@pytest.mark.parametrize("shape", [(40, 50, 70), (3, 50, 70), (1, 5, 7), (50, 70)], ids=str)
@pytest.mark.parametrize("budget", [40 * 50 * 70, 7 * 50 * 70, 50 * 70, 25 * 70, 12 * 70, 70, 1])
@pytest.mark.parametrize("L", [1, 4, 8])
def test_plane_lag_chunks(shape, budget, L):
    Z, Y, X = shape if len(shape) == 3 else (1,) + shape
    chunks = U.plane_lag_chunks(shape, L, budget)
    seen = np.zeros((Z, Y), np.int64)
    for (cz, cy, cx), (rz, ry, rx) in chunks:
        seen[cz[0]:cz[1], cy[0]:cy[1]] += 1
        assert cx == rx == (0, X) and rz == cz and ry[0] == cy[0]                    # no halo along z
        whole = cy == (0, Y)
        assert ry == ((0, Y) if whole else (cy[0], min(cy[1] + L, Y)))                # the halo: L rows, clipped
        assert whole or cz[1] - cz[0] == 1
        assert _bytes((rz, ry, rx)) <= budget or (cz[1] - cz[0] == 1 and cy[1] - cy[0] == 1)
    assert (seen == 1).all()                                                        # disjoint, and the whole volume
    assert [c for c, _ in chunks] == U.hist_chunks(U.hist_box(shape), budget) or Y * X > budget   # hist_chunks' kinds
    parts = [U.plane_lag_chunks(shape, L, budget, r, 3) for r in range(3)]
    assert all(parts[r] == chunks[r::3] for r in range(3))                          # round-robin


def test_plane_lag_chunks_cuts_rows_with_their_halo_in_the_budget():
    chunks = U.plane_lag_chunks((2, 50, 70), 8, 20 * 70)
    assert [c[1] for c, _ in chunks[:5]] == [(0, 12), (12, 24), (24, 36), (36, 48), (48, 50)]
    assert [r[1] for _, r in chunks[:5]] == [(0, 20), (12, 32), (24, 44), (36, 50), (48, 50)]
    assert len(chunks) == 10 and chunks[5][0][0] == (1, 2)


def test_plane_lag_chunks_refuses():
    for bad in (0, 9, 1.5, True):
        with pytest.raises(ValueError):
            U.plane_lag_chunks((4, 5, 6), bad)
    with pytest.raises(ValueError):
        U.plane_lag_chunks((4, 5, 6), 2, 0)
    with pytest.raises(ValueError):
        U.plane_lag_chunks((4, 5, 6), 2, 100, 2, 2)
    with pytest.raises(ValueError):
        U.plane_lag_chunks((4, 5, 6, 7), 2)
    assert U.plane_lag_chunks((0, 5, 6), 2) == []


# --------------------------------------------------------------------------------------------------- plane_lag_counts
@pytest.mark.parametrize("shape, tile", [((3, 10, 13), (4, 5)), ((7, 9), (7, 9)), ((5, 7), (2048, 2048)),
                                         ((2, 33, 70), (32, 32)), ((6, 4), (1, 1)), ((2, 17, 3), (5, 2))], ids=str)
def test_plane_lag_counts_equal_brute_force(shape, tile):
    for L in (1, 3, 8):
        n = U.plane_lag_counts(shape, tile, L)
        assert n.dtype == np.int64 and np.array_equal(n, PR.counts(shape, tile, L))
    Y, X = shape[-2:]
    assert n[:, :, 0].sum(axis=(0, 1)).tolist() == [max(Y - k, 0) * X for k in range(1, 9)]
    assert n[:, :, 1].sum(axis=(0, 1)).tolist() == [max(X - k, 0) * Y for k in range(1, 9)]
    assert U.plane_lag_counts(shape, tile[0] if tile[0] == tile[1] else tile, 2).shape == n.shape[:3] + (2,)


def test_counts_and_sums_refuse():
    for bad in (0, 9, 2.0, None):
        with pytest.raises(ValueError):
            U.plane_lag_counts((4, 5, 6), 4, bad)
    with pytest.raises(ValueError):
        U.plane_lag_counts((4, 5, 6), 0, 2)
    with pytest.raises(ValueError):
        U.plane_lag_counts((4, 5, 6, 7), 4, 2)
    vol = np.zeros((2, 8, 8), np.uint8)
    for kw in ({"max_lag": 0}, {"max_lag": 9}, {"tile": 0}, {"tile": 4096}, {"chunk_bytes": 0}, {"rank": 1}):
        with pytest.raises(ValueError):                                              # before any GPU work
            U.section_plane_sums(vol, **kw)
    with pytest.raises(ValueError):
        U.section_plane_sums(vol.astype(np.int16))


# ------------------------------------------------------------------------------------------------- scores and verdicts
def _sums(vol, tile, L):
    return PR.volume_plane_sums(vol, tile, L), PR.counts(vol.shape, tile, L)


def test_scores_of_special_tiles():
    vol = np.zeros((3, 8, 12), np.uint8)
    vol[1] = 200                                                                     # constant: no correlation
    vol[2] = (np.arange(12) % 2 * 255)[None, :]                                      # columns alternate
    s, n = _sums(vol, (8, 12), 8)
    r = U.plane_scores(s, n)
    assert r.shape == (3, 1, 1, 2, 8) and not r[:2].any()
    assert r[2, 0, 0, 0].tolist() == [1.0] * 7 + [0.0]                               # rows equal; lag 8 of 8 rows: no pair
    assert np.allclose(r[2, 0, 0, 1], [-1, 1] * 4)                                   # columns flip
    assert not U.section_sharpness(s, n)[:2].any()
    s, n = _sums(vol[:, :, :3], (8, 12), 8)                                          # lags past the 3 columns: no pair
    assert (n[0, 0, 1, 3:] == 0).all() and not U.plane_scores(s, n)[:, 0, 0, 1, 3:].any()


def test_single_images_and_short_stacks():
    fx = PR.fixture()
    s, n = _sums(fx.volume[:1], TILE, 2)
    d = U.find_blurred(s, n)                                                         # judged against nothing
    assert d.sections == [] and not d.tiles.any() and d.undecided.all() and d.scores.shape == (1, 2, 3)
    assert np.array_equal(d.scores, U.section_sharpness(s, n)) and (d.scores > 0).all()
    assert U.plane_curve(s, n).size == 3                                             # the curve needs no second section
    d = U.find_blurred(*_sums(fx.volume[6:9], TILE, 2))                              # 6, 7 (blurred), 8
    assert d.sections == [1] and not d.undecided.any()


def test_estimators_refuse():
    s, n = PR.fixture_sums(), PR.fixture_counts()
    for fn in (U.plane_scores, U.section_sharpness, U.find_blurred, U.plane_curve):
        for bs, bn in ((s[..., :4], n), (s[..., :6], n[..., :1]), (s.astype(np.float64), n), (s, n.astype(np.float64)),
                       (s[0], n), (s, n[1:]), (np.zeros((2, 2, 3, 21), np.int64), np.zeros((2, 3, 2, 9), np.int64))):
            with pytest.raises(ValueError):
                fn(bs, bn)
    one = (s[..., [0, 1, 2, 3, 11]], n[..., :1])                                     # one lag
    assert U.plane_scores(*one).shape == (24, 2, 3, 2, 1) and U.plane_curve(*one).size == 2
    for fn in (U.section_sharpness, U.find_blurred):
        with pytest.raises(ValueError):
            fn(*one)
    for kw in ({"ratio": 0}, {"ratio": 1.5}, {"min_corr": 1}, {"min_corr": 0}, {"section_fraction": 0},
               {"section_fraction": "x"}):
        with pytest.raises(ValueError):
            U.find_blurred(s, n, **kw)
    for kw in ({"skip": [24]}, {"skip": [-1]}, {"skip": 3}, {"skip": [1.5]}, {"min_corr": 1}, {"skip": range(24)},
               {"min_corr": 0.99}):
        with pytest.raises(ValueError):
            U.plane_curve(s, n, **kw)
    flat = _sums(np.full((2, 8, 8), 7, np.uint8), (8, 8), 2)
    with pytest.raises(ValueError):
        U.plane_curve(*flat)
    assert U.find_blurred(*flat).undecided.all()


def test_plane_curve_is_cut_where_it_stops_decreasing():
    rng = np.random.default_rng(4)
    vol = rng.integers(0, 256, (3, 64, 64), dtype=np.uint8)                          # white noise: r_k ~ 0 for every k
    vol = np.repeat(np.repeat(vol, 2, axis=1), 2, axis=2)[:, :64, :64]               # 2 x 2 blocks: r_1 ~ 0.5, r_2 ~ 0
    s, n = _sums(vol, (64, 64), 8)
    c = U.plane_curve(s, n)
    assert 2 <= c.size < 9 and np.all(np.diff(c) < 0) and abs(c[1] - 0.5) < 0.05
    assert np.array_equal(c, PR.curve(s, n))
    m = PR.mean_scores(s, n)
    assert not np.median(m[:, 0, 0, c.size - 1]) < c[-1]                            # the next lag did not decrease


def test_join_defects():
    D = U.Defects
    t = lambda *idx: np.isin(np.arange(24).reshape(4, 2, 3), idx)
    a = D([1], t(0, 13), np.array([[True, False, False], [False, True, False]]), np.ones((4, 2, 3)))
    b = D([3, 1], t(6, 7, 13, 14), np.array([[True, True, False], [False, False, False]]), np.zeros((4, 2, 3)))
    j = U.join_defects(a, b)
    assert j.sections == [1, 3] and np.array_equal(j.tiles, t(0, 13, 14))            # 6, 7: in section 1, cleared
    assert j.undecided.tolist() == [[True, False, False], [False, False, False]] and j.scores is a.scores
    one = U.join_defects(a)
    assert one.sections == [1] and np.array_equal(one.tiles, a.tiles) and np.array_equal(one.undecided, a.undecided)
    r = U.defects_repair(j, (2, 2), (4, 4, 6))
    assert r.sections == [1, 3] and r.mask.shape == (4, 4, 6) and r.mask[0, :2, :2].all() and not r.mask[1].any()
    for bad in ((), (a, None), (a, D([1], t(0)[:3], a.undecided, None)), (a, D([1], t(0), a.undecided[:1], None)),
                (a, D([4], t(0), a.undecided, None)), (a, D([1.5], t(0), a.undecided, None)), (a, (1, 2, 3, 4))):
        with pytest.raises(ValueError):
            U.join_defects(*bad)
    fx, s, n = PR.fixture(), PR.fixture_sums(), PR.fixture_counts()                   # the chain's two verdicts
    both = U.join_defects(U.find_defects(ZS.volume_lag_sums(fx.volume, TILE, 1)[..., [0, 1, 3, 2]]), U.find_blurred(s, n))
    assert both.sections == [7, 15] and np.argwhere(both.tiles).tolist() == [[19, 1, 2]]


def test_z_pitch_by_cases():
    p = np.array([1.0, 0.8, 0.5, 0.2])
    zp = U.z_pitch([1.0, 0.5, 0.1], p)                                               # 0.5 is 2 px; 0.1 is out of reach
    assert zp.pixels == 2.0 and zp.used.tolist() == [True, False] and zp.per_lag[0] == 2.0 and np.isnan(zp.per_lag[1])
    zp = U.z_pitch([1.0, 0.9, 0.65, 0.35, 0.2], p)                                   # 0.5, 1.5, 2.5 px and 0.2: not above
    assert np.allclose(zp.per_lag[:3], [0.5, 0.75, 2.5 / 3]) and zp.used.tolist() == [True, True, True, False]
    assert zp.pixels == zp.per_lag[1] and U.z_pitch([1.0, 0.9, 0.65, 0.35, 0.2], p).pixels == PR.pitch([1.0, 0.9, 0.65, 0.35, 0.2], p)[0]
    for z, q in (([1.0, 0.1], p), ([1.0, 0.2], p), ([0.9, 0.5], p), ([1.0, 0.5, 0.5], p), ([1.0], p), ([1.0, 0.5], [1.0]),
                 ([1.0, 0.5], [1.0, 0.5, 0.6]), ([1.0, np.nan], p), ([[1.0, 0.5]], p), ([1.0, 0.5], [0.99, 0.5])):
        with pytest.raises(ValueError):
            U.z_pitch(z, q)


def test_pitch_step_by_cases():
    one = Fraction(1)
    assert U.pitch_step(2.0) == (one, one, Fraction(1, 2)) and U.pitch_step(1) == (one, one, one)
    assert U.pitch_step(0.125)[2] == 8 and U.pitch_step(8)[2] == Fraction(1, 8) and U.pitch_step(Fraction(5, 2))[2] == Fraction(2, 5)
    for px in (1.97, 0.3, 3.3333, 7.9, 0.1251, 1.0 / 3, 2.71828, 5.5):
        f = U.pitch_step(px)[2]
        assert f == PR.step(px) and max(f.numerator, f.denominator) <= 64 and Fraction(1, 8) <= f <= 8
        assert U.volume_rescale is not None and U._rescale_fraction(f) == f                # a step volume_rescale takes
    for bad in (0, -1.0, 8.01, 0.1249, np.inf, np.nan, "2", True, None):
        with pytest.raises(ValueError):
            U.pitch_step(bad)
