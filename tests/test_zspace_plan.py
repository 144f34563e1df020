"""The host side of the spacing measurement along z: the planners zlag_chunks and resample_z_chunks, the taps, every
ValueError, the estimator's special cases, and the conditions on the shared fixture (zspace_ref) -- checked here on the
CPU, from the reference alone, before any GPU test relies on them."""
import numpy as np
import pytest

import zspace_ref as ZR
from transfer_em_amd import utils as U


def _bytes(box):
    return int(np.prod([hi - lo for lo, hi in box]))


# -------------------------------------------------------------------------------------------------------- the fixture
def test_the_fixture_meets_its_conditions():
    P, curve, e_est, e_even, r_raw, r_res = ZR.check_fixture()
    assert e_est <= 0.25 and e_even >= 1.0 and r_res <= 0.5 * r_raw
    assert [round(float(v), 4) for v in curve] == [1.0, 0.9449, 0.7992, 0.5974, 0.4187]   # the docstring's values
    assert (round(e_est, 4), round(e_even, 4), round(r_raw, 4), round(r_res, 4)) == (0.1477, 1.4186, 11.9121, 2.4943)


def test_the_estimator_equals_the_reference_on_the_fixture():
    fx, s = ZR.fixture(), ZR.fixture_sums()
    assert np.array_equal(U.lag_scores(s), ZR.scores(s))
    sp = U.section_spacing(s, fx.skip)
    P, curve, used, clipped, unresolved = ZR.spacing(s, fx.skip)
    assert np.array_equal(sp.curve, curve) and sp.clipped == [] and sp.unresolved == []
    assert [(int(z), int(k) + 1) for z, k in np.argwhere(sp.used)] == [(z, k) for z, k, _ in used]
    assert np.abs(sp.positions - P).max() < 1e-9                                    # band elimination against lstsq
    assert sp.positions[0] == 0 and sp.positions[-1] == 39
    assert np.array_equal(U.resample_z_taps(U.quantize_positions(sp.positions)), ZR.taps(ZR.quantize(P)))
    assert not sp.used[ZR.FIX_SKIP].any() and not sp.used[ZR.FIX_SKIP - 1, 0]          # no pair touches the black section


def test_the_fast_reference_of_the_lag_sums_equals_the_loops():
    """The GPU tests of grids of many small tiles use lag_tile_sums_fast; here it is held to the loops, on the grid and
    off it, for cores inside the block and for more lags than the block has planes."""
    rng = np.random.default_rng(2)
    for (D, H, W), (th, tw), (y_org, x_org) in (((4, 33, 70), (3, 5), (4, 12)), ((4, 33, 70), (32, 32), (42, 80)),
                                                ((3, 5, 7), (1, 1), (0, 0)), ((1, 5, 7), (2048, 2048), (0, 0)),
                                                ((10, 20, 30), (7, 9), (9, 22))):
        block = rng.integers(0, 256, (D, H, W), dtype=np.uint8)
        gy, gx = -(-(y_org + H) // th) + 1, -(-(x_org + W) // tw) + 1
        for nlag in (1, 4, 8):
            for c0, c1 in ((0, D), (0, D - 1), (min(1, D), min(2, D)), (D, D)):
                a = ZR.lag_tile_sums(block, c0, c1, y_org, x_org, th, tw, gy, gx, nlag)
                b = ZR.lag_tile_sums_fast(block, c0, c1, y_org, x_org, th, tw, gy, gx, nlag)
                assert a.shape == b.shape and np.array_equal(a, b)
                assert int(a[..., 2].sum()) == (c1 - c0) * H * W and not a[..., 2 + D:].any()


# -------------------------------------------------------------------------------------------------------- zlag_chunks
@pytest.mark.parametrize("shape", [(40, 50, 70), (3, 50, 70), (1, 5, 7), (50, 70)], ids=str)
@pytest.mark.parametrize("budget", [40 * 50 * 70, 7 * 50 * 70, 50 * 70, 25 * 70, 70, 1])
@pytest.mark.parametrize("L", [1, 4, 8])
def test_zlag_chunks(shape, budget, L):
    Z, Y, X = shape if len(shape) == 3 else (1,) + shape
    halo = min(L, Z - 1)
    chunks = U.zlag_chunks(shape, L, budget)
    seen = np.zeros((Z, Y), np.int64)
    for (cz, cy, cx), (rz, ry, rx) in chunks:
        seen[cz[0]:cz[1], cy[0]:cy[1]] += 1
        assert cx == rx == (0, X) and ry == cy and rz[0] == cz[0] and rz[1] == min(cz[1] + halo, Z)
        rows = cy[1] - cy[0]
        assert _bytes((rz, ry, rx)) <= budget or (cz[1] - cz[0] == 1 and (rows == 1 or (1 + halo) * rows * X <= budget))
    assert (seen == 1).all()                                                        # disjoint, and the whole volume
    parts = [U.zlag_chunks(shape, L, budget, r, 3) for r in range(3)]
    assert sorted(sum(parts, [])) == sorted(chunks) and sum(map(len, parts)) == len(chunks)
    if L == 1:
        assert chunks == U.zcorr_chunks(shape, budget)


def test_zlag_chunks_refuses():
    for bad in (0, 9, 1.5, True):
        with pytest.raises(ValueError):
            U.zlag_chunks((4, 5, 6), bad)
    with pytest.raises(ValueError):
        U.zlag_chunks((4, 5, 6), 2, 0)
    with pytest.raises(ValueError):
        U.zlag_chunks((4, 5, 6), 2, 100, 2, 2)


# --------------------------------------------------------------------------------------------------------------- taps
def test_taps_of_identity_positions():
    t = U.resample_z_taps(np.arange(7) * U.ZSPACE_UNIT)
    assert t.dtype == np.int32 and t.tolist() == [[j, 0] for j in range(7)]
    assert U.resample_z_taps(np.arange(7.0)).tolist() == t.tolist()
    assert U.resample_z_taps(np.arange(7.0), 9).tolist() == t.tolist() + [[6, 0], [6, 0]]   # past the end: the last one
    assert U.resample_z_taps(np.arange(7.0), 3).tolist() == t.tolist()[:3]


def test_taps_equal_the_reference_and_are_monotone_within_a_pair():
    rng = np.random.default_rng(3)
    for _ in range(20):
        Q = np.concatenate([[0], np.cumsum(rng.integers(1 << 13, (1 << 19) + 1, 30))])
        t = U.resample_z_taps(Q)
        assert np.array_equal(t, ZR.taps(Q)) and t.shape[0] == Q[-1] // 65536 + 1
        assert (np.diff(t[:, 0]) >= 0).all()
        same = np.diff(t[:, 0]) == 0
        assert (np.diff(t[:, 1])[same] >= 0).all()                                  # w grows inside a source pair
        assert (t[:, 1] >= 0).all() and (t[:, 1] <= 255).all() and (t[t[:, 0] == 30, 1] == 0).all()


def test_taps_carry_and_the_last_section():
    # section 1 sits one 2^-16 above position 1: w = 256 (1 - 2^-16) rounds to 256 and becomes (1, 0)
    Q = np.array([0, 65537, 2 * 65536 + 1, 3 * 65536], np.int64)
    t = U.resample_z_taps(Q)
    assert t.tolist() == ZR.taps(Q).tolist() == [[0, 0], [1, 0], [2, 0], [3, 0]]
    # ... and one that does not carry: half way
    assert U.resample_z_taps(np.array([0, 2 * 65536])).tolist() == [[0, 0], [0, 128], [1, 0]]
    assert U.resample_z_taps(np.array([0, 3 * 65536])).tolist() == [[0, 0], [0, 85], [0, 171], [1, 0]]
    # the last section never asks for the plane above it
    for Z in (1, 2, 5):
        t = U.resample_z_taps(np.arange(Z) * 40000 if Z > 1 else np.zeros(1, np.int64), 6)
        assert (t[t[:, 0] == Z - 1, 1] == 0).all() and t[-1].tolist() == [Z - 1, 0]


def test_quantize_positions():
    assert U.quantize_positions([0, 0.5, 1.75]).tolist() == [0, 32768, 114688]
    assert U.quantize_positions(np.array([0, 70000])).tolist() == [0, 70000]       # integers: quantised already
    for bad, word in (([0.0, 1, 1], "section 2"), ([0, 2, 1.5], "section 2"), ([0, 1, 1.1], "sections 1 and 2"),
                      ([0, 1, 9.5], "sections 1 and 2"), ([0.5, 1], "section 0"), ([0, np.nan], "finite"),
                      ([[0, 1]], "one number"), ([], "one number")):
        with pytest.raises(ValueError, match=word):
            U.quantize_positions(bad)
    assert U.quantize_positions([0, 0.125, 8.125]).tolist() == [0, 8192, 8192 + 8 * 65536]     # the limits themselves
    with pytest.raises(ValueError):
        U.resample_z_taps([0.0, 1, 2], 0)
    with pytest.raises(ValueError):
        U.resample_z_taps([0.0, 1, 1])


# -------------------------------------------------------------------------------------------------- resample_z_chunks
def _taps_case():
    rng = np.random.default_rng(9)
    gaps = rng.uniform(0.3, 2.5, 29)
    gaps[7] = 6.5
    return U.resample_z_taps(U.quantize_positions(np.concatenate([[0], np.cumsum(gaps)])))


@pytest.mark.parametrize("box", [None, ((3, 20), (5, 41), (8, 60))], ids=["whole", "roi"])
@pytest.mark.parametrize("budget", [1 << 20, 9 * 50 * 70, 3 * 50 * 70, 50 * 70, 5 * 70, 1])
def test_resample_z_chunks(box, budget):
    taps, vol = _taps_case(), (30, 50, 70)
    NZ = taps.shape[0]
    box = ((0, NZ), (0, 50), (0, 70)) if box is None else box
    chunks = U.resample_z_chunks(box, vol, taps, budget)
    seen = np.zeros((NZ, 50), np.int64)
    for (oz, oy, ox), (rz, ry, rx) in chunks:
        seen[oz[0]:oz[1], oy[0]:oy[1]] += 1
        assert ox == rx == box[2] and ry == oy
        need = [z for j in range(*oz) for z in ([int(taps[j, 0])] + ([int(taps[j, 0]) + 1] if taps[j, 1] else []))]
        assert (rz[0], rz[1]) == (min(need), max(need) + 1) and 0 <= rz[0] and rz[1] <= 30   # the dense hull, no more
        rows, nx = oy[1] - oy[0], ox[1] - ox[0]
        planes = 1 + rz[1] - rz[0]
        assert _bytes((oz, oy, ox)) + _bytes((rz, ry, rx)) <= budget or \
            (oz[1] - oz[0] == 1 and (rows == 1 or planes * rows * nx <= budget))
    want = np.zeros((NZ, 50), np.int64)
    want[box[0][0]:box[0][1], box[1][0]:box[1][1]] = 1
    assert np.array_equal(seen, want)                                               # disjoint, and the whole box
    parts = [U.resample_z_chunks(box, vol, taps, budget, r, 3) for r in range(3)]
    assert sorted(sum(parts, [])) == sorted(chunks) and sum(map(len, parts)) == len(chunks)
    if budget == 1 << 20:
        assert len(chunks) == 1
    if budget == 5 * 70:
        assert any(o[1] != box[1] for o, _ in chunks)                               # rows of one section


def test_resample_z_chunks_refuses():
    taps = _taps_case()
    NZ = taps.shape[0]
    whole = ((0, NZ), (0, 50), (0, 70))
    for args in ((whole, (30, 50, 70), taps, 0), (whole, (30, 50, 70), taps, 100, 1, 1), (whole, (50, 70), taps),
                 (((0, NZ + 1), (0, 50), (0, 70)), (30, 50, 70), taps), (((0, NZ), (0, 51), (0, 70)), (30, 50, 70), taps),
                 (whole, (20, 50, 70), taps), (whole, (30, 50, 70), taps.astype(np.float64)),
                 (whole, (30, 50, 70), taps[:, :1]), (whole, (30, 50, 70), np.array([[0, 256]])),
                 (whole, (30, 50, 70), np.array([[-1, 0]]))):
        with pytest.raises(ValueError):
            U.resample_z_chunks(*args)
    assert U.resample_z_chunks(((2, 2), (0, 50), (0, 70)), (30, 50, 70), taps) == []


# ------------------------------------------------------------------------------------------------------ the estimator
def _sums_from_curve(pos, L=4, sigma=2.0, skip=()):
    """Synthetic lag sums [Z, 1, 1, 3 + L] of one tile whose correlation at distance d is exp(-d^2 / (4 sigma^2)):
    n = 1000, mean 100, variance 400; a skipped section is constant (variance 0)."""
    Z = len(pos)
    n, mean, var = 1000, 100, 400
    s = np.zeros((Z, 1, 1, 3 + L), np.int64)
    for z in range(Z):
        v = 0 if z in skip else var
        s[z, 0, 0, :3] = (n * mean, n * (v + mean * mean), n)
        for k in range(1, L + 1):
            if z + k < Z:
                rho = 0.0 if z in skip or z + k in skip else np.exp(-((pos[z + k] - pos[z]) ** 2) / (4 * sigma ** 2))
                s[z, 0, 0, 2 + k] = int(round(n * (rho * var + mean * mean)))
    return s


def test_lag_scores_formula_and_edges():
    pos = np.arange(6.0)
    s = _sums_from_curve(pos, skip=(2,))
    c = U.lag_scores(s)
    assert c.shape == (6, 1, 1, 4) and np.allclose(c[0, 0, 0, 0], np.exp(-1 / 16), atol=1e-5)
    assert not c[2].any() and not c[1, 0, 0, 0] and not c[5].any() and not c[3, 0, 0, 2:].any()   # constant; past the end
    assert U.lag_scores(s[:1]).shape == (1, 1, 1, 4) and not U.lag_scores(s[:1]).any()
    with pytest.raises(ValueError):
        U.lag_scores(s[..., :3])
    with pytest.raises(ValueError):
        U.lag_scores(s.astype(np.float64))


def test_spacing_recovers_planted_positions_and_bridges_a_skipped_section():
    rng = np.random.default_rng(1)
    pos = np.concatenate([[0], np.cumsum(rng.uniform(0.7, 1.3, 29))])
    pos *= 29 / pos[-1]
    sp = U.section_spacing(_sums_from_curve(pos, skip=(11,)), skip=[11])
    good = [z for z in range(30) if z != 11]
    assert np.abs(sp.positions[good] - pos[good]).max() < 0.15 and sp.clipped == [] and sp.unresolved == []
    assert not sp.used[11].any() and not sp.used[10, 0] and sp.used[10, 1]         # (10, 12) bridges it
    assert sp.positions[11] == pytest.approx((sp.positions[10] + sp.positions[12]) / 2)     # placed linearly between
    ref = ZR.spacing(_sums_from_curve(pos, skip=(11,)), skip=[11])
    assert np.abs(sp.positions - ref[0]).max() < 1e-9
    # skipped sections at both ends sit at spacing 1 outside the good ones, before the scale to [0, Z - 1]
    ends = U.section_spacing(_sums_from_curve(np.arange(12.0), skip=(0, 11)), skip=[0, 11])
    assert np.allclose(ends.positions, np.arange(12.0), atol=1e-9)


def test_spacing_lists_a_broken_chain_as_unresolved():
    """Sections 10 and 11 are 9 apart: no pair across the gap correlates above curve[L], the two halves are solved on
    their own, and the gap keeps the nominal spacing 1."""
    pos = np.concatenate([np.arange(11.0), 19.0 + np.arange(11.0)])
    sp = U.section_spacing(_sums_from_curve(pos))
    assert sp.unresolved == [(10, 11)] and sp.clipped == []
    assert not sp.used[7:11].any(axis=0)[3] and not sp.used[10].any()
    gaps = np.diff(sp.positions)
    assert np.allclose(gaps / gaps[0], 1.0, atol=0.02)                              # 1 across the gap as everywhere
    ref = ZR.spacing(_sums_from_curve(pos))
    assert ref[4] == [(10, 11)] and np.abs(sp.positions - ref[0]).max() < 1e-9


def test_spacing_clips_to_the_limits():
    """Two sections that are all but identical (distance 0.01 of a section) are held ZSPACE_MIN apart."""
    pos = np.concatenate([np.arange(8.0), [7.01], 8.0 + np.arange(8.0)])
    sp = U.section_spacing(_sums_from_curve(pos))
    assert sp.clipped == [(7, 8)] and sp.unresolved == []
    ref = ZR.spacing(_sums_from_curve(pos))
    assert ref[3] == [(7, 8)] and np.abs(sp.positions - ref[0]).max() < 1e-9
    U.quantize_positions(sp.positions)                                              # and so the resampler takes them


def test_spacing_refuses():
    s = _sums_from_curve(np.arange(10.0))
    flat = s.copy()
    flat[..., 3:] = flat[..., 3:4]                                                  # the same correlation at every lag
    for args in ((s[..., :3],), (s.astype(np.float32),), (s, [10]), (s, [-1]), (s, [1.5]), (s, 3), (s, (), 0.0),
                 (s, (), 1.0), (s, (), "x"), (s, range(1, 10)), (flat,), (s[:1],),
                 (_sums_from_curve(np.arange(10.0) * 9),)):                         # nothing correlates: no decided column
        with pytest.raises(ValueError):
            U.section_spacing(*args)
    with pytest.raises(ValueError, match="decrease"):
        U.section_spacing(flat)


def test_volume_resample_z_refuses_before_any_gpu_work():
    vol = np.zeros((4, 5, 6), np.uint8)
    P = np.arange(4.0)
    for args, kw in (((vol.astype(np.int8), P), {}), ((vol[0], P[:1]), {}), ((vol, P[:3]), {}), ((vol, [0.0, 1, 1, 2]), {}),
                     ((vol, P), {"start": (0, 0, 3), "size": (6, 5, 2)}), ((vol, P), {"out": np.zeros((4, 5, 5), np.uint8)}),
                     ((vol, P), {"out": np.zeros((4, 5, 6), np.int8)}), ((vol, P), {"nz": 0}),
                     ((vol, P), {"chunk_bytes": 0}), ((vol, P), {"rank": 1})):
        with pytest.raises(ValueError):
            U.volume_resample_z(*args, **kw)
    with pytest.raises(ValueError):
        U.section_lag_sums(vol, 4, 9)
    with pytest.raises(ValueError):
        U.section_lag_sums(vol.astype(np.int8), 4, 2)
