"""The host side of the centred section-shift measurement, without a GPU: the slab plan zshift_chunks_at, shift_counts_at
against brute force, shift_centers, the `_at` verdicts against their siblings at zero centres and rule by rule on
hand-made tables, and the coarse-to-fine driver's logic run on the host with the numpy reference (zshift_at_ref) in
place of the two device passes, on the fixture of sections with large planted jumps."""
import inspect

import numpy as np
import pytest

import zshift_at_ref as AR
import zshift_ref as SR
from transfer_em_amd import utils
from transfer_em_amd.utils import (HIST_CHUNK_BYTES, CoarseShifts, Shifts, SubShifts, section_shift_sums_at,
                                   section_shifts, section_shifts_at, section_shifts_coarse_to_fine, shift_centers,
                                   shift_counts, shift_counts_at, shift_scores, shift_scores_at, shift_subpixel,
                                   shift_subpixel_at, zshift_chunks, zshift_chunks_at)

TILE, RADIUS = (SR.FIX_TILE, SR.FIX_TILE), SR.FIX_RADIUS


# ------------------------------------------------------------------------------------------------- zshift_chunks_at
def _size(box):
    return int(np.prod([hi - lo for lo, hi in box]))


@pytest.mark.parametrize("shape", [(7, 9, 5), (1, 9, 5), (2, 3, 4), (9, 5)])
def test_chunks_partition_the_volume_with_their_halo_within_the_budget(shape):
    Z, Y, X = shape if len(shape) == 3 else (1,) + shape
    for r, (lo, hi) in ((1, (0, 0)), (2, (-3, 0)), (2, (0, 5)), (8, (-2, 1)), (1, (-1024, 1024))):
        for budget in (None, Z * Y * X, 3 * Y * X, 2 * Y * X, 2 * Y * X - 1, Y * X, 14 * X, 12 * X, 7 * X, 2 * X, X, 1):
            chunks = zshift_chunks_at(shape, r, (lo, hi), budget)
            seen = np.zeros((Z, Y, X), np.int32)
            for (cz, cy, cx), (rz, ry, rx) in chunks:
                seen[cz[0]:cz[1], cy[0]:cy[1], cx[0]:cx[1]] += 1
                assert cz[0] < cz[1] and cy[0] < cy[1] and cx == (0, X) and rx == cx
                assert rz == (cz[0], min(cz[1] + 1, Z))                            # one section more, but at the last
                assert ry == (max(cy[0] - r + lo, 0), min(cy[1] + r + hi, Y))      # the reach and r rows more
                assert cy == (0, Y) or cz[1] - cz[0] == 1                           # whole sections, or rows of one
                b = HIST_CHUNK_BYTES if budget is None else budget
                assert _size((rz, ry, rx)) <= b or cy[1] - cy[0] == 1               # one core row at the least
            assert (seen == 1).all()
            order = [(c[0][0], c[1][0]) for c, _ in chunks]
            assert order == sorted(order)


def test_chunks_count_the_reach_into_the_row_budget():
    shape = (10, 12, 40)
    rows = zshift_chunks_at(shape, 1, (-2, 1), 2 * 10 * 40)      # 10 rows twice: 5 of core + 3 below + 2 above
    assert rows[0] == (((0, 1), (0, 5), (0, 40)), ((0, 2), (0, 7), (0, 40)))
    assert rows[1] == (((0, 1), (5, 10), (0, 40)), ((0, 2), (2, 12), (0, 40)))
    assert rows[2] == (((0, 1), (10, 12), (0, 40)), ((0, 2), (7, 12), (0, 40)))
    assert rows[-1] == (((9, 10), (10, 12), (0, 40)), ((9, 10), (7, 12), (0, 40)))
    assert len(rows) == 30 and len(zshift_chunks(shape, 1, 2 * 10 * 40)) == 20     # the sibling: 8 rows of core
    assert len(zshift_chunks_at(shape, 1, (-500, 500), 2 * 10 * 40)) == 120        # one core row at the least


def test_chunks_equal_the_sibling_at_no_reach_and_go_round_robin():
    for shape in ((7, 9, 5), (1, 9, 5), (9, 5)):
        for r in (1, 8):
            for budget in (None, 90, 45, 10, 1):
                assert zshift_chunks_at(shape, r, (0, 0), budget) == zshift_chunks(shape, r, budget)
    shape, budget = (9, 8, 6), 90
    everything = zshift_chunks_at(shape, 1, (-1, 2), budget)
    assert len(everything) == 9 * 4
    for world in (1, 2, 3, 4):
        parts = [zshift_chunks_at(shape, 1, (-1, 2), budget, r, world) for r in range(world)]
        assert all(p == everything[r::world] for r, p in enumerate(parts))


def test_chunks_refuse_bad_arguments():
    for kw in (dict(chunk_bytes=0), dict(chunk_bytes=-5), dict(rank=1), dict(rank=-1), dict(rank=2, world_size=2),
               dict(world_size=0)):
        with pytest.raises(ValueError):
            zshift_chunks_at((4, 4, 4), 2, (0, 0), **kw)
    for r in (0, 9, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            zshift_chunks_at((4, 4, 4), r, (0, 0))
    for reach in ((1, 2), (-2, -1), (0,), (0, 0, 0), 0, None, (0.0, 1), (True, 1), (-1025, 0), (0, 1025), "ab"):
        with pytest.raises(ValueError):
            zshift_chunks_at((4, 4, 4), 2, reach)
    for shape in ((4,), (1, 2, 3, 4)):
        with pytest.raises(ValueError):
            zshift_chunks_at(shape, 2, (0, 0))


# -------------------------------------------------------------------------------------------------- shift_counts_at
def test_counts_equal_brute_force():
    rng = np.random.default_rng(5)
    for shape, tile, r in (((3, 11, 13), (4, 5), 2), ((3, 7, 9), (7, 5), 3), ((4, 5, 7), (1, 1), 1), ((3, 9, 6), (2048, 4), 1)):
        gy, gx = AR.grid(shape, tile)
        C = rng.integers(-3, 4, (shape[0] - 1, gy, gx, 2))
        C[0, 0, 0] = (shape[1] + r, 0)                                              # the window wholly below the section
        C[-1, -1, -1] = (0, -shape[2] - r)                                          # and wholly left of it
        C[0, 0, -1] = (-1024, 1024)
        n = shift_counts_at(shape, tile, r, C)
        assert n.dtype == np.int64 and np.array_equal(n, AR.counts_at_brute(shape, tile, r, C))
        assert not n[0, 0, 0].any() and not n[-1, -1, -1].any() and n.any()
        assert tile == (1, 1) or ((n > 0) & (n < n.max())).any()                    # windows partly outside
        zero = shift_counts_at(shape, tile, r, np.zeros((shape[0] - 1, 2), np.int64))
        assert np.array_equal(zero, np.broadcast_to(shift_counts(shape, tile, r), zero.shape))
    assert shift_counts_at((9, 6), 4, 2, np.zeros((0, 2), np.int64)).shape == (0, 3, 2, 5, 5)
    for a in (((4, 4, 4), 0, 2), ((4, 4, 4), 2049, 2), ((4, 4, 4), 4, 0), ((4, 4, 4), 4, 9), ((4,), 4, 2)):
        with pytest.raises(ValueError):
            shift_counts_at(*a, np.zeros((3, 2), np.int64))


# ---------------------------------------------------------------------------------------------------- shift_centers
def test_centers_broadcast_and_refusals():
    per_pair = np.array([[1, -2], [1024, -1024], [0, 7]], np.int32)
    C = shift_centers(per_pair, (4, 9, 6), (4, 4))
    assert C.dtype == np.int64 and C.shape == (3, 3, 2, 2) and (C == per_pair[:, None, None, :]).all()
    C[0, 0, 0] = 5                                                                  # a copy of its own: writable
    full = np.arange(3 * 3 * 2 * 2).reshape(3, 3, 2, 2).astype(np.uint8)
    assert np.array_equal(shift_centers(full, (4, 9, 6), 4), full) and shift_centers(full, (4, 9, 6), 4).dtype == np.int64
    assert shift_centers(np.zeros((0, 2), np.int64), (9, 6), 4).shape == (0, 3, 2, 2)          # one image: no pairs
    assert shift_centers(np.zeros((0, 3, 2, 2), np.int64), (1, 9, 6), 4).shape == (0, 3, 2, 2)
    for bad in (per_pair[:2], per_pair.astype(np.float64), per_pair[:, :1], full[:, :2], full[..., :1], per_pair == 0,
                per_pair[0], None, full.reshape(3, 6, 2)):
        with pytest.raises(ValueError):
            shift_centers(bad, (4, 9, 6), 4)
    far = full.astype(np.int64)
    far[2, 1, 0] = (3, -1025)
    with pytest.raises(ValueError, match=r"pair 2, tile \(1, 0\)"):
        shift_centers(far, (4, 9, 6), 4)
    with pytest.raises(ValueError, match="pair 1"):
        shift_centers(np.array([[0, 0], [1025, 0], [0, 0]]), (4, 9, 6), 4)
    for shape, tile in (((4,), 4), ((4, 9, 6), 0), ((4, 9, 6), 2049)):
        with pytest.raises(ValueError):
            shift_centers(per_pair, shape, tile)


# --------------------------------------------------------------------------------- zero centres: the existing functions
def test_zero_centres_reproduce_the_siblings_on_the_fixture():
    q = SR.fixture_sums()
    n = shift_counts(SR.FIX_SHAPE, TILE, RADIUS)
    Z = SR.FIX_SHAPE[0]
    zero = np.zeros((Z - 1, 2), np.int64)
    n_at = shift_counts_at(SR.FIX_SHAPE, TILE, RADIUS, zero)
    assert n_at.shape == (Z - 1,) + n.shape and (n_at == n).all()
    c, c_at = shift_scores(q, n), shift_scores_at(q, n_at)
    assert c_at.dtype == c.dtype and c_at.tobytes() == c.tobytes()
    for centers in (zero, np.zeros((Z - 1, 3, 4, 2), np.int32)):
        s, s_at = section_shifts(q, n), section_shifts_at(q, n_at, centers)
        assert isinstance(s_at, Shifts)
        for a, b in zip(s[:4], s_at[:4]):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        assert s.unresolved == s_at.unresolved == sorted(SR.FIX_PLANTED)
        u, u_at = shift_subpixel(q, n), shift_subpixel_at(q, n_at, centers)
        assert isinstance(u_at, SubShifts)
        for a, b in zip(u, u_at):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    s_at = section_shifts_at(q, n_at, zero, min_corr=0.95)
    assert s_at.decided.tobytes() == section_shifts(q, n, min_corr=0.95).decided.tobytes()
    assert shift_scores_at(q[:1], n_at[:0]).shape == (0, 3, 4, 9, 9)


# ---------------------------------------------------------------------------------------------------- rule by rule
def _sums(scores):
    """q of one pair and 1 x 3 tiles with the given correlations (in hundredths) per tile and offset, for n = 100."""
    q = np.zeros((2, 1, 3, 5, 5, 5), np.int64)
    q[0, ..., 1] = q[0, ..., 3] = 100                            # A = B = 100 x 100
    q[0, ..., 4] = scores                                        # N = 100 x scores: c = scores / 100
    return q


def test_section_shifts_at_rule_by_rule():
    n = np.full((1, 1, 3, 5, 5), 100, np.int64)
    C = np.array([[[[10, -20], [12, -20], [10, 30]]]], np.int64)                    # [1, 1, 3, 2]
    sc = np.zeros((1, 3, 5, 5), np.int64)
    sc[0, 0, 2, 2] = sc[0, 0, 1, 2] = sc[0, 0, 3, 3] = 50                           # a tie: the smallest LOCAL displacement,
    sc[0, 1, 1, 2] = sc[0, 1, 2, 1] = sc[0, 1, 3, 2] = 50                           # then the smaller dy, then dx
    sc[0, 2, 3, 1] = sc[0, 2, 1, 3] = sc[0, 2, 3, 3] = 50
    s = section_shifts_at(_sums(sc), n, C)
    assert s.tiles[0, 0].tolist() == [[10, -20], [11, -20], [9, 31]]                # totals: centre + local
    assert s.decided.all() and (s.peak == 0.5).all() and s.unresolved == []
    assert s.pairs.tolist() == [[10, -20]]                                          # lower medians of (10, 11, 9), (-20, -20, 31)
    sc[0, 1] = 0
    sc[0, 1, 0, 2] = 90                                                             # local (-2, 0): on the rim of ITS window,
    s = section_shifts_at(_sums(sc), n, C)                                          # though the total (10, -20) is not far
    assert s.tiles[0, 0, 1].tolist() == [10, -20] and s.decided[0, 0].tolist() == [True, False, True]
    assert s.pairs.tolist() == [[9, -20]]                                           # sorted[(2 - 1) // 2] of (10, 9), (-20, 31)
    sc[0, 1] = 0
    sc[0, 1, 2, 2] = 90                                                             # the centre itself, a total of (12, -20)
    s = section_shifts_at(_sums(sc), n, C)                                          # beyond any radius: decided
    assert s.tiles[0, 0, 1].tolist() == [12, -20] and s.decided.all()
    s = section_shifts_at(_sums(sc * 0), n, C)                                      # nothing correlates: the guess stands
    assert s.unresolved == [0] and not s.decided.any()
    assert s.pairs.tolist() == [[10, -20]]                                          # lower medians of the centres
    assert s.tiles[0, 0].tolist() == C[0, 0].tolist()                               # local (0, 0) everywhere
    s = section_shifts_at(_sums(sc * 0), n, np.array([[7, -3]]))                    # one centre per pair
    assert s.pairs.tolist() == [[7, -3]] and s.unresolved == [0]
    u = shift_subpixel_at(_sums(sc), n, C)
    assert u.offsets[0, 0, 1].tolist() == [12.0, -20.0]                             # a lone peak: the vertex is its middle
    sc[0, 1, 2, 3] = 45                                                             # a neighbour along x pulls it over
    u = shift_subpixel_at(_sums(sc), n, C)
    want = (0 - 45) / (2.0 * (0 - 2 * 90 + 45))
    assert u.offsets[0, 0, 1, 0] == 12.0 and u.offsets[0, 0, 1, 1] == -20.0 + want and 0 < want < 0.5
    s = section_shifts_at(_sums(sc)[:1], n[:0], C[:0])                              # one section: no pair
    assert s.pairs.shape == (0, 2) and s.tiles.shape == (0, 1, 3, 2) and s.unresolved == []


def test_the_at_verdicts_refuse_bad_arguments():
    n = np.full((1, 1, 3, 5, 5), 100, np.int64)
    q, C = _sums(np.zeros((1, 3, 5, 5), np.int64)), np.zeros((1, 1, 3, 2), np.int64)
    for bq, bn, bc in ((q, n[0], C), (q, n.astype(np.float64), C), (q[..., :4], n, C), (q, n, C[0]), (q, n, C[:, :, :2]),
                       (q, n, C.astype(np.float64)), (q, n, np.zeros((2, 2), np.int64)), (q.astype(np.float32), n, C)):
        with pytest.raises(ValueError):
            section_shifts_at(bq, bn, bc)
        with pytest.raises(ValueError):
            shift_subpixel_at(bq, bn, bc)
    with pytest.raises(ValueError):
        shift_scores_at(q, n[0])
    for kw in (dict(min_corr=0), dict(min_corr=1), dict(min_corr="0.1"), dict(min_corr=None), dict(min_corr=True)):
        with pytest.raises(ValueError):
            section_shifts_at(q, n, C, **kw)


# ------------------------------------------------------------------------------------------- the driver, on the host
GOOD = list(range(8))


def test_the_fixture_is_what_it_claims():
    v, pairs = AR.big_jump_volume(), AR.big_pairs()
    assert v.shape == AR.BIG_SHAPE == (10, 160, 192) and v.dtype == np.uint8
    assert {z: tuple(pairs[z]) for z in AR.BIG_PLANTED} == AR.BIG_PLANTED
    assert (np.abs(np.delete(pairs, list(AR.BIG_PLANTED), axis=0)) <= 1).all()
    for z in range(9):                                           # section z + 1 at (y + dy, x + dx) is section z at (y, x)
        dy, dx = pairs[z]
        a = v[z, max(0, -dy):160 - max(0, dy), max(0, -dx):192 - max(0, dx)].astype(np.int64)
        b = v[z + 1, max(0, dy):160 + min(0, dy), max(0, dx):192 + min(0, dx)].astype(np.int64)
        assert np.corrcoef(a.ravel(), b.ravel())[0, 1] > 0.9
    # the coarsest search sees d / 2^levels, and trusts it where it rounds to at most radius - 1: |d| < (radius - 1/2) 2^levels
    reach = (AR.BIG_RADIUS - 0.5) * 2 ** AR.BIG_LEVELS
    assert all(max(abs(a), abs(b)) < reach for z, (a, b) in AR.BIG_PLANTED.items() if z != 8) and 44 > reach
    assert all(max(abs(a), abs(b)) > reach / 2 for a, b in (AR.BIG_PLANTED[5], AR.BIG_PLANTED[7]))   # beyond two levels
    assert max(abs(a) for a in AR.BIG_PLANTED[2]) < reach / 2


def test_plain_section_shifts_gets_the_jumps_wrong_without_saying_so():
    """The defect: at radius 4 the planted pairs come back as small offsets decided by a few chance peaks."""
    v = AR.big_jump_volume()
    s = section_shifts(SR.volume_sums(v, (AR.BIG_TILE,) * 2, AR.BIG_RADIUS), shift_counts(v.shape, AR.BIG_TILE, AR.BIG_RADIUS))
    for z in (2, 5, 7):
        assert tuple(s.pairs[z]) != AR.BIG_PLANTED[z] and z not in s.unresolved
        assert 0 < s.decided[z].sum() < 10


def test_the_driver_finds_the_jumps_within_reach_and_reports_the_one_beyond():
    got = AR.host_driver()
    assert isinstance(got, CoarseShifts) and isinstance(got.shifts, Shifts)
    s, pairs = got.shifts, AR.big_pairs()
    assert s.pairs.dtype == np.int64 and s.pairs.shape == (9, 2) and s.tiles.shape == (9, 5, 6, 2)
    assert got.q.shape == (10, 5, 6, 9, 9, 5) and got.n.shape == (9, 5, 6, 9, 9) and got.centers.shape == (9, 5, 6, 2)
    assert np.array_equal(s.pairs[GOOD], pairs[GOOD])                               # exact, the three planted ones too
    for z in GOOD:
        exact = (s.tiles[z] == pairs[z]).all(axis=-1) & s.decided[z]
        print(z, "decided", int(s.decided[z].sum()), "exact and decided", int(exact.sum()), "of 30")
        assert exact.sum() >= 27, z                                                 # at least 90 % of 30 tiles
    assert s.unresolved == [8] and tuple(s.pairs[8]) == (0, 0)                      # beyond reach: not moved on a guess
    assert 0 < s.decided[8].sum() < 15                                              # chance peaks decide some: the fraction tells
    # the verdict is section_shifts_at's on the returned sums, counts and centres, but for the unresolved pair
    again = section_shifts_at(got.q, got.n, got.centers)
    assert np.array_equal(again.pairs[GOOD], s.pairs[GOOD]) and np.array_equal(again.tiles, s.tiles)
    assert np.array_equal(got.n, shift_counts_at(AR.BIG_SHAPE, AR.BIG_TILE, AR.BIG_RADIUS, got.centers))
    assert np.array_equal(got.q, AR.volume_sums_at(AR.big_jump_volume(), got.centers, (32, 32), 4))
    assert np.abs(got.centers).max() <= 3 * (2 ** 4 - 2)                            # (radius - 1) (2^(levels + 1) - 2)
    sub = shift_subpixel_at(got.q, got.n, got.centers)
    assert np.abs(sub.offsets[GOOD] - s.tiles[GOOD])[s.decided[GOOD]].max() <= 0.5


def test_fewer_levels_reach_less_far():
    s, pairs = AR.host_driver(2).shifts, AR.big_pairs()
    for z in (5, 7):                                             # beyond 3 x 2^2 = 12
        assert z in s.unresolved or tuple(s.pairs[z]) != tuple(pairs[z])
    for z in (0, 1, 2, 3, 4, 6):                                 # (11, -9) is within it
        assert tuple(s.pairs[z]) == tuple(pairs[z]) and z not in s.unresolved


def test_min_decided_moves_a_pair_to_unresolved(monkeypatch):
    monkeypatch.setattr(utils, "volume_rescale", AR.host_rescale)
    monkeypatch.setattr(utils, "section_shift_sums_at", AR.host_sums_at)
    v = AR.big_jump_volume()[7:, :64, :96]                       # 3 sections: (6, 27), (44, 0); 2 x 3 tiles, two levels
    assert section_shifts_coarse_to_fine(v, 32, 4, 2, min_decided=1.0).shifts.unresolved == [0, 1]
    loose = section_shifts_coarse_to_fine(v, 32, 4, 2, min_decided=0).shifts
    strict = section_shifts_coarse_to_fine(v, 32, 4, 2, min_decided=0.5).shifts
    k = loose.decided.sum(axis=(1, 2))
    assert np.array_equal(loose.decided, strict.decided) and np.array_equal(loose.tiles, strict.tiles)
    for z in range(2):
        assert (z in loose.unresolved) == (k[z] == 0)
        assert (z in strict.unresolved) == (k[z] < 3)
        assert z not in strict.unresolved or tuple(strict.pairs[z]) == (0, 0)
    out = [np.zeros((3, 32, 48), np.uint8), np.zeros((3, 16, 24), np.uint8)]        # the pyramid lands in `coarse`
    st = {}
    section_shifts_coarse_to_fine(v, 32, 4, 2, coarse=out, stats=st)
    assert np.array_equal(out[0], AR.halve(v)) and np.array_equal(out[1], AR.halve(AR.halve(v)))
    assert set(st) == {"read_s", "chunks"}


def test_the_driver_refuses_bad_arguments_on_the_host():
    v = np.zeros((3, 64, 80), np.uint8)
    for a, kw in (((v.astype(np.int16),), {}), ((v[0],), {}), ((v,), dict(tile=0)), ((v,), dict(radius=0)),
                  ((v,), dict(radius=9)), ((v,), dict(levels=0)), ((v,), dict(levels=7)), ((v,), dict(levels=2.0)),
                  ((v,), dict(levels=True)), ((v,), dict(levels=3)), ((v,), dict(levels=2, radius=5)),
                  ((v,), dict(min_corr=0)), ((v,), dict(min_corr=1)), ((v,), dict(min_decided=-0.1)),
                  ((v,), dict(min_decided=1.5)), ((v,), dict(min_decided="1")), ((v,), dict(min_decided=None)),
                  ((v,), dict(min_decided=True)), ((v,), dict(chunk_bytes=0)),
                  ((v,), dict(levels=2, coarse=[np.zeros((3, 32, 40), np.uint8)])),
                  ((v,), dict(levels=1, coarse=[np.zeros((3, 32, 41), np.uint8)])),
                  ((v,), dict(levels=1, coarse=[np.zeros((3, 32, 40), np.int8)]))):
        with pytest.raises(ValueError):
            section_shifts_coarse_to_fine(*a, **kw)
    vol = np.zeros((4, 6, 8), np.uint8)
    zero = np.zeros((3, 2), np.int64)
    for a, kw in (((vol.astype(np.int16), zero), {}), ((vol, zero), dict(tile=0)), ((vol, zero), dict(radius=9)),
                  ((vol, zero), dict(chunk_bytes=0)), ((vol, zero), dict(rank=1)), ((vol, zero[:2]), {}),
                  ((vol, zero.astype(np.float64)), {}), ((vol, zero + 1025), {}), ((vol, None), {}),
                  ((vol[0, 0], zero), {})):
        with pytest.raises(ValueError):
            section_shift_sums_at(*a, **kw)


def test_signatures_and_the_reference_alias():
    import transfer_em.utils as alias
    from transfer_em_amd import _lib
    names = ("shift_centers", "zshift_chunks_at", "shift_counts_at", "section_shift_sums_at", "shift_scores_at",
             "section_shifts_at", "shift_subpixel_at", "section_shifts_coarse_to_fine", "CoarseShifts",
             "SHIFT_MAX_CENTER")
    for name in names:
        assert getattr(alias, name) is getattr(utils, name)
    sig = lambda f: list(inspect.signature(f).parameters)
    assert utils.SHIFT_MAX_CENTER == 1024
    assert sig(shift_centers) == ["centers", "vol_shape", "tile"]
    assert sig(zshift_chunks_at) == ["vol_shape", "radius", "reach", "chunk_bytes", "rank", "world_size"]
    assert sig(shift_counts_at) == ["vol_shape", "tile", "radius", "centers"]
    assert sig(section_shift_sums_at) == ["volume", "centers", "tile", "radius", "chunk_bytes", "rank", "world_size",
                                          "device", "stats"]
    assert sig(shift_scores_at) == ["q", "n"]
    assert sig(section_shifts_at) == sig(shift_subpixel_at) == ["q", "n", "centers", "min_corr"]
    assert sig(section_shifts_coarse_to_fine) == ["volume", "tile", "radius", "levels", "min_corr", "min_decided", "coarse",
                                                  "chunk_bytes", "device", "stats"]
    d = {k: p.default for k, p in inspect.signature(section_shifts_coarse_to_fine).parameters.items()}
    assert (d["tile"], d["radius"], d["levels"], d["min_corr"], d["min_decided"]) == (128, 4, 3, 0.1, 0.5)
    assert CoarseShifts._fields == ("shifts", "q", "n", "centers")
    assert len(_lib._SIGS["tem_u8_zshift_tiles_at"]) == 21
    assert len(_lib._SIGS["tem_u8_zshift_tiles"]) == 17
