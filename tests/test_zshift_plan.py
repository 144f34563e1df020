"""The host side of the section-shift measurement, without a GPU: the slab plan zshift_chunks, shift_counts against
brute force, shift_scores against np.corrcoef, section_shifts on the fixture of jittered sections (its sums from the
numpy reference zshift_ref), shift_positions, volume_shift, the link to the defect detector, and every ValueError."""
import inspect

import numpy as np
import pytest

import zcorr_ref as ZR
import zshift_ref as SR
from transfer_em_amd.utils import (HIST_CHUNK_BYTES, SHIFT_MAX_RADIUS, Shifts, hist_chunks, section_scores,
                                   section_shift_sums, section_shifts, shift_counts, shift_positions, shift_scores,
                                   volume_shift, zshift_chunks)

TILE, RADIUS = (SR.FIX_TILE, SR.FIX_TILE), SR.FIX_RADIUS
ORDINARY = [z for z in range(SR.FIX_SHAPE[0] - 1) if z not in SR.FIX_PLANTED]


# ---------------------------------------------------------------------------------------------------- zshift_chunks
def _size(box):
    return int(np.prod([hi - lo for lo, hi in box]))


@pytest.mark.parametrize("shape", [(7, 9, 5), (1, 9, 5), (2, 3, 4), (9, 5)])
def test_chunks_partition_the_volume_with_their_halo_within_the_budget(shape):
    Z, Y, X = shape if len(shape) == 3 else (1,) + shape
    for r in (1, 2, 8):
        for budget in (None, Z * Y * X, 3 * Y * X, 2 * Y * X, 2 * Y * X - 1, Y * X, 14 * X, 12 * X, 7 * X, 2 * X, X, 1):
            chunks = zshift_chunks(shape, r, budget)
            seen = np.zeros((Z, Y, X), np.int32)
            for (cz, cy, cx), (rz, ry, rx) in chunks:
                seen[cz[0]:cz[1], cy[0]:cy[1], cx[0]:cx[1]] += 1
                assert cz[0] < cz[1] and cy[0] < cy[1] and cx == (0, X) and rx == cx
                assert rz == (cz[0], min(cz[1] + 1, Z))                            # one section more, but at the last
                assert ry == (max(cy[0] - r, 0), min(cy[1] + r, Y))                # r rows more, but at the faces
                assert cy == (0, Y) or cz[1] - cz[0] == 1                           # whole sections, or rows of one
                b = HIST_CHUNK_BYTES if budget is None else budget
                assert _size((rz, ry, rx)) <= b or cy[1] - cy[0] == 1               # one core row at the least
            assert (seen == 1).all()
            order = [(c[0][0], c[1][0]) for c, _ in chunks]
            assert order == sorted(order)
            cores = [c for c, _ in chunks]                                          # hist_chunks' kind of cuts
            assert all(c[1] == (0, Y) for c in cores) or all(c[0][1] - c[0][0] == 1 for c in cores)


def test_chunks_take_as_much_as_the_budget_allows():
    shape = (10, 6, 8)
    assert zshift_chunks(shape, 2) == [(((0, 10), (0, 6), (0, 8)),) * 2]
    assert [c[0] for c, _ in zshift_chunks(shape, 2, 4 * 48)] == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert [s[0] for _, s in zshift_chunks(shape, 2, 4 * 48)] == [(0, 4), (3, 7), (6, 10), (9, 10)]
    assert [c for c, _ in zshift_chunks(shape, 2, 4 * 48)] == hist_chunks(((0, 10), (0, 6), (0, 8)), 3 * 48)
    rows = zshift_chunks(shape, 1, 2 * 48 - 1)                   # two sections no longer fit: 5 rows twice, 3 + 2 halo
    assert len(rows) == 10 * 2 and rows[0] == (((0, 1), (0, 3), (0, 8)), ((0, 2), (0, 4), (0, 8)))
    assert rows[1] == (((0, 1), (3, 6), (0, 8)), ((0, 2), (2, 6), (0, 8)))
    assert rows[-1] == (((9, 10), (3, 6), (0, 8)), ((9, 10), (2, 6), (0, 8)))
    assert len(zshift_chunks(shape, 2, 2 * 48 - 1)) == 60                           # 5 rows twice: 1 + 4 of halo
    assert len(zshift_chunks(shape, 8, 1)) == 60
    assert zshift_chunks((1, 6, 8), 3, 48) == [(((0, 1), (0, 6), (0, 8)),) * 2]     # one section: nothing above it


def test_chunks_go_round_robin_to_the_ranks():
    shape, budget = (9, 8, 6), 60
    everything = zshift_chunks(shape, 1, budget)
    assert len(everything) == 9 * 3
    for world in (1, 2, 3, 4):
        parts = [zshift_chunks(shape, 1, budget, r, world) for r in range(world)]
        assert all(p == everything[r::world] for r, p in enumerate(parts))
        assert max(map(len, parts)) - min(map(len, parts)) <= 1


def test_chunks_refuse_bad_arguments():
    for kw in (dict(chunk_bytes=0), dict(chunk_bytes=-5), dict(rank=1), dict(rank=-1), dict(rank=2, world_size=2),
               dict(world_size=0)):
        with pytest.raises(ValueError):
            zshift_chunks((4, 4, 4), 2, **kw)
    for r in (0, 9, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            zshift_chunks((4, 4, 4), r)
    for shape in ((4,), (1, 2, 3, 4)):
        with pytest.raises(ValueError):
            zshift_chunks(shape, 2)


# ----------------------------------------------------------------------------------------------------- shift_counts
def test_counts_equal_brute_force():
    for shape, tile, r in (((3, 11, 13), (4, 5), 2), ((11, 13), (4, 5), 2), ((2, 7, 9), (7, 9), 8), ((1, 5, 7), (1, 1), 1),
                           ((2, 9, 6), (2048, 4), 3)):
        n = shift_counts(shape, tile, r)
        assert n.dtype == np.int64 and np.array_equal(n, SR.counts_brute(shape, tile, r))
        assert np.array_equal(n, SR.counts(shape, tile, r))
        assert n[:, :, r, r].sum() == shape[-2] * shape[-1]                         # no offset: every voxel, once
    n = shift_counts(SR.FIX_SHAPE, SR.FIX_TILE, RADIUS)
    assert n.shape == (3, 4, 9, 9) and n[1, 1].min() == 32 * 32 and n[2, 3, 4, 4] == 26 * 24
    assert n[0, 0, 0, 0] == 28 * 28 and n[2, 3, 8, 8] == 22 * 20                    # the corners lose r rows and columns
    for a in (((4, 4, 4), 0, 2), ((4, 4, 4), 2049, 2), ((4, 4, 4), 4, 0), ((4, 4, 4), 4, 9), ((4,), 4, 2)):
        with pytest.raises(ValueError):
            shift_counts(*a)


# ----------------------------------------------------------------------------------------------------- shift_scores
def test_the_two_references_agree():
    v = SR.jitter_volume()[:3, :40, :50]
    a = SR.tile_sums_direct(v, 0, 3, 0, 40, 0, 40, 16, 24, 3, 3, 2)
    assert np.array_equal(a, SR.tile_sums(v, 0, 3, 0, 40, 0, 40, 16, 24, 3, 3, 2))
    assert not a[2].any() and a[:2, :, :2].all() and not a[:2, :, 2, :, 4].any()    # the 2 last columns at dx = 2: none
    a = SR.tile_sums_direct(v[:, 5:30], 1, 3, 2, 20, 7, 40, 16, 24, 4, 3, 2)       # a block of rows 7...31 of 40
    assert np.array_equal(a, SR.tile_sums(v[:, 5:30], 1, 3, 2, 20, 7, 40, 16, 24, 4, 3, 2))
    assert a[0, :2, :2].all() and not a[0, 2:].any() and not a[1].any()            # core rows 9...26: tiles 0 and 1


def test_scores_equal_corrcoef_on_the_fixture():
    v = SR.jitter_volume()[:5]
    q = SR.fixture_sums()[:5]
    n = shift_counts(v.shape, TILE, RADIUS)
    c = shift_scores(q, n)
    want = SR.shifted_corr(v, TILE, RADIUS)
    assert c.dtype == np.float64 and c.shape == want.shape == (4, 3, 4, 9, 9)
    assert np.abs(c - want).max() <= 1e-12
    flat = np.array(v)
    flat[2, :40, :40] = 77                                                          # a constant tile and its surroundings
    c = shift_scores(SR.volume_sums(flat, TILE, RADIUS), n)
    assert np.abs(c - SR.shifted_corr(flat, TILE, RADIUS)).max() <= 1e-12
    assert not c[1, 0, 0].any() and not c[2, 0, 0].any() and c[0, 0, 0].all()
    assert shift_scores(q[:1], n).shape == (0, 3, 4, 9, 9) and shift_scores(q[:0], n).shape == (0, 3, 4, 9, 9)


def test_scores_at_the_extremes_stay_exact():
    """A full 2048 x 2048 tile of 0 / 255 halves: the terms reach 2^60 and the result is still +-1 to the last bits."""
    N, k = 2048 * 2048, 2048 * 1024
    q = np.zeros((3, 1, 1, 3, 3, 5), np.int64)
    q[:2, 0, 0, 1, 1] = [255 * k, 65025 * k, 255 * k, 65025 * k, 65025 * k]        # the same half ...
    q[1, 0, 0, 1, 1, 4] = 0                                                         # ... and its complement
    n = np.full((1, 1, 3, 3), N, np.int64)
    c = shift_scores(q, n)
    assert abs(c[0, 0, 0, 1, 1] - 1.0) <= 1e-12 and abs(c[1, 0, 0, 1, 1] + 1.0) <= 1e-12
    assert shift_scores(q.astype(np.uint64), n.astype(np.int32))[0, 0, 0, 1, 1] == c[0, 0, 0, 1, 1]


# --------------------------------------------------------------------------------------------------- section_shifts
def test_section_shifts_finds_every_ordinary_pair_and_leaves_the_planted_ones_unresolved():
    q, pairs = SR.fixture_sums(), SR.fixture_pairs()
    n = shift_counts(SR.FIX_SHAPE, TILE, RADIUS)
    s = section_shifts(q, n)
    assert isinstance(s, Shifts) and s.pairs.dtype == np.int64 and s.pairs.shape == (23, 2)
    assert s.tiles.dtype == np.int64 and s.tiles.shape == (23, 3, 4, 2)
    assert s.peak.shape == (23, 3, 4) and s.decided.dtype == bool and s.decided.shape == (23, 3, 4)
    c = shift_scores(q, n)
    assert np.array_equal(s.peak, c.max(axis=(3, 4)))
    assert (np.abs(pairs[ORDINARY]) <= 1).all()
    for z in ORDINARY:                                           # every tile: exactly the planted offset, and decided
        assert (s.tiles[z] == pairs[z]).all() and s.decided[z].all(), z
        assert tuple(s.pairs[z]) == tuple(pairs[z])
    for z, step in SR.FIX_PLANTED.items():                       # every tile on the rim: unresolved, (0, 0)
        assert max(abs(step[0]), abs(step[1])) >= RADIUS
        assert (np.abs(s.tiles[z]).max(axis=-1) == RADIUS).all() and not s.decided[z].any(), z
        assert tuple(s.pairs[z]) == (0, 0) and (s.peak[z] > 0.1).all()
    assert s.unresolved == sorted(SR.FIX_PLANTED)
    assert (s.tiles[7] == (4, -1)).all()                         # at the radius the offset is seen, and not trusted


def test_section_shifts_rule_by_rule():
    n = np.full((1, 3, 5, 5), 100, np.int64)

    def sums(scores):
        """q of one pair and 1 x 3 tiles with the given correlations (in hundredths) per tile and offset."""
        q = np.zeros((2, 1, 3, 5, 5, 5), np.int64)
        q[0, ..., 0] = q[0, ..., 2] = 0
        q[0, ..., 1] = q[0, ..., 3] = 100                        # A = B = 100 x 100
        q[0, ..., 4] = scores                                    # N = 100 x scores: c = scores / 100
        return q
    sc = np.zeros((1, 3, 5, 5), np.int64)
    sc[0, 0, 2, 2] = sc[0, 0, 1, 2] = sc[0, 0, 2, 3] = sc[0, 0, 3, 3] = 50          # a tie: the smallest displacement,
    sc[0, 1, 1, 2] = sc[0, 1, 2, 1] = sc[0, 1, 3, 2] = 50                           # then the smaller dy, then dx
    sc[0, 2, 3, 1] = sc[0, 2, 1, 3] = sc[0, 2, 3, 3] = 50
    s = section_shifts(sums(sc), n)
    assert s.tiles[0, 0].tolist() == [[0, 0], [-1, 0], [-1, 1]] and s.decided.all() and (s.peak == 0.5).all()
    assert s.pairs.tolist() == [[-1, 0]] and s.unresolved == []                     # lower medians of (0, -1, -1), (0, 0, 1)
    sc[0, 2] = 0
    sc[0, 2, 3, 3] = 10                                                             # not above min_corr: two tiles left
    s = section_shifts(sums(sc), n)
    assert s.decided[0, 0].tolist() == [True, True, False] and s.pairs.tolist() == [[-1, 0]]   # sorted[(2 - 1) // 2]
    assert section_shifts(sums(sc), n, min_corr=0.05).decided.all()
    sc[0, 1] = 0
    sc[0, 1, 0, 2] = 90                                                             # on the rim: not decided
    s = section_shifts(sums(sc), n)
    assert s.tiles[0, 0, 1].tolist() == [-2, 0] and s.decided[0, 0].tolist() == [True, False, False]
    assert s.pairs.tolist() == [[0, 0]] and s.unresolved == []
    s = section_shifts(sums(sc * 0), n)                                             # nothing correlates
    assert s.unresolved == [0] and s.pairs.tolist() == [[0, 0]] and not s.tiles.any()
    s = section_shifts(sums(sc)[:1], n)                                             # one section: no pair
    assert s.pairs.shape == (0, 2) and s.tiles.shape == (0, 1, 3, 2) and s.unresolved == []


def test_section_shifts_and_scores_refuse_bad_arguments():
    q, n = SR.fixture_sums(), shift_counts(SR.FIX_SHAPE, TILE, RADIUS)
    for kw in (dict(min_corr=0), dict(min_corr=1), dict(min_corr="0.1"), dict(min_corr=None), dict(min_corr=True)):
        with pytest.raises(ValueError):
            section_shifts(q, n, **kw)
    for bq, bn in ((q[..., :4], n), (q[0], n), (q.astype(np.float64), n), (q, n[:2]), (q, n.astype(np.float64)),
                   (q[:, :, :, :8], n[:, :, :8]), (q[:, :, :, :8, :8], n[:, :, :8, :8]), (q[:, :, :, :1, :1], n[:, :, :1, :1])):
        with pytest.raises(ValueError):
            shift_scores(bq, bn)
        with pytest.raises(ValueError):
            section_shifts(bq, bn)


# -------------------------------------------------------------------------------------------------- shift_positions
def test_positions_add_the_pairs_up_and_the_window_takes_the_trend_out():
    pairs = SR.fixture_pairs()
    P = shift_positions(pairs)
    assert P.dtype == np.int64 and P.shape == (24, 2) and np.array_equal(P, SR.fixture_positions())
    assert shift_positions(np.zeros((0, 2), np.int64)).tolist() == [[0, 0]]
    for w in (3, 5, 23, 99):
        got = shift_positions(pairs, w)
        want = np.empty_like(P)
        for z in range(24):
            for a in range(2):
                run = sorted(P[max(z - w // 2, 0):z + w // 2 + 1, a].tolist())
                want[z, a] = P[z, a] - run[(len(run) - 1) // 2]
        assert got.dtype == np.int64 and np.array_equal(got, want)
    # a steady oblique cut plus one jittered section: the window keeps the trend out of the correction
    steps = np.tile(np.array([[1, -2]], np.int64), (10, 1))
    steps[4] += (3, 0)
    steps[5] -= (3, 0)
    assert shift_positions(steps)[:, 0].tolist() == [0, 1, 2, 3, 4, 8, 6, 7, 8, 9, 10]
    assert shift_positions(steps, 3)[:, 0].tolist() == [0, 0, 0, 0, 0, 2, -1, 0, 0, 0, 1]
    assert not shift_positions(steps, 3)[1:-1, 1].any()
    assert shift_positions(steps.astype(np.int32)).dtype == np.int64
    for bad, kw in ((steps[:, :1], {}), (steps.astype(np.float64), {}), (steps[0], {}), (steps, dict(window=2)),
                    (steps, dict(window=1)), (steps, dict(window=4)), (steps, dict(window=3.0)), (steps, dict(window=True))):
        with pytest.raises(ValueError):
            shift_positions(bad, **kw)


# ----------------------------------------------------------------------------------------------------- volume_shift
def _kept(P, z, Y, X):
    dy, dx = int(P[z, 0]), int(P[z, 1])
    return slice(max(0, -dy), min(Y, Y - dy)), slice(max(0, -dx), min(X, X - dx))


def test_volume_shift_undoes_the_jitter(tmp_path):
    v, flat, P = SR.jitter_volume(), SR.flat_volume(), SR.fixture_positions()
    _, Y, X = v.shape
    got = volume_shift(v, P, fill=7)
    assert got.dtype == np.uint8 and got.shape == v.shape
    filled = np.ones(v.shape, bool)
    for z in range(v.shape[0]):
        ys, xs = _kept(P, z, Y, X)
        assert np.array_equal(got[z, ys, xs], flat[z, ys, xs]), z                  # the un-jittered crop
        filled[z, ys, xs] = False
        assert filled[z].sum() == Y * X - (Y - abs(P[z, 0])) * (X - abs(P[z, 1])) and (got[z][filled[z]] == 7).all()
    assert np.array_equal(got[0], v[0]) and np.abs(P).max() >= 8
    assert np.array_equal(volume_shift(v, P), np.where(filled, 0, got))             # the default fill: 0
    out = np.memmap(tmp_path / "out.u8", np.uint8, "w+", shape=v.shape)
    out[...] = 0xA5                                                                 # every voxel is written
    assert volume_shift(v, P, out=out, fill=7) is out and np.array_equal(np.asarray(out), got)
    src = np.memmap(tmp_path / "src.u8", np.uint8, "w+", shape=v.shape)
    src[...] = v
    src.flush()
    assert np.array_equal(volume_shift(np.memmap(tmp_path / "src.u8", np.uint8, "r", shape=v.shape), P, fill=7), got)
    for start, size in (((0, 0, 0), (120, 90, 24)), ((5, 7, 3), (100, 60, 11)), ((119, 89, 23), (1, 1, 1)),
                        ((0, 80, 10), (13, 10, 0))):
        (x, y, z), (nx, ny, nz) = start, size
        roi = volume_shift(v, P, start=start, size=size, fill=7)
        assert roi.shape == (nz, ny, nx) and np.array_equal(roi, got[z:z + nz, y:y + ny, x:x + nx])
    mask = (v > 128).astype(np.uint8)                                               # the same call moves a mask
    assert np.array_equal(volume_shift(mask, P, fill=1), np.where(filled, 1, got > 128).astype(np.uint8))
    wide = volume_shift(v.astype(np.int16), P, fill=-1)                             # another dtype: it is a copy
    assert wide.dtype == np.int16 and np.array_equal(wide, np.where(filled, -1, got.astype(np.int16)))
    far = np.zeros_like(P)
    far[1], far[2] = (90, 0), (0, -120)                                             # nothing of the section is left
    assert (volume_shift(v, far, fill=3)[1:3] == 3).all() and np.array_equal(volume_shift(v, far)[3:], v[3:])


def test_volume_shift_refuses_bad_arguments():
    v, P = np.zeros((4, 6, 8), np.uint8), np.zeros((4, 2), np.int64)
    for a, kw in (((v[0], P), {}), ((v, P[:3]), {}), ((v, P.astype(np.float64)), {}), ((v, P[:, :1]), {}),
                  ((v, P), dict(fill=256)), ((v, P), dict(fill=-1)), ((v, P), dict(fill=1.5)), ((v, P), dict(fill=None)),
                  ((v, P), dict(fill=True)), ((v, P), dict(out=np.zeros((4, 6, 8), np.int8))),
                  ((v, P), dict(out=np.zeros((4, 6, 9), np.uint8))), ((v, P), dict(start=(0, 0, 0), size=(9, 6, 4))),
                  ((v, P), dict(start=(0, 0), size=(8, 6))), ((v, P), dict(start=(1, 1, 1), size=(2, 2, 2), out=v))):
        with pytest.raises(ValueError):
            volume_shift(*a, **kw)


# ------------------------------------------------------------------------------------------ the link to the detector
def test_the_detector_sees_a_sound_stack_after_the_shift():
    """section_scores of the ordinary pairs that were displaced rises once the measured shifts are undone: compared on
    whole 32 x 32 tiles inside the frame that no fill reaches, before and after."""
    v = SR.jitter_volume()
    s = section_shifts(SR.fixture_sums(), shift_counts(v.shape, TILE, RADIUS))
    P = shift_positions(s.pairs)
    m = int(np.abs(P).max())
    moved = volume_shift(v, P)
    assert m + 64 <= v.shape[1] - m and m + 96 <= v.shape[2] - m
    frame = (slice(None), slice(m, m + 64), slice(m, m + 96))                       # 2 x 3 whole tiles
    assert volume_shift(np.ones_like(v), P)[frame].all()                            # no fill inside the frame
    before = section_scores(ZR.volume_sums(np.ascontiguousarray(v[frame]), TILE))
    after = section_scores(ZR.volume_sums(np.ascontiguousarray(moved[frame]), TILE))
    stepped = [z for z in ORDINARY if s.pairs[z].any()]
    assert len(stepped) >= 15
    for z in stepped:
        assert (after[z] > before[z]).all(), z                                      # every tile of every displaced pair
    for z in SR.FIX_PLANTED:                                                        # the unresolved pairs stay apart
        assert after[z].max() < after[ORDINARY].min()


# -------------------------------------------------------------------- section_shift_sums: refused before any GPU work
def test_section_shift_sums_refuses_bad_arguments_on_the_host():
    vol = np.zeros((4, 6, 8), np.uint8)
    for a, kw in (((vol.astype(np.int16),), {}), ((vol,), dict(tile=0)), ((vol,), dict(tile=2049)),
                  ((vol,), dict(tile=(4, 4, 4))), ((vol,), dict(tile=2.5)), ((vol,), dict(chunk_bytes=0)),
                  ((vol,), dict(rank=1)), ((vol,), dict(rank=0, world_size=0)), ((vol[0, 0],), {}),
                  ((vol[None],), {}), ((vol,), dict(radius=0)), ((vol,), dict(radius=9)), ((vol,), dict(radius=2.0)),
                  ((vol,), dict(radius=True)), ((vol,), dict(radius=None))):
        with pytest.raises(ValueError):
            section_shift_sums(*a, **kw)


def test_signatures_and_the_reference_alias():
    import transfer_em.utils as alias
    from transfer_em_amd import _lib, utils
    for name in ("zshift_chunks", "shift_counts", "section_shift_sums", "shift_scores", "section_shifts",
                 "shift_positions", "volume_shift", "Shifts", "SHIFT_MAX_RADIUS"):
        assert getattr(alias, name) is getattr(utils, name)
    sig = lambda f: list(inspect.signature(f).parameters)
    assert SHIFT_MAX_RADIUS == 8
    assert sig(zshift_chunks) == ["vol_shape", "radius", "chunk_bytes", "rank", "world_size"]
    assert sig(shift_counts) == ["vol_shape", "tile", "radius"]
    assert sig(section_shift_sums) == ["volume", "tile", "radius", "chunk_bytes", "rank", "world_size", "device", "stats"]
    assert inspect.signature(section_shift_sums).parameters["radius"].default == 4
    assert sig(shift_scores) == ["q", "n"] and sig(section_shifts) == ["q", "n", "min_corr"]
    assert sig(shift_positions) == ["pairs", "window"]
    assert sig(volume_shift) == ["volume", "positions", "out", "start", "size", "fill"]
    assert Shifts._fields == ("pairs", "tiles", "peak", "decided", "unresolved")
    assert len(_lib._SIGS["tem_u8_zshift_tiles"]) == 17
