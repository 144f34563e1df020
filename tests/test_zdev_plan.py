"""Host side of the z-median outliers, no GPU: section_neighbours, outlier_chunks and outlier_thresholds against the numpy
reference (zdev_ref) and their own contracts, the reference's identities, and the fixture's verdict from the reference
alone."""
import numpy as np
import pytest

import zdev_ref as ZD
from transfer_em_amd.utils import (OUTLIER_MAX_THR, OutlierThresholds, find_debris, hist_chunks, outlier_chunks,
                                   outlier_thresholds, section_neighbours, volume_outliers)


# ------------------------------------------------------------------------------------------------ section_neighbours
def test_neighbours_chain_bridges_gaps_and_ends():
    t = section_neighbours(6)
    assert t.dtype == np.int32 and t.tolist() == [[-1, -1], [0, 2], [1, 3], [2, 4], [3, 5], [-1, -1]]
    assert section_neighbours(0).shape == (0, 2) and section_neighbours(1).tolist() == [[-1, -1]]
    assert section_neighbours(2).tolist() == [[-1, -1]] * 2 and section_neighbours(3).tolist()[1] == [0, 2]
    t = section_neighbours(8, [3]).tolist()                                # a bridge: lag 2 on both sides of it
    assert t[2] == [1, 4] and t[3] == [-1, -1] and t[4] == [2, 5]
    t = section_neighbours(8, [0, 7]).tolist()                             # the first and last GOOD section
    assert t[0] == t[1] == t[6] == t[7] == [-1, -1] and t[2] == [1, 3]
    t = section_neighbours(12, [4, 5, 6], max_lag=3).tolist()              # 3 -> 7 is 4 apart: no verdict on either side
    assert t[3] == t[7] == [-1, -1] and t[2] == [1, 3] and t[8] == [7, 9]
    t = section_neighbours(12, [4, 5, 6], max_lag=4).tolist()
    assert t[3] == [2, 7] and t[7] == [3, 8]
    t = section_neighbours(17, list(range(1, 8)) + list(range(9, 16)), 8).tolist()
    assert t[8] == [0, 16] and sum(r != [-1, -1] for r in t) == 1
    rng = np.random.default_rng(0)
    for _ in range(40):
        Z, lag = int(rng.integers(0, 30)), int(rng.integers(1, 9))
        skip = rng.choice(Z, int(rng.integers(0, Z + 1)), replace=False).tolist() if Z else []
        assert np.array_equal(section_neighbours(Z, skip, lag), ZD.neighbours(Z, skip, lag)), (Z, skip, lag)
    assert np.array_equal(section_neighbours(9, iter([2, 2, 5])), ZD.neighbours(9, [2, 5]))


def test_neighbours_refuse_what_section_pairs_refuses():
    for kw in (dict(Z=-1), dict(Z=2.5), dict(Z=True), dict(Z=5, skip=[5]), dict(Z=5, skip=[-1]), dict(Z=5, skip=[1.5]),
               dict(Z=5, skip=3), dict(Z=5, max_lag=0), dict(Z=5, max_lag=9), dict(Z=5, max_lag="2")):
        with pytest.raises(ValueError):
            section_neighbours(**kw)


# ---------------------------------------------------------------------------------------------------- outlier_chunks
SHAPE = (32, 128, 192)


def _covers(chunks, box):
    seen = np.zeros(tuple(hi - lo for lo, hi in box), np.int32)
    for (cz, cy, cx), _ in chunks:
        seen[cz[0] - box[0][0]:cz[1] - box[0][0], cy[0] - box[1][0]:cy[1] - box[1][0], cx[0] - box[2][0]:cx[1] - box[2][0]] += 1
    return bool((seen == 1).all())


@pytest.mark.parametrize("radius", [0, 4, 7])
def test_chunks_cover_the_box_and_hold_their_hull(radius):
    Z, Y, X = SHAPE
    nbr = section_neighbours(Z, [12, 20, 21], 4)
    for box in (((0, Z), (0, Y), (0, X)), ((3, 29), (5, 99), (8, 68))):
        ny = min(box[1][1] + radius, Y) - max(box[1][0] - radius, 0)
        for budget, kind in ((1 << 30, "whole"), (7 * ny * X, "sections"), (3 * 20 * X, "rows"), (1, "one_row")):
            chunks = outlier_chunks(box, SHAPE, nbr, radius, budget)
            assert _covers(chunks, box), (box, kind)
            for (cz, cy, cx), (rz, ry, rx) in chunks:
                assert cx == box[2] and rx == (0, X)
                assert ry == (max(cy[0] - radius, 0), min(cy[1] + radius, Y))
                need = [z for z in range(*cz)] + [int(v) for z in range(*cz) for v in nbr[z] if v >= 0]
                assert rz == (min(need), max(need) + 1)                   # the hull, and nothing more
                planes, rows = rz[1] - rz[0], cy[1] - cy[0]
                halo = ry[1] - ry[0] - rows                               # the rows this slab reads around its core
                if planes * (rows + halo) * X > budget:                   # only where one row with its halo cannot fit
                    assert cz[1] - cz[0] == 1 and rows == 1 and planes * (1 + halo) * X > budget
                if cy != box[1]:                                          # rows of one section: whole, it does not fit,
                    assert cz[1] - cz[0] == 1 and planes * ny * X > budget
                    if cy[1] < box[1][1]:                                 # and no run could take one more row
                        assert planes * (rows + 1 + 2 * radius) * X > budget
                elif cz[1] < box[0][1]:                                   # sections: the next one's hull no longer fits
                    more = need + [cz[1]] + [int(v) for v in nbr[cz[1]] if v >= 0]
                    assert (max(more) + 1 - min(more)) * ny * X > budget
            if kind == "whole":
                assert len(chunks) == 1
            if kind == "sections":
                assert 1 < len(chunks) <= box[0][1] - box[0][0] and all(c[1] == box[1] for c, _ in chunks)
            if kind == "rows":
                assert all(c[0][1] - c[0][0] == 1 for c, _ in chunks) and any(c[1] != box[1] for c, _ in chunks)
            if kind == "one_row":
                assert len(chunks) == (box[0][1] - box[0][0]) * (box[1][1] - box[1][0])
            parts = [outlier_chunks(box, SHAPE, nbr, radius, budget, r, 3) for r in range(3)]
            assert sorted(sum(parts, [])) == sorted(chunks) and parts[0] == chunks[0::3]


def test_chunks_cut_where_hist_chunks_cuts_without_neighbours():
    """A table without any verdict asks for no other section: the cores and the read slabs are hist_chunks' slabs."""
    box = ((0, 9), (0, 20), (0, 50))
    none = np.full((9, 2), -1, np.int32)
    for budget in (1 << 20, 3 * 20 * 50, 7 * 50, 1):
        got = outlier_chunks(box, (9, 20, 50), none, 0, budget)
        assert [c for c, _ in got] == [r for _, r in got] == hist_chunks(box, budget)


def test_chunks_refuse_bad_arguments():
    nbr, box = section_neighbours(9), ((0, 9), (0, 20), (0, 50))
    assert outlier_chunks(((2, 2), (0, 20), (0, 50)), (9, 20, 50), nbr, 4) == []
    bad = nbr.copy()
    bad[4] = (4, 5)
    for kw in (dict(radius=-1), dict(radius=8), dict(radius=1.5), dict(chunk_bytes=0), dict(rank=2, world_size=2),
               dict(nbr=nbr[:8]), dict(nbr=nbr.astype(np.float64)), dict(nbr=bad), dict(box=((0, 10), (0, 20), (0, 50))),
               dict(box=((0, 9), (-1, 20), (0, 50))), dict(vol_shape=(20, 50))):
        a = dict(dict(box=box, vol_shape=(9, 20, 50), nbr=nbr, radius=4), **kw)
        with pytest.raises(ValueError):
            outlier_chunks(**a)


# ------------------------------------------------------------------------------------------------ outlier_thresholds
def test_thresholds_median_floor_equality_and_clipping():
    s = np.zeros((5, 1, 4, 2), np.int64)
    s[..., 1] = 100
    s[0, :, :, 1] = s[4, :, :, 1] = 0                                      # no verdict: not part of the median
    s[1:4, 0, 0, 0] = (100, 300, 200)                                      # means 1, 3, 2: scale 2, thr = 256 * 24
    s[1:4, 0, 1, 0] = (0, 0, 5000)                                         # scale 0: the floor, 256 * 16
    s[1:4, 0, 2, 0] = (2200, 2200, 2200)                                   # 12 * 22 = 264 grey levels: clipped
    s[1:4, 0, 3, 0] = (133, 134, 9999)                                     # 12 * 1.34 = 16.08 > the floor: ceil
    t = outlier_thresholds(s)
    assert isinstance(t, OutlierThresholds) and t.thr.dtype == np.int32 and t.scale.dtype == np.float64
    assert t.scale.tolist() == [[2.0, 0.0, 22.0, 1.34]]
    assert t.thr.tolist() == [[6144, 4096, OUTLIER_MAX_THR, int(np.ceil(256 * 12 * 1.34))]] and t.thr[0, 3] == 4117
    assert outlier_thresholds(s, ratio=8.0, min_dev=16.0).thr.tolist()[0][:2] == [4096, 4096]     # 8 * 2 = the floor
    assert outlier_thresholds(s, 1.0, 255).thr.tolist() == [[65280] * 4]
    assert outlier_thresholds(s, 0.5, 0.001).thr.tolist()[0][:2] == [256, 1]
    none = np.zeros((3, 2, 2, 2), np.int64)                                # a column without any verdict: the floor
    assert outlier_thresholds(none).thr.tolist() == [[4096] * 2] * 2 and not outlier_thresholds(none).scale.any()
    fx = ZD.fixture()
    sums = ZD.volume_sums(fx.volume, ZD.neighbours(32, [12]), (64, 64))
    mine, ref = outlier_thresholds(sums), ZD.thresholds(sums)
    assert np.array_equal(mine.thr, ref[0]) and np.array_equal(mine.scale, ref[1])
    for kw in (dict(ratio=0), dict(ratio=-1), dict(ratio="3"), dict(ratio=float("inf")), dict(min_dev=0),
               dict(min_dev=255.5), dict(min_dev=True), dict(s=s[..., :1]), dict(s=s.astype(np.float64)), dict(s=s[0])):
        with pytest.raises(ValueError):
            outlier_thresholds(**dict(dict(s=s), **kw))


def test_host_checks_come_before_any_gpu_work():
    """Every ValueError of volume_outliers and find_debris is raised on a machine without a GPU as well."""
    vol, thr = np.zeros((4, 20, 30), np.uint8), np.full((2, 2), 4096, np.int32)
    for kw in (dict(volume=vol.astype(np.int16)), dict(window=8), dict(window=1), dict(window=17), dict(window=9.0),
               dict(thr=thr[:1]), dict(thr=thr.astype(np.float32)), dict(thr=thr * 0), dict(thr=thr + 65280),
               dict(skip=[4]), dict(max_lag=9), dict(tile=0), dict(tiles=np.zeros((4, 2, 3), bool)),
               dict(tiles=np.zeros((4, 2, 2))), dict(out=np.zeros((4, 20, 31), np.uint8)),
               dict(out=np.zeros((4, 20, 30), np.int8)), dict(start=(0, 0, 2), size=(30, 20, 3)), dict(chunk_bytes=0),
               dict(rank=1, world_size=1)):
        with pytest.raises(ValueError):
            volume_outliers(**dict(dict(volume=vol, thr=thr, tile=16), **kw))
    from transfer_em_amd.utils import Defects
    d = Defects([1], np.zeros((4, 2, 2), bool), np.zeros((2, 2), bool), np.zeros((4, 2, 2)))
    for kw in (dict(max_gap=0), dict(max_gap=33), dict(rank=0), dict(volume=vol[0]), dict(skip=3), dict(defects=7),
               dict(window=4), dict(ratio=0), dict(tile=0), dict(tile="16"), dict(tile=0, defects=d),
               dict(tile="16", defects=d), dict(tile=2049, defects=d), dict(tile=8, defects=d),
               dict(defects=d._replace(sections=[4])), dict(volume=vol.astype(np.int16), defects=d),
               dict(mask_out=np.zeros((4, 20, 31), np.uint8)), dict(mask_out=np.zeros((4, 20, 30), np.int8))):
        with pytest.raises(ValueError):
            find_debris(**dict(dict(volume=vol, tile=16), **kw))


# ------------------------------------------------------------------------------------------ the reference's identities
def test_a_volume_linear_along_z_has_no_deviation():
    z, y, x = np.meshgrid(np.arange(9), np.arange(6), np.arange(7), indexing="ij")
    up = (3 * z + 2 * y + 5 * x).astype(np.uint8)
    for vol in (up, up[::-1].copy()):
        for nbr in (ZD.neighbours(9), ZD.neighbours(9, [3, 4], 3)):
            assert not ZD.deviation(vol, nbr).any()
            assert not ZD.mask(vol, nbr, np.ones((1, 1), np.int32), (16, 16), 1).any()
    e = ZD.deviation(np.array([[[0]], [[255]], [[7]], [[200]], [[100]], [[100]]], np.uint8), ZD.neighbours(6))
    assert e.reshape(-1).tolist() == [0, 248, 193, 100, 0, 0]             # the distance to the nearer neighbour


def test_equality_does_not_flag_in_the_reference():
    vol = np.zeros((3, 21, 37), np.uint8)
    vol[1] = 10
    nbr = ZD.neighbours(3)
    for r in (1, 4, 7):
        Ws, c = ZD.window_sums(ZD.deviation(vol, nbr), r)
        assert np.array_equal(Ws[1], 10 * c) and c.max() == (2 * r + 1) ** 2 and c[0, 0] == (r + 1) ** 2
        assert ZD.mask(vol, nbr, np.full((2, 3), 2559), (16, 16), r)[1].all()
        assert not ZD.mask(vol, nbr, np.full((2, 3), 2560), (16, 16), r).any()
    s = ZD.volume_sums(vol, nbr, (16, 16))
    assert s[1, 0, 0].tolist() == [2560, 256] and s[1, 1, 2].tolist() == [10 * 5 * 5, 25] and not s[0].any() and not s[2].any()


# ---------------------------------------------------------------------------------------------- the fixture's verdict
def test_the_fixtures_verdict_from_the_reference_alone():
    """This fixture's own values, at the defaults (tile 64, window 9, ratio 12, min_dev 16, skip [12])."""
    fx, vd = ZD.fixture(), ZD.check_fixture()
    assert fx.volume.shape == ZD.FIX_SHAPE and int(fx.planted.sum()) == 901 and int(fx.thick.sum()) == 200
    assert not fx.volume[12].any() and 64 <= min(h * w for _, _, _, h, w, _ in ZD.FIX_BLOBS) and \
        max(h * w for _, _, _, h, w, _ in ZD.FIX_BLOBS) == 196
    off = np.abs(fx.volume.astype(np.int64) - fx.clean.astype(np.int64))[fx.planted]
    assert 90 < off.mean() < 100                                          # the particles: about 95 grey levels off
    print(f"thr {vd.thr.min()}...{vd.thr.max()}, flagged {vd.flagged}, planted hit {vd.hits} of 901, least recall "
          f"{min(vd.recall):.3f}, far {vd.far}, largest ratio away {vd.ratio_away:.3f}, thick {vd.thick_hits} of 200")
    assert vd.far == 0 and min(vd.recall) >= 0.9 and vd.thick_hits == 0
    assert (int(vd.thr.min()), int(vd.thr.max()), vd.flagged, vd.hits) == (4285, 4635, 1557, 887)
    assert abs(min(vd.recall) - 0.948) < 5e-4 and abs(vd.ratio_away - 0.69) < 5e-3
