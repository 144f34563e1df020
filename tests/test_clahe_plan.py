"""The host side of CLAHE: clahe_tables against the in-test reference (clahe_ref: integers throughout, so every
comparison is exact), clahe_grid, and the ValueErrors that come before any GPU work.  No GPU is needed."""
import numpy as np
import pytest

from clahe_ref import ref_clipped, ref_remap, ref_tables, ref_tile_hist


def _histograms():
    """Random tile histograms [3, 2, 3, 256] with an empty bin range, a constant tile and a one-pixel tile."""
    rng = np.random.default_rng(0)
    h = rng.integers(0, 50, (3, 2, 3, 256))
    h[0, 0, 0, :100] = 0
    h[0, 0, 0, 200:] = 0                        # an empty bin range at both ends
    h[1, 1, 1] = 0
    h[1, 1, 1, 77] = 384                        # a constant tile
    h[2, 0, 2] = 0
    h[2, 0, 2, 5] = 1                           # a one-pixel tile: n = 1, clip = 1
    h[0, 1, 2] = rng.integers(0, 3, 256) * rng.integers(0, 2, 256) * 400      # a few tall bins: a large excess
    return h


@pytest.mark.parametrize("z_radius", [0, 1])
@pytest.mark.parametrize("clip_limit", [None, 1.0, 3.0, 40.0])
def test_tables_equal_the_reference(clip_limit, z_radius):
    from transfer_em_amd.utils import clahe_tables
    h = _histograms()
    got = clahe_tables(h.astype(np.uint32), clip_limit, z_radius)
    assert got.dtype == np.uint8 and got.shape == h.shape
    assert np.array_equal(got, ref_tables(h, clip_limit, z_radius))
    assert (np.diff(got.astype(np.int64), axis=-1) >= 0).all() and (got[..., 255] == 255).all()      # monotone rows
    if z_radius == 0 and clip_limit is None:                            # the constant tile unclipped: a step
        assert (got[1, 1, 1, :77] == 0).all() and (got[1, 1, 1, 77:] == 255).all()
    if z_radius == 1:
        assert not np.array_equal(got, clahe_tables(h, clip_limit, 0))


@pytest.mark.parametrize("clip_limit", [1.0, 3.0, 40.0])
def test_clipping_keeps_the_total(clip_limit):
    h = _histograms().reshape(-1, 256)
    for row in h:
        n = int(row.sum())
        c = ref_clipped(row, clip_limit)
        clip = max(1, int(np.floor(clip_limit * n / 256)))
        assert sum(c) == n and min(c) >= 0
        assert max(c) <= clip + (sum(max(int(v) - clip, 0) for v in row) + 255) // 256
    assert ref_clipped([0] * 5 + [1] + [0] * 250, 3.0) == [0] * 5 + [1] + [0] * 250          # n = 1: clip = 1, no excess


def test_reference_properties():
    """What the reference itself must satisfy: a one-tile grid is the plain lookup, and a sub-block remapped with its
    origins is the sub-block of the whole result."""
    rng = np.random.default_rng(1)
    vol = rng.integers(0, 256, (3, 37, 53), dtype=np.uint8)
    T1 = ref_tables(ref_tile_hist(vol, 64, 64), 3.0)
    assert T1.shape == (3, 1, 1, 256)
    assert np.array_equal(ref_remap(vol, T1, 64, 64), np.stack([T1[z, 0, 0][vol[z]] for z in range(3)]))
    T = ref_tables(ref_tile_hist(vol, 7, 19), 3.0)
    whole = ref_remap(vol, T, 7, 19)
    assert np.array_equal(ref_remap(vol[1:3, 5:30, 11:50], T, 7, 19, 1, 5, 11), whole[1:3, 5:30, 11:50])


def test_grid():
    from transfer_em_amd.utils import clahe_grid
    assert clahe_grid((9, 70, 150), (16, 24)) == (5, 7)
    assert clahe_grid((70, 150), 16) == (5, 10)
    assert clahe_grid((1, 64, 48), (16, 24)) == (4, 2)                   # exact multiples: no partial tiles
    assert clahe_grid((5, 1, 1), 2048) == (1, 1)
    assert clahe_grid((5, 2049, 4097), (2048, 1)) == (2, 4097)
    for tile in (0, 2049, (16, 0), (-1, 4), (16, 24, 3), 1.5, "a", None):
        with pytest.raises(ValueError):
            clahe_grid((9, 70, 150), tile)


def test_value_errors_come_before_any_gpu_work():
    """Every malformed argument raises ValueError, from checks that run ahead of the first GPU call: this test passes
    without a GPU, where that call would raise another error."""
    from transfer_em_amd.utils import (ClaheTables, clahe_fit, clahe_histograms, clahe_tables, clahe_volume,
                                       predict_cube, predict_volume)
    vol = np.zeros((4, 40, 50), np.uint8)
    good = np.zeros((4, 3, 3, 256), np.uint8)                            # tile (16, 24): gy = 3, gx = 3
    h = np.ones((4, 3, 3, 256), np.uint32)

    class Model:                                                         # never reached
        outdimsize, buffer, device = 36, 19, "cuda"

        class generator_g:
            is3d = True

            @staticmethod
            def plan(shape):
                raise AssertionError

    bad_tables = [good.astype(np.int32), good.astype(np.float32), good.tolist(), good[:3], good[:, :2],
                  np.zeros((4, 3, 3, 255), np.uint8), good[0]]
    for t in bad_tables:
        c = ClaheTables(t, (16, 24))
        with pytest.raises(ValueError):
            clahe_volume(vol, c)
        with pytest.raises(ValueError):
            predict_cube(vol, (0, 0, 0), (36, 36, 4), Model, (0, 1), (0, 1), clahe=c)
        with pytest.raises(ValueError):
            predict_volume(vol, (0, 0, 0), (36, 36, 4), Model, (0, 1), (0, 1), clahe=c)
    with pytest.raises(ValueError):                                      # the tables of another tile
        clahe_volume(vol, ClaheTables(good, (16, 16)))
    for tile in (0, 2049, (16, 4000), (0, 24)):
        with pytest.raises(ValueError):
            clahe_histograms(vol, tile)
        with pytest.raises(ValueError):
            clahe_fit(vol, tile)
        with pytest.raises(ValueError):
            clahe_volume(vol, ClaheTables(good, tile))
        with pytest.raises(ValueError):
            predict_cube(vol, (0, 0, 0), (36, 36, 4), Model, (0, 1), (0, 1), clahe=ClaheTables(good, tile))
    for r in (-1, 0.5, None):
        with pytest.raises(ValueError):
            clahe_tables(h, 3.0, r)
        with pytest.raises(ValueError):
            clahe_fit(vol, (16, 24), z_radius=r)
    for c in (0, 0.0, -2.0, float("nan")):
        with pytest.raises(ValueError):
            clahe_tables(h, c)
        with pytest.raises(ValueError):
            clahe_fit(vol, (16, 24), clip_limit=c)
    for bad_h in (h.astype(np.float64), h[0], np.ones((4, 3, 3, 100), np.uint32), -h.astype(np.int64)):
        with pytest.raises(ValueError):
            clahe_tables(bad_h)
    f32 = vol.astype(np.float32)
    c = ClaheTables(good, (16, 24))
    for call in (lambda: clahe_histograms(f32, (16, 24)), lambda: clahe_fit(f32, (16, 24)), lambda: clahe_volume(f32, c),
                 lambda: predict_cube(f32, (0, 0, 0), (36, 36, 4), Model, (0, 1), (0, 1), clahe=c),
                 lambda: predict_volume(f32, (0, 0, 0), (36, 36, 4), Model, (0, 1), (0, 1), clahe=c)):
        with pytest.raises(ValueError):
            call()
    for start, size in (((0, 0, 0), (51, 40, 4)), ((-1, 0, 0), (5, 5, 2)), ((0, 0, 3), (5, 5, 2)), ((0, 0), (5, 5))):
        with pytest.raises(ValueError):
            clahe_volume(vol, c, start=start, size=size)
    with pytest.raises(ValueError):
        clahe_volume(vol, c, out=np.zeros((4, 40, 49), np.uint8))
    with pytest.raises(ValueError):
        clahe_volume(vol, c, histogram=True)                             # histogram=True reports in a `stats` dict
