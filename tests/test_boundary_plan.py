"""Host side of the reflect / edge boundary modes of tiled inference: utils.fold is numpy.pad's index rule, and the
chunk footprints of chunk_plan(..., boundary=...) hold every folded coordinate of every tile voxel, tightly."""
import numpy as np
import pytest

MODES = ("reflect", "edge")
GEOMETRY = {74: (40, 17), 132: (96, 18)}            # dimsize: (outdimsize, buffer) that EM2EM gives the generators

# a volume thinner than one tile along x (and than a 132 tile along every axis); ROI past all six faces
VOL, START, SIZE = (50, 61, 45), (-20, -15, -10), (90, 100, 80)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 2, 3, 7, 45])
def test_fold_is_numpy_pad(n, mode):
    from transfer_em_amd.utils import fold
    a = np.arange(n)
    for pad in sorted({0, 1, n - 1, n, n + 1, 2 * n + 3, 2 * n + 4, 3 * n + 11, 113}):
        want = np.pad(a, pad, mode=mode)                                    # the index each padded position reads
        i = np.arange(-pad, n + pad)
        got = fold(i, n, mode)
        assert got.shape == want.shape and np.array_equal(got, want), (n, pad)
        assert [fold(int(v), n, mode) for v in i] == want.tolist()         # the scalar form
    lo, hi = 2 * n + 5, 3 * n + 9                                            # asymmetric, as a far-face tile pads
    assert np.array_equal(fold(np.arange(-lo, n + hi), n, mode), np.pad(a, (lo, hi), mode=mode))


@pytest.mark.parametrize("mode", MODES)
def test_fold_3d_equals_numpy_pad(mode):
    from transfer_em_amd.utils import fold
    vol = np.random.default_rng(0).integers(0, 256, (4, 1, 6), dtype=np.uint8)
    pad = ((9, 3), (2, 5), (13, 20))
    ix = [fold(np.arange(-lo, n + hi), n, mode) for n, (lo, hi) in zip(vol.shape, pad)]
    assert np.array_equal(vol[np.ix_(*ix)], np.pad(vol, pad, mode=mode))


def test_fold_rejects_zeros_unknown_and_empty():
    from transfer_em_amd.utils import fold
    for bad in ("zeros", "wrap", None):
        with pytest.raises(ValueError):
            fold(3, 5, bad)
    with pytest.raises(ValueError):
        fold(0, 0, "reflect")


def _tile_coordinates(chunk, edge, is3d):
    """Per axis, the volume coordinates of every voxel of every tile of the chunk (duplicates dropped)."""
    ext = (edge, edge, edge) if is3d else (1, edge, edge)
    return [np.unique(np.concatenate([chunk.read[d][0] + o[d] + np.arange(ext[d]) for o in chunk.origins]))
            for d in range(3)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chunk_tiles", [(1, 2, 2), None], ids=["1x2x2", "default"])
@pytest.mark.parametrize("dimsize", [74, 132])
def test_chunk_footprints_hold_every_folded_coordinate_tightly(dimsize, chunk_tiles, mode):
    from transfer_em_amd.utils import chunk_plan, fold, tile_plan
    od, buf = GEOMETRY[dimsize]
    od2, buf2, _, rois, _ = tile_plan(START, SIZE, od, buf)
    edge = od2 + 2 * buf2
    chunks = chunk_plan(START, SIZE, od, buf, VOL, chunk_tiles, boundary=mode)
    assert sorted(t for c in chunks for t in c.tiles) == list(range(len(rois)))
    multi_bounce = False
    for c in chunks:
        assert min(c.block) > 0 and c.block == tuple(hi - lo for lo, hi in c.read)
        for t, o in zip(c.tiles, c.origins):                                  # origins are relative to read[*][0]
            assert tuple(c.read[d][0] + o[d] for d in range(3)) == (rois[t][2], rois[t][1], rois[t][0])
        for d, coords in enumerate(_tile_coordinates(c, edge, True)):
            f = fold(coords, VOL[d], mode)
            lo, hi = c.read[d]
            assert 0 <= lo < hi <= VOL[d]
            assert f.min() == lo and f.max() == hi - 1, (c.read, d)           # inside, and both ends attained
            multi_bounce |= bool((coords < -(VOL[d] - 1)).any() or (coords > 2 * (VOL[d] - 1)).any())
    assert multi_bounce                                                       # further past a face than the axis is long


@pytest.mark.parametrize("mode", MODES)
def test_chunk_footprints_2d(mode):
    """2-D chunks fold along z too: ROI sections -1 and 3 of a 3-section stack."""
    from transfer_em_amd.utils import chunk_plan, fold, tile_plan_2d
    vol, start, size = (3, 50, 45), (-20, -15, -1), (90, 100, 5)
    od, buf = 40, 17
    od2, buf2, _, rois, _ = tile_plan_2d(start, size, od, buf)
    edge = od2 + 2 * buf2
    for chunk_tiles in ((2, 1, 2), None):
        chunks = chunk_plan(start, size, od, buf, vol, chunk_tiles, is3d=False, boundary=mode)
        assert sorted(t for c in chunks for t in c.tiles) == list(range(len(rois)))
        for c in chunks:
            assert min(c.block) > 0
            for d, coords in enumerate(_tile_coordinates(c, edge, False)):
                f = fold(coords, vol[d], mode)
                assert f.min() == c.read[d][0] and f.max() == c.read[d][1] - 1, (c.read, d)


@pytest.mark.parametrize("mode", MODES)
def test_interior_chunks_read_what_zeros_reads(mode):
    """Away from the faces nothing folds: the footprints are the zero-mode ones."""
    from transfer_em_amd.utils import chunk_plan
    args = ((100, 120, 90), (150, 140, 160), 40, 17, (400, 400, 400), (2, 2, 1))
    assert chunk_plan(*args, boundary=mode) == chunk_plan(*args)


def test_zeros_is_the_plan_without_the_keyword():
    from transfer_em_amd.utils import chunk_plan
    for od, buf in GEOMETRY.values():
        for chunk_tiles in ((1, 2, 2), None):
            for rank in (0, 1, 2):
                a = chunk_plan(START, SIZE, od, buf, VOL, chunk_tiles, rank, 3, boundary="zeros")
                b = chunk_plan(START, SIZE, od, buf, VOL, chunk_tiles, rank, 3)
                assert a == b and (len(a) > 0 or rank > 0)                    # one chunk in all: rank 0 has it
    start, size, vol = (-20, -15, -1), (190, 165, 8), (6, 130, 150)
    for chunk_tiles in ((3, 2, 2), None):
        for rank in (0, 1):
            a = chunk_plan(start, size, 40, 17, vol, chunk_tiles, rank, 2, is3d=False, boundary="zeros")
            assert a == chunk_plan(start, size, 40, 17, vol, chunk_tiles, rank, 2, False) and (len(a) > 0 or rank > 0)
    # zero-mode chunks wholly outside the volume keep their empty footprint
    far = chunk_plan((500, 0, 0), (40, 40, 40), 40, 17, (50, 50, 50), None, boundary="zeros")
    assert min(far[0].block) == 0


def test_unknown_mode_and_empty_volume_raise():
    from transfer_em_amd.utils import chunk_plan
    with pytest.raises(ValueError):
        chunk_plan(START, SIZE, 40, 17, VOL, None, boundary="wrap")
    for mode in MODES:
        with pytest.raises(ValueError):
            chunk_plan(START, SIZE, 40, 17, (50, 0, 45), None, boundary=mode)
    assert chunk_plan(START, SIZE, 40, 17, (50, 0, 45), None)                 # zeros: as before


def test_ranks_partition_the_chunks():
    from transfer_em_amd.utils import chunk_plan
    whole = chunk_plan(START, SIZE, 40, 17, VOL, (1, 2, 2), boundary="reflect")
    parts = [chunk_plan(START, SIZE, 40, 17, VOL, (1, 2, 2), r, 3, boundary="reflect") for r in range(3)]
    assert sorted(c.base for p in parts for c in p) == sorted(c.base for c in whole)
