"""The host side of the defect detector, without a GPU: the slab plan zcorr_chunks, section_scores against np.corrcoef,
find_defects on the fixture with planted defects (its sums from the numpy reference zcorr_ref), defect_mask against a
direct expansion, defects_repair, and every ValueError."""
import functools
import inspect

import numpy as np
import pytest

import zcorr_ref as ZR
from transfer_em_amd.utils import (HIST_CHUNK_BYTES, Defects, Repair, _check_repair, defect_mask, defects_repair,
                                   find_defects, section_scores, section_sums, zcorr_chunks)


# ----------------------------------------------------------------------------------------------------- zcorr_chunks
def _size(box):
    return int(np.prod([hi - lo for lo, hi in box]))


@pytest.mark.parametrize("shape", [(7, 5, 9), (1, 5, 9), (2, 3, 4), (5, 9)])
def test_chunks_partition_the_volume_within_the_budget(shape):
    Z, Y, X = shape if len(shape) == 3 else (1,) + shape
    for budget in (None, Z * Y * X, 3 * Y * X, 2 * Y * X, 2 * Y * X - 1, Y * X, 4 * X, 2 * X, X, 1):
        chunks = zcorr_chunks(shape, budget)
        seen = np.zeros((Z, Y, X), np.int32)
        for (cz, cy, cx), (rz, ry, rx) in chunks:
            seen[cz[0]:cz[1], cy[0]:cy[1], cx[0]:cx[1]] += 1
            assert cz[0] < cz[1] and cy[0] < cy[1] and cx == (0, X)
            assert (ry, rx) == (cy, cx) and rz == (cz[0], min(cz[1] + 1, Z))       # one section more, but at the last
            assert cy == (0, Y) or cz[1] - cz[0] == 1                               # whole sections, or rows of one
            b = HIST_CHUNK_BYTES if budget is None else budget
            assert _size((rz, ry, rx)) <= b or cy[1] - cy[0] == 1                   # one row at the least
        assert (seen == 1).all()
        order = [(c[0][0], c[1][0]) for c, _ in chunks]
        assert order == sorted(order)


def test_chunks_take_as_much_as_the_budget_allows():
    shape = (10, 6, 8)
    assert zcorr_chunks(shape) == [(((0, 10), (0, 6), (0, 8)),) * 2]
    assert [c[0] for c, _ in zcorr_chunks(shape, 4 * 48)] == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert [r[0] for _, r in zcorr_chunks(shape, 4 * 48)] == [(0, 4), (3, 7), (6, 10), (9, 10)]
    rows = zcorr_chunks(shape, 2 * 48 - 1)                                           # two sections no longer fit
    assert len(rows) == 10 * 2 and rows[0] == (((0, 1), (0, 5), (0, 8)), ((0, 2), (0, 5), (0, 8)))
    assert rows[-1] == (((9, 10), (5, 6), (0, 8)), ((9, 10), (5, 6), (0, 8)))
    assert len(zcorr_chunks(shape, 1)) == 60
    assert zcorr_chunks((1, 6, 8), 48) == [(((0, 1), (0, 6), (0, 8)),) * 2]          # one section: nothing above it


def test_chunks_go_round_robin_to_the_ranks():
    shape, budget = (9, 4, 6), 30
    everything = zcorr_chunks(shape, budget)
    for world in (1, 2, 3, 4):
        parts = [zcorr_chunks(shape, budget, r, world) for r in range(world)]
        assert all(p == everything[r::world] for r, p in enumerate(parts))
        assert max(map(len, parts)) - min(map(len, parts)) <= 1


def test_chunks_refuse_bad_arguments():
    for kw in (dict(chunk_bytes=0), dict(chunk_bytes=-5), dict(rank=1), dict(rank=-1), dict(rank=2, world_size=2),
               dict(world_size=0)):
        with pytest.raises(ValueError):
            zcorr_chunks((4, 4, 4), **kw)
    for shape in ((4,), (1, 2, 3, 4)):
        with pytest.raises(ValueError):
            zcorr_chunks(shape)


# --------------------------------------------------------------------------------------------------- section_scores
def test_scores_equal_corrcoef():
    rng = np.random.default_rng(5)
    vol = rng.integers(0, 256, (6, 37, 50), dtype=np.uint8)
    vol[1:] = (vol[1:].astype(np.int64) // 2 + vol[:-1] // 2).astype(np.uint8)      # neighbours correlate
    vol[3, :16, :24] = 77                                                           # a constant tile
    for tile in ((16, 24), (37, 50), (5, 7)):
        c = section_scores(ZR.volume_sums(vol, tile))
        want = ZR.tile_corr(vol, tile)
        assert c.dtype == np.float64 and c.shape == want.shape
        assert np.abs(c - want).max() <= 1e-12
    c = section_scores(ZR.volume_sums(vol, (16, 24)))
    assert c[2, 0, 0] == 0.0 and c[3, 0, 0] == 0.0 and (np.abs(c[:2, 0, 0]) > 0.1).all()


def test_scores_at_the_extremes_stay_exact():
    """A full 2048 x 2048 tile of 0 / 255 halves: the terms reach 2^60 and the result is still +-1 to the last bits."""
    n, k = 2048 * 2048, 2048 * 1024                                                # k voxels of 255, the rest 0
    s = np.zeros((3, 1, 1, 4), np.int64)
    s[:, 0, 0, 3] = n
    s[:, 0, 0, 0], s[:, 0, 0, 1] = 255 * k, 255 * 255 * k
    s[0, 0, 0, 2] = 255 * 255 * k                                                   # section 1 = section 0
    s[1, 0, 0, 2] = 0                                                               # section 2 = its complement
    c = section_scores(s)
    assert abs(c[0, 0, 0] - 1.0) <= 1e-12 and abs(c[1, 0, 0] + 1.0) <= 1e-12
    assert section_scores(s[:1]).shape == (0, 1, 1) and section_scores(s[:0]).shape == (0, 1, 1)
    assert section_scores(s.astype(np.uint64))[0, 0, 0] == c[0, 0, 0]


# ----------------------------------------------------------------------------------------------------- find_defects
@functools.lru_cache(maxsize=None)
def _fixture_sums():
    return ZR.volume_sums(ZR.defect_volume(), (ZR.FIX_TILE, ZR.FIX_TILE))


def test_find_defects_finds_exactly_the_planted_ones():
    d = find_defects(_fixture_sums())
    assert isinstance(d, Defects) and d.sections == ZR.FIX_SECTIONS
    assert d.tiles.dtype == bool and d.tiles.shape == (48, 3, 4)
    assert [tuple(int(v) for v in p) for p in np.argwhere(d.tiles)] == ZR.FIX_TILES
    assert d.undecided.shape == (3, 4) and not d.undecided.any()
    c = section_scores(_fixture_sums())
    assert d.scores.shape == (48, 3, 4)
    assert np.array_equal(d.scores[0], c[0]) and np.array_equal(d.scores[47], c[46])
    assert np.array_equal(d.scores[1:47], np.maximum(c[:-1], c[1:]))


def test_find_defects_rule_by_rule():
    s = _fixture_sums()
    # a clean cut (sections 24 | 47 next to each other) flags nothing: each side still resembles its other neighbour;
    # the planted tile of section 40 now sits at 25 + 47 - 40
    v = np.array(ZR.defect_volume())
    cut = np.concatenate([v[:25], v[32:48][::-1]])
    d = find_defects(ZR.volume_sums(cut, (32, 32)))
    assert section_scores(ZR.volume_sums(cut, (32, 32)))[24].max() < 0.3           # the cut is one
    assert d.sections == [10, 20] and [tuple(int(x) for x in p) for p in np.argwhere(d.tiles)] == [(32, 1, 2)]
    # a column of resin (constant) is undecided and never bad
    flat = np.array(v)
    flat[:, :32, :32] = 90
    d = find_defects(ZR.volume_sums(flat, (32, 32)))
    assert d.undecided[0, 0] and d.undecided.sum() == 1 and not d.tiles[:, 0, 0].any()
    assert d.sections == ZR.FIX_SECTIONS                                            # 11 of the 11 decided tiles
    # section_fraction: with 1.0 section 40 stays a tile; at 1 / 12 it becomes a section
    assert find_defects(s, section_fraction=1.0).sections == ZR.FIX_SECTIONS
    d = find_defects(s, section_fraction=1 / 12)
    assert d.sections == [10, 20, 30, 31, 40] and not d.tiles.any()
    # the limit: a run of sections from the wrong place that resemble each other shows only as the two cuts at its
    # ends in section_scores; each end still resembles its inner neighbour, so no section of the run is flagged
    run = np.array(v)
    run[30:34] = v[2:6]
    rs = ZR.volume_sums(run, (32, 32))
    d = find_defects(rs)
    assert d.sections == [10, 20] and [tuple(int(x) for x in p) for p in np.argwhere(d.tiles)] == ZR.FIX_TILES
    c = section_scores(rs)
    assert c[29].max() < 0.3 and c[33].max() < 0.3 and c[30:33].min() > 0.8
    # Z < 2: no verdict
    d = find_defects(s[:1])
    assert d.sections == [] and not d.tiles.any() and d.undecided.all() and d.scores.shape == (1, 3, 4)
    d = find_defects(s[:2])                                                         # one pair: its own median
    assert d.sections == [] and not d.tiles.any() and not d.undecided.any()


def test_find_defects_refuses_bad_arguments():
    s = _fixture_sums()
    for kw in (dict(ratio=0), dict(ratio=1.5), dict(ratio=-0.1), dict(ratio=None), dict(ratio=True),
               dict(ratio=float("nan")), dict(min_corr=0), dict(min_corr=1), dict(min_corr="0.1"),
               dict(section_fraction=0), dict(section_fraction=1.01), dict(section_fraction=[0.5])):
        with pytest.raises(ValueError):
            find_defects(s, **kw)
    assert find_defects(s, ratio=1, section_fraction=1).sections == ZR.FIX_SECTIONS
    for bad in (s[..., :3], s[0], s.astype(np.float64), np.zeros((2, 3, 4, 4), bool)):
        with pytest.raises(ValueError):
            find_defects(bad)
        with pytest.raises(ValueError):
            section_scores(bad)


# ------------------------------------------------------------------------------------- defect_mask, defects_repair
def _expand(tiles, th, tw, shape):
    want = np.zeros(shape, np.uint8)
    for z, i, j in np.argwhere(tiles):
        want[z, i * th:(i + 1) * th, j * tw:(j + 1) * tw] = 1
    return want


def test_defect_mask_equals_the_direct_expansion(tmp_path):
    shape, (th, tw) = (5, 37, 50), (16, 24)                                         # 3 x 3 tiles, the last ones partial
    rng = np.random.default_rng(2)
    tiles = rng.random((5, 3, 3)) < 0.3
    tiles[2] = False
    tiles[4, 2, 2] = True
    want = _expand(tiles, th, tw, shape)
    got = defect_mask(tiles, (th, tw), shape)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    out = np.memmap(tmp_path / "mask.u8", np.uint8, "w+", shape=shape)
    out[...] = 0xA5                                                                 # every section is written
    assert defect_mask(tiles.astype(np.uint8) * 7, (th, tw), shape, out=out) is out
    assert np.array_equal(np.asarray(out), want)
    assert np.array_equal(defect_mask(np.ones((2, 1, 1), bool), 64, (2, 3, 4)), np.ones((2, 3, 4), np.uint8))
    for a, kw in (((tiles[:4], (th, tw), shape), {}), ((tiles, 16, shape), {}), ((tiles, (th, tw), shape[1:]), {}),
                  ((tiles, 0, shape), {}), ((tiles, (th, tw), shape), dict(out=np.zeros(shape, np.int8))),
                  ((tiles, (th, tw), shape), dict(out=np.zeros((5, 37, 51), np.uint8)))):
        with pytest.raises(ValueError):
            defect_mask(*a, **kw)


def test_defects_repair_is_a_repair():
    v = ZR.defect_volume()
    d = find_defects(_fixture_sums())
    out = np.full(v.shape, 9, np.uint8)
    rp = defects_repair(d, ZR.FIX_TILE, v.shape, mask_out=out, max_gap=4)
    assert isinstance(rp, Repair) and rp.sections == ZR.FIX_SECTIONS and rp.mask is out and rp.max_gap == 4
    assert rp.missing_value is None
    assert np.array_equal(out, _expand(d.tiles, 32, 32, v.shape)) and out.sum() == 32 * 32
    spec = _check_repair(rp, v.shape)                                               # what volume_repair does with it
    assert list(np.flatnonzero(spec.flags)) == ZR.FIX_SECTIONS and spec.max_gap == 4
    assert defects_repair(d, ZR.FIX_TILE, v.shape).max_gap == 8
    # no bad tile: no mask, and mask_out is left alone; no defect at all: a Repair that changes nothing
    only = d._replace(tiles=np.zeros_like(d.tiles))
    out[...] = 9
    rp = defects_repair(only, ZR.FIX_TILE, v.shape, mask_out=out)
    assert rp.mask is None and rp.sections == ZR.FIX_SECTIONS and (out == 9).all()
    none = defects_repair(only._replace(sections=[]), ZR.FIX_TILE, v.shape)
    assert none.sections == [] and none.mask is None
    assert not _check_repair(none, v.shape).flags.any()
    for gap in (0, 33, 2.5, True):
        with pytest.raises(ValueError):
            defects_repair(d, ZR.FIX_TILE, v.shape, max_gap=gap)
    with pytest.raises(ValueError):
        defects_repair((1, 2), ZR.FIX_TILE, v.shape)
    with pytest.raises(ValueError):
        defects_repair(d, ZR.FIX_TILE, (48, 96, 129))                               # another grid


# ------------------------------------------------------------------------- section_sums: refused before any GPU work
def test_section_sums_refuses_bad_arguments_on_the_host():
    vol = np.zeros((4, 6, 8), np.uint8)
    for a, kw in (((vol.astype(np.int16),), {}), ((vol,), dict(tile=0)), ((vol,), dict(tile=2049)),
                  ((vol,), dict(tile=(4, 4, 4))), ((vol,), dict(tile=2.5)), ((vol,), dict(chunk_bytes=0)),
                  ((vol,), dict(rank=1)), ((vol,), dict(rank=0, world_size=0)), ((vol[0, 0],), {}),
                  ((vol[None],), {})):
        with pytest.raises(ValueError):
            section_sums(*a, **kw)


def test_signatures_and_the_reference_alias():
    import transfer_em.utils as alias
    from transfer_em_amd import _lib, utils
    for name in ("zcorr_chunks", "section_sums", "section_scores", "find_defects", "defect_mask", "defects_repair",
                 "Defects"):
        assert getattr(alias, name) is getattr(utils, name)
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(zcorr_chunks) == ["vol_shape", "chunk_bytes", "rank", "world_size"]
    assert sig(section_sums) == ["volume", "tile", "chunk_bytes", "rank", "world_size", "device", "stats"]
    assert sig(find_defects) == ["s", "ratio", "min_corr", "section_fraction"]
    assert sig(defect_mask) == ["tiles", "tile", "vol_shape", "out"]
    assert sig(defects_repair) == ["d", "tile", "vol_shape", "mask_out", "max_gap"]
    assert Defects._fields == ("sections", "tiles", "undecided", "scores")
    assert len(_lib._SIGS["tem_u8_zcorr_tiles"]) == 14
