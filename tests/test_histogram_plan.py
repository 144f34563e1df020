"""Host side of the intensity histograms and lookup tables of tiled inference: the slab plan of volume_histogram,
meanstd_from_histogram, match_lut, and the argument checks of `lut` / `histogram` / the ROI that are made before any GPU
work.  No GPU is needed."""
import itertools

import numpy as np
import pytest

from transfer_em_amd import utils
from transfer_em_amd.utils import hist_box, hist_chunks, match_lut, meanstd_from_histogram


# ---------------------------------------------------------------------------------------------------- hist_chunks
BOXES = [((0, 40), (0, 50), (0, 70)),           # a whole (40, 50, 70) volume
         ((3, 17), (5, 44), (9, 62)),           # an inner ROI
         ((7, 8), (0, 33), (1, 2)),             # one section, one column
         ((0, 1), (0, 1), (0, 1))]


def _budgets(box):
    (z0, z1), (y0, y1), (x0, x1) = box
    row, sec = x1 - x0, (y1 - y0) * (x1 - x0)
    # below a row, one row, some rows, just below / at / above one section, several sections, everything
    return sorted({1, row, 3 * row + 1, max(1, sec - 1), sec, sec + 1, 3 * sec + 5, sec * (z1 - z0), 10 ** 9})


@pytest.mark.parametrize("box", BOXES, ids=[str(b).replace(" ", "") for b in BOXES])
@pytest.mark.parametrize("world_size", [1, 2, 3])
def test_hist_chunks_tile_the_box(box, world_size):
    (z0, z1), (y0, y1), (x0, x1) = box
    row, sec = x1 - x0, (y1 - y0) * (x1 - x0)
    for budget in _budgets(box):
        cover = np.zeros((z1, y1, x1), np.int32)
        per_rank = [hist_chunks(box, budget, r, world_size) for r in range(world_size)]
        for slabs in per_rank:
            for (a0, a1), (b0, b1), (c0, c1) in slabs:
                assert z0 <= a0 < a1 <= z1 and y0 <= b0 < b1 <= y1 and (c0, c1) == (x0, x1)
                nbytes = (a1 - a0) * (b1 - b0) * (c1 - c0)
                assert nbytes <= max(budget, row), (budget, nbytes)         # one row at the least
                if budget < sec:
                    assert a1 - a0 == 1                                     # a section is split along y
                else:
                    assert (b0, b1) == (y0, y1)
                cover[a0:a1, b0:b1, c0:c1] += 1
        inside = np.zeros_like(cover)
        inside[z0:z1, y0:y1, x0:x1] = 1
        assert np.array_equal(cover, inside), budget                        # pairwise disjoint, union = the box
        n = sum(len(s) for s in per_rank)
        assert [len(s) for s in per_rank] == [len(range(r, n, world_size)) for r in range(world_size)]   # round-robin
        if budget < row:
            assert n == (z1 - z0) * (y1 - y0)
        if budget >= sec * (z1 - z0):
            assert n == 1


def test_hist_chunks_edge_cases():
    assert hist_chunks(((0, 0), (0, 5), (0, 5))) == [] and hist_chunks(((0, 3), (2, 2), (0, 5)), 10) == []
    assert hist_chunks(((0, 3), (0, 5), (0, 7))) == [((0, 3), (0, 5), (0, 7))]          # the default budget: one slab
    with pytest.raises(ValueError):
        hist_chunks(BOXES[0], 0)
    with pytest.raises(ValueError):
        hist_chunks(BOXES[0], 100, rank=2, world_size=2)


def test_hist_box():
    assert hist_box((40, 50, 70)) == ((0, 40), (0, 50), (0, 70))
    assert hist_box((40, 50, 70), (9, 5, 3), (53, 39, 14)) == ((3, 17), (5, 44), (9, 62))
    assert hist_box((40, 50, 70), (70, 50, 40), (0, 0, 0)) == ((40, 40), (50, 50), (70, 70))     # empty, at the far corner
    assert hist_box((50, 70)) == ((0, 1), (0, 50), (0, 70))
    assert hist_box((50, 70), (2, 3), (10, 20)) == ((0, 1), (3, 23), (2, 12))
    for start, size in (((-1, 0, 0), (5, 5, 5)), ((0, 0, 0), (71, 50, 40)), ((0, 46, 0), (5, 5, 5)), ((0, 0, 39), (1, 1, 2)),
                        ((0, 0, 0), (5, -1, 5)), ((0, 0), (5, 5)), ((0, 0, 0), (5, 5))):
        with pytest.raises(ValueError):
            hist_box((40, 50, 70), start, size)
    with pytest.raises(ValueError):
        hist_box((50, 70), (0, 0, 0), (5, 5, 1))
    with pytest.raises(ValueError):
        hist_box((70,))


# ------------------------------------------------------------------------------------------ meanstd_from_histogram
def _within_one_ulp(got, want64):
    want = np.float32(want64)
    assert isinstance(got, np.float32)
    return abs(float(got) - float(want)) <= float(np.spacing(np.abs(want)))


def test_meanstd_from_histogram_against_numpy():
    rng = np.random.default_rng(3)
    arrays = [rng.integers(0, 256, (9, 31, 45), dtype=np.uint8),
              np.clip(rng.normal(120, 9, (6, 20, 33)), 0, 255).astype(np.uint8),      # a few dozen bins, as EM data
              np.full((4, 5, 6), 201, np.uint8)]
    for a in arrays:
        h = np.bincount(a.ravel(), minlength=256)
        scaled = a.astype(np.float64) / 127.5 - 1.0
        mean, std = meanstd_from_histogram(h)
        assert _within_one_ulp(mean, scaled.mean()), (mean, scaled.mean())
        if len(np.unique(a)) > 1:
            assert _within_one_ulp(std, scaled.std()), (std, scaled.std())
        else:
            # a constant array has std 0 exactly, which the counts give; numpy's float64 mean of the scaled array is
            # off by its own rounding (~1e-16 here), and that error, not a rounding tie, is all its std consists of:
            # the reference is held to its float64 error, the function to the exact value
            assert std == 0 and scaled.std() <= 4 * np.finfo(np.float64).eps * abs(scaled.mean())
        per_section = np.stack([np.bincount(s.ravel(), minlength=256) for s in a])     # rows add
        assert meanstd_from_histogram(per_section) == (mean, std)
    mean, std = meanstd_from_histogram(np.bincount([201] * 120, minlength=256))
    assert std == 0 and mean == np.float32(201 / 127.5 - 1)


def test_meanstd_from_histogram_rejects():
    with pytest.raises(ValueError):
        meanstd_from_histogram(np.zeros(256, np.int64))
    with pytest.raises(ValueError):
        meanstd_from_histogram(np.ones(255, np.int64))


# -------------------------------------------------------------------------------------------------------- match_lut
def _brute_match(hs, hr):
    """lut[v] = the smallest w with cdf_ref(w) >= cdf_src(v), on exact fractions."""
    from fractions import Fraction
    cum = lambda h: list(itertools.accumulate(int(c) for c in h))
    cs, cr = cum(hs), cum(hr)
    if cs[-1] == 0:
        return np.arange(256, dtype=np.uint8)
    fs, fr = [Fraction(c, cs[-1]) for c in cs], [Fraction(c, cr[-1]) for c in cr]
    return np.array([next(w for w in range(256) if fr[w] >= fs[v]) for v in range(256)], np.uint8)


def _hists():
    rng = np.random.default_rng(5)
    dense = rng.integers(0, 1000, 256)
    narrow = np.bincount(np.clip(rng.normal(110, 7, 5000), 0, 255).astype(np.uint8), minlength=256)
    wide = np.bincount(np.clip(rng.normal(140, 30, 7000), 0, 255).astype(np.uint8), minlength=256)
    one = np.bincount([37] * 11, minlength=256)
    huge = dense.astype(np.int64) << 40                               # products past 2^64: exact integers are needed
    return dense, narrow, wide, one, huge


def test_match_lut_equals_the_brute_force():
    hs = _hists()
    for a, b in itertools.product(hs, hs):
        lut = match_lut(a, b)
        assert lut.dtype == np.uint8 and lut.shape == (256,)
        assert np.array_equal(lut, _brute_match(a, b))
        assert (np.diff(lut.astype(int)) >= 0).all()                                   # monotone
        if a is b:
            occupied = a > 0
            assert np.array_equal(lut[occupied], np.arange(256)[occupied])             # identity where there is data


def test_match_lut_row_wise():
    dense, narrow, wide, one, huge = _hists()
    empty = np.zeros(256, np.int64)
    src = np.stack([dense, narrow, empty, one])
    lut = match_lut(src, wide)                                                         # one reference for all rows
    assert lut.shape == (4, 256) and lut.dtype == np.uint8
    for z in range(4):
        assert np.array_equal(lut[z], _brute_match(src[z], wide))
    assert np.array_equal(lut[2], np.arange(256))                                      # no voxels: the identity
    refs = np.stack([wide, dense, one, narrow])
    lut = match_lut(src, refs)                                                         # a reference per row
    for z in range(4):
        assert np.array_equal(lut[z], _brute_match(src[z], refs[z]))
    for bad in ((src, refs[:3]), (dense, refs), (dense[:255], dense), (dense.astype(np.float64), dense),
                (dense, empty), (-dense - 1, dense)):
        with pytest.raises(ValueError):
            match_lut(*bad)


# -------------------------------------------------------------------------- argument errors before any GPU work
class _Model2d:
    """Enough of a model for the argument checks; a call that gets past them reaches require_gpu, patched to fail."""
    class generator_g:
        is3d = False
    outdimsize, buffer, device = 36, 17, "cpu"


class _Model3d(_Model2d):
    class generator_g:
        is3d = True


class _Reached(Exception):
    pass


@pytest.fixture
def no_gpu(monkeypatch):
    def reached():
        raise _Reached
    monkeypatch.setattr(utils.H, "require_gpu", reached)


def test_check_lut():
    t = np.arange(256, dtype=np.uint8)
    assert utils._check_lut(None, (4, 5, 6)) is None
    assert np.array_equal(utils._check_lut(t, (4, 5, 6)), t)
    assert utils._check_lut(np.tile(t, (4, 1)), (4, 5, 6)).shape == (4, 256)
    assert utils._check_lut(t[None], (5, 6)).shape == (1, 256)                         # one image: one section
    strided = np.tile(t, (2, 1)).T[:, 0]
    assert utils._check_lut(strided, (4, 5, 6)).flags.c_contiguous
    for bad in (t.astype(np.int64), t.astype(np.float32), list(range(256)), t[:255], np.tile(t, (3, 1)),
                np.tile(t, (4, 1)).T, t[None, None]):
        with pytest.raises(ValueError):
            utils._check_lut(bad, (4, 5, 6))


@pytest.mark.parametrize("fn", ["predict_cube", "predict_volume"])
def test_lut_and_histogram_errors_come_before_gpu_work(no_gpu, fn):
    call = getattr(utils, fn)
    vol, t = np.zeros((4, 50, 60), np.uint8), np.arange(256, dtype=np.uint8)
    args = (vol, (0, 0, 0), (40, 40, 4), _Model3d(), (0, 1), (0, 1))
    for kw in (dict(lut=t.astype(np.int32)), dict(lut=t[:100]), dict(lut=np.tile(t, (5, 1))), dict(lut="identity"),
               dict(histogram=True), dict(histogram=True, stats=[]), dict(histogram=1, stats={})):
        with pytest.raises(ValueError):
            call(*args, **kw)
    for kw in (dict(), dict(lut=t), dict(lut=np.tile(t, (4, 1))), dict(histogram=True, stats={}), dict(lut=None, histogram=False)):
        with pytest.raises(_Reached):                                                  # well-formed: on to the GPU
            call(*args, **kw)
    img = (vol[0], (0, 0), (40, 40), _Model2d(), (0, 1), (0, 1))
    with pytest.raises(ValueError):
        call(*img, lut=np.tile(t, (4, 1)))                                             # one image has one section
    with pytest.raises(_Reached):
        call(*img, lut=t[None])


def test_volume_histogram_errors_come_before_gpu_work(no_gpu):
    vol = np.zeros((4, 50, 60), np.uint8)
    for kw in (dict(start=(0, 0, 0), size=(61, 50, 4)), dict(start=(-1, 0, 0), size=(5, 5, 1)),
               dict(start=(0, 0, 3), size=(5, 5, 2)), dict(start=(0, 0), size=(5, 5)), dict(chunk_bytes=0),
               dict(rank=1, world_size=1)):
        with pytest.raises(ValueError):
            utils.volume_histogram(vol, **kw)
    with pytest.raises(ValueError):
        utils.volume_histogram(vol.astype(np.uint16))
    with pytest.raises(ValueError):
        utils.volume_histogram(vol[0], start=(0, 0), size=(61, 5))
    with pytest.raises(_Reached):
        utils.volume_histogram(vol, start=(1, 2, 3), size=(59, 48, 1))
    with pytest.raises(_Reached):
        utils.volume_histogram(vol[0], per_section=True)


def test_the_alias_exports_the_new_functions():
    import transfer_em.utils as alias
    for name in ("volume_histogram", "hist_chunks", "meanstd_from_histogram", "match_lut"):
        assert getattr(alias, name) is getattr(utils, name)
