"""Host side of the 16-bit ingest: window16, window_lut16 and match_lut16 against their restatement in u16_ref, the
slab plan at two bytes per voxel (and, at one, the cuts this project has always made), and every argument check of
volume_histogram16 / volume_to_u8 that is made before any GPU work.  No GPU is needed."""
from fractions import Fraction

import numpy as np
import pytest

import u16_ref as R
from transfer_em_amd import utils
from transfer_em_amd.utils import (hist_chunks, match_lut, match_lut16, volume_histogram16, volume_to_u8, window16,
                                   window_lut16)

BINS = 65536


def _sparse(rng, n, lo=0, hi=BINS, most=1000):
    """A histogram with n occupied bins in [lo, hi)."""
    h = np.zeros(BINS, np.int64)
    h[rng.choice(np.arange(lo, hi), n, replace=False)] = rng.integers(1, most, n)
    return h


def _hists():
    rng = np.random.default_rng(5)
    one = np.zeros(BINS, np.int64)
    one[12345] = 77
    at0, at_top = np.zeros(BINS, np.int64), np.zeros(BINS, np.int64)
    at0[0], at_top[BINS - 1] = 5, 9
    steps = np.zeros(BINS, np.int64)                     # 1000 voxels: the 0.1 % and 99.9 % quantiles land exactly on steps
    steps[[10, 20, 30, 40]] = [1, 499, 499, 1]
    ends = np.zeros(BINS, np.int64)
    ends[[0, 32767, 32768, BINS - 1]] = [3, 1000, 2000, 3]
    return {"empty": np.zeros(BINS, np.int64), "one_bin": one, "all_at_0": at0, "all_at_65535": at_top, "steps": steps,
            "ends": ends, "sparse": _sparse(rng, 300), "dense": rng.integers(0, 50, BINS).astype(np.int64),
            "narrow": _sparse(rng, 200, 20000, 21000), "big": _sparse(rng, 500, most=1 << 40)}


HISTS = _hists()
QUANTILES = [((1, 1000), (999, 1000)), ((0, 1), (1, 1)), ((1, 2), (1, 2)), ((1, 100), (3, 4))]


@pytest.mark.parametrize("name", sorted(HISTS))
def test_window16_equals_the_reference(name):
    h = HISTS[name]
    for low, high in QUANTILES:
        got = window16(h, Fraction(*low), Fraction(*high))
        assert got == R.ref_window(h, low, high), (low, high)
        assert all(isinstance(v, int) for v in got) and 0 <= got[0] < got[1] <= BINS - 1
    assert window16(h) == R.ref_window(h, (1, 1000), (999, 1000))        # the defaults


def test_window16_known_values():
    assert window16(HISTS["empty"]) == (0, 65535)
    assert window16(HISTS["one_bin"]) == (12345, 12346)                  # hi == lo: widened by one
    assert window16(HISTS["all_at_0"]) == (0, 1)
    assert window16(HISTS["all_at_65535"]) == (65534, 65535)             # ... downwards at the top
    assert window16(HISTS["steps"]) == (10, 30)                          # C = 1 >= 1000 / 1000; C = 999 >= 999 at bin 30
    assert window16(HISTS["steps"], Fraction(1, 1000) + Fraction(1, 10 ** 9)) == (20, 30)
    assert window16(HISTS["ends"]) == (32767, 32768)                     # 3 of 3006 voxels lie below 0.1 % on either side


def test_window16_row_wise_and_errors():
    names = sorted(HISTS)
    lo, hi = window16(np.stack([HISTS[n] for n in names]))
    assert lo.dtype == hi.dtype == np.int64 and lo.shape == hi.shape == (len(names),)
    assert [(int(a), int(b)) for a, b in zip(lo, hi)] == [window16(HISTS[n]) for n in names]
    assert window16(HISTS["sparse"].astype(np.uint64)) == window16(HISTS["sparse"])
    h = HISTS["sparse"]
    for bad in (dict(low=-0.1), dict(high=1.5), dict(low=Fraction(3, 4), high=Fraction(1, 4)), dict(low="x")):
        with pytest.raises(ValueError):
            window16(h, **bad)
    neg = h.copy()
    neg[5] = -1
    for bad in (h[:256], h.astype(np.float64), neg, np.zeros((2, 3, BINS), np.int64)):
        with pytest.raises(ValueError):
            window16(bad)


@pytest.mark.parametrize("lo,hi", [(0, 65535), (0, 1), (65534, 65535), (1000, 1255), (1000, 1256), (300, 40000),
                                   (12345, 12346), (7, 518)])
def test_window_lut16_equals_the_reference(lo, hi):
    for invert in (False, True):
        t = window_lut16(lo, hi, invert)
        assert t.dtype == np.uint8 and t.shape == (BINS,) and np.array_equal(t, R.ref_window_lut(lo, hi, invert))
    t = window_lut16(lo, hi)
    assert t[lo] == 0 and t[hi] == 255 and (np.diff(t.astype(int)) >= 0).all()


def test_window_lut16_rows_and_errors():
    lo, hi = np.array([0, 1000, 65534]), np.array([65535, 1255, 65535])
    t = window_lut16(lo, hi)
    assert t.shape == (3, BINS) and all(np.array_equal(t[i], R.ref_window_lut(int(lo[i]), int(hi[i]))) for i in range(3))
    assert np.array_equal(window_lut16(lo, hi, invert=True), 255 - t)
    assert np.array_equal(window_lut16(*window16(HISTS["sparse"])), R.ref_window_lut(*R.ref_window(HISTS["sparse"],
                                                                                                  *QUANTILES[0])))
    for a, b in ((5, 5), (6, 5), (-1, 5), (0, 65536), (1.5, 7), (np.array([1, 2]), np.array([3])),
                 (np.array([1, 9]), np.array([3, 9]))):
        with pytest.raises(ValueError):
            window_lut16(a, b)


def _refs():
    rng = np.random.default_rng(6)
    flat = np.full(256, 10, np.int64)
    bell = np.rint(1000 * np.exp(-((np.arange(256) - 120) / 30.0) ** 2)).astype(np.int64)
    two = np.zeros(256, np.int64)
    two[[3, 250]] = [1, 4]
    return {"flat": flat, "bell": bell, "two": two, "random": rng.integers(0, 100, 256).astype(np.int64)}


REFS = _refs()


@pytest.mark.parametrize("ref", sorted(REFS))
@pytest.mark.parametrize("name", sorted(HISTS))
def test_match_lut16_equals_the_reference(name, ref):
    t = match_lut16(HISTS[name], REFS[ref])
    assert t.dtype == np.uint8 and t.shape == (BINS,) and np.array_equal(t, R.ref_match(HISTS[name], REFS[ref]))
    assert (np.diff(t.astype(int)) >= 0).all()                           # non-decreasing
    if name == "empty":
        assert np.array_equal(t, np.arange(BINS) >> 8)


def test_match_lut16_beyond_int64():
    """N_src N_ref >= 2^63: the Python-int path gives what the reference's Python ints give."""
    hs, hr = HISTS["sparse"] << 30, REFS["random"] << 30
    assert int(hs.sum()) * int(hr.sum()) >= 1 << 63
    assert np.array_equal(match_lut16(hs, hr), R.ref_match(hs, hr))
    assert np.array_equal(match_lut16(hs, hr), match_lut16(HISTS["sparse"], REFS["random"]))    # the rule is scale-free


def test_match_lut16_on_multiples_of_256_is_match_lut():
    rng = np.random.default_rng(7)
    h8 = rng.integers(0, 1000, 256).astype(np.int64)
    h8[rng.choice(256, 100, replace=False)] = 0
    h16 = np.zeros(BINS, np.int64)
    h16[::256] = h8
    for ref in REFS.values():
        assert np.array_equal(match_lut16(h16, ref)[::256], match_lut(h8, ref))
    same = np.zeros(BINS, np.int64)                                      # the same occupied levels: the identity on them
    same[np.arange(256) << 8] = REFS["bell"]
    occupied = np.flatnonzero(REFS["bell"])
    assert np.array_equal(match_lut16(same, REFS["bell"])[occupied << 8], occupied)


def test_match_lut16_rows_and_errors():
    names = sorted(HISTS)
    hs = np.stack([HISTS[n] for n in names])
    t = match_lut16(hs, REFS["bell"])
    assert t.shape == (len(names), BINS) and t.dtype == np.uint8
    assert all(np.array_equal(t[i], R.ref_match(hs[i], REFS["bell"])) for i in range(len(names)))
    refs = np.stack([list(REFS.values())[i % len(REFS)] for i in range(len(names))])
    t = match_lut16(hs, refs)
    assert all(np.array_equal(t[i], R.ref_match(hs[i], refs[i])) for i in range(len(names)))
    h = HISTS["sparse"]
    neg = REFS["bell"].copy()
    neg[0] = -1
    for a, b in ((h, np.zeros(256, np.int64)), (h, neg), (h, refs), (hs, refs[:3]), (h[:256], REFS["bell"]),
                 (h, h), (h.astype(np.float32), REFS["bell"]), (hs[None], REFS["bell"])):
        with pytest.raises(ValueError):
            match_lut16(a, b)


def test_match_lut16_is_vectorised():
    """64 rows of 65,536 bins in well under the time a Python loop over bins would take (~2 s)."""
    import time
    hs = np.random.default_rng(8).integers(0, 100, (64, BINS)).astype(np.int64)
    t0 = time.perf_counter()
    t = match_lut16(hs, REFS["bell"])
    assert time.perf_counter() - t0 < 1.0 and t.shape == (64, BINS)


# -------------------------------------------------------------------------------------------------------- the slab plan
BOXES = [((0, 9), (0, 50), (0, 70)), ((3, 8), (5, 44), (9, 62)), ((7, 8), (0, 33), (1, 2)), ((0, 1), (0, 1), (0, 1))]


@pytest.mark.parametrize("box", BOXES, ids=[str(b).replace(" ", "") for b in BOXES])
@pytest.mark.parametrize("world_size", [1, 2, 3])
def test_hist_chunks_of_two_byte_voxels_tile_the_box(box, world_size):
    (z0, z1), (y0, y1), (x0, x1) = box
    row, sec = 2 * (x1 - x0), 2 * (y1 - y0) * (x1 - x0)                  # bytes
    for budget in sorted({1, row - 1, row, 3 * row + 1, max(1, sec - 1), sec, sec + 1, 3 * sec + 5, sec * (z1 - z0),
                          10 ** 9}):
        cover = np.zeros((z1, y1, x1), np.int32)
        per_rank = [hist_chunks(box, budget, r, world_size, itemsize=2) for r in range(world_size)]
        for slabs in per_rank:
            for (a0, a1), (b0, b1), (c0, c1) in slabs:
                assert z0 <= a0 < a1 <= z1 and y0 <= b0 < b1 <= y1 and (c0, c1) == (x0, x1)
                assert 2 * (a1 - a0) * (b1 - b0) * (c1 - c0) <= max(budget, row), budget     # one row at the least
                if budget < sec:
                    assert a1 - a0 == 1
                else:
                    assert (b0, b1) == (y0, y1)
                cover[a0:a1, b0:b1, c0:c1] += 1
        inside = np.zeros_like(cover)
        inside[z0:z1, y0:y1, x0:x1] = 1
        assert np.array_equal(cover, inside), budget                      # pairwise disjoint, union = the box
        n = sum(len(s) for s in per_rank)
        assert [len(s) for s in per_rank] == [len(range(r, n, world_size)) for r in range(world_size)]
        if budget < 2 * row:
            assert n == (z1 - z0) * (y1 - y0)                            # one-row slabs
        # two bytes per voxel under a budget are one byte per voxel under half of it
        if budget >= 2:
            wide = ((z0, z1), (y0, y1), (2 * x0, 2 * x1))
            assert [s[:2] for s in hist_chunks(box, budget, 0, 1, itemsize=2)] == [s[:2] for s in hist_chunks(wide, budget)]
    with pytest.raises(ValueError):
        hist_chunks(box, 100, itemsize=4)


def test_hist_chunks_of_one_byte_voxels_have_not_moved():
    """The cuts recorded from the commit before `itemsize` existed."""
    whole = lambda z: ((z[0], z[1]), (0, 6), (0, 7))
    assert hist_chunks(((0, 5), (0, 6), (0, 7)), 100) == [whole((0, 2)), whole((2, 4)), whole((4, 5))]
    assert hist_chunks(((2, 9), (3, 10), (1, 20)), 50) == [((z, z + 1), y, (1, 20)) for z in (2, 3, 4, 5, 6, 7, 8)
                                                           for y in ((3, 5), (5, 7), (7, 9), (9, 10))]
    assert hist_chunks(((0, 3), (0, 4), (0, 10)), 7) == [((z, z + 1), (y, y + 1), (0, 10)) for z in (0, 1, 2)
                                                         for y in (0, 1, 2, 3)]
    assert hist_chunks(((1, 8), (0, 50), (5, 70)), 9850, 1, 2) == [((4, 7), (0, 50), (5, 70))]
    assert hist_chunks(((0, 2), (0, 9), (0, 11)), 11, 1, 3) == [((z, z + 1), (y, y + 1), (0, 11)) for z in (0, 1)
                                                                for y in (1, 4, 7)]
    assert hist_chunks(((0, 40), (0, 50), (0, 70))) == [((0, 40), (0, 50), (0, 70))]
    assert hist_chunks(((0, 3), (2, 2), (0, 5)), 10) == []
    for box in BOXES:
        assert hist_chunks(box, 977, itemsize=1) == hist_chunks(box, 977)


# ------------------------------------------------------------------------------------------------------ argument checks
@pytest.fixture()
def no_gpu(monkeypatch):
    """Any attempt to reach the GPU fails the test: the checks come first."""
    def refuse(*a, **k):
        raise AssertionError("GPU work before the argument checks")
    monkeypatch.setattr(utils.H, "require_gpu", refuse)


def test_dtype_checks_come_before_any_gpu_work(no_gpu):
    lut = np.zeros(BINS, np.uint8)
    other = ">u2" if np.dtype(np.uint16).byteorder in "=<" and np.little_endian else "<u2"
    for dt in (np.uint8, np.int8, np.uint32, np.int32, np.float32, np.float64, other, other.replace("u", "i")):
        vol = np.zeros((3, 4, 5), dt)
        with pytest.raises(ValueError, match="uint16 or int16"):
            volume_histogram16(vol)
        with pytest.raises(ValueError, match="uint16 or int16"):
            volume_to_u8(vol, lut)


def test_argument_checks_come_before_any_gpu_work(no_gpu):
    vol, img = np.zeros((3, 4, 5), np.uint16), np.zeros((4, 5), np.int16)
    lut, luts = np.zeros(BINS, np.uint8), np.zeros((3, BINS), np.uint8)
    for start, size in (((0, 0, 0), (6, 4, 3)), ((-1, 0, 0), (2, 2, 2)), ((0, 0, 2), (5, 4, 2)), ((0, 0), (5, 4))):
        with pytest.raises(ValueError):
            volume_histogram16(vol, start, size)
        with pytest.raises(ValueError):
            volume_to_u8(vol, lut, start=start, size=size)
    for bad in (lut.astype(np.int8), lut[:256], np.zeros((2, BINS), np.uint8), np.zeros((3, 256), np.uint8),
                list(lut[:4]), None):
        with pytest.raises(ValueError):
            volume_to_u8(vol, bad)
    with pytest.raises(ValueError):
        volume_to_u8(img, luts)                                          # one image has one section
    with pytest.raises(ValueError, match="shape"):
        volume_to_u8(vol, luts, out=np.zeros((3, 4, 6), np.uint8))
    with pytest.raises(ValueError, match="shape"):
        volume_to_u8(vol, lut, out=np.zeros((1, 2, 2), np.uint8), start=(0, 0, 0), size=(2, 2, 2))
    with pytest.raises(ValueError, match="shape"):
        volume_to_u8(img, lut, out=np.zeros((1, 4, 5), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        volume_to_u8(vol, lut, out=np.zeros((3, 4, 5), np.uint16))
    with pytest.raises(ValueError):
        volume_to_u8(vol, lut, histogram=True)                           # reports in stats: needs the dict
    with pytest.raises(ValueError):
        volume_to_u8(vol, lut, histogram=1, stats={})
    for kw in (dict(chunk_bytes=0), dict(rank=2, world_size=2)):
        with pytest.raises(ValueError):
            volume_histogram16(vol, **kw)
        with pytest.raises(ValueError):
            volume_to_u8(vol, lut, **kw)


def test_the_fixture_orders_the_routes():
    """The numpy routes on the seeded stack: each step that keeps more of the 16 bits, or follows the sections, is
    closer to the ground truth."""
    G, raw = R.fixture_stack()
    maes = [R.mae(r, G) for r in R.fixture_routes(raw, G)]
    print("MAE (grey levels): per-section 16-bit match %.4f, per-section window + per-section 8-bit match %.4f, "
          "global window + per-section 8-bit match %.4f, global window + global 8-bit match %.4f" % tuple(maes))
    assert maes[0] < maes[1] < maes[2] < maes[3]
