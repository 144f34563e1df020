"""Host side of the mip pyramid of tiled inference (mips=L): the level limit and the level shapes, the argument checks
made before anything touches a GPU, and the planner rule that lets every chunk of predict_volume pool on its own --
checked with a numpy model of the pipeline against the numpy reference pooling of the whole array."""
import types

import numpy as np
import pytest

from transfer_em_amd import utils
from transfer_em_amd.utils import predict_cube, predict_volume


def ref_pool(a, valid=None, fz=2):
    """The reference pooling of a [z, y, x] uint8 array by (fz, 2, 2): pad with zeros to whole cells, sum the children,
    count the children inside `valid` (default: the whole array), (sum + (cnt >> 1)) >> log2(cnt); no child: 0."""
    a = np.asarray(a, np.uint8)
    valid = a.shape if valid is None else valid
    f = (fz, 2, 2)
    inside = np.zeros(a.shape, bool)
    inside[:valid[0], :valid[1], :valid[2]] = True
    pad = [(0, -n % k) for n, k in zip(a.shape, f)]
    v = np.pad(np.where(inside, a, 0).astype(np.int64), pad)
    c = np.pad(inside.astype(np.int64), pad)
    cells = lambda t: t.reshape(t.shape[0] // f[0], f[0], t.shape[1] // 2, 2, t.shape[2] // 2, 2).sum(axis=(1, 3, 5))
    s, cnt = cells(v), cells(c)
    assert set(np.unique(cnt)) <= {0, 1, 2, 4, 8}
    sh = np.log2(np.maximum(cnt, 1)).astype(np.int64)
    return ((s + (cnt >> 1)) >> sh).astype(np.uint8)


def test_reference_pooling_by_hand():
    a = np.array([[[1, 2, 255], [4, 4, 255]], [[0, 1, 254], [1, 1, 255]]], np.uint8)     # (2, 2, 3)
    assert ref_pool(a).tolist() == [[[2, 255]]]                  # 14 / 8 = 1.75 -> 2; 1019 / 4 = 254.75 -> 255
    assert ref_pool(a, fz=1).tolist() == [[[3, 255]], [[1, 255]]]   # 11 / 4 -> 3; 3 / 4 -> 1; 509 / 2 = 254.5 -> 255
    assert ref_pool(a, valid=(1, 2, 2)).tolist() == [[[3, 0]]]   # one section, two columns: 11 / 4; no child: 0
    assert ref_pool(np.array([[[1, 2]]], np.uint8)).tolist() == [[[2]]]                   # a tie: 1.5 -> 2


@pytest.mark.parametrize("od, want", [(96, 5), (36, 2), (222, 1), (7, 0), (1, 0), (64, 6), (2, 1)])
def test_max_mips(od, want):
    assert utils.max_mips(od) == want


def test_max_mips_of_an_odd_outdimsize_is_zero():
    assert all(utils.max_mips(od) == 0 for od in range(1, 300, 2))
    for od in range(2, 300, 2):
        L = utils.max_mips(od)
        assert od % (1 << L) == 0 and od % (1 << (L + 1)) != 0


SIZES = [(1, 1, 1), (77, 50, 41), (90, 100, 80), (64, 32, 16), (75, 61, 3), (5, 7, 10), (2, 3, 1)]     # (x, y, z)


@pytest.mark.parametrize("size", SIZES)
def test_mip_shapes(size):
    ceil = lambda n, l: -(-n // (1 << l))
    x, y, z = size
    for L in range(6):
        s3, s2, s1 = utils.mip_shapes(size, L), utils.mip_shapes(size, L, is3d=False), utils.mip_shapes((x, y), L, False)
        assert len(s3) == len(s2) == len(s1) == L + 1
        assert s3 == [(ceil(z, l), ceil(y, l), ceil(x, l)) for l in range(L + 1)]
        assert s2 == [(z, ceil(y, l), ceil(x, l)) for l in range(L + 1)]              # sections are kept
        assert s1 == [(ceil(y, l), ceil(x, l)) for l in range(L + 1)]
    assert utils.mip_shapes(size, 2) == utils.mip_shapes(size, 2, True)               # 3-D is the default
    for is3d in (True, False):                                   # the cascade's shapes: ceil of ceil == ceil by 2^l
        a = np.zeros((z, y, x), np.uint8)
        for s in utils.mip_shapes(size, 3, is3d):
            assert a.shape == s
            a = ref_pool(a, fz=2 if is3d else 1)


def _model(is3d, od=36):
    return types.SimpleNamespace(generator_g=types.SimpleNamespace(is3d=is3d), outdimsize=od, buffer=19, device="cpu")


@pytest.mark.parametrize("fn", [predict_cube, predict_volume], ids=["cube", "volume"])
@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
@pytest.mark.parametrize("mips", [3, 17, -1, 1.0, 2.5, "2", True, (1,)], ids=repr)
def test_bad_mips_raise_before_any_gpu_work(fn, is3d, mips):
    """A ValueError that names the limit, not the TemError / RuntimeError of a missing GPU or of the stand-in model:
    the check comes first.  The 74 model (outdimsize 36) allows 2 levels."""
    vol = np.zeros((40, 40, 40) if is3d else (3, 40, 40), np.uint8)
    size = (36, 36, 36) if is3d else (36, 36, 3)
    with pytest.raises(ValueError, match=r"\b2\b"):
        fn(vol, (0, 0, 0), size, _model(is3d), (0.0, 1.0), (0.0, 1.0), mips=mips)


def test_the_limit_follows_the_tile_plans_outdimsize():
    """The 'multiple of 6' quirk comes first: outdimsize 100 tiles by 96 (5 levels), 226 by 222 (1 level); the
    `outdimsize` keyword overrides the model's."""
    vol, ms = np.zeros((8, 8, 8), np.uint8), (0.0, 1.0)
    assert utils._plan_outdimsize(100) == 96 and utils._plan_outdimsize(226) == 222 and utils._plan_outdimsize(5) == 5
    for od in (100, 226, 36, 5):
        assert utils._plan_outdimsize(od) == utils.tile_plan((0, 0, 0), (1, 1, 1), od, 0)[0]
    with pytest.raises(ValueError, match=r"\b5\b"):
        predict_cube(vol, (0, 0, 0), (8, 8, 8), _model(True, 100), ms, ms, mips=6)
    with pytest.raises(ValueError, match=r"\b1\b"):
        predict_volume(vol, (0, 0, 0), (8, 8, 8), _model(True, 226), ms, ms, mips=2)
    with pytest.raises(ValueError, match=r"\b1\b"):
        predict_volume(vol, (0, 0, 0), (8, 8, 8), _model(True, 100), ms, ms, mips=2, outdimsize=226)


def test_accepted_mips():
    assert utils._check_mips(None, 36) == 0 and utils._check_mips(0, 36) == 0 and utils._check_mips(0, 7) == 0
    assert utils._check_mips(2, 36) == 2 and utils._check_mips(np.int64(5), 96) == 5 and utils._check_mips(1, 222) == 1
    with pytest.raises(ValueError):
        utils._check_mips(1, 7)


@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
def test_bad_out_lists_raise_before_any_gpu_work(is3d):
    size = (41, 50, 37) if is3d else (41, 50, 3)
    vol, ms = np.zeros((40, 60, 50), np.uint8), (0.0, 1.0)
    shapes = utils.mip_shapes(size, 2, is3d)
    good = [np.zeros(s, np.uint8) for s in shapes]
    assert utils._check_mip_outs(good, size, 2, is3d) == good and utils._check_mip_outs(None, size, 2, is3d) is None
    assert utils._check_mip_outs(tuple(good), size, 2, is3d) == good
    bad = {
        "one array": good[0],
        "too short": good[:2],
        "too long": good + [np.zeros((1, 1, 1), np.uint8)],
        "level 1 of the other kind of model": [good[0], np.zeros(utils.mip_shapes(size, 1, not is3d)[1], np.uint8), good[2]],
        "level 2 floored": [good[0], good[1],
                            np.zeros(tuple(n // 4 if (is3d or a) else n for a, n in enumerate(shapes[0])), np.uint8)],
        "not arrays": [1, 2, 3],
    }
    for name, out in bad.items():
        with pytest.raises(ValueError):
            utils._check_mip_outs(out, size, 2, is3d)
        with pytest.raises(ValueError):
            predict_volume(vol, (0, 0, 0), size, _model(is3d), ms, ms, out=out, mips=2)
    if not is3d:                                                          # the single-image form: [y, x] levels
        img = [np.zeros(s, np.uint8) for s in utils.mip_shapes(size[:2], 2, False)]
        assert utils._check_mip_outs(img, size[:2], 2, False) == img
        with pytest.raises(ValueError):
            predict_volume(vol[0], (0, 0), size[:2], _model(False), ms, ms, out=img[:2], mips=2)
        with pytest.raises(ValueError):
            predict_volume(vol[0], (0, 0), size[:2], _model(False), ms, ms, out=good, mips=2)


# ------------------------------------------------------------------------------------------------------- the planner
# the 74 model: outdimsize 36 (2 levels), halo 19.  ROIs that are no multiple of 36, start outside the volume.
PLANS = [  # vol (z, y, x), start (x, y, z), size (x, y, z), chunk_tiles, is3d
    ((60, 70, 90), (-5, 3, -4), (77, 50, 41), (1, 2, 2), True),
    ((60, 70, 90), (-5, 3, -4), (77, 50, 41), (2, 1, 1), True),
    ((60, 70, 90), (-40, -3, 50), (109, 75, 73), (1, 1, 2), True),
    ((60, 70, 90), (0, 0, 0), (72, 36, 37), None, True),
    ((3, 90, 75), (0, 0, 0), (75, 61, 3), (1, 2, 2), False),
    ((3, 90, 75), (-7, 9, -1), (111, 83, 5), (2, 1, 2), False),
]


def _all_chunks(plan, world_size):
    vol, start, size, ct, is3d = plan
    per_rank = [utils.chunk_plan(start, size, 36, 19, vol, ct, r, world_size, is3d) for r in range(world_size)]
    assert all(per_rank) or world_size > 1
    return [c for chunks in per_rank for c in chunks]


@pytest.mark.parametrize("world_size", [1, 3])
@pytest.mark.parametrize("plan", PLANS, ids=[f"{p[2]}-{p[3]}-{'3d' if p[4] else '2d'}" for p in PLANS])
def test_level_boxes_tile_every_level(plan, world_size):
    """At every level the boxes of mip_box over all ranks' chunks are pairwise disjoint and cover mip_shapes[l]
    exactly: painting each box adds 1 to every voxel of the level exactly once."""
    _, _, size, _, is3d = plan
    chunks = _all_chunks(plan, world_size)
    assert any(hi - lo < d for c in chunks for (lo, hi), d in zip(c.out_box, c.dims))      # far-face partial tiles
    L = utils.max_mips(36)
    for l, shape in enumerate(utils.mip_shapes(size, L, is3d)):
        hits = np.zeros(shape, np.int32)
        for c in chunks:
            box, ext = utils.mip_box(c, l, is3d)
            assert all(0 <= lo <= hi <= n for (lo, hi), n in zip(box, shape)), (box, shape)
            assert ext == tuple(hi - lo for lo, hi in box)
            lvl_dims = tuple(d >> (l if (is3d or a) else 0) for a, d in enumerate(c.dims))
            assert all(e <= d for e, d in zip(ext, lvl_dims))                               # inside the level block
            if l == 0:
                assert box == c.out_box
            hits[tuple(slice(lo, hi) for lo, hi in box)] += 1
        assert (hits == 1).all(), (l, np.argwhere(hits != 1)[:5])


@pytest.mark.parametrize("plan", PLANS, ids=[f"{p[2]}-{p[3]}-{'3d' if p[4] else '2d'}" for p in PLANS])
def test_chunks_pool_on_their_own(plan):
    """A numpy model of the pipeline: every chunk holds a block of whole tiles whose voxels past the ROI are junk (255);
    it is pooled on its own, level by level, with the valid extents of its out_box, and the levels are assembled by
    mip_box.  The result equals the reference pooling of the whole level-0 array."""
    _, _, size, _, is3d = plan
    fz, L = (2 if is3d else 1), utils.max_mips(36)
    shapes = utils.mip_shapes(size, L, is3d)
    level0 = np.random.default_rng(7).integers(0, 256, shapes[0], dtype=np.uint8)
    want = [level0]
    for _ in range(L):
        want.append(ref_pool(want[-1], fz=fz))
    assert [w.shape for w in want] == shapes
    got = [np.full(s, 0xEE, np.uint8) for s in shapes]
    half = lambda v: (-(-v[0] // fz), -(-v[1] // 2), -(-v[2] // 2))
    for c in _all_chunks(plan, 2):
        block = np.full(c.dims, 255, np.uint8)
        valid = tuple(hi - lo for lo, hi in c.out_box)
        block[:valid[0], :valid[1], :valid[2]] = level0[tuple(slice(lo, hi) for lo, hi in c.out_box)]
        for l in range(L + 1):
            box, ext = utils.mip_box(c, l, is3d)
            assert ext == valid
            got[l][tuple(slice(lo, hi) for lo, hi in box)] = block[:ext[0], :ext[1], :ext[2]]
            block, valid = ref_pool(block, valid, fz), half(valid)
    for l in range(L + 1):
        assert np.array_equal(got[l], want[l]), (l, np.argwhere(got[l] != want[l])[:5])


def test_a_third_level_would_cross_chunks():
    """Why the limit is there: with outdimsize 36 a chunk boundary at 36 is no multiple of 8, so pooling chunks on their
    own for a third level does not give the pooling of the whole array."""
    size, L = (72, 36, 36), 3
    level0 = np.random.default_rng(8).integers(0, 256, (36, 36, 72), dtype=np.uint8)
    whole = level0
    for _ in range(L):
        whole = ref_pool(whole)
    parts = []
    for x0 in (0, 36):
        blk = level0[:, :, x0:x0 + 36]
        for _ in range(L):
            blk = ref_pool(blk)
        parts.append(blk)
    assert whole.shape[2] == 9 and sum(p.shape[2] for p in parts) == 10
    assert utils.max_mips(36) == 2
