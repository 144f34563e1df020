"""The repair along z on the device: tem_u8_repair_z against the numpy reference (repair_ref), volume_repair out of core,
and `repair=` of predict_cube / predict_volume against the same call on the host-repaired volume.  Everything is
integers, so every comparison is exact.  The kernel runs on blocks between guards of fill bytes, which must come back
untouched, as must the halo planes around the core.  Helpers are those of test_gpu_histogram.py / test_gpu_clahe.py."""
import functools
import itertools

import numpy as np
import pytest
import torch

import repair_ref as RR
from clahe_ref import ramp_volume
from test_gpu_clahe import _model
from test_gpu_histogram import _env

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
BLOCKS = [(1, 5, 7), (9, 3, 5), (41, 19, 37), (70, 8, 64)]            # H W: 35, 15, 703 (byte path), 512 (dword path)
GAPS = [1, 3, 8, 32]
MISSING = 77
SOURCES = [("sections",), ("mask",), ("missing",), ("sections", "mask", "missing")]


@functools.lru_cache(maxsize=None)
def _defects(shape, R, seed=7):
    """(vol, mask, sections) of a block with every defect pattern the march has a branch for, column by column over the
    flat (y, x) index i, so that the four columns of one dword are always in different phases:
      i % 8 == 0: a run touching z = 0;  1: a run touching z = Z - 1;  2: a wholly bad column;  3: alternating bad, good;
      4 ... 7: runs of the lengths 1, R, R + 1, 2R - 1, 2R, 2R + 1 in turn, one good voxel apart, from a phase of their own.
    vol holds MISSING at one voxel in ten, at random (good voxels next to them); the sections are the first, two
    neighbours and the last."""
    D, H, W = shape
    rng = np.random.default_rng(seed)
    vol = rng.integers(0, 256, shape, dtype=np.uint8)
    vol[rng.random(shape) < 0.1] = MISSING
    lengths = [1, R, R + 1, max(2 * R - 1, 1), 2 * R, 2 * R + 1]
    mask = np.zeros((D, H * W), np.uint8)
    for i in range(H * W):
        k = i % 8
        if k == 0:
            mask[:lengths[(i // 8) % 6], i] = 1
        elif k == 1:
            mask[max(D - lengths[(i // 8) % 6], 0):, i] = 255
        elif k == 2:
            mask[:, i] = 2
        elif k == 3:
            mask[(i // 8) % 2::2, i] = 3
        else:
            z, j = 1 + (3 * i) % (R + 2), i
            while z < D:
                n = lengths[j % 6]
                mask[z:z + n, i] = 128
                z, j = z + n + 1, j + 1
    sections = tuple(sorted({0, D // 3, min(D // 3 + 1, D - 1), D - 1}))
    vol.setflags(write=False), mask.setflags(write=False)
    return vol, mask.reshape(shape), sections


def _args(shape, R, srcs):
    vol, mask, sections = _defects(shape, R)
    return vol, dict(sections=sections if "sections" in srcs else None, mask=mask if "mask" in srcs else None,
                     missing_value=MISSING if "missing" in srcs else None, max_gap=R)


def _guarded(a, off):
    """The bytes of `a` on the device `off` bytes into a 256-byte-aligned allocation, between guards of FILL."""
    flat = np.array(a).reshape(-1)                                          # a copy: the cached cases stay read-only
    t = torch.full((flat.size + off + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    t[GUARD + off:GUARD + off + flat.size] = torch.from_numpy(flat).cuda()
    return t, t.data_ptr() + GUARD + off


def _run(block, kw, c0, c1, off=0, mask_off=None, zsec0=0, flags=None, counts=True):
    """tem_u8_repair_z on `block` (plane 0 is section zsec0 of a volume whose section flags are `flags`) -> (the block as
    the kernel left it, (repaired, unrepaired)); the guards around it must be untouched."""
    L, lib, stream = _env()
    D, H, W = block.shape
    t, p = _guarded(block, off)
    mt, mp = (None, None) if kw["mask"] is None else _guarded(kw["mask"], off if mask_off is None else mask_off)
    ft = None
    if kw["sections"] is not None:
        if flags is None:
            flags = np.zeros(D, np.uint8)
            flags[list(kw["sections"])] = 1
        ft = torch.from_numpy(flags).cuda()
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    missing = -1 if kw["missing_value"] is None else kw["missing_value"]
    L.check(lib.tem_u8_repair_z(p, D, H, W, zsec0, c0, c1, mp, None if ft is None else ft.data_ptr(), missing,
                                kw["max_gap"], cnt.data_ptr() if counts else None, stream), "tem_u8_repair_z")
    got = t.cpu().numpy()
    n = block.size
    assert (got[:GUARD + off] == FILL).all() and (got[GUARD + off + n:] == FILL).all()
    if mt is not None:
        assert np.array_equal(mt.cpu().numpy()[GUARD + (off if mask_off is None else mask_off):][:n],
                              kw["mask"].reshape(-1))
    return got[GUARD + off:GUARD + off + n].reshape(block.shape), tuple(int(v) for v in cnt.cpu().numpy())


def _want(block, kw, c0, c1):
    """The block with its core planes [c0, c1) repaired, and the two counts of the core."""
    want = np.array(block)
    want[c0:c1] = RR.repair(block, **kw)[c0:c1]
    bad, fil = RR.bad_voxels(block, kw["sections"], kw["mask"], kw["missing_value"])[c0:c1], RR.filled(block, **kw)[c0:c1]
    return want, (int(fil.sum()), int(bad.sum() - fil.sum()))


def _same(got, want):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    assert got[1] == want[1]


# ------------------------------------------------------------------------------------------------- tem_u8_repair_z
@pytest.mark.parametrize("R", GAPS)
@pytest.mark.parametrize("shape", BLOCKS, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_reference(shape, R):
    """Each source alone and all three together, the base pointer aligned and 1 and 3 bytes off; the core is the block."""
    for srcs in SOURCES:
        vol, kw = _args(shape, R, srcs)
        want = _want(vol, kw, 0, shape[0])
        if shape[0] > 2 * R + 1 and "mask" in srcs:
            assert want[1][0] > 0 and want[1][1] > 0                        # both counts are exercised
        for off in (0, 1, 3):
            _same(_run(vol, kw, 0, shape[0], off), want)


def test_kernel_defect_patterns_are_all_there():
    """What the parametrised test relies on, asserted on the patterns themselves."""
    for shape, R in itertools.product(BLOCKS[2:], GAPS[:3]):
        vol, mask, sections = _defects(shape, R)
        cols = (mask.reshape(shape[0], -1) != 0).T
        runs = lambda c: [(k, len(list(g))) for k, g in itertools.groupby(c)]
        seen = {n for c in cols for k, n in runs(c)[1:-1] if k}
        assert {1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1} <= seen, (shape, R, seen)
        assert any(c[0] and not c.all() for c in cols) and any(c[-1] and not c.all() for c in cols)
        assert any(c.all() for c in cols) and any(runs(c)[:4] == [(True, 1), (False, 1)] * 2 for c in cols)
        assert len({tuple(c) for c in cols[4:8]}) == 4                      # one dword, four phases
        good = (mask == 0)
        assert ((vol[1:] == MISSING) & (vol[:-1] != MISSING) & good[:-1]).any()
        assert 0 in sections and shape[0] - 1 in sections


@pytest.mark.parametrize("R", [3, 8])
def test_kernel_writes_the_core_only(R):
    """A core strictly inside the block, the block inside a larger volume (zsec0 > 0, flags of the whole volume): the
    halo planes are read and come back untouched, and only the core's voxels are counted."""
    for shape in BLOCKS[2:]:
        D = shape[0]
        vol, kw = _args(shape, R, SOURCES[3])
        zsec0 = 5
        flags = np.zeros(zsec0 + D + 4, np.uint8)
        flags[[zsec0 + z for z in kw["sections"]]] = 1
        flags[[0, zsec0 - 1, zsec0 + D]] = 1                                # other sections' flags: not this block's
        for c0, c1 in ((R, D - R), (R + 1, R + 2), (D - R - 1, D - R), (0, 1), (D - 1, D), (4, 4)):
            want = _want(vol, kw, c0, c1)
            for off in (0, 3):
                got = _run(vol, kw, c0, c1, off, zsec0=zsec0, flags=flags)
                _same(got, want)
                assert np.array_equal(got[0][:c0], vol[:c0]) and np.array_equal(got[0][c1:], vol[c1:])


def test_kernel_without_counts_and_with_a_mask_off_the_blocks_alignment():
    shape, R = BLOCKS[3], 3
    vol, kw = _args(shape, R, SOURCES[3])
    want = _want(vol, kw, 0, shape[0])
    got = _run(vol, kw, 0, shape[0], counts=False)
    assert np.array_equal(got[0], want[0]) and got[1] == (0, 0)
    _same(_run(vol, kw, 0, shape[0], off=0, mask_off=1), want)              # the byte path of an aligned block
    _same(_run(vol, kw, 0, shape[0], off=2, mask_off=3), want)


def test_kernel_leaves_good_data_alone_and_long_runs_in_the_middle():
    shape, R = (40, 4, 8), 3
    vol = np.random.default_rng(3).integers(1, 256, shape, dtype=np.uint8)
    kw = dict(sections=None, mask=np.zeros(shape, np.uint8), missing_value=None, max_gap=R)
    _same(_run(vol, kw, 0, 40), (vol, (0, 0)))
    kw = dict(sections=tuple(range(10, 20)), mask=None, missing_value=None, max_gap=R)          # a run of 10 > 2 R
    got, counts = _run(vol, kw, 0, 40)
    assert counts == (6 * 32, 4 * 32) and np.array_equal(got[13:17], vol[13:17])
    assert (got[10:13] == vol[9]).all() and (got[17:20] == vol[20]).all()
    _same((got, counts), _want(vol, kw, 0, 40))


def test_kernel_refuses_bad_arguments():
    L, lib, stream = _env()
    t = torch.full((4 * 4 * 4,), FILL, dtype=torch.uint8, device="cuda")
    p, f = t.data_ptr(), torch.zeros(8, dtype=torch.uint8, device="cuda").data_ptr()
    call = lambda *a: lib.tem_u8_repair_z(*a, stream)
    ok = [p, 4, 4, 4, 0, 0, 4, None, f, -1, 8, None]
    for i, v in [(0, None), (1, 0), (2, 0), (3, -1), (4, -1), (10, 0), (10, 33), (5, -1), (6, 5), (5, 3), (8, None),
                 (9, 256), (9, -2), (11, f + 1)]:
        a = list(ok)
        a[i] = v
        if i == 5 and v == 3:
            a[6] = 2                                                        # c0 > c1
        assert call(*a) == L.TEM_EINVAL, (i, v)
    assert call(*ok) == 0 and call(*ok[:5], 2, 2, *ok[7:]) == 0             # an empty core launches nothing
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == FILL).all()


# --------------------------------------------------------------------------------------------------- volume_repair
VSHAPE, VGAP = (40, 21, 30), 3
ROI = dict(start=(4, 3, 2), size=(25, 17, 37))                              # (x, y, z): off every face but z's far one


@functools.lru_cache(maxsize=None)
def _vcase():
    vol, kw = _args(VSHAPE, VGAP, SOURCES[3])
    want = RR.repair(vol, **kw)
    want.setflags(write=False)
    return vol, kw, want


def _roi_counts(vol, kw, box):
    sl = tuple(slice(lo, hi) for lo, hi in box)
    bad, fil = RR.bad_voxels(vol, kw["sections"], kw["mask"], kw["missing_value"])[sl], RR.filled(vol, **kw)[sl]
    return int(fil.sum()), int(bad.sum() - fil.sum())


@pytest.mark.parametrize("chunk_bytes", [None, 5000, 1500, 1], ids=["one_slab", "sections", "rows", "one_row"])
def test_volume_repair_equals_the_reference(chunk_bytes):
    from transfer_em_amd.utils import Repair, hist_box, repair_chunks, volume_repair
    vol, kw, want = _vcase()
    rp = Repair(**kw)
    st = {}
    got = volume_repair(vol, rp, chunk_bytes=chunk_bytes, stats=st)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert (st["repaired"], st["unrepaired"]) == _roi_counts(vol, kw, hist_box(VSHAPE)) and st["unrepaired"] > 0
    assert st["chunks"] == len(repair_chunks(hist_box(VSHAPE), VSHAPE, VGAP, chunk_bytes))
    box = hist_box(VSHAPE, ROI["start"], ROI["size"])
    sl = tuple(slice(lo, hi) for lo, hi in box)
    out = np.full(want[sl].shape, FILL, np.uint8)
    st = {}
    assert volume_repair(vol, rp, out=out, chunk_bytes=chunk_bytes, stats=st, **ROI) is out
    assert np.array_equal(out, want[sl])                                    # the ROI of the whole result
    assert (st["repaired"], st["unrepaired"]) == _roi_counts(vol, kw, box)
    n = len(repair_chunks(box, VSHAPE, VGAP, chunk_bytes))
    assert st["chunks"] == n and {None: n == 1, 5000: n > 3, 1500: n > 37, 1: n == 37 * 17}[chunk_bytes]
    assert st["read_s"] >= 0 and st["write_s"] >= 0


def test_volume_repair_memmap_and_two_ranks(tmp_path):
    from transfer_em_amd.utils import Repair, hist_box, volume_repair
    vol, kw, want = _vcase()
    src = np.memmap(tmp_path / "vol.u8", np.uint8, "w+", shape=VSHAPE)
    msk = np.memmap(tmp_path / "mask.u8", np.uint8, "w+", shape=VSHAPE)
    src[...], msk[...] = vol, kw["mask"]
    box = hist_box(VSHAPE, ROI["start"], ROI["size"])
    sl = tuple(slice(lo, hi) for lo, hi in box)
    out = np.memmap(tmp_path / "out.u8", np.uint8, "w+", shape=want[sl].shape)
    out[...] = FILL
    rp = Repair(kw["sections"], msk, kw["missing_value"], VGAP)
    stats = [{}, {}]
    for rank in (1, 0):                                                     # two ranks into one `out`
        volume_repair(src, rp, out=out, chunk_bytes=1500, stats=stats[rank], rank=rank, world_size=2, **ROI)
        if rank == 1:
            assert (np.asarray(out) == FILL).any()                          # rank 0's boxes are still to come
    assert np.array_equal(np.asarray(out), want[sl])
    assert abs(stats[0]["chunks"] - stats[1]["chunks"]) <= 1
    total = tuple(stats[0][k] + stats[1][k] for k in ("repaired", "unrepaired"))
    assert total == _roi_counts(vol, kw, box)                               # cores are disjoint: the ranks' counts add
    assert np.array_equal(np.asarray(src), vol) and np.array_equal(np.asarray(msk), kw["mask"])     # inputs: read only


# -------------------------------------------------------------------------------------------------- tiled inference
# the 74 model: tiles of 36 under a halo of 19.  Tile faces of the ROI lie at x = 31, y = 39, z = 32; with chunk_tiles
# (1, 1, 1) they are chunk faces too.  The blob crosses all three; the bad sections sit at the volume's faces, in the
# halo of the first tile and across the tile face.
MS_X, MS_Y = (0.02, 0.58), (-0.1, 0.4)
VOL, START, SIZE, GAP = (50, 60, 70), (-5, 3, -4), (50, 41, 40), 4
VOL2, START2, SIZE2 = (7, 60, 70), (-5, 3, 1), (50, 41, 5)                  # 2-D: 2 x 2 tiles in each of 5 sections


def _pcase(shape, seed, sections, blob):
    vol = ramp_volume(shape, seed)
    mask = np.zeros(shape, np.uint8)
    mask[blob[0]:blob[1], 30:48, 22:40] = 9
    mask[:, 5, 6] = 1                                                       # a wholly bad column
    kw = dict(sections=sections, mask=mask, missing_value=None, max_gap=GAP)
    fixed = RR.repair(vol, **kw)
    assert (fixed != vol).mean() > 0.1 and RR.filled(vol, **kw).sum() < RR.bad_voxels(vol, sections, mask).sum()
    return vol, kw, fixed


@pytest.fixture(scope="module")
def model3(tmp_path_factory):
    return _model(tmp_path_factory.mktemp("repair3"), "repair3", True)


@pytest.fixture(scope="module")
def model2(tmp_path_factory):
    return _model(tmp_path_factory.mktemp("repair2"), "repair2", False)


@pytest.fixture(scope="module")
def case3():
    return _pcase(VOL, 81, [0, 1, 12, 13, 14, 31, 32, 49], (28, 37))       # a blob of 9 sections > 2 GAP: a middle stays


@pytest.fixture(scope="module")
def case2():
    return _pcase(VOL2, 82, [0, 3, 6], (4, 6))


def _eq(a, b):
    assert a.shape == b.shape and np.array_equal(a, b), np.argwhere(a != b)[:5]


def _all_ways(model, case, start, size, **kw):
    """predict_cube, predict_volume in chunks of one tile and with its default chunks, with `repair`, against
    predict_cube on the host-repaired volume; fetch_input is the repaired ROI."""
    from transfer_em_amd.utils import Repair, predict_cube, predict_volume
    vol, rkw, fixed = case
    rp = Repair(**rkw)
    want_in, want = predict_cube(fixed, start, size, model, MS_X, MS_Y, fetch_input=True, **kw)
    got_in, got = predict_cube(vol, start, size, model, MS_X, MS_Y, fetch_input=True, repair=rp, **kw)
    levels = lambda r: r if isinstance(r, list) else [r]
    first = levels(want)[0]
    # not the check, its precondition: a flat prediction would make the equalities below vacuous.  Ten grey levels of
    # spread over sixteen values or more is far from flat, whatever the keywords do to the contrast
    assert first.std() > 10 and len(np.unique(first)) >= 16
    plain = predict_cube(vol, start, size, model, MS_X, MS_Y, **kw)
    assert not np.array_equal(levels(plain)[0], first)                      # ... and the defects reach the prediction
    _eq(got_in, want_in)
    for g, w in zip(levels(got), levels(want)):
        _eq(g, w)
    for chunk_tiles in ((1, 1, 1), None):
        st = {}
        res = predict_volume(vol, start, size, model, MS_X, MS_Y, chunk_tiles=chunk_tiles, repair=rp, stats=st, **kw)
        assert st["chunks"] >= (8 if chunk_tiles and len(size) == 3 and model.generator_g.is3d else 1)
        assert len(levels(res)) == len(levels(want))
        for g, w in zip(levels(res), levels(want)):
            _eq(g, w)
    return want_in


COMBINED = dict(boundary="reflect", ensemble="flips", mips=1)


def _combined(case):
    """COMBINED plus a per-section lut and the CLAHE tables of the repaired volume."""
    from transfer_em_amd.utils import clahe_fit
    Z = case[0].shape[0]
    t = (255 - (np.arange(256) // 2) * 2).astype(np.uint8)
    return dict(COMBINED, lut=np.stack([np.roll(t, z) for z in range(Z)]), clahe=clahe_fit(case[2], (16, 24)))


def test_predict_3d_with_repair_equals_predict_on_the_repaired_volume(model3, case3):
    want_in = _all_ways(model3, case3, START, SIZE)
    z0, y0, x0 = -START[2], START[1], -START[0]
    _eq(want_in[z0:, :, x0:], case3[2][:SIZE[2] - z0, y0:y0 + SIZE[1], :SIZE[0] - x0])      # the repaired ROI ...
    assert (want_in[:z0] == 0).all() and (want_in[:, :, :x0] == 0).all()     # ... and 0 outside the volume, not "missing"


def test_predict_3d_with_repair_composes(model3, case3):
    _all_ways(model3, case3, START, SIZE, **_combined(case3))


def test_predict_2d_with_repair_equals_predict_on_the_repaired_volume(model2, case2):
    _all_ways(model2, case2, START2, SIZE2)


def test_predict_2d_with_repair_composes(model2, case2):
    _all_ways(model2, case2, START2, SIZE2, **_combined(case2))


def test_predict_with_repair_across_ranks_and_with_compare(model3, case3):
    from transfer_em_amd.utils import Repair, predict_cube, predict_volume
    vol, rkw, fixed = case3
    rp = Repair(**rkw)
    gt = ramp_volume(VOL, 83)
    st_w, st_g = {}, {}
    want = predict_cube(fixed, START, SIZE, model3, MS_X, MS_Y, compare=gt, stats=st_w)
    out = np.zeros(want.shape, np.uint8)
    joint = np.zeros((256, 256), np.int64)
    for rank in (0, 1):
        predict_volume(vol, START, SIZE, model3, MS_X, MS_Y, out=out, chunk_tiles=(1, 1, 1), tile_batch=1, rank=rank,
                       world_size=2, repair=rp, compare=gt, stats=st_g)
        joint += st_g["joint_histogram"]
    _eq(out, want)
    assert np.array_equal(joint, st_w["joint_histogram"])


def test_predict_without_repair_runs_the_unchanged_launches(model3, case3):
    from test_gpu_histogram import _counted
    from transfer_em_amd.utils import Repair, predict_volume
    vol, rkw, _ = case3
    run = lambda **kw: predict_volume(vol, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 1), **kw)
    _, plain = _counted(run)
    _, with_rp = _counted(lambda: run(repair=Repair(**rkw)))
    assert "tem_u8_repair_z" not in plain and with_rp.pop("tem_u8_repair_z") == 8      # one launch per chunk
    assert with_rp == plain


# ----------------------------------------------------------------------------------------------------------- errors
def test_every_refusal_comes_before_any_gpu_work(model3, model2, case3):
    from transfer_em_amd.utils import Repair, predict_cube, predict_volume, volume_repair
    vol = case3[0]
    mask = np.zeros(VOL, np.uint8)
    bad = [Repair(), Repair(sections=[1], max_gap=0), Repair(sections=[1], max_gap=33), Repair(sections=[VOL[0]]),
           Repair(sections=[-1]), Repair(mask=mask[1:]), Repair(mask=mask.astype(np.int8)), Repair(missing_value=256),
           Repair(missing_value=-1), "sections"]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for rp in bad:
        for fn in (predict_cube, predict_volume):
            with pytest.raises(ValueError):
                fn(vol, START, SIZE, model3, MS_X, MS_Y, repair=rp)
        with pytest.raises(ValueError):
            volume_repair(vol, rp)
    for fn in (predict_cube, predict_volume):                               # one image has no z
        with pytest.raises(ValueError, match="z"):
            fn(vol[0], START[:2], SIZE[:2], model2, MS_X, MS_Y, repair=Repair(missing_value=0))
        with pytest.raises(ValueError, match="uint8"):
            fn(vol.astype(np.int16), START, SIZE, model3, MS_X, MS_Y, repair=Repair(missing_value=0))
    with pytest.raises(ValueError):
        volume_repair(vol, Repair(missing_value=0), out=np.zeros(VOL, np.int8))
    with pytest.raises(ValueError):
        volume_repair(vol, Repair(missing_value=0), start=(0, 0, 1), size=(70, 60, 50))
    assert torch.cuda.memory_allocated() == before
