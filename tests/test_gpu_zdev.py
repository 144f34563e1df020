"""The z-median outliers on the device: tem_u8_zdev_tiles and tem_u8_zdev_mask against the numpy reference (zdev_ref) at
the smallest shapes where they can go wrong, the two out-of-core passes however they are cut, and the fixture with
planted particles end to end through volume_repair.  Every comparison of sums and bytes is exact.  The kernels read src
and write dst between guards of fill bytes; src and all guards must come back untouched.  Helpers are those of
test_gpu_histogram.py and test_gpu_resample_z.py."""
import functools

import numpy as np
import pytest
import torch

import repair_ref as RR
import zdev_ref as ZD
from test_gpu_histogram import _counted, _env
from test_gpu_resample_z import DFILL, FILL, _Dev

pytestmark = pytest.mark.gpu

VOLUMES = [(5, 37, 53), (9, 20, 131), (17, 6, 21)]
TILES = [(16, 16), (7, 19)]


@functools.lru_cache(maxsize=None)
def _data(shape):
    a = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    a[:3, 0, :4] = ((0, 255, 7, 7), (255, 0, 7, 200), (0, 255, 7, 100))       # the extremes; equal; inside the range
    a.setflags(write=False)
    return a


def _tables(Z):
    """name -> nbr [Z, 2]: consecutive, bridged at lag 2 and (Z = 17) lag 8, rows without a verdict."""
    t = {"consecutive": ZD.neighbours(Z), "bridged_lag_2": ZD.neighbours(Z, [2])}
    if Z >= 9:
        t["gaps_and_no_verdict"] = ZD.neighbours(Z, [1, 4, 5], 2)
        assert t["gaps_and_no_verdict"][3].tolist() == [-1, -1] and t["gaps_and_no_verdict"][2].tolist() == [0, 3]
    if Z == 17:
        t["bridged_lag_8"] = ZD.neighbours(Z, list(range(1, 8)) + list(range(9, 16)), 8)
        assert t["bridged_lag_8"][8].tolist() == [0, 16]
    return t


def _grid(Y, X, tile):
    return -(-Y // tile[0]), -(-X // tile[1])


def _thr(gy, gx, seed=0):
    """Thresholds around the mean deviation of random bytes (about 42 grey levels), so that both verdicts occur."""
    return np.random.default_rng(seed).integers(7000, 15000, (gy, gx)).astype(np.int32)


def _tiles_call(src, dims, sz0, Z, c0, c1, y_org, x_org, tile, grid, nbr, acc, dev_nbr=None):
    L, lib, stream = _env()
    host = np.ascontiguousarray(nbr, np.int32)
    devt = torch.from_numpy(np.ascontiguousarray(host if dev_nbr is None else dev_nbr, np.int32)).cuda()
    rc = lib.tem_u8_zdev_tiles(src.ptr, *dims, sz0, Z, c0, c1, y_org, x_org, *tile, *grid, host.ctypes.data,
                               devt.data_ptr(), acc.data_ptr(), stream)
    torch.cuda.synchronize()
    return rc


def _mask_call(src, dims, sz0, Z, Y, y_org, core, tile, grid, radius, nbr, thr, dst, marks=None, count=None,
               dev_nbr=None, dev_thr=None):
    """One tem_u8_zdev_mask call; core = ((c0, c1), (r0, r1), (x0, x1)) in the block; marks: the uint8 table [Z, gy, gx]."""
    L, lib, stream = _env()
    host, th = np.ascontiguousarray(nbr, np.int32), np.ascontiguousarray(thr, np.int32)
    devt = torch.from_numpy(np.ascontiguousarray(host if dev_nbr is None else dev_nbr, np.int32)).cuda()
    devh = torch.from_numpy(np.ascontiguousarray(th if dev_thr is None else dev_thr, np.int32)).cuda()
    (c0, c1), (r0, r1), (x0, x1) = core
    mk = None if marks is None else torch.from_numpy(np.ascontiguousarray(marks, np.uint8)).cuda()
    rc = lib.tem_u8_zdev_mask(src.ptr, *dims, sz0, Z, Y, y_org, c0, c1, r0, r1, x0, x1, *tile, *grid, radius,
                              host.ctypes.data, devt.data_ptr(), th.ctypes.data, devh.data_ptr(),
                              None if mk is None else mk.data_ptr() + (sz0 + c0) * grid[0] * grid[1], dst.ptr,
                              None if count is None else count.data_ptr(), stream)
    torch.cuda.synchronize()
    return rc


# -------------------------------------------------------------------------------------------------- tem_u8_zdev_tiles
@pytest.mark.parametrize("shape", VOLUMES, ids=lambda s: "x".join(map(str, s)))
def test_tiles_kernel_equals_the_reference(shape):
    """Every table and tile, the block on and off the grid, the base pointer at byte offsets 0, 1 and 3; W = 53, 131 and
    21 are no multiple of 4."""
    L = _env()[0]
    Z, Y, X = shape
    vol = _data(shape)
    srcs = {off: _Dev(vol.size, off, FILL, vol) for off in (0, 1, 3)}
    for name, nbr in _tables(Z).items():
        e, verdict = ZD.deviation(vol, nbr), (nbr[:, 0] >= 0).tolist()
        assert e.any()
        for tile in TILES:
            for y_org, x_org in ((0, 0), (5, 9)):
                grid = _grid(y_org + Y, x_org + X, tile)
                want = ZD.tile_sums(e, verdict, y_org, x_org, *tile, *grid)
                assert want[..., 1].sum() == sum(verdict) * Y * X
                for off, src in srcs.items():
                    acc = torch.zeros(want.shape, dtype=torch.int64, device="cuda")
                    L.check(_tiles_call(src, shape, 0, Z, 0, Z, y_org, x_org, tile, grid, nbr, acc), "tem_u8_zdev_tiles")
                    assert np.array_equal(acc.cpu().numpy(), want), (name, tile, y_org, x_org, off)
    for s in srcs.values():
        assert np.array_equal(s.body(), vol.reshape(-1))


def test_tile_sums_accumulate_across_cuts_in_z_y_and_x():
    """Blocks that cut the volume -- and its tiles -- along z (each with the planes its table names), y and x add up to
    the sums of the whole; a block of one tile row taller than a part (more than one workgroup per tile)."""
    L = _env()[0]
    shape, tile = (9, 20, 131), (7, 19)
    Z, Y, X = shape
    vol, nbr, grid = _data(shape), ZD.neighbours(Z, [4]), _grid(Y, X, tile)
    want = ZD.volume_sums(vol, nbr, tile)
    acc = torch.zeros(want.shape, dtype=torch.int64, device="cuda")
    sec = grid[0] * grid[1] * 2
    for (c0, c1), (s0, s1) in (((0, 3), (0, 4)), ((3, 6), (2, 7)), ((6, 9), (3, 9))):      # 3 and 5 bridge section 4
        for y0, y1 in ((0, 9), (9, 20)):
            for x0, x1 in ((0, 30), (30, 131)):
                block = vol[s0:s1, y0:y1, x0:x1]
                src = _Dev(block.size, (c0 + y0 + x0) % 4, FILL, block)
                L.check(_tiles_call(src, block.shape, s0, Z, c0 - s0, c1 - s0, y0, x0, tile, grid, nbr,
                                    acc.view(-1)[c0 * sec:]), "tem_u8_zdev_tiles")
                assert np.array_equal(src.body(), block.reshape(-1))
    assert np.array_equal(acc.cpu().numpy(), want)
    tall = np.random.default_rng(3).integers(0, 256, (3, 300, 70), dtype=np.uint8)          # 300 rows x 5 pieces: 2 parts
    nb3 = ZD.neighbours(3)
    acc = torch.zeros((3, 1, 1, 2), dtype=torch.int64, device="cuda")
    L.check(_tiles_call(_Dev(tall.size, 2, FILL, tall), tall.shape, 0, 3, 0, 3, 0, 0, (2048, 2048), (1, 1), nb3, acc),
            "tem_u8_zdev_tiles")
    assert np.array_equal(acc.cpu().numpy(), ZD.volume_sums(tall, nb3, (2048, 2048)))
    assert acc.cpu().numpy()[1, 0, 0].tolist() == [int(ZD.deviation(tall, nb3)[1].astype(np.int64).sum()), 300 * 70]


def test_tiles_kernel_refuses_bad_arguments():
    """TEM_EINVAL from the host-side checks, nothing launched: the sums stay zero."""
    L, lib, stream = _env()
    Z, H, W = 8, 6, 10
    vol = _data((Z, H, W))
    src = _Dev(4 * H * W, 0, FILL, vol[2:6])                              # sections 2...5; the core: 3 and 4
    nbr = ZD.neighbours(Z)
    acc = torch.zeros((2, 1, 1, 2), dtype=torch.int64, device="cuda")
    good = dict(dims=(4, H, W), sz0=2, Z=Z, c0=1, c1=3, y_org=0, x_org=0, tile=(16, 16), grid=(1, 1), nbr=nbr)

    def call(**kw):
        a = dict(good, **kw)
        return _tiles_call(a.get("src", src), a["dims"], a["sz0"], a["Z"], a["c0"], a["c1"], a["y_org"], a["x_org"],
                           a["tile"], a["grid"], a["nbr"], a.get("acc", acc))

    class _Null:
        ptr = None

    def tab(z, lo, hi):
        t = nbr.copy()
        t[z] = (lo, hi)
        return t

    for kw in (dict(src=_Null), dict(dims=(0, H, W)), dict(dims=(4, 0, W)), dict(dims=(4, H, 0)), dict(Z=0), dict(sz0=-1),
               dict(sz0=5), dict(c0=-1), dict(c0=3, c1=2), dict(c1=5), dict(y_org=-1), dict(x_org=-1), dict(y_org=11),
               dict(x_org=7), dict(tile=(0, 16)), dict(tile=(16, 2049)), dict(grid=(0, 1)), dict(grid=(1, 0)),
               dict(acc=acc.view(-1).view(torch.uint8)[4:].view(torch.int32)),              # sums off 8-byte alignment
               dict(nbr=tab(3, -1, 4)), dict(nbr=tab(3, 2, -1)), dict(nbr=tab(3, 3, 4)), dict(nbr=tab(3, 2, 3)),
               dict(nbr=tab(4, 3, 8)), dict(nbr=tab(4, 5, 3)),
               dict(nbr=tab(3, 1, 4)), dict(nbr=tab(4, 3, 6)),                              # named sections outside the block
               dict(c0=0, c1=1)):                                                           # section 2 needs section 1
        assert call(**kw) == L.TEM_EINVAL, kw
    far = ZD.neighbours(30)
    far[12] = (3, 13)                                                                       # z - lo = 9 > 8
    big = _Dev(12 * 2 * 2, 0, FILL, np.zeros((12, 2, 2), np.uint8))
    assert _tiles_call(big, (12, 2, 2), 2, 30, 10, 11, 0, 0, (16, 16), (1, 1), far, acc) == L.TEM_EINVAL
    devt = torch.from_numpy(nbr).cuda()
    assert lib.tem_u8_zdev_tiles(src.ptr, 4, H, W, 2, Z, 1, 3, 0, 0, 16, 16, 1, 1, None, devt.data_ptr(), acc.data_ptr(),
                                 stream) == L.TEM_EINVAL
    assert lib.tem_u8_zdev_tiles(src.ptr, 4, H, W, 2, Z, 1, 3, 0, 0, 16, 16, 1, 1, nbr.ctypes.data, None, acc.data_ptr(),
                                 stream) == L.TEM_EINVAL
    assert lib.tem_u8_zdev_tiles(src.ptr, 4, H, W, 2, Z, 1, 3, 0, 0, 16, 16, 1, 1, nbr.ctypes.data, devt.data_ptr(), None,
                                 stream) == L.TEM_EINVAL
    wide = torch.zeros(2 * Z + 1, dtype=torch.int32, device="cuda")                         # nbr_dev off 4-byte alignment
    assert lib.tem_u8_zdev_tiles(src.ptr, 4, H, W, 2, Z, 1, 3, 0, 0, 16, 16, 1, 1, nbr.ctypes.data, wide.data_ptr() + 2,
                                 acc.data_ptr(), stream) == L.TEM_EINVAL
    # more workgroups than one launch holds, with dimensions that are only claimed; refused before anything is touched:
    # 4096 x 4096 tiles of one voxel are 2^24 parts; 4096 x 2048 of them in 2 runs of up to 16 planes are 2^24 workgroups
    none = np.full((17, 2), -1, np.int32)
    dnone = torch.from_numpy(none).cuda()
    many = lambda D, W, gx: lib.tem_u8_zdev_tiles(src.ptr, D, 4096, W, 0, D, 0, D, 0, 0, 1, 1, 4096, gx, none.ctypes.data,
                                                  dnone.data_ptr(), acc.data_ptr(), stream)
    assert many(1, 4096, 4096) == L.TEM_EUNSUPPORTED and many(17, 2048, 2048) == L.TEM_EUNSUPPORTED
    torch.cuda.synchronize()
    assert not acc.cpu().numpy().any()
    # rows of the table outside the core are not looked at; an empty core launches nothing; the good call counts
    assert call(nbr=tab(0, 99, -99)) == 0 and call(c0=2, c1=2, nbr=tab(3, 9, 9)) == 0 and call() == 0
    want = ZD.volume_sums(vol, nbr, (16, 16))[3:5]
    assert np.array_equal(acc.cpu().numpy(), 2 * want)
    # a device table that disagrees with the host's: other sums, clamped into the block, never a fault
    wild = nbr.copy()
    wild[3], wild[4] = (-7, 1 << 30), (1 << 30, 0)
    acc.zero_()
    assert _tiles_call(src, (4, H, W), 2, Z, 1, 3, 0, 0, (16, 16), (1, 1), nbr, acc, dev_nbr=wild) == 0
    assert acc.cpu().numpy().shape == (2, 1, 1, 2)
    assert np.array_equal(src.body(), vol[2:6].reshape(-1))


# --------------------------------------------------------------------------------------------------- tem_u8_zdev_mask
def _mask_whole(vol, nbr, thr, tile, radius, marks, off=0, with_count=True):
    """The kernel's mask of a whole volume in one call, its count, after the guards were checked."""
    L = _env()[0]
    Z, Y, X = vol.shape
    src, dst = _Dev(vol.size, off, FILL, vol), _Dev(vol.size, (off + 1) % 4, DFILL)
    count = torch.full((1,), 5, dtype=torch.int64, device="cuda") if with_count else None
    L.check(_mask_call(src, vol.shape, 0, Z, Y, 0, ((0, Z), (0, Y), (0, X)), tile, _grid(Y, X, tile), radius, nbr, thr,
                       dst, marks, count), "tem_u8_zdev_mask")
    assert np.array_equal(src.body(), vol.reshape(-1))
    return dst.body().reshape(vol.shape), None if count is None else int(count.cpu()[0]) - 5


@pytest.mark.parametrize("radius", [1, 4, 7])
@pytest.mark.parametrize("shape", VOLUMES, ids=lambda s: "x".join(map(str, s)))
def test_mask_kernel_equals_the_reference(shape, radius):
    """Every table and tile; tiles_dev and count present and null; the base pointers at every byte offset."""
    Z, Y, X = shape
    vol = _data(shape)
    k = mixed = 0
    for name, nbr in _tables(Z).items():
        for tile in TILES:
            gy, gx = _grid(Y, X, tile)
            thr = _thr(gy, gx, radius)
            marks = (np.random.default_rng(9).integers(0, 7, (Z, gy, gx)) == 0).astype(np.uint8) * 3
            for mk in (None, marks):
                want = ZD.mask(vol, nbr, thr, tile, radius, mk)
                got, n = _mask_whole(vol, nbr, thr, tile, radius, mk, off=k % 4, with_count=k % 3 != 2)
                k += 1
                assert np.array_equal(got, want), (name, tile, mk is None, np.argwhere(got != want)[:5])
                assert n is None or n == int(want.sum())
                mixed += 0 < want.sum() < want.size
                assert mk is None or want[marks.repeat(tile[0], 1).repeat(tile[1], 2)[:, :Y, :X] != 0].all()
    assert mixed >= k // 2                                                # most cases hold both verdicts


def test_mask_of_a_section_smaller_than_the_window():
    """Y = 5, X = 3 under windows of 3, 9 and 15: c is the whole section for the larger two."""
    vol = np.random.default_rng(2).integers(0, 256, (4, 5, 3), dtype=np.uint8)
    nbr, thr = ZD.neighbours(4), np.array([[9000]], np.int32)
    for radius in (1, 4, 7):
        want = ZD.mask(vol, nbr, thr, (16, 16), radius)
        got, n = _mask_whole(vol, nbr, thr, (16, 16), radius, None, off=radius % 4)
        assert np.array_equal(got, want) and n == int(want.sum())
        if radius >= 4:
            assert all(len(np.unique(want[z])) == 1 for z in range(4))                      # one window: one verdict


def test_mask_equality_does_not_flag_and_nothing_overflows():
    """A constant plane of 10 between planes of 0: Ws = 10 c everywhere, flagged at thr = 2559 and not at 2560.  A plane
    of 255 between zeros at radius 7: Ws = 57,375 at the full windows, flagged at 65279 and not at 65280."""
    shape = (3, 21, 37)
    vol = np.zeros(shape, np.uint8)
    vol[1] = 10
    nbr, grid = ZD.neighbours(3), _grid(21, 37, (16, 16))
    for radius in (1, 4, 7):
        for t, flagged in ((2559, True), (2560, False)):
            thr = np.full(grid, t, np.int32)
            got, n = _mask_whole(vol, nbr, thr, (16, 16), radius, None)
            assert np.array_equal(got, ZD.mask(vol, nbr, thr, (16, 16), radius))
            assert not got[0].any() and not got[2].any() and got[1].all() == flagged and got[1].any() == flagged
            assert n == (21 * 37 if flagged else 0)
    vol = np.zeros(shape, np.uint8)
    vol[1] = 255
    assert int(ZD.window_sums(ZD.deviation(vol, nbr), 7)[0].max()) == 57375
    for t, flagged in ((65279, True), (65280, False)):
        thr = np.full(grid, t, np.int32)
        got, n = _mask_whole(vol, nbr, thr, (16, 16), 7, None)
        assert np.array_equal(got, ZD.mask(vol, nbr, thr, (16, 16), 7)) and got[1].all() == flagged and n == flagged * 777


@pytest.mark.parametrize("radius", [1, 4, 7])
def test_mask_of_sub_blocks_with_cores_cut_in_z_y_and_x(radius):
    """Blocks that hold only what their core needs -- the planes its table names, `radius` rows more on each side where
    the section has them -- at sz0 > 0 and y_org > 0, cores cut along every axis inside them: each equals the same box of
    the whole volume's reference."""
    L = _env()[0]
    shape, tile = (9, 20, 131), (7, 19)
    Z, Y, X = shape
    vol, nbr, grid = _data(shape), ZD.neighbours(Z, [4]), _grid(Y, X, tile)
    thr = _thr(*grid, 5)
    marks = (np.random.default_rng(1).integers(0, 9, (Z,) + grid) == 0).astype(np.uint8)
    want = ZD.mask(vol, nbr, thr, tile, radius, marks)
    total = 0
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    for (c0, c1), (s0, s1) in (((0, 3), (0, 4)), ((3, 6), (2, 7)), ((6, 9), (3, 9))):
        for y0, y1 in ((0, 3), (3, 12), (12, 20)):
            b0, b1 = max(y0 - radius, 0), min(y1 + radius, Y)
            for x0, x1 in ((0, 33), (33, 34), (34, 131)):
                block = vol[s0:s1, b0:b1]
                src, dst = _Dev(block.size, (y0 + x0) % 4, FILL, block), _Dev((c1 - c0) * (y1 - y0) * (x1 - x0), x1 % 4, DFILL)
                L.check(_mask_call(src, block.shape, s0, Z, Y, b0, ((c0 - s0, c1 - s0), (y0 - b0, y1 - b0), (x0, x1)), tile,
                                   grid, radius, nbr, thr, dst, marks, count), "tem_u8_zdev_mask")
                box = want[c0:c1, y0:y1, x0:x1]
                assert np.array_equal(dst.body().reshape(box.shape), box), (c0, y0, x0)
                assert np.array_equal(src.body(), block.reshape(-1))
                total += int(box.sum())
    assert total == int(want.sum()) == int(count.cpu()[0])


def test_mask_workgroups_that_own_a_run_of_tiles():
    """From 16384 tiles of 8 x 32 outputs on, a workgroup owns two tiles or more: 10 core planes of 65 x 33 tiles are
    21450, so runs of 2 with a last run of 1 per plane (2145 is odd), and the count takes one add per run."""
    shape, tile = (10, 520, 1030), (128, 128)
    Z, Y, X = shape
    vol, nbr = _data(shape), ZD.neighbours(Z, [5])
    thr = _thr(*_grid(Y, X, tile), 2)
    want = ZD.mask(vol, nbr, thr, tile, 1)
    got, n = _mask_whole(vol, nbr, thr, tile, 1, None, off=3)
    assert np.array_equal(got, want) and n == int(want.sum()) and 0 < n < want.size and not want[5].any()


def test_mask_kernel_refuses_bad_arguments():
    """TEM_EINVAL from the host-side checks, nothing launched: dst keeps its fill."""
    L, lib, stream = _env()
    Z, Y, X, r = 8, 30, 10, 2
    vol = _data((Z, Y, X))
    block = vol[2:6, 8:20]                                                # sections 2...5, rows 8...19; core rows 10...17
    src, dst = _Dev(block.size, 0, FILL, block), _Dev(2 * 8 * X, 0, DFILL)
    nbr, thr = ZD.neighbours(Z), np.full((2, 1), 9000, np.int32)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    good = dict(dims=(4, 12, X), sz0=2, Z=Z, Y=Y, y_org=8, core=((1, 3), (2, 10), (0, X)), tile=(16, 16), grid=(2, 1),
                radius=r, nbr=nbr, thr=thr, count=count)

    def call(**kw):
        a = dict(good, **kw)
        return _mask_call(a.get("src", src), a["dims"], a["sz0"], a["Z"], a["Y"], a["y_org"], a["core"], a["tile"],
                          a["grid"], a["radius"], a["nbr"], a["thr"], a.get("dst", dst), None, a["count"])

    class _Null:
        ptr = None

    def tab(z, lo, hi):
        t = nbr.copy()
        t[z] = (lo, hi)
        return t

    def core(c=(1, 3), rows=(2, 10), cols=(0, X)):
        return dict(core=(c, rows, cols))

    for kw in (dict(src=_Null), dict(dst=_Null), dict(dims=(0, 12, X)), dict(dims=(4, 0, X)), dict(dims=(4, 12, 0)),
               dict(Z=0), dict(Y=0), dict(sz0=-1), dict(sz0=5), dict(y_org=-1), dict(y_org=19), dict(Y=33), dict(grid=(2, 0)),
               dict(grid=(0, 1)), dict(grid=(1, 1)), dict(tile=(16, 9)), dict(tile=(0, 16)), dict(tile=(2049, 16)),
               dict(radius=0), dict(radius=8), core(c=(-1, 3)), core(c=(3, 1)), core(c=(1, 5)), core(rows=(-1, 10)),
               core(rows=(10, 2)), core(rows=(2, 13)), core(cols=(-1, X)), core(cols=(5, 4)), core(cols=(0, X + 1)),
               core(rows=(1, 10)), core(rows=(2, 11)),                                      # a window's row is not held
               dict(thr=np.array([[9000], [0]], np.int32)), dict(thr=np.array([[65281], [9000]], np.int32)),
               dict(nbr=tab(3, -1, 4)), dict(nbr=tab(3, 3, 4)), dict(nbr=tab(4, 3, 8)), dict(nbr=tab(3, 1, 4)),
               dict(nbr=tab(4, 3, 6)), core(c=(0, 1)),
               dict(count=torch.zeros(4, dtype=torch.int32, device="cuda")[1:])):           # count off 8-byte alignment
        assert call(**kw) == L.TEM_EINVAL, kw
    devt, devh = torch.from_numpy(nbr).cuda(), torch.from_numpy(thr).cuda()
    tables = [nbr.ctypes.data, devt.data_ptr(), thr.ctypes.data, devh.data_ptr()]
    for k in range(4):
        t = list(tables)
        t[k] = None
        assert lib.tem_u8_zdev_mask(src.ptr, 4, 12, X, 2, Z, Y, 8, 1, 3, 2, 10, 0, X, 16, 16, 2, 1, r, *t, None, dst.ptr,
                                    None, stream) == L.TEM_EINVAL
    wide = torch.zeros(2 * Z + 1, dtype=torch.int32, device="cuda")                         # the device tables off alignment
    for k in (1, 3):
        t = list(tables)
        t[k] = wide.data_ptr() + 2
        assert lib.tem_u8_zdev_mask(src.ptr, 4, 12, X, 2, Z, Y, 8, 1, 3, 2, 10, 0, X, 16, 16, 2, 1, r, *t, None, dst.ptr,
                                    count.data_ptr(), stream) == L.TEM_EINVAL
    # more workgroups than one launch holds, with dimensions that are only claimed; refused before anything is touched:
    # 2^17 x 2^15 tiles of 8 x 32 outputs are past 2^31 - 1; 2^15 x 2^15 tiles in runs of 64 are 2^24 workgroups; so are
    # 2^14 x 2^15 tiles in runs of 64 on 2 planes
    none, big = np.full((2, 2), -1, np.int32), np.full((512, 512), 9000, np.int32)
    dnone, dbig = torch.from_numpy(none).cuda(), torch.from_numpy(big).cuda()
    many = lambda D, H: lib.tem_u8_zdev_mask(src.ptr, D, H, 1 << 20, 0, D, H, 0, 0, D, 0, H, 0, 1 << 20, 2048, 2048,
                                             H // 2048, 512, r, none.ctypes.data, dnone.data_ptr(), big.ctypes.data,
                                             dbig.data_ptr(), None, dst.ptr, count.data_ptr(), stream)
    assert [many(1, 1 << 20), many(1, 1 << 18), many(2, 1 << 17)] == [L.TEM_EUNSUPPORTED] * 3
    torch.cuda.synchronize()
    assert (dst.body() == DFILL).all() and int(count.cpu()[0]) == 0
    # at the section's first and last rows the window is cut, and the block need not hold what the section has not
    top, bot = _Dev(4 * 5 * X, 0, FILL, vol[2:6, :5]), _Dev(4 * 5 * X, 0, FILL, vol[2:6, 25:])
    small = _Dev(2 * 3 * X, 0, DFILL)
    assert call(src=top, dims=(4, 5, X), y_org=0, dst=small, count=None, **core(rows=(0, 3))) == 0
    assert call(src=bot, dims=(4, 5, X), y_org=25, dst=small, count=None, **core(rows=(2, 5))) == 0
    want = ZD.mask(vol, nbr, np.full((2, 1), 9000), (16, 16), r)
    assert np.array_equal(small.body().reshape(2, 3, X), want[3:5, 27:30])
    # rows of the table outside the core are not looked at; an empty core launches nothing; the good call
    assert call(nbr=tab(0, 99, -99)) == 0 and call(nbr=tab(3, 9, 9), **core(c=(2, 2))) == 0
    assert call(**core(cols=(4, 4))) == 0 and call(**core(rows=(5, 5))) == 0 and call() == 0
    assert np.array_equal(dst.body().reshape(2, 8, X), want[3:5, 10:18]) and int(count.cpu()[0]) == 2 * int(want[3:5, 10:18].sum())
    # device tables that disagree with the host's: another result, never a fault
    wild, wthr = nbr.copy(), np.array([[-5], [1 << 30]], np.int32)
    wild[3], wild[4] = (-7, 1 << 30), (1 << 30, 0)
    dst2 = _Dev(2 * 8 * X, 0, DFILL)
    assert _mask_call(src, (4, 12, X), 2, Z, Y, 8, ((1, 3), (2, 10), (0, X)), (16, 16), (2, 1), r, nbr, thr, dst2, None,
                      None, dev_nbr=wild, dev_thr=wthr) == 0
    assert dst2.body().shape == (2 * 8 * X,)
    assert np.array_equal(src.body(), block.reshape(-1))


# ------------------------------------------------------------------------------------------------------- the passes
Z, Y, X = ZD.FIX_SHAPE
TILE, SKIP, R = ZD.FIX_TILE, ZD.FIX_SKIP, ZD.FIX_WINDOW // 2


@pytest.fixture(scope="module")
def vmap(tmp_path_factory):
    path = tmp_path_factory.mktemp("zdev") / "vol.u8"
    m = np.memmap(path, np.uint8, "w+", shape=ZD.FIX_SHAPE)
    m[...] = ZD.fixture().volume
    m.flush()
    return np.memmap(path, np.uint8, "r", shape=ZD.FIX_SHAPE)


@functools.lru_cache(maxsize=None)
def _want_sums():
    s = ZD.volume_sums(ZD.fixture().volume, ZD.neighbours(Z, SKIP), (TILE, TILE))
    s.setflags(write=False)
    return s


BUDGETS = {"whole": 1 << 30, "sections": 7 * Y * X, "rows": 3 * 20 * X}


@pytest.mark.parametrize("budget", list(BUDGETS), ids=list(BUDGETS))
def test_passes_equal_the_reference_however_they_are_cut(vmap, budget, monkeypatch):
    from transfer_em_amd import utils as U
    vd, b = ZD.check_fixture(), BUDGETS[budget]
    nbr = ZD.neighbours(Z, SKIP)
    whole = ((0, Z), (0, Y), (0, X))
    st = {}
    s, counts = _counted(lambda: U.section_outlier_sums(vmap, TILE, SKIP, chunk_bytes=b, stats=st))
    assert s.dtype == np.int64 and np.array_equal(s, _want_sums())
    chunks = U.outlier_chunks(whole, ZD.FIX_SHAPE, nbr, 0, b)
    assert st["chunks"] == len(chunks) == counts["tem_u8_zdev_tiles"] and st["read_s"] >= 0
    if budget == "sections":                                              # an accumulator of one slab's sections
        monkeypatch.setattr(U, "CLAHE_ACC_BYTES", 64)
        assert np.array_equal(U.section_outlier_sums(vmap, TILE, SKIP, chunk_bytes=b), _want_sums())
    st = {}
    m, counts = _counted(lambda: U.volume_outliers(vmap, vd.thr, TILE, ZD.FIX_WINDOW, SKIP, chunk_bytes=b, stats=st))
    assert m.dtype == np.uint8 and np.array_equal(m, vd.mask)
    chunks = U.outlier_chunks(whole, ZD.FIX_SHAPE, nbr, R, b)
    assert st["chunks"] == len(chunks) == counts["tem_u8_zdev_mask"] and st["read_s"] >= 0 and st["write_s"] >= 0
    assert st["flagged"] == vd.flagged == int(m.sum())
    assert {"whole": len(chunks) == 1, "sections": 1 < len(chunks) <= Z and all(c[1] == (0, Y) for c, _ in chunks),
            "rows": len(chunks) > Z and all(c[1] != (0, Y) for c, _ in chunks)}[budget]
    assert np.array_equal(np.asarray(vmap), ZD.fixture().volume)          # the input: read only


def test_ranks_an_roi_marked_tiles_and_one_image(vmap, tmp_path):
    from transfer_em_amd import utils as U
    vd = ZD.check_fixture()
    parts = [U.section_outlier_sums(vmap, TILE, SKIP, chunk_bytes=5 * Y * X, rank=r, world_size=2) for r in (0, 1)]
    assert parts[0].any() and parts[1].any() and np.array_equal(parts[0] + parts[1], _want_sums())
    out = np.memmap(tmp_path / "mask.u8", np.uint8, "w+", shape=ZD.FIX_SHAPE)              # two ranks write one output
    out[...] = 7
    flagged = 0
    for r in (1, 0):
        st = {}
        assert U.volume_outliers(vmap, vd.thr, TILE, ZD.FIX_WINDOW, SKIP, out=out, chunk_bytes=5 * Y * X, rank=r,
                                 world_size=2, stats=st) is out
        assert np.array_equal(np.asarray(out), vd.mask) == (r == 0)
        flagged += st["flagged"]
    assert flagged == vd.flagged
    th = U.OutlierThresholds(vd.thr, np.zeros(vd.thr.shape))
    roi = U.volume_outliers(vmap, th, TILE, ZD.FIX_WINDOW, SKIP, start=(88, 35, 3), size=(60, 41, 25), chunk_bytes=4 * 49 * X)
    assert np.array_equal(roi, vd.mask[3:28, 35:76, 88:148]) and roi.any()
    marks = np.zeros((Z, 2, 3), bool)
    marks[5, 1, 2] = marks[12, 0, 0] = True
    got = U.volume_outliers(vmap, vd.thr, TILE, ZD.FIX_WINDOW, SKIP, tiles=marks, chunk_bytes=6 * Y * X)
    assert np.array_equal(got, ZD.mask(ZD.fixture().volume, ZD.neighbours(Z, SKIP), vd.thr, (TILE, TILE), R, marks))
    assert got[5, 64:, 128:].all() and got[12, :64, :64].all() and got.sum() == vd.flagged + 64 * 64 * 2
    image = np.asarray(vmap[4])
    st = {}
    assert not U.section_outlier_sums(image, TILE).any()
    one = U.volume_outliers(image, vd.thr, TILE, stats=st)
    assert one.shape == (Y, X) and not one.any() and st["flagged"] == 0


def test_the_fixture_end_to_end(vmap):
    """Tile 64 and the defaults: find_defects sees the black section and nothing else; find_debris' mask equals the
    reference's, meets the fixture's conditions, and its Repair goes through volume_repair unchanged."""
    from transfer_em_amd import utils as U
    fx, vd = ZD.fixture(), ZD.check_fixture()
    d = U.find_defects(U.section_sums(vmap, TILE))
    assert d.sections == SKIP and not d.tiles.any()
    rep = U.find_debris(vmap, tile=TILE, skip=SKIP)
    assert isinstance(rep, U.Repair) and rep.sections == SKIP and rep.missing_value is None and rep.max_gap == 8
    mask = np.asarray(rep.mask)
    assert np.array_equal(mask, vd.mask)
    assert np.array_equal(np.asarray(U.find_debris(vmap, tile=TILE, defects=d, chunk_bytes=5 * Y * X).mask), vd.mask)
    far = mask.astype(bool) & ~(ZD.window_sums(fx.planted.astype(np.uint8), R)[0] > 0)
    recall = [float(mask[fx.labels == k + 1].mean()) for k in range(len(ZD.FIX_BLOBS))]
    st = {}
    fixed = U.volume_repair(vmap, rep, stats=st)
    assert np.array_equal(fixed, RR.repair(fx.volume, sections=SKIP, mask=vd.mask, max_gap=8))
    clean = fx.clean.astype(np.int64)
    before = np.abs(fx.volume.astype(np.int64) - clean)[fx.planted].mean()
    after = np.abs(fixed.astype(np.int64) - clean)[fx.planted].mean()
    print(f"flagged {int(mask.sum())}, planted hit {int(mask[fx.planted].sum())} of {int(fx.planted.sum())}, least recall "
          f"{min(recall):.3f}, far {int(far.sum())}, thick {int(mask[fx.thick].sum())} of {int(fx.thick.sum())}, "
          f"error {before:.2f} -> {after:.2f}")
    assert far.sum() == 0 and min(recall) >= 0.9 and after < before / 10
    assert mask[fx.thick].sum() == 0                                      # the limit: two sections thick is not seen
    assert st["repaired"] == int(mask.sum()) + Y * X - int(mask[SKIP].sum()) and st["unrepaired"] == 0
