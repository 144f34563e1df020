"""The centred section-shift measurement on the device: tem_u8_zshift_tiles_at against its sibling at zero centres and
against the numpy reference (zshift_at_ref) with per-tile centres, section_shift_sums_at out of core, and
section_shifts_coarse_to_fine on the fixture of sections with large planted jumps.  Everything is integers, so every
comparison is exact.  Blocks lie between guards of fill bytes and sums between guards of fill words, as in
test_gpu_zshift.py, whose helpers these tests share."""
import functools

import numpy as np
import pytest
import torch

import zshift_at_ref as AR
import zshift_ref as SR
from test_gpu_histogram import _counted, _env
from test_gpu_zcorr import FILL, GUARD, SFILL, _data
from test_gpu_zshift import LONG_R, LONG_SHAPE, LONG_TILE, _geometry, _launch, _Sums

pytestmark = pytest.mark.gpu

BLOCKS = [(3, 33, 70), (2, 64, 257)]
TILES = [(32, 32), (7, 64), (3, 5)]
RADII = [1, 4, 8]


def _table(centers):
    """The int32 device table of integer centres [planes, gy, gx, 2]."""
    return torch.from_numpy(np.ascontiguousarray(centers, dtype=np.int32)).cuda()


def _bounds(centers):
    c = np.asarray(centers)
    return min(int(c[..., 0].min()), 0), max(int(c[..., 0].max()), 0), int(np.abs(c[..., 1]).max())


def _launch_at(block, c0, c1, geo, tile, r, table, bounds, sums_ptr, off=0, plane=0):
    """One tem_u8_zshift_tiles_at call on `block`, `off` bytes into an aligned allocation between guards of FILL, with
    the table's rows from `plane` on; block, guards and table must be untouched."""
    L, lib, stream = _env()
    r0, r1, y_org, Y, gy, gx = geo
    flat = np.ascontiguousarray(block).reshape(-1)
    t = torch.full((flat.size + off + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0 and table.dtype == torch.int32 and table.shape[1:] == (gy, gx, 2)
    t[GUARD + off:GUARD + off + flat.size] = torch.from_numpy(flat.copy()).cuda()
    before = table.clone()
    L.check(lib.tem_u8_zshift_tiles_at(t.data_ptr() + GUARD + off, *block.shape, c0, c1, r0, r1, y_org, Y, *tile, gy, gx,
                                       r, table.data_ptr() + 8 * gy * gx * plane, *bounds, sums_ptr, stream),
            "tem_u8_zshift_tiles_at")
    got = t.cpu().numpy()
    assert (got[:GUARD + off] == FILL).all() and (got[GUARD + off + flat.size:] == FILL).all()
    assert np.array_equal(got[GUARD + off:GUARD + off + flat.size], flat) and torch.equal(table, before)


def _run_at(block, c0, c1, geo, tile, r, centers, bounds=None, off=0):
    s = _Sums(max(c1 - c0, 1), geo[4], geo[5], r)
    _launch_at(block, c0, c1, geo, tile, r, _table(centers), _bounds(centers) if bounds is None else bounds, s.ptr(), off)
    return s.result()[:c1 - c0]


def _run(block, c0, c1, geo, tile, r, off=0):
    s = _Sums(max(c1 - c0, 1), geo[4], geo[5], r)
    _launch(block, c0, c1, geo, tile, r, s.ptr(), off)
    return s.result()[:c1 - c0]


def _reach_geometry(shape, tile, r, lo, hi):
    """(r0, r1, y_org, Y, gy, gx) of a block off the tile grid inside a taller section that holds EXACTLY the rows its
    core needs at a reach of [lo, hi]: [r0 - r + lo, r1 + r + hi) = [0, H), and not one more."""
    (D, H, W), (th, tw) = shape, tile
    y_org = th + th // 3 + 1024 if th > 1 else 1025              # the section goes on for more than any centre below
    Y = y_org + H + 1024 + th // 2 + 1                           # and above the block
    r0, r1 = r - lo, H - r - hi
    assert r0 < r1
    return r0, r1, y_org, Y, -(-Y // th) + 1, -(-W // tw) + 1


def _centers(seed, planes, gy, gx, ylim, xlim):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(ylim[0], ylim[1] + 1, (planes, gy, gx)),
                     rng.integers(xlim[0], xlim[1] + 1, (planes, gy, gx))], axis=-1).astype(np.int64)


# ------------------------------------------------------------------------------- zero centres: the sibling, byte for byte
@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("tile", TILES, ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("shape", BLOCKS, ids=lambda s: "x".join(map(str, s)))
def test_zero_centres_equal_the_sibling_byte_for_byte(shape, tile, r):
    block, D = _data(shape, "random"), shape[0]
    for mode, (c0, c1), off in (("whole", (0, D), 0), ("whole", (0, D - 1), 3), ("inside", (0, D), 1), ("bottom", (0, D), 2)):
        geo = _geometry(shape, tile, r, mode)
        assert mode == "whole" or (geo[2] > 0 and geo[2] % tile[0])  # the block off the tile grid: its rows cut through tiles
        want = _run(block, c0, c1, geo, tile, r, off)
        zero = np.zeros((D, geo[4], geo[5], 2), np.int64)
        got = _run_at(block, c0, c1, geo, tile, r, zero, (0, 0, 0), off)
        assert want.any() and got.tobytes() == want.tobytes(), (mode, np.argwhere(got != want)[:5])
    geo = _geometry(shape, tile, r, "whole")                     # wide promises on a zero table change nothing
    got = _run_at(block, 0, D, geo, tile, r, np.zeros((D, geo[4], geo[5], 2), np.int64), (-1024, 1024, 1024))
    assert got.tobytes() == _run(block, 0, D, geo, tile, r).tobytes()


# ---------------------------------------------------------------------------- per-tile centres: the numpy reference
# every tile and radius of the comparison above, but the 3 x 5 tiles at the radii where the plain-slicing reference would
# take many seconds (some 10^5 slices)
REF_CASES = [(shape, tile, r) for shape in BLOCKS for tile in TILES for r in RADII
             if tile != (3, 5) or r == 1 or (shape, r) == ((3, 33, 70), 4)]


@pytest.mark.parametrize("shape,tile,r", REF_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_kernel_equals_the_reference_with_per_tile_centres(shape, tile, r):
    block, (D, H, W), (th, tw) = _data(shape, "random"), shape, tile
    # the block is the section: centres in [-20, 20] x [-40, 40], a window that leaves the section entirely, and one
    # whose dx_total takes nearly all, or all, of its part's columns away
    geo = r0, r1, y_org, Y, gy, gx = _geometry(shape, tile, r, "whole")
    C = _centers(41, D, gy, gx, (-20, 20), (-40, 40))
    C[0, 0, 0] = (H + r, 3)                                      # wholly below the section
    w0 = min(tw, W)                                              # tile (1, 0) is one part, w0 <= 128 columns wide: at
    C[0, 1, 0] = (-2, -(w0 + r - 2))                             # dx_total = -(w0 + r - 2) + dx only its columns
    assert w0 <= 128                                             # x >= w0 - 2 + r - dx have a partner: two at dx = r, one
    want = AR.tile_sums_at(block, C, 0, D, *geo[:4], th, tw, gy, gx, r)      # at r - 1, else none -- the whole width is missing
    assert not want[0, 0, 0].any() and want[0, 1, 0, :, 2 * r - 1:].any() and not want[0, 1, 0, :, :2 * r - 1].any()
    assert not want[-1].any() and want[0].any()
    for c0, c1, off in ((0, D, 0), (0, D - 1, 3)):
        got = _run_at(block, c0, c1, geo, tile, r, C, off=off)
        assert np.array_equal(got, want[c0:c1]), (c0, c1, np.argwhere(got != want[c0:c1])[:5])
    # the block off the grid inside a taller section, holding exactly the rows of its reach and not one more
    lo, hi = (-5, 6) if H < 64 else (-20, 20)
    geo = r0, r1, y_org, Y, gy, gx = _reach_geometry(shape, tile, r, lo, hi)
    C = _centers(43, D, gy, gx, (lo, hi), (-40, 40))
    i0, i1 = (y_org + r0) // th, (y_org + r1 - 1) // th
    C[0, i0, 0], C[0, i1, -2] = (lo, -40), (hi, 40)              # both ends of the reach are used
    assert r0 - r + lo == 0 and r1 + r + hi == H and _bounds(C)[:2] == (lo, hi)
    want = AR.tile_sums_at(block, C, 0, D, *geo[:4], th, tw, gy, gx, r)   # asserts that the block holds the partner rows
    got = _run_at(block, 0, D, geo, tile, r, C, off=1)
    assert want[0].any() and np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_the_largest_centres_on_a_tiny_block():
    """(2, 5, 7) with centres of +-1024: windows a thousand pixels outside add nothing, the others are the reference's."""
    shape, tile, r = (2, 5, 7), (3, 5), 2
    block = _data(shape, "random")
    geo = _geometry(shape, tile, r, "whole")
    C = np.zeros((2, geo[4], geo[5], 2), np.int64)
    C[0, 0, 0], C[0, 0, 1], C[0, 1, 0], C[0, 1, 1] = (1024, -1024), (-1, 2), (-1024, 3), (2, 1024)
    want = AR.tile_sums_at(block, C, 0, 2, *geo[:4], *tile, *geo[4:], r)
    assert want[0, 0, 1].any() and not want[0, 0, 0].any() and not want[0, 1].any()
    for off in (0, 3):
        assert np.array_equal(_run_at(block, 0, 2, geo, tile, r, C, (-1024, 1024, 1024), off), want)


def test_a_centred_search_is_a_window_of_the_wider_search():
    """Centre (3, -2) at radius 4 is the sub-block [3 - 4 + 8 : 3 + 4 + 9, -2 - 4 + 8 : -2 + 4 + 9] of the sibling's
    radius-8 table: an exact identity, device against device."""
    for shape, tile in (((3, 33, 70), (32, 32)), ((2, 64, 257), (7, 64))):
        block, D = _data(shape, "random"), shape[0]
        for mode in ("whole", "inside"):
            geo = _geometry(shape, tile, 8, mode)                # the halo of radius 8 holds that of centre + radius 4
            wide = _run(block, 0, D, geo, tile, 8)
            C = np.zeros((D, geo[4], geo[5], 2), np.int64)
            C[...] = (3, -2)
            got = _run_at(block, 0, D, geo, tile, 4, C)
            assert got.any() and np.array_equal(got, wide[:, :, :, 3 - 4 + 8:3 + 4 + 9, -2 - 4 + 8:-2 + 4 + 9])


def test_kernel_fills_whole_workgroups_with_centres():
    """The sibling's shape of a real call at the largest radius -- tiles of 100 x 144 in parts of 32 x 128, 32 x 16 and
    4 x 128, an odd plane stride, W no multiple of 4 -- with non-zero centres per tile."""
    D, H, W = LONG_SHAPE
    assert (H * W) % 2 == 1 and W % 4 == 1
    block = _data(LONG_SHAPE, "random")
    geo = _geometry(LONG_SHAPE, LONG_TILE, LONG_R, "whole")
    C = _centers(47, D, geo[4], geo[5], (-20, 20), (-40, 40))
    want = AR.tile_sums_at(block, C[1:], 1, D, *geo[:4], *LONG_TILE, *geo[4:], LONG_R)
    s = _Sums(D - 1, geo[4], geo[5], LONG_R)
    _launch_at(block, 1, D, geo, LONG_TILE, LONG_R, _table(C), _bounds(C), s.ptr(), 0, plane=1)
    assert want[:-1].all(axis=(3, 4, 5))[:, :2, :3].all() and np.array_equal(s.result(), want)
    geo = _reach_geometry(LONG_SHAPE, LONG_TILE, LONG_R, -11, 9)
    C = _centers(53, D, geo[4], geo[5], (-11, 9), (-40, 40))
    C[0, (geo[2] + geo[0]) // 100, 0], C[1, (geo[2] + geo[0]) // 100, 1] = (-11, 7), (9, -7)
    want = AR.tile_sums_at(block, C, 0, D - 1, *geo[:4], *LONG_TILE, *geo[4:], LONG_R)
    assert np.array_equal(_run_at(block, 0, D - 1, geo, LONG_TILE, LONG_R, C, off=1), want)


def test_kernel_accumulates_across_cuts():
    """One launch equals two launches on core rows cut through a tile, two launches on blocks cut along y that hold
    just the rows of their reach, and two launches cut along z, where the table's pointer moves with c0."""
    shape, tile, r = (4, 33, 70), (32, 32), 4
    block = _data(shape, "random")
    r0, r1, y_org, Y, gy, gx = geo = _geometry(shape, tile, r, "whole")
    C = _centers(59, 4, gy, gx, (-3, 2), (-40, 40))
    C[0, 0, 0], C[1, 1, 1] = (-3, 5), (2, -5)
    table, bounds = _table(C), _bounds(C)
    assert bounds[:2] == (-3, 2)
    want = AR.tile_sums_at(block, C, 0, 4, *geo[:4], *tile, gy, gx, r)
    for off in (0, 1):
        s = _Sums(4, gy, gx, r)
        _launch_at(block, 0, 4, geo, tile, r, table, bounds, s.ptr(), off)
        assert np.array_equal(s.result(), want)
        s = _Sums(4, gy, gx, r)                                                     # core rows [0, 17) | [17, 33)
        _launch_at(block, 0, 4, (0, 17) + geo[2:], tile, r, table, bounds, s.ptr(), off)
        _launch_at(block, 0, 4, (17, 33) + geo[2:], tile, r, table, bounds, s.ptr(), off)
        assert np.array_equal(s.result(), want)
        s = _Sums(4, gy, gx, r)                                                     # blocks of rows [0, 23) | [10, 33):
        _launch_at(block[:, :23], 0, 4, (0, 17, 0, Y, gy, gx), tile, r, table, bounds, s.ptr(), off)   # 17 + 4 + 2
        _launch_at(block[:, 10:], 0, 4, (7, 23, 10, Y, gy, gx), tile, r, table, bounds, s.ptr(), off)  # 17 - 4 - 3
        assert np.array_equal(s.result(), want)
        s = _Sums(4, gy, gx, r)                                                     # planes [0, 2) + halo | [2, 4)
        _launch_at(block[:3], 0, 2, geo, tile, r, table, bounds, s.ptr(0), off, plane=0)
        _launch_at(block[2:], 0, 2, geo, tile, r, table, bounds, s.ptr(2), off, plane=2)
        assert np.array_equal(s.result(), want)
    assert not np.array_equal(C[0], C[2])                                           # the moved pointer matters


def test_kernel_clamps_a_table_that_breaks_the_promise():
    """Centres just outside the promised bounds, in a block with spare rows so that a read would stay inside the
    allocation either way: the sums are those of the clamped table."""
    shape, tile, r = (3, 33, 70), (7, 64), 2
    block = _data(shape, "random")
    lo, hi, xm = -3, 2, 6
    r0, r1, y_org, Y, gy, gx = _reach_geometry(shape, tile, r, lo - 4, hi + 4)      # 4 spare rows on each side
    geo = (r0, r1, y_org, Y, gy, gx)
    C = _centers(61, 3, gy, gx, (lo, hi), (-xm, xm))
    i0 = (y_org + r0) // 7
    C[0, i0, 0], C[0, i0, 1], C[1, i0 + 1, 0], C[1, i0 + 1, 1] = (lo - 1, 0), (hi + 1, xm + 1), (lo - 4, -xm - 1), (hi + 4, -xm - 9)
    clamped = np.stack([np.clip(C[..., 0], lo, hi), np.clip(C[..., 1], -xm, xm)], axis=-1)
    assert (clamped != C).sum() == 7
    want = AR.tile_sums_at(block, clamped, 0, 3, *geo[:4], *tile, gy, gx, r)
    honest = AR.tile_sums_at(block, C, 0, 3, *geo[:4], *tile, gy, gx, r)
    assert not np.array_equal(want, honest)
    got = _run_at(block, 0, 3, geo, tile, r, C, (lo, hi, xm))
    assert np.array_equal(got, want)


def test_kernel_holds_the_largest_tile_of_the_largest_values():
    """Two planes of 2048 x 2048 voxels of 255 in one tile at r = 1, centred on (5, -7), against the closed form."""
    block = np.full((2, 2048, 2048), 255, np.uint8)
    C = np.zeros((2, 1, 1, 2), np.int64)
    C[0, 0, 0] = (5, -7)
    got = _run_at(block, 0, 2, (0, 2048, 0, 2048, 1, 1), (2048, 2048), 1, C)
    assert not got[1].any()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            n = (2048 - abs(5 + dy)) * (2048 - abs(-7 + dx))
            assert n * 65025 > 2 ** 32
            assert got[0, 0, 0, dy + 1, dx + 1].tolist() == [255 * n, 65025 * n, 255 * n, 65025 * n, 65025 * n]


def test_kernel_refuses_bad_arguments():
    """TEM_EINVAL from the host-side checks, nothing launched: sums keeps its fill."""
    L, lib, stream = _env()
    src = torch.ones(4 * 6 * 8 + 16, dtype=torch.uint8, device="cuda")
    sums = torch.full((4 * 2 * 2 * 125 + 1,), SFILL, dtype=torch.int64, device="cuda")
    ctr = torch.zeros(4 * 3 * 2 * 2 + 1, dtype=torch.int32, device="cuda")
    p, s, c = src.data_ptr(), sums.data_ptr(), ctr.data_ptr()
    call = lambda *a: lib.tem_u8_zshift_tiles_at(*a, stream)
    # 0 src, 1 D, 2 H, 3 W, 4 c0, 5 c1, 6 r0, 7 r1, 8 y_org, 9 Y, 10 th, 11 tw, 12 gy, 13 gx, 14 radius, 15 centers,
    # 16 cy_lo, 17 cy_hi, 18 cx_max, 19 sums
    ok = [p, 4, 6, 8, 0, 4, 0, 6, 0, 6, 4, 4, 2, 2, 2, c, -1, 1, 3, s]
    for i, v in [(0, None), (19, None), (19, s + 4), (19, s + 1), (1, 0), (2, 0), (3, 0), (1, -1), (9, 0), (12, 0),
                 (13, 0), (12, -1), (10, 0), (10, 2049), (11, 0), (11, 2049), (14, 0), (14, 9), (14, -1), (8, -1),
                 (12, 1), (13, 1), (9, 5), (8, 1), (4, -1), (5, 5), (4, 3), (6, -1), (7, 7), (6, 4),
                 (15, None), (15, c + 1), (15, c + 2), (16, 1), (16, -1025), (17, -1), (17, 1025), (18, -1), (18, 1025)]:
        a = list(ok)
        a[i] = v
        if (i, v) == (4, 3):
            a[5] = 2                                                                # c0 > c1
        if (i, v) == (6, 4):
            a[7] = 3                                                                # r0 > r1
        assert call(*a) == L.TEM_EINVAL, (i, v)
    # rows 2...7 of 12, core rows [3, 4): radius 2 and a reach of [-1, 1] need rows [0, 7) of the block's 6 -- and so on
    inside = [p, 4, 6, 8, 0, 4, 3, 3, 2, 12, 4, 4, 3, 2, 2, c, 0, 0, 0, s]
    for r0, r1, lo, hi in ((3, 4, -1, 1), (3, 4, -2, 0), (2, 4, -1, 0), (3, 5, 0, 0), (2, 4, 0, 1), (1, 4, 0, 0)):
        assert call(*inside[:6], r0, r1, *inside[8:16], lo, hi, 0, s) == L.TEM_EINVAL, (r0, r1, lo, hi)
    assert call(*ok[:4], 2, 2, *ok[6:]) == 0 and call(*ok[:6], 3, 3, *ok[8:]) == 0  # an empty core launches nothing
    assert call(*ok[:4], 3, 4, *ok[6:]) == 0                                        # as does the last plane alone
    assert call(p, 2 ** 31 - 1, 4, 4, 0, 2 ** 31 - 1, 0, 4, 0, 4, 1, 1, 4, 4, 1, c, 0, 0, 0, s) == L.TEM_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (sums.cpu().numpy() == SFILL).all()
    sums.zero_()
    assert call(*ok) == 0 and call(p + 3, *ok[1:]) == 0                             # and the good call runs
    torch.cuda.synchronize()
    got = sums.cpu().numpy()[:2000].reshape(4, 2, 2, 5, 5, 5)
    assert got[:3, ..., 2, 2, 0].sum() == 2 * 3 * 6 * 8 and not got[3].any()       # three planes have one above them
    sums2 = torch.zeros(4 * 3 * 2 * 125, dtype=torch.int64, device="cuda")
    assert call(*inside[:6], 3, 4, *inside[8:16], -1, 0, 0, sums2.data_ptr()) == 0  # the one with just its reach: [0, 6)
    assert call(*inside[:6], 2, 3, *inside[8:16], 0, 1, 0, sums2.data_ptr()) == 0
    torch.cuda.synchronize()
    assert sums2.cpu().numpy().reshape(4, 3, 2, 5, 5, 5)[:3, ..., 2, 2, 0].sum() == 3 * 2 * 8


# -------------------------------------------------------------------------------------------- section_shift_sums_at
VSHAPE, VTILE, VR = (8, 70, 96), (32, 32), 4
BUDGETS = {"one_slab": 9 * 70 * 96, "three_sections": 3 * 70 * 96, "row_cuts": 2 * 30 * 96}


@functools.lru_cache(maxsize=None)
def _vcase():
    vol = np.random.default_rng(19).integers(0, 256, VSHAPE, dtype=np.uint8)
    vol[1::2] = vol[1::2] // 2 + vol[:-1:2] // 2                                   # neighbours correlate
    C = _centers(67, 7, 3, 3, (-9, 6), (-40, 40))
    C[3, 1, 1], C[4, 0, 2] = (-9, 1), (6, -1)
    want = AR.volume_sums_at(vol, C, VTILE, VR)
    for a in (vol, C, want):
        a.setflags(write=False)
    return vol, C, want


@pytest.fixture(scope="module")
def vmap(tmp_path_factory):
    path = tmp_path_factory.mktemp("zshift_at") / "vol.u8"
    m = np.memmap(path, np.uint8, "w+", shape=VSHAPE)
    m[...] = _vcase()[0]
    m.flush()
    return np.memmap(path, np.uint8, "r", shape=VSHAPE)


@pytest.mark.parametrize("budget", list(BUDGETS), ids=list(BUDGETS))
def test_section_shift_sums_at_equals_the_reference_however_it_is_cut(vmap, budget):
    from transfer_em_amd.utils import section_shift_sums_at, zshift_chunks_at
    vol, C, want = _vcase()
    st = {}
    got, counts = _counted(lambda: section_shift_sums_at(vmap, C, VTILE, VR, chunk_bytes=BUDGETS[budget], stats=st))
    assert got.dtype == np.int64 and got.shape == (8, 3, 3, 9, 9, 5) and np.array_equal(got, want)
    assert not got[-1].any() and got[:-1].any(axis=(1, 2, 3, 4, 5)).all()
    chunks = zshift_chunks_at(VSHAPE, VR, (-9, 6), BUDGETS[budget])
    n = len(chunks)
    assert st["chunks"] == n and st["read_s"] >= 0
    assert counts["tem_u8_zshift_tiles_at"] == n and counts["tem_u8_zshift_tiles"] == 0    # one launch per slab
    assert {"one_slab": n == 1, "three_sections": n == 4, "row_cuts": n == 8 * 10}[budget]       # 30 rows: 7 + 8 + 15
    assert budget != "row_cuts" or chunks[1] == (((0, 1), (7, 14), (0, 96)), ((0, 2), (0, 24), (0, 96)))
    assert np.array_equal(np.asarray(vmap), vol)                                    # the input: read only


def test_section_shift_sums_at_ranks_the_per_slab_read_back_and_zero_centres(vmap, monkeypatch):
    from transfer_em_amd import utils
    vol, C, want = _vcase()
    assert np.array_equal(utils.section_shift_sums_at(vol, C, VTILE, VR), want)     # an ndarray, one slab
    parts = [utils.section_shift_sums_at(vmap, C, VTILE, VR, chunk_bytes=BUDGETS["three_sections"], rank=r, world_size=2)
             for r in (1, 0)]
    assert parts[0].any() and parts[1].any() and not np.array_equal(parts[0], want)
    assert np.array_equal(parts[0] + parts[1], want)                                # the ranks' results add
    zero = np.zeros((7, 2), np.int64)
    plain = utils.section_shift_sums(vmap, VTILE, VR, chunk_bytes=BUDGETS["three_sections"])
    assert np.array_equal(plain, SR.volume_sums(vol, VTILE, VR))
    for budget in BUDGETS.values():
        assert utils.section_shift_sums_at(vmap, zero, VTILE, VR, chunk_bytes=budget).tobytes() == plain.tobytes()
    monkeypatch.setattr(utils, "CLAHE_ACC_BYTES", 8 * 3 * 3 * 81 * 40 - 1)          # the accumulator no longer fits
    for budget in ("three_sections", "row_cuts"):
        got, counts = _counted(lambda: utils.section_shift_sums_at(vmap, C, VTILE, VR, chunk_bytes=BUDGETS[budget]))
        assert np.array_equal(got, want)
        assert counts["tem_u8_zshift_tiles_at"] == len(utils.zshift_chunks_at(VSHAPE, VR, (-9, 6), BUDGETS[budget]))
    both = [utils.section_shift_sums_at(vmap, C, VTILE, VR, chunk_bytes=BUDGETS["row_cuts"], rank=r, world_size=2)
            for r in (0, 1)]
    assert np.array_equal(both[0] + both[1], want)
    one = utils.section_shift_sums_at(vol[3], np.zeros((0, 2), np.int64), 32)       # one image: no pairs, no sums
    assert one.shape == (1, 3, 3, 9, 9, 5) and not one.any()


# ------------------------------------------------------------------------------------------------------- end to end
def test_the_large_jumps_are_measured_and_undone():
    from transfer_em_amd.utils import (section_shift_sums, section_shifts, section_shifts_coarse_to_fine, shift_counts,
                                       shift_positions, volume_shift)
    v = AR.big_jump_volume()
    st = {}
    got = section_shifts_coarse_to_fine(v, AR.BIG_TILE, AR.BIG_RADIUS, AR.BIG_LEVELS, chunk_bytes=4 * 160 * 192, stats=st)
    want = AR.host_driver()
    for a, b in zip(got.shifts[:4], want.shifts[:4]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert got.shifts.unresolved == want.shifts.unresolved == [8]
    assert np.array_equal(got.q, want.q) and np.array_equal(got.n, want.n) and np.array_equal(got.centers, want.centers)
    assert st["chunks"] >= 3 + 3 + 4 and st["read_s"] >= 0                          # three rescales, four searches
    assert np.array_equal(got.shifts.pairs[:8], AR.big_pairs()[:8])
    P = shift_positions(got.shifts.pairs)
    moved = volume_shift(v, P)
    whole = volume_shift(np.ones_like(v), P).astype(bool)                           # where no fill entered
    q = section_shift_sums(moved, AR.BIG_TILE, AR.BIG_RADIUS)
    s = section_shifts(q, shift_counts(v.shape, AR.BIG_TILE, AR.BIG_RADIUS))
    t, r, seen = AR.BIG_TILE, AR.BIG_RADIUS, 0
    for z in range(8):
        for i in range(5):
            for j in range(6):
                box = (slice(max(i * t - r, 0), (i + 1) * t + r), slice(max(j * t - r, 0), (j + 1) * t + r))
                if whole[z][box].all() and whole[z + 1][box].all():                 # an interior tile: no fill near it
                    seen += 1
                    assert s.decided[z, i, j] and tuple(s.tiles[z, i, j]) == (0, 0), (z, i, j)
        assert tuple(s.pairs[z]) == (0, 0)
    assert seen >= 8 * 6
