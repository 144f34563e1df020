"""The shift measurement over a list of section pairs on the device: tem_u8_zshift_tiles_pairs against its sibling
tem_u8_zshift_tiles_at for the pairs (d, d + 1) and against the numpy reference (zshift_pairs_ref) for lags 1...8,
section_shift_sums_pairs out of core, and section_shifts_bridged -> chain_pairs -> shift_positions -> volume_shift ->
volume_repair on the fixture with bad sections.  Everything is integers, so every comparison is exact.  Blocks lie
between guards of fill bytes and sums between guards of fill words, as in test_gpu_zshift_at.py, whose helpers these
tests share."""
import functools

import numpy as np
import pytest
import torch

import zshift_at_ref as AR
import zshift_pairs_ref as PR
from test_gpu_histogram import _counted, _env
from test_gpu_zcorr import FILL, GUARD, SFILL, _data
from test_gpu_zshift import _geometry, _Sums
from test_gpu_zshift_at import _bounds, _centers, _run_at, _table

pytestmark = pytest.mark.gpu


def _pairs_table(pairs):
    """The int32 device table [P, 2] of section pairs."""
    return torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)).cuda()


def _launch_pairs(block, z_org, pairs, geo, tile, r, table, bounds, sums_ptr, off=0, row=0, npairs=None):
    """One tem_u8_zshift_tiles_pairs call on `block`, `off` bytes into an aligned allocation between guards of FILL,
    with both tables' rows from `row` on; block, guards and tables must be untouched."""
    L, lib, stream = _env()
    r0, r1, y_org, Y, gy, gx = geo
    flat = np.ascontiguousarray(block).reshape(-1)
    t = torch.full((flat.size + off + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0 and table.dtype == torch.int32 and table.shape[1:] == (gy, gx, 2)
    assert pairs.dtype == torch.int32 and pairs.shape == (table.shape[0], 2)
    t[GUARD + off:GUARD + off + flat.size] = torch.from_numpy(flat.copy()).cuda()
    before, pbefore = table.clone(), pairs.clone()
    n = pairs.shape[0] - row if npairs is None else npairs
    L.check(lib.tem_u8_zshift_tiles_pairs(t.data_ptr() + GUARD + off, *block.shape, z_org, n, pairs.data_ptr() + 8 * row,
                                          r0, r1, y_org, Y, *tile, gy, gx, r, table.data_ptr() + 8 * gy * gx * row,
                                          *bounds, sums_ptr, stream), "tem_u8_zshift_tiles_pairs")
    got = t.cpu().numpy()
    assert (got[:GUARD + off] == FILL).all() and (got[GUARD + off + flat.size:] == FILL).all()
    assert np.array_equal(got[GUARD + off:GUARD + off + flat.size], flat)
    assert torch.equal(table, before) and torch.equal(pairs, pbefore)


def _run_pairs(block, z_org, pairs, geo, tile, r, centers, bounds=None, off=0):
    pairs = np.asarray(pairs).reshape(-1, 2)
    s = _Sums(max(len(pairs), 1), geo[4], geo[5], r)
    _launch_pairs(block, z_org, _pairs_table(pairs), geo, tile, r, _table(centers),
                  _bounds(centers) if bounds is None else bounds, s.ptr(), off)
    return s.result()[:len(pairs)]


def _inside(shape, tile, r, lo, hi, margin=48):
    """(r0, r1, y_org, Y, gy, gx) of a block off the tile grid inside a taller section that holds EXACTLY the rows its
    core needs at a reach of [lo, hi]: [r0 - r + lo, r1 + r + hi) = [0, H); the section goes on for `margin` rows and
    more on either side, further than any centre of these tests."""
    (D, H, W), (th, tw) = shape, tile
    y_org = th + th // 3 + margin
    Y = y_org + H + margin + th // 2 + 1
    r0, r1 = r - lo, H - r - hi
    assert r0 < r1 and max(-lo, hi) <= margin
    return r0, r1, y_org, Y, -(-Y // th) + 1, -(-W // tw) + 1


# ------------------------------------------------------------------- the pairs (d, d + 1): the sibling, byte for byte
BLOCKS = [(3, 37, 53), (4, 70, 131)]
TILES = [(16, 16), (32, 48), (7, 5)]
RADII = [1, 4, 8]


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("tile", TILES, ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("shape", BLOCKS, ids=lambda s: "x".join(map(str, s)))
def test_consecutive_pairs_equal_the_sibling_byte_for_byte(shape, tile, r):
    block, D = _data(shape, "random"), shape[0]
    assert shape[2] % 4
    for k, (geo, ylim, off, z_org) in enumerate(((_geometry(shape, tile, r, "whole"), (-20, 20), 0, 0),
                                                 (_inside(shape, tile, r, -5, 6), (-5, 6), 3, 7))):
        C = _centers(71 + k, D, geo[4], geo[5], ylim, (-40, 40))
        bounds = _bounds(C)
        want = _run_at(block, 0, D, geo, tile, r, C, bounds, off)                   # D rows, the last one zero
        pairs = [(z_org + d, z_org + d + 1) for d in range(D - 1)]
        got = _run_pairs(block, z_org, pairs, geo, tile, r, C[:D - 1], bounds, off)
        assert want[:-1].any() and not want[-1].any()
        assert got.tobytes() == want[:-1].tobytes(), (k, np.argwhere(got != want[:-1])[:5])
    got = _run_pairs(block, z_org, pairs[1:], geo, tile, r, C[1:D - 1], bounds, 1)  # a part of the list: its own rows
    assert got.tobytes() == want[1:-1].tobytes()


# ------------------------------------------------------------------------------------ lags 1...8: the numpy reference
LAGS = [(0, 1), (0, 8), (1, 3), (1, 4), (2, 7), (2, 9), (3, 9), (4, 8)]           # lags 1, 8, 2, 3, 5, 7, 6, 4


@pytest.mark.parametrize("shape,tile,r", [((10, 40, 61), (16, 24), 2), ((10, 33, 70), (32, 32), 4), ((10, 19, 23), (7, 5), 8)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_kernel_equals_the_reference_for_every_lag(shape, tile, r):
    block, (D, H, W), (th, tw) = _data(shape, "random"), shape, tile
    assert sorted(b - a for a, b in LAGS) == list(range(1, 9)) and len({a for a, _ in LAGS}) < len(LAGS) < D - 1
    z_org = 3
    pairs = np.array(LAGS) + z_org
    geo = r0, r1, y_org, Y, gy, gx = _geometry(shape, tile, r, "whole")
    C = _centers(73, len(LAGS), gy, gx, (-20, 20), (-40, 40))
    C[0, 0, 0], C[1, 0, 0] = (H + r, 3), (-2, -(min(tw, W) + r - 2))               # a window wholly outside; nearly
    want = PR.tile_sums_pairs(block, pairs, C, z_org, *geo[:4], th, tw, gy, gx, r)
    assert not want[0, 0, 0].any() and want[1, 0, 0].any() and want.any(axis=(1, 2, 3, 4, 5)).all()
    for off in (0, 3):
        got = _run_pairs(block, z_org, pairs, geo, tile, r, C, off=off)
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    cut = (th // 2 + 1, H - th // 3 - 1) + geo[2:]                                  # core rows cut inside tiles
    want = PR.tile_sums_pairs(block, pairs, C, z_org, *cut[:4], th, tw, gy, gx, r)
    assert np.array_equal(_run_pairs(block, z_org, pairs, cut, tile, r, C, off=1), want)
    # the block off the grid inside a taller section, holding exactly the rows of its reach; two pairs of ten planes
    lo, hi = (-3, 2)
    geo = r0, r1, y_org, Y, gy, gx = _inside(shape, tile, min(r, 4), lo, hi)
    rr = min(r, 4)
    C = _centers(79, 2, gy, gx, (lo, hi), (-40, 40))
    i0, i1 = (y_org + r0) // th, (y_org + r1 - 1) // th
    C[0, i0, 0], C[1, i1, -2] = (lo, -40), (hi, 40)
    want = PR.tile_sums_pairs(block, [(4, 9), (6, 7)], C, 0, *geo[:4], th, tw, gy, gx, rr)   # asserts the partner rows
    got = _run_pairs(block, 0, [(4, 9), (6, 7)], geo, tile, rr, C, off=2)
    assert want.any(axis=(1, 2, 3, 4, 5)).all() and np.array_equal(got, want)


def test_a_lag_k_pair_is_the_sibling_on_the_two_planes_stacked():
    shape, tile, r = (10, 33, 70), (32, 32), 4
    block = _data(shape, "random")
    geo = _geometry(shape, tile, r, "whole")
    for a, b in ((0, 2), (3, 8), (1, 9)):
        C = _centers(83 + b, 1, geo[4], geo[5], (-9, 9), (-40, 40))
        want = _run_at(np.stack([block[a], block[b]]), 0, 1, geo, tile, r, C)
        got = _run_pairs(block, 100, [(100 + a, 100 + b)], geo, tile, r, C)
        assert want.any() and got.tobytes() == want.tobytes(), (a, b)


def test_the_largest_centres_on_a_tiny_block():
    """(3, 5, 7) with centres of +-1024 and a lag-2 pair: windows a thousand pixels outside add nothing."""
    shape, tile, r = (3, 5, 7), (3, 5), 2
    block = _data(shape, "random")
    geo = _geometry(shape, tile, r, "whole")
    C = np.zeros((1, geo[4], geo[5], 2), np.int64)
    C[0, 0, 0], C[0, 0, 1], C[0, 1, 0], C[0, 1, 1] = (1024, -1024), (-1, 2), (-1024, 3), (2, 1024)
    want = PR.tile_sums_pairs(block, [(0, 2)], C, 0, *geo[:4], *tile, *geo[4:], r)
    assert want[0, 0, 1].any() and not want[0, 0, 0].any() and not want[0, 1].any()
    for off in (0, 3):
        assert np.array_equal(_run_pairs(block, 0, [(0, 2)], geo, tile, r, C, (-1024, 1024, 1024), off), want)


def test_kernel_accumulates_across_row_cuts_and_chunk_cuts():
    """One launch equals two launches on core rows cut through a tile, two launches on blocks cut along y that hold just
    the rows of their reach, two launches on halves of the list, where the tables' pointers move, and two launches on
    blocks cut along z, where z_org moves."""
    shape, tile, r = (8, 33, 70), (32, 32), 4
    block = _data(shape, "random")
    r0, r1, y_org, Y, gy, gx = geo = _geometry(shape, tile, r, "whole")
    pairs = np.array([(0, 1), (1, 4), (2, 3), (4, 5), (5, 7)])
    C = _centers(89, 5, gy, gx, (-3, 2), (-40, 40))
    C[0, 0, 0], C[1, 1, 1] = (-3, 5), (2, -5)
    table, ptable, bounds = _table(C), _pairs_table(pairs), _bounds(C)
    assert bounds[:2] == (-3, 2)
    want = PR.tile_sums_pairs(block, pairs, C, 0, *geo[:4], *tile, gy, gx, r)
    for off in (0, 1):
        s = _Sums(5, gy, gx, r)
        _launch_pairs(block, 0, ptable, geo, tile, r, table, bounds, s.ptr(), off)
        assert np.array_equal(s.result(), want)
        s = _Sums(5, gy, gx, r)                                                     # core rows [0, 17) | [17, 33)
        _launch_pairs(block, 0, ptable, (0, 17) + geo[2:], tile, r, table, bounds, s.ptr(), off)
        _launch_pairs(block, 0, ptable, (17, 33) + geo[2:], tile, r, table, bounds, s.ptr(), off)
        assert np.array_equal(s.result(), want)
        s = _Sums(5, gy, gx, r)                                                     # blocks of rows [0, 23) | [10, 33)
        _launch_pairs(block[:, :23], 0, ptable, (0, 17, 0, Y, gy, gx), tile, r, table, bounds, s.ptr(), off)
        _launch_pairs(block[:, 10:], 0, ptable, (7, 23, 10, Y, gy, gx), tile, r, table, bounds, s.ptr(), off)
        assert np.array_equal(s.result(), want)
        s = _Sums(5, gy, gx, r)                                                     # the list's rows [0, 2) | [2, 5)
        _launch_pairs(block, 0, ptable, geo, tile, r, table, bounds, s.ptr(0), off, row=0, npairs=2)
        _launch_pairs(block, 0, ptable, geo, tile, r, table, bounds, s.ptr(2), off, row=2)
        assert np.array_equal(s.result(), want)
        s = _Sums(5, gy, gx, r)                                                     # sections [0, 5) | [4, 8)
        _launch_pairs(block[:5], 0, ptable, geo, tile, r, table, bounds, s.ptr(0), off, row=0, npairs=3)
        _launch_pairs(block[4:], 4, ptable, geo, tile, r, table, bounds, s.ptr(3), off, row=3)
        assert np.array_equal(s.result(), want)
    assert not np.array_equal(C[0], C[2])                                           # the moved pointers matter


def test_kernel_holds_the_largest_tile_of_the_largest_values():
    """Three planes of 2048 x 2048 voxels of 255 in one tile at r = 1, the pair (0, 2) centred on (5, -7), against the
    closed form."""
    block = np.full((3, 2048, 2048), 255, np.uint8)
    C = np.zeros((1, 1, 1, 2), np.int64)
    C[0, 0, 0] = (5, -7)
    got = _run_pairs(block, 0, [(0, 2)], (0, 2048, 0, 2048, 1, 1), (2048, 2048), 1, C)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            n = (2048 - abs(5 + dy)) * (2048 - abs(-7 + dx))
            assert n * 65025 > 2 ** 32
            assert got[0, 0, 0, dy + 1, dx + 1].tolist() == [255 * n, 65025 * n, 255 * n, 65025 * n, 65025 * n]


def test_kernel_clamps_pairs_and_centres_that_break_the_promise():
    """The block is the middle of a larger device buffer that the test owns: a pair table that names sections outside
    [z_org, z_org + D), and centres past the promised bounds, give the sums of the clamped tables -- a kernel that did
    not clamp would read the test's own planes and give other sums."""
    L, lib, stream = _env()
    shape, tile, r, M, z_org = (4, 33, 70), (7, 64), 2, 9, 20
    big = np.random.default_rng(97).integers(0, 256, (shape[0] + 2 * M,) + shape[1:], dtype=np.uint8)
    block = big[M:M + 4]
    r0, r1, y_org, Y, gy, gx = geo = _geometry(shape, tile, r, "whole")
    lo, hi, xm = -3, 2, 6
    pairs = np.array([(z_org - 1, z_org + 1), (z_org, z_org + 9), (z_org + 2, z_org + 4), (z_org - 8, z_org - 7),
                      (z_org + 1, z_org + 3), (z_org + 7, z_org + 8)])
    clamped_pairs = np.clip(pairs, z_org, z_org + 3)
    assert (clamped_pairs != pairs).sum() == 7
    C = _centers(101, len(pairs), gy, gx, (lo, hi), (-xm, xm))
    C[0, 0, 0], C[0, 1, 1], C[4, 2, 0], C[4, 3, 1] = (lo - 1, 0), (hi + 1, xm + 1), (lo - 4, -xm - 1), (hi + 4, -xm - 9)
    clamped = np.stack([np.clip(C[..., 0], lo, hi), np.clip(C[..., 1], -xm, xm)], axis=-1)
    assert (clamped != C).sum() == 7
    want = PR.tile_sums_pairs(block, clamped_pairs, clamped, z_org, *geo[:4], *tile, gy, gx, r)
    honest = PR.tile_sums_pairs(big, pairs, C, z_org - M, *geo[:4], *tile, gy, gx, r)
    assert all(not np.array_equal(want[k], honest[k]) for k in (0, 1, 2, 3, 4, 5))
    dev = torch.from_numpy(big.copy()).cuda()
    s = _Sums(len(pairs), gy, gx, r)
    table, ptable = _table(C), _pairs_table(pairs)
    L.check(lib.tem_u8_zshift_tiles_pairs(dev.data_ptr() + M * 33 * 70, *shape, z_org, len(pairs), ptable.data_ptr(),
                                          r0, r1, y_org, Y, *tile, gy, gx, r, table.data_ptr(), lo, hi, xm, s.ptr(),
                                          stream), "tem_u8_zshift_tiles_pairs")
    got = s.result()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(dev.cpu().numpy(), big)


def test_kernel_refuses_bad_arguments():
    """TEM_EINVAL / TEM_EUNSUPPORTED from the host-side checks, nothing launched, nothing allocated: sums keeps its
    fill."""
    L, lib, stream = _env()
    src = torch.ones(4 * 6 * 8 + 16, dtype=torch.uint8, device="cuda")
    sums = torch.full((3 * 2 * 2 * 125 + 1,), SFILL, dtype=torch.int64, device="cuda")
    ctr = torch.zeros(3 * 3 * 2 * 2 + 1, dtype=torch.int32, device="cuda")
    prs = torch.tensor([[0, 1], [0, 3], [2, 3], [0, 0]], dtype=torch.int32, device="cuda").reshape(-1)
    p, s, c, t = src.data_ptr(), sums.data_ptr(), ctr.data_ptr(), prs.data_ptr()
    call = lambda *a: lib.tem_u8_zshift_tiles_pairs(*a, stream)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    # 0 src, 1 D, 2 H, 3 W, 4 z_org, 5 npairs, 6 pairs, 7 r0, 8 r1, 9 y_org, 10 Y, 11 th, 12 tw, 13 gy, 14 gx,
    # 15 radius, 16 centers, 17 cy_lo, 18 cy_hi, 19 cx_max, 20 sums
    ok = [p, 4, 6, 8, 0, 3, t, 0, 6, 0, 6, 4, 4, 2, 2, 2, c, -1, 1, 3, s]
    for i, v in [(0, None), (20, None), (20, s + 4), (20, s + 1), (1, 0), (2, 0), (3, 0), (1, -1), (10, 0), (13, 0),
                 (14, 0), (13, -1), (11, 0), (11, 2049), (12, 0), (12, 2049), (15, 0), (15, 9), (15, -1), (9, -1),
                 (13, 1), (14, 1), (10, 5), (9, 1), (7, -1), (8, 7), (7, 4),
                 (16, None), (16, c + 1), (16, c + 2), (17, 1), (17, -1025), (18, -1), (18, 1025), (19, -1), (19, 1025),
                 (6, None), (6, t + 1), (6, t + 2), (5, -1), (5, -2 ** 31)]:
        a = list(ok)
        a[i] = v
        if (i, v) == (7, 4):
            a[8] = 3                                                                # r0 > r1
        assert call(*a) == L.TEM_EINVAL, (i, v)
    # rows 2...7 of 12, core rows [3, 4): radius 2 and a reach of [-1, 1] need rows [0, 7) of the block's 6 -- and so on
    inside = [p, 4, 6, 8, 0, 3, t, 3, 3, 2, 12, 4, 4, 3, 2, 2, c, 0, 0, 0, s]
    for r0, r1, lo, hi in ((3, 4, -1, 1), (3, 4, -2, 0), (2, 4, -1, 0), (3, 5, 0, 0), (2, 4, 0, 1), (1, 4, 0, 0)):
        assert call(*inside[:7], r0, r1, *inside[9:17], lo, hi, 0, s) == L.TEM_EINVAL, (r0, r1, lo, hi)
    assert call(*ok[:5], 0, *ok[6:]) == 0 and call(*ok[:7], 3, 3, *ok[9:]) == 0     # no pairs, an empty core: no launch
    assert call(p, 4, 4, 4, 0, 2 ** 31 - 1, t, 0, 4, 0, 4, 1, 1, 4, 4, 1, c, 0, 0, 0, s) == L.TEM_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (sums.cpu().numpy() == SFILL).all() and torch.cuda.memory_allocated() == held
    sums.zero_()
    assert call(*ok) == 0 and call(p + 3, *ok[1:]) == 0                             # and the good call runs, any z_org
    assert call(*ok[:4], -5, 1, t + 24, *ok[7:]) == 0                               # (0, 0) against section -5: plane 0 twice
    torch.cuda.synchronize()
    got = sums.cpu().numpy()[:1500].reshape(3, 2, 2, 5, 5, 5)
    assert got[1:, ..., 2, 2, 0].sum() == 2 * 2 * 6 * 8 and got[0, ..., 2, 2, 0].sum() == 3 * 6 * 8
    sums2 = torch.zeros(3 * 3 * 2 * 125, dtype=torch.int64, device="cuda")
    assert call(*inside[:7], 3, 4, *inside[9:17], -1, 0, 0, sums2.data_ptr()) == 0  # the one with just its reach: [0, 6)
    assert call(*inside[:7], 2, 3, *inside[9:17], 0, 1, 0, sums2.data_ptr()) == 0
    torch.cuda.synchronize()
    assert sums2.cpu().numpy().reshape(3, 3, 2, 5, 5, 5)[..., 2, 2, 0].sum() == 3 * 2 * 8


# ----------------------------------------------------------------------------------------- section_shift_sums_pairs
VSHAPE, VTILE, VR = (8, 70, 96), (32, 32), 4
VPAIRS = [(0, 1), (1, 2), (2, 5), (5, 6), (6, 7)]
BUDGETS = {"one_slab": 9 * 70 * 96, "three_sections": 3 * 70 * 96, "row_cuts": 2 * 30 * 96}


@functools.lru_cache(maxsize=None)
def _vcase():
    vol = np.random.default_rng(19).integers(0, 256, VSHAPE, dtype=np.uint8)
    vol[1::2] = vol[1::2] // 2 + vol[:-1:2] // 2                                   # neighbours correlate
    C = _centers(103, len(VPAIRS), 3, 3, (-9, 6), (-40, 40))
    C[2, 1, 1], C[3, 0, 2] = (-9, 1), (6, -1)
    want = PR.volume_sums_pairs(vol, VPAIRS, C, VTILE, VR)
    for a in (vol, C, want):
        a.setflags(write=False)
    return vol, C, want


@pytest.fixture(scope="module")
def vmap(tmp_path_factory):
    path = tmp_path_factory.mktemp("zshift_pairs") / "vol.u8"
    m = np.memmap(path, np.uint8, "w+", shape=VSHAPE)
    m[...] = _vcase()[0]
    m.flush()
    return np.memmap(path, np.uint8, "r", shape=VSHAPE)


@pytest.mark.parametrize("budget", list(BUDGETS), ids=list(BUDGETS))
def test_section_shift_sums_pairs_equals_the_reference_however_it_is_cut(vmap, budget):
    from transfer_em_amd.utils import section_shift_sums_pairs, zshift_chunks_pairs
    vol, C, want = _vcase()
    st = {}
    got, counts = _counted(lambda: section_shift_sums_pairs(vmap, VPAIRS, C, VTILE, VR, chunk_bytes=BUDGETS[budget], stats=st))
    assert got.dtype == np.int64 and got.shape == (5, 3, 3, 9, 9, 5) and np.array_equal(got, want)
    assert got.any(axis=(1, 2, 3, 4, 5)).all()
    chunks = zshift_chunks_pairs(VSHAPE, VPAIRS, VR, (-9, 6), BUDGETS[budget])
    n = len(chunks)
    assert st["chunks"] == n and st["read_s"] >= 0
    assert counts["tem_u8_zshift_tiles_pairs"] == n and counts["tem_u8_zshift_tiles_at"] == 0   # one launch per chunk
    # three sections: (0,1)(1,2) | the lag-3 pair in rows, 4 planes of 52 rows less 23 of halo: 29 + 29 + 12 | (5,6)(6,7)
    assert {"one_slab": n == 1, "three_sections": n == 1 + 3 + 1, "row_cuts": n > 5 * 3}[budget]
    assert budget != "three_sections" or chunks[2] == ((2, 3), (29, 58), ((2, 6), (16, 68), (0, 96)))
    assert np.array_equal(np.asarray(vmap), vol)                                    # the input: read only


def test_section_shift_sums_pairs_ranks_the_per_chunk_read_back_and_the_sibling(vmap, monkeypatch):
    from transfer_em_amd import utils
    vol, C, want = _vcase()
    assert np.array_equal(utils.section_shift_sums_pairs(vol, VPAIRS, C, VTILE, VR), want)      # an ndarray, one slab
    for budget in ("three_sections", "row_cuts"):
        parts = [utils.section_shift_sums_pairs(vmap, VPAIRS, C, VTILE, VR, chunk_bytes=BUDGETS[budget], rank=r, world_size=2)
                 for r in (1, 0)]
        assert parts[0].any() and parts[1].any() and not np.array_equal(parts[0], want)
        assert np.array_equal(parts[0] + parts[1], want)                            # the ranks' results add
    chain = utils.section_pairs(8).pairs                                            # the chain (z, z + 1): the sibling's rows
    C7 = _centers(107, 7, 3, 3, (-9, 6), (-40, 40))
    at = utils.section_shift_sums_at(vmap, C7, VTILE, VR, chunk_bytes=BUDGETS["three_sections"])
    assert np.array_equal(at, AR.volume_sums_at(vol, C7, VTILE, VR))
    for budget in BUDGETS.values():
        assert utils.section_shift_sums_pairs(vmap, chain, C7, VTILE, VR, chunk_bytes=budget).tobytes() == at[:-1].tobytes()
    zero = utils.section_shift_sums_pairs(vmap, VPAIRS, None, VTILE, VR)            # no centres: zero
    assert np.array_equal(zero, PR.volume_sums_pairs(vol, VPAIRS, np.zeros((5, 3, 3, 2), np.int64), VTILE, VR))
    few = utils.section_shift_sums_pairs(vmap, [(2, 5)], C[2:3, 0, 0], VTILE, VR)   # one pair, one centre for its tiles
    one = np.broadcast_to(C[2:3, :1, :1], (1, 3, 3, 2))
    assert np.array_equal(few, PR.volume_sums_pairs(vol, [(2, 5)], one, VTILE, VR))
    monkeypatch.setattr(utils, "CLAHE_ACC_BYTES", 5 * 3 * 3 * 81 * 40 - 1)          # the accumulator no longer fits
    for budget in ("three_sections", "row_cuts"):
        got, counts = _counted(lambda: utils.section_shift_sums_pairs(vmap, VPAIRS, C, VTILE, VR, chunk_bytes=BUDGETS[budget]))
        assert np.array_equal(got, want)
        assert counts["tem_u8_zshift_tiles_pairs"] == len(utils.zshift_chunks_pairs(VSHAPE, VPAIRS, VR, (-9, 6), BUDGETS[budget]))
    both = [utils.section_shift_sums_pairs(vmap, VPAIRS, C, VTILE, VR, chunk_bytes=BUDGETS["row_cuts"], rank=r, world_size=2)
            for r in (0, 1)]
    assert np.array_equal(both[0] + both[1], want)


# ------------------------------------------------------------------------------------------------------- end to end
def _interior_tiles_measure_zero(v, pair_shifts):
    """(tiles seen, tiles that do not re-measure (0, 0)) after shift_positions -> volume_shift -> volume_repair of the
    skipped sections, over every interior tile -- no fill near it, in either section or in the sections a repaired one
    was blended from -- of every consecutive pair."""
    from transfer_em_amd.utils import (Repair, section_shift_sums, section_shifts, shift_counts, shift_positions,
                                       volume_repair, volume_shift)
    Z, t, r = v.shape[0], PR.BAD_TILE, PR.BAD_RADIUS
    P = shift_positions(pair_shifts)
    moved = volume_repair(volume_shift(v, P), Repair(sections=PR.BAD_SKIP))
    whole = volume_shift(np.ones_like(v), P).astype(bool)                           # where no fill entered
    good = [z for z in range(Z) if z not in PR.BAD_SKIP]
    for z in PR.BAD_SKIP:
        whole[z] = whole[max(g for g in good if g < z)] & whole[min(g for g in good if g > z)]
    s = section_shifts(section_shift_sums(moved, t, r), shift_counts(v.shape, t, r))
    seen = wrong = 0
    for z in range(Z - 1):
        for i in range(5):
            for j in range(6):
                box = (slice(max(i * t - r, 0), (i + 1) * t + r), slice(max(j * t - r, 0), (j + 1) * t + r))
                if whole[z][box].all() and whole[z + 1][box].all():
                    seen += 1
                    wrong += not (s.decided[z, i, j] and tuple(s.tiles[z, i, j]) == (0, 0))
    return seen, wrong


def test_the_bad_sections_are_bridged_and_the_stack_is_aligned_across_them():
    from transfer_em_amd.utils import chain_pairs, section_shifts_bridged, section_shifts_coarse_to_fine, suspect_sections
    v = PR.bad_volume()
    plain = section_shifts_coarse_to_fine(v, PR.BAD_TILE, PR.BAD_RADIUS, PR.BAD_LEVELS)
    assert plain.shifts.unresolved == PR.host_plain().shifts.unresolved == [2, 3, 6, 7, 8]
    assert suspect_sections(plain.shifts.unresolved, 12) == list(PR.BAD_SKIP)       # where the skip list comes from
    st = {}
    got = section_shifts_bridged(v, PR.chain_list(), PR.BAD_TILE, PR.BAD_RADIUS, PR.BAD_LEVELS, chunk_bytes=4 * 160 * 192,
                                 stats=st)
    want = PR.host_bridged()
    for a, b in zip(got.shifts[:4], want.shifts[:4]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert got.shifts.unresolved == want.shifts.unresolved == []
    assert np.array_equal(got.q, want.q) and np.array_equal(got.n, want.n) and np.array_equal(got.centers, want.centers)
    assert np.array_equal(got.pairs, want.pairs) and st["chunks"] >= 3 + 5 + 3 and st["read_s"] >= 0
    only = section_shifts_bridged(v, PR.BAD_BRIDGES, PR.BAD_TILE, PR.BAD_RADIUS, PR.BAD_LEVELS)
    assert np.array_equal(only.q, want.q[[2, 5]]) and np.array_equal(only.shifts.pairs, want.shifts.pairs[[2, 5]])
    seen, wrong = _interior_tiles_measure_zero(v, chain_pairs(got.pairs, got.shifts.pairs, 12))
    assert seen >= 11 * 12 and wrong == 0
    seen, wrong = _interior_tiles_measure_zero(v, plain.shifts.pairs)               # the chain alone: blended out of place
    assert seen >= 11 * 12 and wrong > 0
