"""The defect detector on the device: tem_u8_zcorr_tiles against the numpy reference (zcorr_ref), section_sums out of
core, and the chain section_sums -> find_defects -> defects_repair -> volume_repair on the fixture with planted
defects.  Everything is integers, so every comparison is exact.  The kernel reads blocks between guards of fill bytes
and adds into sums between guards of fill words; block and guards must come back untouched.  Helpers are those of
test_gpu_histogram.py."""
import functools

import numpy as np
import pytest
import torch

import repair_ref as RR
import zcorr_ref as ZR
from test_gpu_histogram import _counted, _env

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
SGUARD, SFILL = 8, 0x5A5A5A5A5A5A5A5A
BLOCKS = [(1, 5, 7), (3, 5, 7), (4, 33, 70), (2, 64, 257)]
TILES = [(1, 1), (3, 5), (7, 64), (32, 32), (2048, 2048)]
DATA = ["random", "zeros", "ones", "alternating"]


@functools.lru_cache(maxsize=None)
def _data(shape, kind):
    if kind == "random":
        a = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    elif kind == "alternating":
        a = ((np.arange(int(np.prod(shape))) % 2) * 255).astype(np.uint8).reshape(shape)
    else:
        a = np.full(shape, 0 if kind == "zeros" else 255, np.uint8)
    a.setflags(write=False)
    return a


def _geometry(shape, tile, on_grid):
    """(y_org, x_org, gy, gx): the block at the grid's origin, or off the grid so that it cuts tiles on every side; the
    grid is one tile larger than the block needs, so that some rows of sums stay untouched."""
    (D, H, W), (th, tw) = shape, tile
    y_org, x_org = (0, 0) if on_grid else (th + th // 3, 2 * tw + tw // 2)
    return y_org, x_org, -(-(y_org + H) // th) + 1, -(-(x_org + W) // tw) + 1


@functools.lru_cache(maxsize=None)
def _want(shape, kind, tile, on_grid):
    """The reference sums of every plane of the block: the core [c0, c1) takes rows c0...c1 - 1 of it."""
    want = ZR.tile_sums(_data(shape, kind), 0, shape[0], *_geometry(shape, tile, on_grid)[:2], *tile,
                        *_geometry(shape, tile, on_grid)[2:])
    want.setflags(write=False)
    return want


class _Sums:
    """Device sums [planes, gy, gx, 4] between guards of SFILL, cleared once."""

    def __init__(self, planes, gy, gx):
        self.shape, self.n = (planes, gy, gx, 4), planes * gy * gx * 4
        self.t = torch.full((self.n + 2 * SGUARD,), SFILL, dtype=torch.int64, device="cuda")
        self.t[SGUARD:SGUARD + self.n] = 0
        self.sec = gy * gx * 4

    def ptr(self, plane=0):
        return self.t.data_ptr() + 8 * (SGUARD + plane * self.sec)

    def result(self):
        got = self.t.cpu().numpy()
        assert (got[:SGUARD] == SFILL).all() and (got[SGUARD + self.n:] == SFILL).all()
        return got[SGUARD:SGUARD + self.n].reshape(self.shape)


def _launch(block, c0, c1, y_org, x_org, tile, gy, gx, sums_ptr, off=0):
    """One tem_u8_zcorr_tiles call on `block`, `off` bytes into an aligned allocation between guards of FILL; block and
    guards must be untouched."""
    L, lib, stream = _env()
    flat = np.ascontiguousarray(block).reshape(-1)
    t = torch.full((flat.size + off + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    t[GUARD + off:GUARD + off + flat.size] = torch.from_numpy(flat.copy()).cuda()
    L.check(lib.tem_u8_zcorr_tiles(t.data_ptr() + GUARD + off, *block.shape, c0, c1, y_org, x_org, *tile, gy, gx,
                                   sums_ptr, stream), "tem_u8_zcorr_tiles")
    got = t.cpu().numpy()
    assert (got[:GUARD + off] == FILL).all() and (got[GUARD + off + flat.size:] == FILL).all()
    assert np.array_equal(got[GUARD + off:GUARD + off + flat.size], flat)


def _run(block, c0, c1, y_org, x_org, tile, gy, gx, off=0):
    s = _Sums(max(c1 - c0, 1), gy, gx)
    _launch(block, c0, c1, y_org, x_org, tile, gy, gx, s.ptr(), off)
    return s.result()[:c1 - c0]


# ----------------------------------------------------------------------------------------------- tem_u8_zcorr_tiles
@pytest.mark.parametrize("tile", TILES, ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("shape", BLOCKS, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_reference(shape, tile):
    """Every kind of data, the block on the grid and off it, the whole block as the core at byte offsets 0...3, and the
    other cores ([0, D - 1): the last plane is halo only; [1, 2); an empty one) at offsets 0 and 3."""
    D = shape[0]
    for kind in DATA:
        block = _data(shape, kind)
        for on_grid in (True, False):
            geo = _geometry(shape, tile, on_grid)
            want = _want(shape, kind, tile, on_grid)
            assert int(want[..., 3].sum()) == block.size                           # every voxel in exactly one tile
            for c0, c1 in ((0, D), (0, D - 1), (min(1, D), min(2, D)), (D, D)):
                for off in ((0, 1, 2, 3) if (c0, c1) == (0, D) else (0, 3)):
                    got = _run(block, c0, c1, geo[0], geo[1], tile, geo[2], geo[3], off)
                    assert got.shape == want[c0:c1].shape and np.array_equal(got, want[c0:c1]), \
                        (kind, on_grid, c0, c1, off, np.argwhere(got != want[c0:c1])[:5])


def test_kernel_cases_cover_what_they_claim():
    """The off-grid blocks cut tiles on all four sides, the pair term is there and absent, rows are long and short."""
    for shape, tile in (((4, 33, 70), (32, 32)), ((2, 64, 257), (7, 64)), ((4, 33, 70), (3, 5))):
        y_org, x_org, gy, gx = _geometry(shape, tile, False)
        assert y_org % tile[0] and x_org % tile[1] and (y_org + shape[1]) % tile[0] and (x_org + shape[2]) % tile[1]
        want = _want(shape, "random", tile, False)
        assert (want[:-1, ..., 2].sum(axis=(1, 2)) > 0).all() and not want[-1, ..., 2].any()
        assert not want[:, -1].any() and not want[:, :, -1].any()                  # the grid's spare row and column
    assert _want((1, 5, 7), "ones", (3, 5), True)[0, 0, 0].tolist() == [15 * 255, 15 * 255 * 255, 0, 15]
    alt = _want((3, 5, 7), "alternating", (2048, 2048), True)                      # H W odd: planes alternate too
    assert alt[0, 0, 0].tolist() == [17 * 255, 17 * 255 * 255, 0, 35]


def _plan(shape, ncore, geo, tile):
    """The launch plan of csrc/zcorr_u8.hip for a block: (workgroups per plane-run, planes per run, 16-byte pieces of
    a whole tile's workgroup) -- 1,024 pieces per workgroup at most, runs sized for about 1,024 workgroups, 16 planes
    at most."""
    (D, H, W), (th, tw), (y_org, x_org) = shape, tile, geo[:2]
    nty, ntx = (y_org + H - 1) // th - y_org // th + 1, (x_org + W - 1) // tw - x_org // tw + 1
    S = (min(tw, W) + 15) // 16
    rpp = 1024 // S
    units = nty * ntx * -(-min(th, H) // rpp)
    return units, min(16, max(1, ncore * units // 1024)), min(th, H, rpp) * S


LONG_SHAPE, LONG_TILE = (25, 1001, 1731), (100, 144)


def test_kernel_marches_full_workgroups_along_z():
    """The shape of a real call: runs of three planes carried in registers, workgroups of 900 pieces -- all four waves,
    all four pieces of a thread, all four words of a piece, nine pieces per row --, a plane stride that is odd, so a
    piece's alignment changes from plane to plane inside a run, W no multiple of 4, and cores that end before D: one
    of whole runs, one that starts inside the block and ends in a run of one plane."""
    D, H, W = LONG_SHAPE
    geo = _geometry(LONG_SHAPE, LONG_TILE, False)
    assert (H * W) % 4 == 3 and W % 4 == 3
    for c0, c1, runs in ((0, D - 1, [3] * 8), (2, D - 1, [3] * 7 + [1])):
        units, zr, pieces = _plan(LONG_SHAPE, c1 - c0, geo, LONG_TILE)
        assert units == 11 * 13 and zr == 3 and pieces == 900 > 3 * 256
        assert [min(zr, c1 - z) for z in range(c0, c1, zr)] == runs
    block = _data(LONG_SHAPE, "random")
    want = _want(LONG_SHAPE, "random", LONG_TILE, False)
    assert (want[:, 2:11, 3:14, 3] == 100 * 144).all()                            # 9 x 11 whole tiles inside the block
    for c0, c1, off in ((0, D - 1, 0), (2, D - 1, 1)):
        got = _run(block, c0, c1, geo[0], geo[1], LONG_TILE, geo[2], geo[3], off)
        assert np.array_equal(got, want[c0:c1]), (c0, c1, off, np.argwhere(got != want[c0:c1])[:5])


def test_kernel_accumulates_across_cuts():
    """One launch equals two launches on halves cut through a tile along y, and two launches cut along z with the lower
    half given its halo plane."""
    shape, tile = (4, 33, 70), (32, 32)
    block = _data(shape, "random")
    y_org, x_org, gy, gx = _geometry(shape, tile, False)
    want = _want(shape, "random", tile, False)
    for off in (0, 1):
        s = _Sums(4, gy, gx)                                                        # rows [0, 17) | [17, 33)
        _launch(block[:, :17], 0, 4, y_org, x_org, tile, gy, gx, s.ptr(), off)
        _launch(block[:, 17:], 0, 4, y_org + 17, x_org, tile, gy, gx, s.ptr(), off)
        assert np.array_equal(s.result(), want)
        s = _Sums(4, gy, gx)                                                        # columns [0, 41) | [41, 70)
        _launch(block[:, :, :41], 0, 4, y_org, x_org, tile, gy, gx, s.ptr(), off)
        _launch(block[:, :, 41:], 0, 4, y_org, x_org + 41, tile, gy, gx, s.ptr(), off)
        assert np.array_equal(s.result(), want)
        s = _Sums(4, gy, gx)                                                        # planes [0, 2) + halo | [2, 4)
        _launch(block[:3], 0, 2, y_org, x_org, tile, gy, gx, s.ptr(0), off)
        _launch(block[2:], 0, 2, y_org, x_org, tile, gy, gx, s.ptr(2), off)
        assert np.array_equal(s.result(), want)
    s = _Sums(4, gy, gx)                                                            # the same launch twice: it ADDS
    for _ in range(2):
        _launch(block, 0, 4, y_org, x_org, tile, gy, gx, s.ptr())
    assert np.array_equal(s.result(), 2 * want)


def test_kernel_holds_the_largest_tile_of_the_largest_values():
    """Two planes of 2048 x 2048 voxels of 255 in one tile: 2^22 x 65025 per plane, far past 32 bits."""
    block = np.full((2, 2048, 2048), 255, np.uint8)
    got = _run(block, 0, 2, 0, 0, (2048, 2048), 1, 1)
    n = 2048 * 2048
    assert n * 65025 > 2 ** 32
    assert got[0, 0, 0].tolist() == [255 * n, 65025 * n, 65025 * n, n]
    assert got[1, 0, 0].tolist() == [255 * n, 65025 * n, 0, n]


def test_kernel_refuses_bad_arguments():
    """TEM_EINVAL from the host-side checks, nothing launched: sums keeps its fill."""
    L, lib, stream = _env()
    src = torch.zeros(4 * 6 * 8 + 16, dtype=torch.uint8, device="cuda")
    sums = torch.full((4 * 2 * 2 * 4 + 1,), SFILL, dtype=torch.int64, device="cuda")
    p, s = src.data_ptr(), sums.data_ptr()
    call = lambda *a: lib.tem_u8_zcorr_tiles(*a, stream)
    ok = [p, 4, 6, 8, 0, 4, 0, 0, 4, 4, 2, 2, s]       # src D H W c0 c1 y_org x_org th tw gy gx sums
    for i, v in [(0, None), (12, None), (12, s + 4), (12, s + 1), (1, 0), (2, 0), (3, 0), (1, -1), (10, 0), (11, 0),
                 (10, -1), (8, 0), (8, 2049), (9, 0), (9, 2049), (6, -1), (7, -1), (10, 1), (11, 1), (6, 3), (7, 1),
                 (4, -1), (5, 5), (4, 3)]:
        a = list(ok)
        a[i] = v
        if (i, v) == (4, 3):
            a[5] = 2                                                                # c0 > c1
        assert call(*a) == L.TEM_EINVAL, (i, v)
    assert call(*ok[:4], 2, 2, *ok[6:]) == 0                                        # an empty core launches nothing
    # more workgroups than one launch holds: 16 tiles x 2^27 runs of 16 planes (refused before anything is touched)
    assert call(p, 2 ** 31 - 1, 4, 4, 0, 2 ** 31 - 1, 0, 0, 1, 1, 4, 4, s) == L.TEM_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (sums.cpu().numpy() == SFILL).all()
    sums.zero_()
    assert call(*ok) == 0 and call(p + 3, *ok[1:]) == 0                             # and the good call runs
    torch.cuda.synchronize()
    assert sums.cpu().numpy()[:64].reshape(4, 2, 2, 4)[..., 3].sum() == 2 * 4 * 6 * 8


# ----------------------------------------------------------------------------------------------------- section_sums
VSHAPE, VTILE = (40, 50, 70), (16, 24)
BUDGETS = {"whole": 40 * 50 * 70, "three_sections": 3 * 50 * 70, "half_a_section": 25 * 70, "one_row": 70}


@functools.lru_cache(maxsize=None)
def _vcase():
    vol = np.random.default_rng(17).integers(0, 256, VSHAPE, dtype=np.uint8)
    vol[1::2] = vol[1::2] // 2 + vol[:-1:2] // 2                                   # neighbours correlate
    want = ZR.volume_sums(vol, VTILE)
    vol.setflags(write=False), want.setflags(write=False)
    return vol, want


@pytest.fixture(scope="module")
def vmap(tmp_path_factory):
    path = tmp_path_factory.mktemp("zcorr") / "vol.u8"
    m = np.memmap(path, np.uint8, "w+", shape=VSHAPE)
    m[...] = _vcase()[0]
    m.flush()
    return np.memmap(path, np.uint8, "r", shape=VSHAPE)


@pytest.mark.parametrize("budget", list(BUDGETS), ids=list(BUDGETS))
def test_section_sums_equals_the_reference_however_it_is_cut(vmap, budget):
    from transfer_em_amd.utils import section_sums, zcorr_chunks
    want = _vcase()[1]
    st = {}
    got, counts = _counted(lambda: section_sums(vmap, VTILE, chunk_bytes=BUDGETS[budget], stats=st))
    assert got.dtype == np.int64 and got.shape == (40, 4, 3, 4) and np.array_equal(got, want)
    n = len(zcorr_chunks(VSHAPE, BUDGETS[budget]))
    assert st["chunks"] == n and st["read_s"] >= 0
    assert counts["tem_u8_zcorr_tiles"] == n                                        # one launch per slab
    assert {"whole": n == 2, "three_sections": n == 20, "half_a_section": n == 40 * 5, "one_row": n == 40 * 50}[budget]
    assert np.array_equal(np.asarray(vmap), _vcase()[0])                            # the input: read only


def test_section_sums_default_slab_ranks_and_the_per_slab_read_back(vmap, monkeypatch):
    from transfer_em_amd import utils
    vol, want = _vcase()
    assert np.array_equal(utils.section_sums(vol, VTILE), want)                     # an ndarray, one slab
    parts = [utils.section_sums(vmap, VTILE, chunk_bytes=BUDGETS["three_sections"], rank=r, world_size=2)
             for r in (1, 0)]
    assert parts[0].any() and parts[1].any() and not np.array_equal(parts[0], want)
    assert np.array_equal(parts[0] + parts[1], want)                                # the ranks' results add
    monkeypatch.setattr(utils, "CLAHE_ACC_BYTES", 40 * 4 * 3 * 32 - 1)              # the accumulator no longer fits
    for budget in ("three_sections", "half_a_section"):
        got, counts = _counted(lambda: utils.section_sums(vmap, VTILE, chunk_bytes=BUDGETS[budget]))
        assert np.array_equal(got, want)
        assert counts["tem_u8_zcorr_tiles"] == len(utils.zcorr_chunks(VSHAPE, BUDGETS[budget]))
    both = [utils.section_sums(vmap, VTILE, chunk_bytes=BUDGETS["half_a_section"], rank=r, world_size=2) for r in (0, 1)]
    assert np.array_equal(both[0] + both[1], want)


def test_section_sums_of_one_image_and_an_int_tile():
    from transfer_em_amd.utils import section_sums
    vol = _vcase()[0]
    got = section_sums(vol[3], 16)
    assert got.shape == (1, 4, 5, 4) and np.array_equal(got, ZR.volume_sums(vol[3:4], (16, 16)))
    assert not got[..., 2].any()


# ------------------------------------------------------------------------------------------------------- end to end
def test_the_planted_defects_are_found_and_repaired():
    from transfer_em_amd.utils import defects_repair, find_defects, section_sums, volume_repair
    v = ZR.defect_volume()
    s = section_sums(v, ZR.FIX_TILE, chunk_bytes=5 * 96 * 128)
    assert np.array_equal(s, ZR.volume_sums(v, (ZR.FIX_TILE, ZR.FIX_TILE)))
    d = find_defects(s)
    assert d.sections == ZR.FIX_SECTIONS
    assert [tuple(int(x) for x in p) for p in np.argwhere(d.tiles)] == ZR.FIX_TILES
    rp = defects_repair(d, ZR.FIX_TILE, v.shape)
    st = {}
    got = volume_repair(v, rp, stats=st)
    want = RR.repair(v, sections=rp.sections, mask=rp.mask, missing_value=None, max_gap=rp.max_gap)
    assert np.array_equal(got, want) and st["unrepaired"] == 0
    assert st["repaired"] == 4 * 96 * 128 + 32 * 32
    changed = np.flatnonzero((got != v).reshape(48, -1).any(axis=1)).tolist()
    assert changed == [10, 20, 30, 31, 40]
    again = find_defects(section_sums(got, ZR.FIX_TILE))                            # and the repaired volume is clean
    assert again.sections == [] and not again.tiles.any()
