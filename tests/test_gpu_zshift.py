"""The section-shift measurement on the device: tem_u8_zshift_tiles against the numpy reference (zshift_ref),
section_shift_sums out of core, and the chain section_shift_sums -> section_shifts -> shift_positions -> volume_shift on
the fixture of jittered sections.  Everything is integers, so every comparison is exact.  The kernel reads blocks
between guards of fill bytes and adds into sums between guards of fill words; block and guards must come back
untouched.  Guards and data are those of test_gpu_zcorr.py, the launch counter that of test_gpu_histogram.py."""
import functools

import numpy as np
import pytest
import torch

import zshift_ref as SR
from test_gpu_histogram import _counted, _env
from test_gpu_zcorr import DATA, FILL, GUARD, SFILL, SGUARD, TILES, _data

pytestmark = pytest.mark.gpu

BLOCKS = [(1, 5, 7), (3, 5, 7), (3, 33, 70), (2, 64, 257)]
RADII = [1, 4, 8]
MODES = ["whole", "inside", "bottom"]


def _geometry(shape, tile, r, mode):
    """(r0, r1, y_org, Y, gy, gx) of a block [D, H, W] and its core rows, with exactly the halo the contract demands:
      whole   the block is the section: rows [0, H) at y_org = 0, Y = H -- partners miss at all four faces
      inside  the block sits off the tile grid at y_org > 0 in a taller section: core rows [r, H - r), empty for H <= 2 r
      bottom  the same y_org, the block ends with the section: core rows [r, H)
    The grid is one tile larger than the section needs, so that some rows of sums stay untouched."""
    (D, H, W), (th, tw) = shape, tile
    if mode == "whole":
        r0, r1, y_org, Y = 0, H, 0, H
    else:
        y_org = th + th // 3 if th > 1 else 1
        Y = y_org + H + (th // 2 + 1 if mode == "inside" else 0)
        r0 = min(r, H)
        r1 = max(H - r, r0) if mode == "inside" else H
    return r0, r1, y_org, Y, -(-Y // th) + 1, -(-W // tw) + 1


@functools.lru_cache(maxsize=4)
def _want(shape, kind, tile, r, mode):
    """The reference sums of every plane of the block over the mode's core rows: the core [c0, c1) takes rows
    c0...c1 - 1 of it."""
    geo = _geometry(shape, tile, r, mode)
    want = SR.tile_sums(_data(shape, kind), 0, shape[0], *geo[:4], *tile, *geo[4:], r)
    want.setflags(write=False)
    return want


class _Sums:
    """Device sums [planes, gy, gx, R, R, 5] between guards of SFILL, cleared once."""

    def __init__(self, planes, gy, gx, r):
        R = 2 * r + 1
        self.shape, self.sec = (planes, gy, gx, R, R, 5), gy * gx * R * R * 5
        self.n = planes * self.sec
        self.t = torch.full((self.n + 2 * SGUARD,), SFILL, dtype=torch.int64, device="cuda")
        self.t[SGUARD:SGUARD + self.n] = 0

    def ptr(self, plane=0):
        return self.t.data_ptr() + 8 * (SGUARD + plane * self.sec)

    def result(self):
        got = self.t.cpu().numpy()
        assert (got[:SGUARD] == SFILL).all() and (got[SGUARD + self.n:] == SFILL).all()
        return got[SGUARD:SGUARD + self.n].reshape(self.shape)


def _launch(block, c0, c1, geo, tile, r, sums_ptr, off=0):
    """One tem_u8_zshift_tiles call on `block`, `off` bytes into an aligned allocation between guards of FILL; block
    and guards must be untouched."""
    L, lib, stream = _env()
    r0, r1, y_org, Y, gy, gx = geo
    flat = np.ascontiguousarray(block).reshape(-1)
    t = torch.full((flat.size + off + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    t[GUARD + off:GUARD + off + flat.size] = torch.from_numpy(flat.copy()).cuda()
    L.check(lib.tem_u8_zshift_tiles(t.data_ptr() + GUARD + off, *block.shape, c0, c1, r0, r1, y_org, Y, *tile, gy, gx, r,
                                    sums_ptr, stream), "tem_u8_zshift_tiles")
    got = t.cpu().numpy()
    assert (got[:GUARD + off] == FILL).all() and (got[GUARD + off + flat.size:] == FILL).all()
    assert np.array_equal(got[GUARD + off:GUARD + off + flat.size], flat)


def _run(block, c0, c1, geo, tile, r, off=0):
    s = _Sums(max(c1 - c0, 1), geo[4], geo[5], r)
    _launch(block, c0, c1, geo, tile, r, s.ptr(), off)
    return s.result()[:c1 - c0]


# ---------------------------------------------------------------------------------------------- tem_u8_zshift_tiles
def _variants(shape, tile, r):
    """(kind, mode, core, byte offsets).  Random data: every mode; the whole block as the core at byte offsets 0...3
    where the block is the section, 0 and 3 elsewhere; the other cores ([0, D - 1): the last plane is halo only; [1, 2);
    an empty one) at offsets 0 and 3.  The other kinds of data: every mode, the whole core, offset 0.  Where one plane
    of sums passes 2^20 entries (1 x 1 tiles of the large blocks) the list is the whole core of random data at the
    section's faces and inside, and all-255 at the faces."""
    D = shape[0]
    entries = max(_geometry(shape, tile, r, m)[4] * _geometry(shape, tile, r, m)[5] for m in MODES) * (2 * r + 1) ** 2 * 5
    if entries > 1 << 20:
        return [("random", "whole", (0, D), (0,)), ("random", "inside", (0, D), (1,)), ("ones", "whole", (0, D), (2,))]
    out = []
    for mode in MODES:
        out.append(("random", mode, (0, D), (0, 1, 2, 3) if mode == "whole" else (0, 3)))
        out += [("random", mode, core, (0, 3)) for core in ((0, D - 1), (min(1, D), min(2, D)), (D, D))]
        out += [(kind, mode, (0, D), (0,)) for kind in DATA if kind != "random"]
    return out


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("tile", TILES, ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("shape", BLOCKS, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_reference(shape, tile, r):
    for kind, mode, (c0, c1), offs in _variants(shape, tile, r):
        geo = _geometry(shape, tile, r, mode)
        want = _want(shape, kind, tile, r, mode)[c0:c1]
        for off in offs:
            got = _run(_data(shape, kind), c0, c1, geo, tile, r, off)
            assert got.shape == want.shape and np.array_equal(got, want), \
                (kind, mode, c0, c1, off, np.argwhere(got != want)[:5])


def test_kernel_cases_cover_what_they_claim():
    """The off-grid blocks cut tiles above and below, core rows cut through tiles, a radius is larger than a block,
    the last plane has no sums, and the sums at the faces are those of fewer voxels."""
    for shape, tile, r in (((3, 33, 70), (32, 32), 4), ((2, 64, 257), (7, 64), 8), ((3, 33, 70), (3, 5), 1)):
        for mode in ("inside", "bottom"):
            r0, r1, y_org, Y, gy, gx = _geometry(shape, tile, r, mode)
            assert y_org % tile[0] and (y_org + r0) % tile[0] and r0 == r and r1 == shape[1] - (r if mode == "inside" else 0)
            assert (Y > y_org + shape[1]) == (mode == "inside")
            want = _want(shape, "random", tile, r, mode)
            assert want[:-1].any(axis=(1, 2, 3, 4, 5)).all() and not want[-1].any()
            assert not want[:, -1].any() and not want[:, :, -1].any()              # the grid's spare row and column
    assert _geometry((3, 5, 7), (3, 5), 8, "inside")[:2] == (5, 5)                 # r = 8 in a 5 x 7 block: no core inside,
    assert _geometry((3, 5, 7), (3, 5), 8, "whole")[:2] == (0, 5)                  # all of it as the whole section
    w = _want((3, 5, 7), "ones", (2048, 2048), 8, "whole")[0, 0, 0]
    assert w[8, 8].tolist() == [35 * 255, 35 * 65025, 35 * 255, 35 * 65025, 35 * 65025]
    assert w[4, 2].tolist() == [v * 1 for v in (255, 65025, 255, 65025, 65025)]   # dy = -4, dx = -6: one voxel is left
    assert not w[:3].any() and not w[:, 0].any()                                   # |dy| >= 5, |dx| >= 7: none
    n = SR.counts((5, 7), (2048, 2048), 8)[0, 0]
    assert np.array_equal(w[..., 0], 255 * n)


LONG_SHAPE, LONG_TILE, LONG_R = (4, 141, 333), (100, 144), 8


def test_kernel_fills_whole_workgroups_on_several_planes():
    """The shape of a real call at the largest radius: tiles of 100 x 144 go to workgroups of 32 x 128 voxels -- the
    most one takes: all four waves with eight rows each, all five passes over the 289 offsets -- and to narrow and
    short rests, 32 x 16 and 4 x 128; the plane stride is odd and W no multiple of 4, so a row's alignment changes from
    row to row and plane to plane; three core planes, the fourth as halo; the block off the grid inside its section,
    and as the whole section."""
    D, H, W = LONG_SHAPE
    assert (H * W) % 2 == 1 and W % 4 == 1
    block = _data(LONG_SHAPE, "random")
    for mode, c0, c1, off in (("inside", 0, D - 1, 1), ("whole", 1, D, 0)):
        geo = _geometry(LONG_SHAPE, LONG_TILE, LONG_R, mode)
        want = _want(LONG_SHAPE, "random", LONG_TILE, LONG_R, mode)
        got = _run(block, c0, c1, geo, LONG_TILE, LONG_R, off)
        assert np.array_equal(got, want[c0:c1]), (mode, np.argwhere(got != want[c0:c1])[:5])


def test_kernel_accumulates_across_cuts():
    """One launch equals two launches on core rows cut through a tile, two launches on blocks cut along y that hold
    just their halo rows, and two launches cut along z with the lower half given its halo plane."""
    shape, tile, r = (4, 33, 70), (32, 32), 4
    block = _data(shape, "random")
    r0, r1, y_org, Y, gy, gx = geo = _geometry(shape, tile, r, "whole")
    want = _want(shape, "random", tile, r, "whole")
    for off in (0, 1):
        s = _Sums(4, gy, gx, r)                                                     # core rows [0, 17) | [17, 33)
        _launch(block, 0, 4, (0, 17) + geo[2:], tile, r, s.ptr(), off)
        _launch(block, 0, 4, (17, 33) + geo[2:], tile, r, s.ptr(), off)
        assert np.array_equal(s.result(), want)
        s = _Sums(4, gy, gx, r)                                                     # blocks of rows [0, 21) | [13, 33)
        _launch(block[:, :21], 0, 4, (0, 17, 0, Y, gy, gx), tile, r, s.ptr(), off)
        _launch(block[:, 13:], 0, 4, (4, 20, 13, Y, gy, gx), tile, r, s.ptr(), off)
        assert np.array_equal(s.result(), want)
        s = _Sums(4, gy, gx, r)                                                     # planes [0, 2) + halo | [2, 4)
        _launch(block[:3], 0, 2, geo, tile, r, s.ptr(0), off)
        _launch(block[2:], 0, 2, geo, tile, r, s.ptr(2), off)
        assert np.array_equal(s.result(), want)
    s = _Sums(4, gy, gx, r)                                                         # the same launch twice: it ADDS
    for _ in range(2):
        _launch(block, 0, 4, geo, tile, r, s.ptr())
    assert np.array_equal(s.result(), 2 * want)


def test_kernel_holds_the_largest_tile_of_the_largest_values():
    """Two planes of 2048 x 2048 voxels of 255 in one tile at r = 1: 2047 x 2047 x 65025 and more per entry, far past
    32 bits, against the closed form."""
    block = np.full((2, 2048, 2048), 255, np.uint8)
    got = _run(block, 0, 2, (0, 2048, 0, 2048, 1, 1), (2048, 2048), 1)
    assert not got[1].any()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            n = (2048 - abs(dy)) * (2048 - abs(dx))
            assert n * 65025 > 2 ** 32
            assert got[0, 0, 0, dy + 1, dx + 1].tolist() == [255 * n, 65025 * n, 255 * n, 65025 * n, 65025 * n]


def test_kernel_refuses_bad_arguments():
    """TEM_EINVAL from the host-side checks, nothing launched: sums keeps its fill."""
    L, lib, stream = _env()
    src = torch.ones(4 * 6 * 8 + 16, dtype=torch.uint8, device="cuda")
    sums = torch.full((4 * 2 * 2 * 125 + 1,), SFILL, dtype=torch.int64, device="cuda")
    p, s = src.data_ptr(), sums.data_ptr()
    call = lambda *a: lib.tem_u8_zshift_tiles(*a, stream)
    # src D H W c0 c1 r0 r1 y_org Y th tw gy gx radius sums
    ok = [p, 4, 6, 8, 0, 4, 0, 6, 0, 6, 4, 4, 2, 2, 2, s]
    for i, v in [(0, None), (15, None), (15, s + 4), (15, s + 1), (1, 0), (2, 0), (3, 0), (1, -1), (9, 0), (12, 0),
                 (13, 0), (12, -1), (10, 0), (10, 2049), (11, 0), (11, 2049), (14, 0), (14, 9), (14, -1), (8, -1),
                 (12, 1), (13, 1), (9, 5), (8, 1), (4, -1), (5, 5), (4, 3), (6, -1), (7, 7), (6, 4)]:
        a = list(ok)
        a[i] = v
        if (i, v) == (4, 3):
            a[5] = 2                                                                # c0 > c1
        if (i, v) == (6, 4):
            a[7] = 3                                                                # r0 > r1
        assert call(*a) == L.TEM_EINVAL, (i, v)
    inside = [p, 4, 6, 8, 0, 4, 2, 4, 2, 12, 4, 4, 3, 2, 2, s]                      # rows 2...7 of 12: the core needs
    for r0, r1 in ((1, 4), (2, 5), (0, 6)):                                         # 2 rows of halo on each side
        assert call(*inside[:6], r0, r1, *inside[8:]) == L.TEM_EINVAL, (r0, r1)
    assert call(*ok[:4], 2, 2, *ok[6:]) == 0 and call(*ok[:6], 3, 3, *ok[8:]) == 0  # an empty core launches nothing
    assert call(*ok[:4], 3, 4, *ok[6:]) == 0                                        # as does the last plane alone
    # more workgroups than one launch holds: 16 tiles x 2^31 - 2 planes (refused before anything is touched)
    assert call(p, 2 ** 31 - 1, 4, 4, 0, 2 ** 31 - 1, 0, 4, 0, 4, 1, 1, 4, 4, 1, s) == L.TEM_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (sums.cpu().numpy() == SFILL).all()
    sums.zero_()
    assert call(*ok) == 0 and call(p + 3, *ok[1:]) == 0                             # and the good call runs
    torch.cuda.synchronize()
    got = sums.cpu().numpy()[:2000].reshape(4, 2, 2, 5, 5, 5)
    assert got[:3, ..., 2, 2, 0].sum() == 2 * 3 * 6 * 8 and not got[3].any()       # three planes have one above them
    sums2 = torch.zeros(4 * 3 * 2 * 125, dtype=torch.int64, device="cuda")
    assert call(*inside[:15], sums2.data_ptr()) == 0                                # as does the one with its halo
    torch.cuda.synchronize()
    assert sums2.cpu().numpy().reshape(4, 3, 2, 5, 5, 5)[:3, ..., 2, 2, 0].sum() == 3 * 2 * 8


# ----------------------------------------------------------------------------------------------- section_shift_sums
VSHAPE, VTILE, VR = (12, 50, 70), (16, 24), 2
BUDGETS = {"whole": 12 * 50 * 70, "three_sections": 3 * 50 * 70, "ten_rows": 2 * 14 * 70, "one_row": 70}


@functools.lru_cache(maxsize=None)
def _vcase():
    vol = np.random.default_rng(17).integers(0, 256, VSHAPE, dtype=np.uint8)
    vol[1::2] = vol[1::2] // 2 + vol[:-1:2] // 2                                   # neighbours correlate
    want = SR.volume_sums(vol, VTILE, VR)
    vol.setflags(write=False), want.setflags(write=False)
    return vol, want


@pytest.fixture(scope="module")
def vmap(tmp_path_factory):
    path = tmp_path_factory.mktemp("zshift") / "vol.u8"
    m = np.memmap(path, np.uint8, "w+", shape=VSHAPE)
    m[...] = _vcase()[0]
    m.flush()
    return np.memmap(path, np.uint8, "r", shape=VSHAPE)


@pytest.mark.parametrize("budget", list(BUDGETS), ids=list(BUDGETS))
def test_section_shift_sums_equals_the_reference_however_it_is_cut(vmap, budget):
    from transfer_em_amd.utils import section_shift_sums, zshift_chunks
    want = _vcase()[1]
    st = {}
    got, counts = _counted(lambda: section_shift_sums(vmap, VTILE, VR, chunk_bytes=BUDGETS[budget], stats=st))
    assert got.dtype == np.int64 and got.shape == (12, 4, 3, 5, 5, 5) and np.array_equal(got, want)
    assert not got[-1].any() and got[:-1].any(axis=(1, 2, 3, 4, 5)).all()
    n = len(zshift_chunks(VSHAPE, VR, BUDGETS[budget]))
    assert st["chunks"] == n and st["read_s"] >= 0
    assert counts["tem_u8_zshift_tiles"] == n                                       # one launch per slab
    assert {"whole": n == 2, "three_sections": n == 6, "ten_rows": n == 12 * 5, "one_row": n == 12 * 50}[budget]
    assert np.array_equal(np.asarray(vmap), _vcase()[0])                            # the input: read only


def test_section_shift_sums_default_slab_ranks_and_the_per_slab_read_back(vmap, monkeypatch):
    from transfer_em_amd import utils
    vol, want = _vcase()
    assert np.array_equal(utils.section_shift_sums(vol, VTILE, VR), want)           # an ndarray, one slab
    parts = [utils.section_shift_sums(vmap, VTILE, VR, chunk_bytes=BUDGETS["three_sections"], rank=r, world_size=2)
             for r in (1, 0)]
    assert parts[0].any() and parts[1].any() and not np.array_equal(parts[0], want)
    assert np.array_equal(parts[0] + parts[1], want)                                # the ranks' results add
    monkeypatch.setattr(utils, "CLAHE_ACC_BYTES", 12 * 4 * 3 * 25 * 40 - 1)         # the accumulator no longer fits
    for budget in ("three_sections", "ten_rows"):
        got, counts = _counted(lambda: utils.section_shift_sums(vmap, VTILE, VR, chunk_bytes=BUDGETS[budget]))
        assert np.array_equal(got, want)
        assert counts["tem_u8_zshift_tiles"] == len(utils.zshift_chunks(VSHAPE, VR, BUDGETS[budget]))
    both = [utils.section_shift_sums(vmap, VTILE, VR, chunk_bytes=BUDGETS["ten_rows"], rank=r, world_size=2)
            for r in (0, 1)]
    assert np.array_equal(both[0] + both[1], want)


def test_section_shift_sums_of_one_image_an_int_tile_and_the_default_radius():
    from transfer_em_amd.utils import section_shift_sums
    vol = _vcase()[0]
    got = section_shift_sums(vol[3], 16)
    assert got.dtype == np.int64 and got.shape == (1, 4, 5, 9, 9, 5) and not got.any()
    got = section_shift_sums(vol[:2], 16)
    assert np.array_equal(got, SR.volume_sums(vol[:2], (16, 16), 4)) and got[0].any()


# ------------------------------------------------------------------------------------------------------- end to end
def test_the_jitter_is_measured_and_undone():
    from transfer_em_amd.utils import section_shift_sums, section_shifts, shift_counts, shift_positions, volume_shift
    v = SR.jitter_volume()
    q = section_shift_sums(v, SR.FIX_TILE, SR.FIX_RADIUS, chunk_bytes=5 * 90 * 120)
    assert np.array_equal(q, SR.fixture_sums())
    n = shift_counts(v.shape, SR.FIX_TILE, SR.FIX_RADIUS)
    got, want = section_shifts(q, n), section_shifts(SR.fixture_sums(), n)
    for a, b in zip(got[:4], want[:4]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert got.unresolved == want.unresolved == sorted(SR.FIX_PLANTED)
    pairs = SR.fixture_pairs()
    ordinary = [z for z in range(23) if z not in SR.FIX_PLANTED]
    assert np.array_equal(got.pairs[ordinary], pairs[ordinary])
    P = shift_positions(got.pairs)
    assert np.array_equal(P, shift_positions(want.pairs))
    moved = volume_shift(v, P)
    assert moved.tobytes() == volume_shift(v, shift_positions(want.pairs)).tobytes()    # byte for byte
    assert np.array_equal(moved[:8, 10:80, 10:110], SR.flat_volume()[:8, 10:80, 10:110])  # up to the first planted pair
