"""The in-plane lag sums on the device: tem_u8_zplane_lags against the numpy reference (zplane_ref),
section_plane_sums out of core on the fixture with planted blur and a planted pitch, and the verdict, the pitch and the
repair on the device's sums.  Everything is integers, so every comparison is exact.  The kernel reads blocks between
guards of fill bytes and adds into sums between guards of fill words; block and guards must come back untouched.
Helpers are those of test_gpu_histogram.py and test_gpu_zlags.py."""
import functools

import numpy as np
import pytest
import torch

import zplane_ref as PR
import zspace_ref as ZS
from test_gpu_histogram import _counted, _env
from test_gpu_zlags import SFILL, SGUARD, _Block, _data

pytestmark = pytest.mark.gpu

BLOCKS = [(1, 5, 7), (3, 5, 7), (4, 33, 70), (2, 64, 257)]
TILES = [(1, 1), (3, 5), (7, 64), (32, 32), (2048, 2048)]
DATA = ["random", "zeros", "ones", "alternating"]
LAGS = [1, 2, 5, 8]
MORE = 3                                                                            # rows of the section past a "mid" block


class _Sums:
    """Device sums [planes, gy, gx, 3 + 2 nlag] between guards of SFILL, cleared once."""

    def __init__(self, planes, gy, gx, nlag):
        self.shape, self.sec = (planes, gy, gx, 3 + 2 * nlag), gy * gx * (3 + 2 * nlag)
        self.n = planes * self.sec
        self.t = torch.full((self.n + 2 * SGUARD,), SFILL, dtype=torch.int64, device="cuda")
        self.t[SGUARD:SGUARD + self.n] = 0

    def ptr(self, plane=0):
        return self.t.data_ptr() + 8 * (SGUARD + plane * self.sec)

    def result(self):
        got = self.t.cpu().numpy()
        assert (got[:SGUARD] == SFILL).all() and (got[SGUARD + self.n:] == SFILL).all()
        return got[SGUARD:SGUARD + self.n].reshape(self.shape)


def _geometry(shape, tile, on_grid, last):
    """(y_org, Y, gy, gx): the block's row 0 on the tile grid or off it, so that the block cuts tiles above and below;
    the block holds the section's last rows (`last`) or the section goes on for MORE rows.  The grid is one tile larger
    than the section needs, so that some rows of sums stay untouched."""
    (D, H, W), (th, tw) = shape, tile
    y_org = 0 if on_grid else th + th // 3
    Y = y_org + H + (0 if last else MORE)
    return y_org, Y, -(-Y // th) + 1, -(-W // tw) + 1


@functools.lru_cache(maxsize=None)
def _want(shape, kind, tile, on_grid, last, core, nlag):
    """The reference sums of every plane of the block's core rows, computed once."""
    y_org, Y, gy, gx = _geometry(shape, tile, on_grid, last)
    ref = PR.plane_tile_sums if tile[0] * tile[1] >= 100 else PR.plane_tile_sums_fast  # many small tiles: without loops
    want = ref(_data(shape, kind), 0, shape[0], core[0], core[1], y_org, Y, *tile, gy, gx, nlag)
    want.setflags(write=False)
    return want


def _launch(dev, c0, c1, r0, r1, y_org, Y, tile, gy, gx, nlag, sums_ptr):
    L, lib, stream = _env()
    L.check(lib.tem_u8_zplane_lags(dev.ptr, *dev.shape, c0, c1, r0, r1, y_org, Y, *tile, gy, gx, nlag, sums_ptr, stream),
            "tem_u8_zplane_lags")


def _run(dev, c0, c1, r0, r1, y_org, Y, tile, gy, gx, nlag):
    s = _Sums(max(c1 - c0, 1), gy, gx, nlag)
    _launch(dev, c0, c1, r0, r1, y_org, Y, tile, gy, gx, nlag, s.ptr())
    return s.result()[:c1 - c0]


def _row_cores(H, nlag, last):
    """The cores of rows of a block of H rows: the whole block and its lower half where it holds the section's last
    rows (no partner rows past it); else rows whose nlag halo rows the block holds; and an empty one."""
    if last:
        return [(0, H), (H // 2, H), (2, 2)]
    top = max(H - nlag, 0)
    return [(0, top), (min(1, top), top), (min(2, H), min(2, H))]


# ----------------------------------------------------------------------------------------------- tem_u8_zplane_lags
@pytest.mark.parametrize("tile", TILES, ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("shape", BLOCKS, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_reference(shape, tile):
    """Every kind of data, y_org on the tile grid and off it, the block at the section's last rows and in its middle,
    1, 2, 5 and 8 lags -- k & 3 = 0...3, k >> 2 = 0, 1, 2, more than the 5 rows and the 7 columns --, cores of rows with
    their halo in the block and without one at the section's end, cores of planes, empty cores, byte offsets 0...3 for
    the whole core and 0 and 3 for the others."""
    D, H, W = shape
    for kind in DATA:
        block = _data(shape, kind)
        devs = [_Block(block, off) for off in range(4)]
        flat = kind in ("zeros", "ones")                                            # constant bytes: fewer combinations
        for on_grid in (True, False):
            for last in (True,) if flat else (True, False):
                y_org, Y, gy, gx = _geometry(shape, tile, on_grid, last)
                for nlag in (2, 8) if flat else LAGS:
                    for n, rows in enumerate(_row_cores(H, nlag, last)):
                        want = _want(shape, kind, tile, on_grid, last, rows, nlag)
                        assert int(want[..., 2].sum()) == D * (rows[1] - rows[0]) * W   # every voxel in exactly one tile
                        for c0, c1 in ((0, D), (min(1, D), min(2, D)), (D, D)) if n == 0 else ((0, D),):
                            for off in ((0, 1, 2, 3) if (n, c0, c1) == (0, 0, D) else (0, 3)):
                                got = _run(devs[off], c0, c1, *rows, y_org, Y, tile, gy, gx, nlag)
                                assert got.shape == want[c0:c1].shape and np.array_equal(got, want[c0:c1]), \
                                    (kind, on_grid, last, nlag, rows, c0, c1, off, np.argwhere(got != want[c0:c1])[:5])
        for dev in devs:
            dev.check()


def test_kernel_cases_cover_what_they_claim():
    """The off-grid blocks cut tiles above and below; a y lag has pairs exactly where the section has the partner
    row and an x lag where it has the partner column; alternating bytes make odd x lags maximal and even ones zero;
    the columns are in the documented order."""
    for shape, tile in (((4, 33, 70), (32, 32)), ((2, 64, 257), (7, 64)), ((2, 64, 257), (3, 5))):
        y_org, Y, gy, gx = _geometry(shape, tile, False, True)
        assert y_org % tile[0] and Y % tile[0] and shape[2] % tile[1]
        want = _want(shape, "random", tile, False, True, (0, shape[1]), 8)
        assert not want[:, -1].any() and not want[:, :, -1].any()                  # the grid's spare row and column
        assert (want[..., 3:].sum(axis=(0, 1, 2)) > 0).all()                        # more rows and columns than lags: all have pairs
    small = _want((1, 5, 7), "random", (2048, 2048), True, True, (0, 5), 8)[0, 0, 0]
    assert (small[3:] > 0).tolist() == [k < 5 for k in range(1, 9)] + [k < 7 for k in range(1, 9)]
    mid = _want((4, 33, 70), "random", (2048, 2048), True, False, (0, 25), 8)[0, 0, 0]   # its 8 halo rows in the block
    assert (mid[3:] > 0).all() and _row_cores(33, 8, False)[0] == (0, 25)
    assert _want((1, 5, 7), "ones", (3, 5), True, True, (0, 5), 8)[0, 0, 0].tolist() == [15 * 255, 15 * 65025, 15] + [0] * 16
    alt = _want((2, 64, 257), "alternating", (2048, 2048), True, True, (0, 64), 8)[0, 0, 0]   # W odd: rows alternate too
    assert alt[3:11].tolist() == [65025 * (64 - k) * 257 * (k % 2) for k in range(1, 9)]
    assert alt[11:].tolist() == [65025 * 64 * (257 - k) * (k % 2) for k in range(1, 9)]


WIDE_SHAPE, WIDE_TILES = (5, 40, 1101), [(2048, 2048), (24, 1030), (16, 128)]


@pytest.mark.parametrize("tile", WIDE_TILES, ids=lambda t: "x".join(map(str, t)))
def test_kernel_marches_full_waves(tile):
    """The shape of a real call: rows of more than 64 pieces, so a tile is cut into column chunks of 1024 (a second
    chunk of 77 or 6 columns); runs of 16 rows behind a full ring, three row parts per tile; five planes, so the second
    workgroup of a part has one wave; W no multiple of 4 at byte offset 1, so a piece's alignment changes from row to
    row; whole pieces everywhere but at the tiles' and the section's right edge.  (16, 128): one wave is 8 pieces x 8
    runs of 2 rows, the ring's halo longer than the run."""
    D, H, W = WIDE_SHAPE
    assert W % 4 and W > 1024 + 64
    block = _data(WIDE_SHAPE, "random")
    dev = _Block(block, 1)
    for on_grid, last in ((True, True), (False, False)):
        y_org, Y, gy, gx = _geometry(WIDE_SHAPE, tile, on_grid, last)
        for nlag in (1, 4, 8):
            rows = (0, H) if last else (3, H - nlag)
            want = PR.plane_tile_sums_fast(block, 0, D, *rows, y_org, Y, *tile, gy, gx, nlag)
            got = _run(dev, 0, D, *rows, y_org, Y, tile, gy, gx, nlag)
            assert np.array_equal(got, want), (on_grid, last, nlag, np.argwhere(got != want)[:5])
    dev.check()


def test_kernel_accumulates_across_cuts():
    """One launch equals two launches on blocks that cut a tile along y between them -- the upper one holds the lower
    one's first rows as its halo -- and two launches cut along z; the same launch twice ADDS."""
    shape, tile = (2, 64, 257), (32, 32)
    block = _data(shape, "random")
    y_org, Y, gy, gx = _geometry(shape, tile, False, True)
    for nlag, off in ((1, 0), (5, 1), (8, 3)):
        want = _want(shape, "random", tile, False, True, (0, 64), nlag)
        s = _Sums(2, gy, gx, nlag)                                                  # rows [0, 17) + halo | [17, 64)
        _launch(_Block(block[:, :17 + nlag], off), 0, 2, 0, 17, y_org, Y, tile, gy, gx, nlag, s.ptr())
        _launch(_Block(block[:, 17:], off), 0, 2, 0, 47, y_org + 17, Y, tile, gy, gx, nlag, s.ptr())
        assert np.array_equal(s.result(), want)
        s = _Sums(2, gy, gx, nlag)                                                  # the same cut as cores of one block
        dev = _Block(block, off)
        _launch(dev, 0, 2, 0, 17, y_org, Y, tile, gy, gx, nlag, s.ptr())
        _launch(dev, 0, 2, 17, 64, y_org, Y, tile, gy, gx, nlag, s.ptr())
        assert np.array_equal(s.result(), want)
        s = _Sums(2, gy, gx, nlag)                                                  # planes [0, 1) | [1, 2): no halo along z
        _launch(_Block(block[:1], off), 0, 1, 0, 64, y_org, Y, tile, gy, gx, nlag, s.ptr(0))
        _launch(_Block(block[1:], off), 0, 1, 0, 64, y_org, Y, tile, gy, gx, nlag, s.ptr(1))
        assert np.array_equal(s.result(), want)
    s = _Sums(2, gy, gx, 2)
    for _ in range(2):
        _launch(dev, 0, 2, 0, 64, y_org, Y, tile, gy, gx, 2, s.ptr())
    assert np.array_equal(s.result(), 2 * _want(shape, "random", tile, False, True, (0, 64), 2))
    dev.check()


def test_kernel_holds_the_largest_tile_of_the_largest_differences():
    """One plane of 2048 x 2048 voxels in one tile whose columns alternate between 0 and 255: every pair of an odd x
    lag differs by 255, 2048 x (2048 - k) x 65025 per lag, far past 32 bits; the y lags and the even x lags are 0."""
    a = np.zeros((1, 2048, 2048), np.uint8)
    a[:, :, 1::2] = 255
    dev = _Block(a)
    n = 2048 * 2048
    assert 2048 * 2047 * 65025 > 2 ** 37
    for nlag in (1, 8):
        got = _run(dev, 0, 1, 0, 2048, 0, 2048, (2048, 2048), 1, 1, nlag)[0, 0, 0].tolist()
        assert got == [255 * n // 2, 65025 * n // 2, n] + [0] * nlag + [2048 * (2048 - k) * 65025 * (k % 2)
                                                                        for k in range(1, nlag + 1)]


def test_kernel_refuses_bad_arguments():
    """TEM_EINVAL from the host-side checks, nothing launched: sums keeps its fill and the block its bytes."""
    L, lib, stream = _env()
    dev = _Block(_data((4, 6, 8), "random"), 1)
    sums = torch.full((4 * 3 * 2 * 19 + 1,), SFILL, dtype=torch.int64, device="cuda")
    p, s = dev.ptr, sums.data_ptr()
    call = lambda *a: lib.tem_u8_zplane_lags(*a, stream)
    # src D H W c0 c1 r0 r1 y_org Y th tw gy gx nlag sums: rows 2...7 of a section of 10 rows, tiles of 4 x 4
    ok = [p, 4, 6, 8, 0, 4, 0, 4, 2, 10, 4, 4, 3, 2, 2, s]
    for i, v in [(0, None), (15, None), (15, s + 4), (15, s + 1), (1, 0), (2, 0), (3, 0), (1, -1), (9, 0), (12, 0),
                 (13, 0), (12, -1), (10, 0), (10, 2049), (11, 0), (11, 2049), (8, -1), (9, 7), (12, 2), (13, 1),
                 (4, -1), (5, 5), (4, 3), (6, -1), (7, 7), (6, 5), (14, 0), (14, 9), (14, -1),
                 (7, 5), (14, 3)]:                 # the last two: rows [0, 5) + 2 and [0, 4) + 3 need row 6, which exists
        a = list(ok)
        a[i] = v
        if (i, v) == (4, 3):
            a[5] = 2                                                                # c0 > c1
        if (i, v) == (6, 5):
            a[7] = 4                                                                # r0 > r1
        assert call(*a) == L.TEM_EINVAL, (i, v)
    assert call(*ok[:4], 2, 2, *ok[6:]) == 0 and call(*ok[:6], 3, 3, *ok[8:]) == 0    # an empty core launches nothing
    # more workgroups than one launch holds: 16 tiles x 2^29 groups of four planes is past 2^24
    assert call(p, 2 ** 31 - 1, 4, 4, 0, 2 ** 31 - 1, 0, 4, 0, 4, 1, 1, 4, 4, 1, s) == L.TEM_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (sums.cpu().numpy() == SFILL).all()
    dev.check()
    sums.zero_()
    assert call(*ok) == 0                                                           # and the good call runs
    last = list(ok)
    last[7], last[8] = 6, 4                                                         # rows 4...9: the section's last rows
    assert call(*last) == 0
    torch.cuda.synchronize()
    assert sums.cpu().numpy()[:4 * 3 * 2 * 7].reshape(4, 3, 2, 7)[..., 2].sum() == 4 * 4 * 8 + 4 * 6 * 8
    dev.check()


# ----------------------------------------------------------------------------------------------- section_plane_sums
Z, Y, X = PR.FIX_SHAPE
VTILE = (PR.FIX_TILE, PR.FIX_TILE)
BUDGETS = {"whole": Z * Y * X, "five_sections": 5 * Y * X, "rows": 40 * X}


@pytest.fixture(scope="module")
def vmap(tmp_path_factory):
    path = tmp_path_factory.mktemp("zplane") / "vol.u8"
    m = np.memmap(path, np.uint8, "w+", shape=PR.FIX_SHAPE)
    m[...] = PR.fixture().volume
    m.flush()
    return np.memmap(path, np.uint8, "r", shape=PR.FIX_SHAPE)


@pytest.mark.parametrize("budget", list(BUDGETS), ids=list(BUDGETS))
def test_section_plane_sums_equals_the_reference_however_it_is_cut(vmap, budget):
    from transfer_em_amd.utils import plane_lag_chunks, section_plane_sums
    want = PR.fixture_sums()
    st = {}
    got, counts = _counted(lambda: section_plane_sums(vmap, VTILE, PR.FIX_LAGS, chunk_bytes=BUDGETS[budget], stats=st))
    assert got.dtype == np.int64 and got.shape == (Z, 2, 3, 19) and np.array_equal(got, want)
    chunks = plane_lag_chunks(PR.FIX_SHAPE, PR.FIX_LAGS, BUDGETS[budget])
    assert st["chunks"] == len(chunks) == counts["tem_u8_zplane_lags"]             # one launch per slab
    assert {"whole": len(chunks) == 1, "five_sections": len(chunks) == 5, "rows": len(chunks) == Z * 4}[budget]
    if budget == "rows":
        assert [c[1] for c, _ in chunks[:4]] == [(0, 32), (32, 64), (64, 96), (96, 128)]   # row cuts through the tiles
        assert [r[1] for _, r in chunks[:4]] == [(0, 40), (32, 72), (64, 104), (96, 128)]  # with their halo
    assert np.array_equal(np.asarray(vmap), PR.fixture().volume)                    # the input: read only


def test_section_plane_sums_ranks_other_lags_and_the_per_slab_read_back(vmap, monkeypatch):
    from transfer_em_amd import utils
    vol, want = PR.fixture().volume, PR.fixture_sums()
    assert np.array_equal(utils.section_plane_sums(vol, PR.FIX_TILE), want)         # an ndarray, one slab, the defaults
    parts = [utils.section_plane_sums(vmap, VTILE, 8, chunk_bytes=BUDGETS["rows"], rank=r, world_size=2) for r in (1, 0)]
    assert parts[0].any() and parts[1].any() and not np.array_equal(parts[0], want)
    assert np.array_equal(parts[0] + parts[1], want)                                # the ranks' results add
    for L, tile in ((1, (64, 64)), (3, (50, 70))):
        got = utils.section_plane_sums(vmap, tile, L, chunk_bytes=(L + 20) * X)
        assert np.array_equal(got, PR.volume_plane_sums(vol, tile, L))
    one = utils.section_plane_sums(vol[3], VTILE, 2)                                # one image [y, x]: Z = 1
    assert one.shape == (1, 2, 3, 7) and np.array_equal(one, PR.volume_plane_sums(vol[3:4], VTILE, 2))
    monkeypatch.setattr(utils, "CLAHE_ACC_BYTES", Z * 6 * 19 * 8 - 1)               # the accumulator no longer fits
    for budget in ("five_sections", "rows"):
        got, counts = _counted(lambda: utils.section_plane_sums(vmap, VTILE, 8, chunk_bytes=BUDGETS[budget]))
        assert np.array_equal(got, want)
        assert counts["tem_u8_zplane_lags"] == len(utils.plane_lag_chunks(PR.FIX_SHAPE, 8, BUDGETS[budget]))


def test_the_verdict_the_pitch_and_the_repair_on_the_device_sums(vmap):
    """The device's verdict and pitch are the reference's, bit for bit; after volume_repair with the Repair of the joined
    verdict (find_defects' and find_blurred's) the planted sections and the planted tile re-measure a relative g above
    the ratio, and nothing is flagged."""
    from transfer_em_amd import utils as U
    fx = PR.fixture()
    s = U.section_plane_sums(vmap, VTILE, PR.FIX_LAGS, chunk_bytes=BUDGETS["rows"])
    n = U.plane_lag_counts(PR.FIX_SHAPE, VTILE, PR.FIX_LAGS)
    d = U.find_blurred(s, n)
    sections, tiles, undecided, g = PR.blurred(PR.fixture_sums(), PR.fixture_counts())
    assert d.sections == sections == list(PR.FIX_SECTIONS) and np.array_equal(d.tiles, tiles)
    assert np.array_equal(d.undecided, undecided) and np.array_equal(d.scores, g)
    pc = U.plane_curve(s, n, skip=d.sections)
    zc = U.section_spacing(U.section_lag_sums(vmap, VTILE, PR.FIX_ZLAGS), skip=d.sections).curve
    zp = U.z_pitch(zc, pc)
    px, per = PR.pitch(PR.fixture_zcurve(), PR.curve(PR.fixture_sums(), PR.fixture_counts(), skip=sections))
    assert zp.pixels == px and zp.per_lag.tolist() == [v for _, v in per] and abs(px - PR.FIX_PITCH) <= 0.05 * PR.FIX_PITCH
    assert U.pitch_step(zp.pixels)[2] == PR.step(px)
    both = U.join_defects(U.find_defects(U.section_sums(vmap, VTILE)), d)
    assert both.sections == d.sections and np.array_equal(both.tiles, d.tiles)      # find_defects saw none of it
    fixed = U.volume_repair(vmap, U.defects_repair(both, VTILE, PR.FIX_SHAPE))
    assert not np.array_equal(fixed[7], fx.volume[7]) and np.array_equal(fixed[8], fx.volume[8])
    s2 = U.section_plane_sums(fixed, VTILE, PR.FIX_LAGS)
    assert np.array_equal(s2, PR.volume_plane_sums(fixed, VTILE, PR.FIX_LAGS))
    d2 = U.find_blurred(s2, n)
    rel = PR.relative_g(d2.scores, d2.undecided)
    print("after the repair: relative g of the planted tiles at least", float(rel[fx.planted].min()))
    assert (rel[fx.planted] > 0.65).all() and d2.sections == [] and not d2.tiles.any()
