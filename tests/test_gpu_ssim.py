"""The windowed SSIM on the device: tem_u8_ssim against the integer numpy reference (ssim_ref), and volume_ssim out of
core.  The contract is integers up to two correctly rounded float64 divisions, so every comparison is exact: sums and
map equal the reference bit for bit.  Helpers are those of test_gpu_histogram.py."""
import os
import re

import numpy as np
import pytest
import torch

import ssim_ref as R
from test_gpu_histogram import FailingReads, _counted, _env, _upload

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "transfer_em_amd", "csrc",
                         "ssim_u8.hip")).read()
TY, TX = (int(v) for v in re.search(r"SSIM_TY = (\d+), SSIM_TX = (\d+);", _SRC).groups())     # the kernel's tile
ZRUN = int(re.search(r"SSIM_ZRUN = (\d+);", _SRC).group(1))                                    # ... and its z-run

WINS = [(w, f) for w in (3, 5, 7, 9, 11) for f in (False, True)]
WIN_IDS = [f"{'flat' if f else 'win'}{w}" for w, f in WINS]
SOME = [(3, False), (7, False), (11, False), (7, True)]
SOME_IDS = ["win3", "win7", "win11", "flat7"]
GUARD, MAP_FILL, SUM_FILL = 61, 0xA5, 0x5A5A5A5A5A5A5A5A                 # an odd guard: the map starts misaligned


def _wshape(n, win, flat):
    return tuple(e - w + 1 for e, w in zip(n, R.window(win, flat)))


class _Out:
    """Device `sums` (rows x 3, cleared) and `map` (nbytes, or none) between guards."""

    def __init__(self, rows, nbytes=None):
        self.rows, self.nbytes = rows, nbytes
        self.sums = torch.full((rows * 3 + 2 * GUARD,), SUM_FILL, dtype=torch.int64, device="cuda")
        self.sums[GUARD:GUARD + rows * 3] = 0
        self.map = None if nbytes is None else torch.full((nbytes + 2 * GUARD,), MAP_FILL, dtype=torch.uint8, device="cuda")

    def sums_ptr(self, row=0):
        return self.sums.data_ptr() + 8 * (GUARD + 3 * row)

    def map_ptr(self):
        return None if self.map is None else self.map.data_ptr() + GUARD

    def read(self, wshape=None):
        """(sums [rows, 3], map of `wshape` or None); the guards must be untouched."""
        s = self.sums.cpu().numpy()
        assert (s[:GUARD] == SUM_FILL).all() and (s[GUARD + 3 * self.rows:] == SUM_FILL).all()
        m = None
        if self.map is not None:
            m = self.map.cpu().numpy()
            assert (m[:GUARD] == MAP_FILL).all() and (m[GUARD + self.nbytes:] == MAP_FILL).all()
            m = m[GUARD:GUARD + self.nbytes].reshape(wshape)
        return s[GUARD:GUARD + 3 * self.rows].reshape(self.rows, 3), m


def _call(pa, da, oa, pb, db, ob, n, win, flat, out, row=0, with_map=True):
    L, lib, stream = _env()
    L.check(lib.tem_u8_ssim(pa, *da, *oa, pb, *db, *ob, *n, win, int(flat), out.sums_ptr(row),
                            out.map_ptr() if with_map else None, stream), "tem_u8_ssim")


def _ssim(a, oa, b, ob, n, win, flat, off=(0, 0), with_map=True):
    """tem_u8_ssim of the box of extents n at origin oa of block a against origin ob of block b: (sums, map)."""
    ws = _wshape(n, win, flat)
    ka, pa = _upload(a, off[0])
    kb, pb = _upload(b, off[1])
    out = _Out(ws[0], int(np.prod(ws)) if with_map else None)
    _call(pa, a.shape, oa, pb, b.shape, ob, n, win, flat, out, with_map=with_map)
    return out.read(ws)


def _box(v, o, n):
    return v[tuple(slice(lo, lo + e) for lo, e in zip(o, n))]


def _same(got, want, what=None):
    (gs, gm), (ws, wm) = got, want
    assert gs.shape == ws.shape and np.array_equal(gs, ws), (what, np.argwhere(gs != ws)[:5], gs.ravel()[:6], ws.ravel()[:6])
    if gm is not None:
        assert gm.shape == wm.shape and np.array_equal(gm, wm), (what, np.argwhere(gm != wm)[:5])


def _random_pair(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------- tem_u8_ssim
@pytest.mark.parametrize("win,flat", WINS, ids=WIN_IDS)
def test_one_window_and_one_voxel_more(win, flat):
    """A box of exactly one window, then one voxel more on each axis in turn, at a non-zero origin of a larger block."""
    wz = 1 if flat else win
    a, b = _random_pair((wz + 3, win + 4, win + 5), 60 + win)
    for extra in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        n = tuple(e + x for e, x in zip((wz, win, win), extra))
        o = (1, 2, 3)
        got = _ssim(a, o, b, o, n, win, flat, off=(1, 0))
        assert got[0].shape == (1 + extra[0], 3) and got[1].size == 1 + sum(extra)
        _same(got, R.reference(_box(a, o, n), _box(b, o, n), win, flat), n)


@pytest.mark.parametrize("win,flat", SOME, ids=SOME_IDS)
def test_extents_around_the_tile_and_the_z_run(win, flat):
    """Window boxes one below, equal to and one above the kernel's tile in y and x and its run length in z."""
    wz = 1 if flat else win
    a, b = _random_pair((ZRUN + wz, TY + win, TX + win), 70 + win)       # the largest box: (ZRUN + 1, TY + 1, TX + 1) windows
    whole = R.ssim_q(a, b, win, flat)
    ka, pa = _upload(a)
    kb, pb = _upload(b, 1)
    for zw in (ZRUN - 1, ZRUN, ZRUN + 1):
        for yw in (TY - 1, TY, TY + 1):
            for xw in (TX - 1, TX, TX + 1):
                n = (zw + wz - 1, yw + win - 1, xw + win - 1)
                out = _Out(zw, zw * yw * xw)
                _call(pa, a.shape, (0, 0, 0), pb, b.shape, (0, 0, 0), n, win, flat, out)
                q = tuple(v[:zw, :yw, :xw] for v in whole)               # windows depend on their own voxels only
                _same(out.read((zw, yw, xw)), (R.ssim_sums(q), R.ssim_map(q[0])), n)


OFFS = [(0, 0), (1, 0), (0, 1), (1, 3), (3, 1)]


@pytest.mark.parametrize("off", OFFS, ids=[f"off{a}{b}" for a, b in OFFS])
@pytest.mark.parametrize("win,flat", [(7, False), (5, True)], ids=["win7", "flat5"])
def test_boxes_inside_blocks_of_different_geometry(win, flat, off):
    """Non-zero origins, a and b in blocks of different width and depth, uploads at byte offsets 0, 1 and 3: the two
    sides' rows are misaligned independently.  Several tiles in y and x."""
    da, db = (13, 27, 83), (15, 30, 90)
    oa, ob, n = (1, 2, 5), (2, 6, 9), (11, 21, 74)
    a, _ = _random_pair(da, 80)
    b, _ = _random_pair(db, 81)
    ws = _wshape(n, win, flat)
    assert ws[1] > TY and ws[2] > TX
    _same(_ssim(a, oa, b, ob, n, win, flat, off=off), R.reference(_box(a, oa, n), _box(b, ob, n), win, flat))


def test_flat_windows_do_not_mix_sections():
    """Sections of very different content: a flat window's row of sums is that of its section alone."""
    rng = np.random.default_rng(82)
    a = np.stack([np.full((20, 50), 10 + 60 * z, np.uint8) + rng.integers(0, 9, (20, 50), dtype=np.uint8) for z in range(4)])
    b = np.stack([rng.integers(0, 256, (20, 50), dtype=np.uint8) if z % 2 else a[z] for z in range(4)])
    got = _ssim(a, (0, 0, 0), b, (0, 0, 0), a.shape, 7, True)
    _same(got, R.reference(a, b, 7, True))
    assert (got[0][0] == 14 * 44 * R.Q).all() and (got[0][2] == 14 * 44 * R.Q).all() and got[0][1, 0] < 14 * 44 * R.Q // 4
    for z in range(4):
        one = _ssim(a[z:z + 1], (0, 0, 0), b[z:z + 1], (0, 0, 0), (1, 20, 50), 7, True)
        assert np.array_equal(one[0][0], got[0][z]) and np.array_equal(one[1][0], got[1][z])


def test_null_map_calls_accumulate_and_boxes_share_one_sums():
    a, b = _random_pair((20, 24, 70), 83)
    ka, pa = _upload(a)
    kb, pb = _upload(b, 3)
    n, win = a.shape, 5
    ws = _wshape(n, win, False)
    want = R.reference(a, b, win, False)
    with_map, without = _Out(ws[0], int(np.prod(ws))), _Out(ws[0])
    _call(pa, n, (0, 0, 0), pb, n, (0, 0, 0), n, win, False, with_map)
    _call(pa, n, (0, 0, 0), pb, n, (0, 0, 0), n, win, False, without, with_map=False)
    _same(with_map.read(ws), want)
    assert np.array_equal(without.read()[0], want[0])                    # map == NULL: the same sums
    _call(pa, n, (0, 0, 0), pb, n, (0, 0, 0), n, win, False, without, with_map=False)
    assert np.array_equal(without.read()[0], 2 * want[0])                # two calls accumulate
    # the box as three boxes of sections that overlap by the window, each into its own rows of one `sums`
    parts = _Out(ws[0])
    for z0, z1 in ((0, 5), (5, 6), (6, ws[0])):                          # window-sections [z0, z1)
        _call(pa, n, (z0, 0, 0), pb, n, (z0, 0, 0), (z1 - z0 + win - 1, n[1], n[2]), win, False, parts, row=z0,
              with_map=False)
    assert np.array_equal(parts.read()[0], want[0])
    # ... and cut along y, into the same rows
    parts = _Out(ws[0])
    for y0, y1 in ((0, 9), (9, ws[1])):
        _call(pa, n, (0, y0, 0), pb, n, (0, y0, 0), (n[0], y1 - y0 + win - 1, n[2]), win, False, parts, with_map=False)
    assert np.array_equal(parts.read()[0], want[0])


def _data(kind, shape):
    rng = np.random.default_rng(84)
    em = np.clip(rng.normal(120, 30, shape), 0, 255).astype(np.uint8)
    if kind == "random":
        return _random_pair(shape, 85)
    if kind == "noisy":
        return em, R.noisy(em, rng)
    if kind == "equal":
        return em, em.copy()
    if kind == "inverse":
        return em, (255 - em).astype(np.uint8)
    if kind == "zeros_255":
        return np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)
    if kind == "all_255":
        return np.full(shape, 255, np.uint8), np.full(shape, 255, np.uint8)
    if kind == "constant_side":
        return em, np.full(shape, 77, np.uint8)
    assert kind == "checkerboard"
    return R.checkerboard(shape)


KINDS = ["random", "noisy", "equal", "inverse", "zeros_255", "all_255", "constant_side", "checkerboard"]


@pytest.mark.parametrize("win,flat", SOME, ids=SOME_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_data(kind, win, flat):
    shape = (14, 21, 47)
    a, b = _data(kind, shape)
    got = _ssim(a, (0, 0, 0), b, (0, 0, 0), shape, win, flat, off=(0, 1))
    _same(got, R.reference(a, b, win, flat), kind)
    windows = got[1][0].size
    if kind in ("equal", "all_255"):
        assert (got[0] == windows * R.Q).all() and (got[1] == 255).all()   # 2^30 in every window
    if kind in ("inverse", "checkerboard"):
        assert (got[0][:, 0] < 0).all() and (got[0][:, 2] < 0).all() and (got[1] == 0).all()   # signed sums survive
    if kind == "zeros_255":
        assert (got[0][:, 0] == windows * 107363).all() and (got[0][:, 2] == windows * R.Q).all()


@pytest.mark.parametrize("off", [(0, 0), (1, 3)], ids=["aligned", "off13"])
def test_nothing_outside_the_boxes_is_read(off):
    """Change every byte outside the two boxes: the result must not change."""
    da, oa, db, ob, n = (12, 25, 60), (2, 3, 4), (11, 30, 71), (1, 8, 13), (9, 17, 45)
    a, _ = _random_pair(da, 86)
    b, _ = _random_pair(db, 87)
    want = R.reference(_box(a, oa, n), _box(b, ob, n), 7, False)
    _same(_ssim(a, oa, b, ob, n, 7, False, off=off), want)
    a2, b2 = (255 - a).astype(np.uint8), (b + 101).astype(np.uint8)
    _box(a2, oa, n)[...] = _box(a, oa, n)
    _box(b2, ob, n)[...] = _box(b, ob, n)
    assert (a2 != a).sum() == a.size - np.prod(n)
    _same(_ssim(a2, oa, b2, ob, n, 7, False, off=off), want)
    _same(_ssim(a2, oa, b2, ob, n, 7, True, off=off), R.reference(_box(a, oa, n), _box(b, ob, n), 7, True))


def test_rejects_malformed_arguments():
    """TEM_EINVAL from the host-side checks, nothing launched: sums and map keep their fill."""
    L, lib, stream = _env()
    a = torch.zeros(8 * 9 * 10, dtype=torch.uint8, device="cuda")
    b = torch.ones(9 * 10 * 11, dtype=torch.uint8, device="cuda")
    out = _Out(2, 2 * 3 * 4)

    def call(pa=None, da=(8, 9, 10), oa=(0, 0, 0), pb=None, db=(9, 10, 11), ob=(1, 1, 1), n=(8, 9, 10), win=7, flat=0,
             sums=None, smap=0):
        return lib.tem_u8_ssim(a.data_ptr() if pa is None else pa, *da, *oa, b.data_ptr() if pb is None else pb, *db,
                               *ob, *n, win, flat, out.sums_ptr() if sums is None else sums,
                               out.map_ptr() if smap == 0 else smap, stream)
    assert call(pa=0) == L.TEM_EINVAL and call(pb=0) == L.TEM_EINVAL and call(sums=0) == L.TEM_EINVAL
    assert call(sums=out.sums_ptr() + 4) == L.TEM_EINVAL                               # off 8-byte alignment
    for win in (0, 1, 2, 4, 6, 8, 10, 12, 13, -7):
        assert call(win=win) == L.TEM_EINVAL and call(win=win, flat=1) == L.TEM_EINVAL
    at = lambda t, d, v: tuple(v if i == d else e for i, e in enumerate(t))
    for d in range(3):
        for v in (0, -1):                                                               # a dim below 1
            assert call(da=at((8, 9, 10), d, v), n=at((8, 9, 10), d, 0)) == L.TEM_EINVAL
            assert call(db=at((9, 10, 11), d, v), ob=(0, 0, 0), n=at((8, 9, 10), d, 0)) == L.TEM_EINVAL
        assert call(oa=at((0, 0, 0), d, -1)) == L.TEM_EINVAL and call(ob=at((1, 1, 1), d, -1)) == L.TEM_EINVAL
        assert call(n=at((8, 9, 10), d, -1)) == L.TEM_EINVAL                            # a negative extent
        assert call(oa=at((0, 0, 0), d, 1)) == L.TEM_EINVAL                             # the box leaves a
        assert call(ob=at((1, 1, 1), d, 2)) == L.TEM_EINVAL                             # ... leaves b
        assert call(n=at((8, 9, 10), d, (9, 10, 11)[d]), ob=(0, 0, 0)) == L.TEM_EINVAL  # fits b, leaves a
    # more workgroups than a launch holds (the bound of include/tem_hip.h); refused on the host, so the extents need
    # no memory behind them
    M = 2 ** 31 - 1
    assert call(da=(M, M, M), db=(M, M, M), ob=(0, 0, 0), n=(M, M, M)) == L.TEM_EINVAL
    assert call(da=(7, M, M), db=(7, M, M), ob=(0, 0, 0), n=(7, M, M)) == L.TEM_EINVAL
    wgs = lambda n, flat: (-(-(n[1] - 6) // TY)) * (-(-(n[2] - 6) // TX)) * (-(-(n[0] - (0 if flat else 6)) // ZRUN))
    over = (ZRUN * 2 ** 12, TY * 2 ** 6 + 6, TX * 2 ** 6 + 6)            # 2^24 workgroups of flat windows: one too many
    assert wgs(over, True) == 2 ** 24 and max(over) < 2 ** 31
    assert call(da=over, db=over, ob=(0, 0, 0), n=over, flat=1) == L.TEM_EINVAL
    torch.cuda.synchronize()
    sums, smap = out.read((2, 3, 4))
    assert (sums == 0).all() and (smap == MAP_FILL).all()
    # a box in which no window fits: fine, nothing launched
    for n, flat in (((6, 9, 10), 0), ((8, 6, 10), 0), ((8, 9, 6), 1), ((0, 9, 10), 1), ((8, 0, 10), 0), ((0, 0, 0), 0)):
        assert call(n=n, flat=flat) == L.TEM_OK
    torch.cuda.synchronize()
    sums, smap = out.read((2, 3, 4))
    assert (sums == 0).all() and (smap == MAP_FILL).all()
    assert call() == L.TEM_OK                                            # all of a against b's box at (1, 1, 1): 2 x 3 x 4 windows
    torch.cuda.synchronize()
    sums, smap = out.read((2, 3, 4))
    want = R.reference(np.zeros((8, 9, 10), np.uint8), np.ones((8, 9, 10), np.uint8), 7, False)
    assert np.array_equal(sums, want[0]) and np.array_equal(smap, want[1])


# ------------------------------------------------------------------------------------------------------- volume_ssim
@pytest.fixture(scope="module")
def memmaps(tmp_path_factory):
    """An EM-like (23, 40, 75) memmap and a noisy copy of it inside a larger (26, 45, 81) one, at (z, y, x) (2, 3, 4)."""
    tmp = tmp_path_factory.mktemp("ssim")
    rng = np.random.default_rng(88)
    a = np.lib.format.open_memmap(str(tmp / "a.npy"), mode="w+", dtype=np.uint8, shape=(23, 40, 75))
    a[...] = np.clip(rng.normal(120, 30, a.shape), 0, 255).astype(np.uint8)
    b = np.lib.format.open_memmap(str(tmp / "b.npy"), mode="w+", dtype=np.uint8, shape=(26, 45, 81))
    b[...] = rng.integers(0, 256, b.shape, dtype=np.uint8)
    b[2:25, 3:43, 4:79] = R.noisy(np.asarray(a), rng, amp=12)
    a.flush(), b.flush()
    return np.load(str(tmp / "a.npy"), mmap_mode="r"), np.load(str(tmp / "b.npy"), mmap_mode="r")


@pytest.fixture(scope="module")
def whole7(memmaps):
    """The one-shot reference of the whole pair at win 7, volumetric and flat; left unchanged."""
    a, b = np.asarray(memmaps[0]), np.asarray(memmaps[1])[2:25, 3:43, 4:79]
    return {flat: R.reference(a, b, 7, flat) for flat in (False, True)}


def test_volume_ssim_under_every_cut(memmaps, whole7):
    from transfer_em_amd.utils import SsimSums, ssim_chunks, ssim_from_sums, volume_ssim
    ma, mb = memmaps
    want_sums, want_map = whole7[False]
    B = (4, 3, 2)                                                        # b_start, (x, y, z)
    st = {}
    got = volume_ssim(ma, mb, b_start=B, stats=st)                       # the default budget: one slab, no map
    assert isinstance(got, SsimSums) and got.sums.dtype == np.int64 and got.windows == 34 * 69 and got.win == (7, 7, 7)
    assert np.array_equal(got.sums, want_sums) and st["chunks"] == 1 and st["read_s"] > 0 and "write_s" not in st
    m = ssim_from_sums(got)
    assert m["n"] == 17 * 34 * 69 and 0 < m["ssim"] < m["contrast_structure"] < m["luminance"] < 1
    box = ((0, 23), (0, 40), (0, 75))
    for budget, chunks in (((7 + 3) * 40 * 75 + 11, 5), (7 * 75 * (7 + 4) + 5, 17 * 7)):        # cut z; cut y
        assert len(ssim_chunks(box, 7, False, budget)) == chunks
        out, st = np.full((17, 34, 69), 3, np.uint8), {}
        got = volume_ssim(ma, mb, b_start=B, chunk_bytes=budget, map_out=out, stats=st)
        assert np.array_equal(got.sums, want_sums) and np.array_equal(out, want_map), budget
        assert st["chunks"] == chunks and st["write_s"] > 0
        assert np.array_equal(volume_ssim(ma, mb, b_start=B, chunk_bytes=budget).sums, want_sums)       # map_out absent
    # an inner ROI under the one-row floor: every slab is one row of windows
    a, b = np.asarray(ma), np.asarray(mb)
    start, size, b_start = (9, 5, 3), (53, 12, 9), (20, 1, 7)            # (x, y, z)
    want = R.reference(a[3:12, 5:17, 9:62], b[7:16, 1:13, 20:73], 7, False)
    out, st = np.zeros((3, 6, 47), np.uint8), {}
    got = volume_ssim(ma, mb, start, size, b_start, chunk_bytes=100, map_out=out, stats=st)
    assert st["chunks"] == 3 * 6 and np.array_equal(got.sums, want[0]) and np.array_equal(out, want[1])
    # b_start=None: a's start; win 3 and 11
    for win in (3, 11):
        want = R.reference(a, b[:23, :40, :75], win, False)
        out = np.zeros(want[1].shape, np.uint8)
        got = volume_ssim(ma, mb, win=win, chunk_bytes=13 * 40 * 75, map_out=out)
        assert got.win == (win, win, win) and np.array_equal(got.sums, want[0]) and np.array_equal(out, want[1])


def test_volume_ssim_flat_images_and_ranks(memmaps, whole7, tmp_path):
    from transfer_em_amd.utils import ssim_from_sums, volume_ssim
    ma, mb = memmaps
    a, b = np.asarray(ma), np.asarray(mb)
    B = (4, 3, 2)
    want_sums, want_map = whole7[True]
    out = np.lib.format.open_memmap(str(tmp_path / "map.npy"), mode="w+", dtype=np.uint8, shape=(23, 34, 69))
    got = volume_ssim(ma, mb, b_start=B, flat=True, chunk_bytes=4 * 40 * 75, map_out=out)       # flat, into a memmap
    assert got.win == (1, 7, 7) and np.array_equal(got.sums, want_sums) and np.array_equal(out, want_map)
    # two ranks: the sums add, the maps together fill map_out
    want_sums, want_map = whole7[False]
    budget = 7 * 75 * (7 + 4) + 5
    shared, parts = np.zeros((17, 34, 69), np.uint8), []
    for rank in range(2):
        st = {}
        parts.append(volume_ssim(ma, mb, b_start=B, chunk_bytes=budget, map_out=shared, rank=rank, world_size=2, stats=st))
        assert (st["chunks"], np.array_equal(shared, want_map)) == ((60, False) if rank == 0 else (59, True))
    assert parts[0].sums.any() and not np.array_equal(parts[0].sums, parts[1].sums)
    assert np.array_equal(parts[0].sums + parts[1].sums, want_sums)
    assert ssim_from_sums((parts[0].sums + parts[1].sums, parts[0].windows, parts[0].win))["n"] == 17 * 34 * 69
    # two images: always flat, 2-element arguments, map [Yw, Xw]
    ia, ib = a[7], b[9]
    want = R.reference(ia[None, 4:34, 3:63], ib[None, 2:32, 11:71], 5, True)
    out = np.zeros((26, 56), np.uint8)
    got = volume_ssim(ia, ib, (3, 4), (60, 30), (11, 2), win=5, chunk_bytes=9 * 60, map_out=out)
    assert got.win == (1, 5, 5) and got.sums.shape == (1, 3) and got.windows == 26 * 56
    assert np.array_equal(got.sums, want[0]) and np.array_equal(out, want[1][0])
    assert np.array_equal(volume_ssim(ia, ib, (3, 4), (60, 30), (11, 2), win=5, flat=False).sums, want[0])
    same = volume_ssim(ma, ma, win=9)                                    # equal volumes
    assert ssim_from_sums(same)["ssim"] == 1.0 and (same.sums == same.windows * R.Q).all()


def test_a_failing_read_surfaces_and_leaves_the_device_usable(memmaps, whole7):
    import threading
    from transfer_em_amd.utils import volume_ssim
    ma, mb = memmaps
    threads = threading.active_count()
    budget = (7 + 3) * 40 * 75 + 11                                      # 5 slabs
    for kw in ({}, dict(map_out=np.zeros((17, 34, 69), np.uint8))):
        bad = FailingReads(np.asarray(ma))
        with pytest.raises(OSError, match="the third read fails"):
            volume_ssim(bad, mb, b_start=(4, 3, 2), chunk_bytes=budget, **kw)
        assert bad.reads >= 3 and threading.active_count() == threads
    out = np.zeros((17, 34, 69), np.uint8)
    got = volume_ssim(ma, mb, b_start=(4, 3, 2), chunk_bytes=budget, map_out=out)
    assert np.array_equal(got.sums, whole7[False][0]) and np.array_equal(out, whole7[False][1])


def test_the_existing_passes_launch_as_before(memmaps):
    """_SlabPass without `slabs` cuts by hist_chunks as ever: one launch per slab of the existing passes."""
    from transfer_em_amd.utils import (clahe_fit, clahe_volume, hist_box, hist_chunks, volume_histogram,
                                       volume_joint_histogram, volume_ssim)
    ma, mb = memmaps
    a = np.asarray(ma)
    budget = 3 * 40 * 75 + 100                                           # 3 sections per slab: 8 slabs
    slabs = len(hist_chunks(hist_box(ma.shape), budget))
    assert slabs == 8
    h, n = _counted(lambda: volume_histogram(ma, chunk_bytes=budget))
    assert dict(n) == {"tem_u8_hist": slabs} and np.array_equal(h, np.bincount(a.ravel(), minlength=256))
    J, n = _counted(lambda: volume_joint_histogram(ma, mb, b_start=(4, 3, 2), chunk_bytes=budget))
    assert dict(n) == {"tem_u8_hist2": slabs} and J.sum() == a.size
    tables = clahe_fit(ma, tile=16)
    one, n1 = _counted(lambda: clahe_volume(ma, tables))
    cut, n = _counted(lambda: clahe_volume(ma, tables, chunk_bytes=budget))
    assert dict(n1) == {"tem_u8_clahe": 1} and dict(n) == {"tem_u8_clahe": slabs} and np.array_equal(one, cut)
    got, n = _counted(lambda: volume_ssim(ma, mb, b_start=(4, 3, 2), chunk_bytes=(7 + 3) * 40 * 75 + 11))
    assert dict(n) == {"tem_u8_ssim": 5}
