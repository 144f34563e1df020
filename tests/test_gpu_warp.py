"""The affine warp of sections on the device: tem_u8_warp_affine against the integer numpy reference (warp_ref), byte for
byte; volume_warp out of core; and the chain section_shift_sums -> shift_subpixel -> fit_section_maps -> section_maps ->
volume_warp on the fixture of rotated sections.  The kernel reads a block between guards of fill bytes and writes a
block between guards; source and guards must come back untouched.  Guards and data are those of test_gpu_zcorr.py, the
launch counter that of test_gpu_histogram.py."""
import functools
import itertools

import numpy as np
import pytest
import torch

import warp_ref as WR
from test_gpu_histogram import _counted, _env
from test_gpu_zcorr import FILL, GUARD, _data

pytestmark = pytest.mark.gpu

I23 = WR.IDENTITY
WARP_TILE = (16, 64)                                 # outputs of a workgroup, (y, x)


def _shift(dy, dx):
    return np.array([[1.0, 0.0, dy], [0.0, 1.0, dx]])


@functools.lru_cache(maxsize=None)
def _maps(Y, X):
    """{name: int64[6]}: the maps of the kernel test for a section of Y x X."""
    c = np.array([(Y - 1) / 2, (X - 1) / 2])
    m = {"identity": I23, "int+": _shift(3, -2), "int-": _shift(-1, 1), "last_row": _shift(Y - 1, 0),
         "last_col": _shift(0, X - 1), "one": _shift(1, 1), "half": _shift(0.5, 0.25), "sub": _shift(-1.37, 2.71),
         "lsb": _shift(1 / 256, -1 / 256), "below_lsb": _shift(127 / 65536, -128 / 65536),
         "out_y": _shift(Y + 100, 0), "out_x": _shift(0, -X - 1000), "far": _shift(2.0 ** 31 - 1, -(2.0 ** 31 - 1)),
         "just_out": _shift(Y - 1 + 1 / 256, 0), "face_y0": _shift(-Y / 2, 0.3), "face_y1": _shift(Y / 2, -0.3),
         "face_x0": _shift(0.3, -X / 2), "face_x1": _shift(-0.3, X / 2), "rot": WR._rigid(0.05, np.array([0.4, -0.6]), c)}
    for s in itertools.product((1, -1), repeat=4):                                  # every sign at the +-1/8 limits
        L = np.eye(2) + np.array(s).reshape(2, 2) / 8
        m["limit" + "".join("+" if v > 0 else "-" for v in s)] = np.concatenate([L, (c - L @ c + [0.3, -0.7])[:, None]], axis=1)
    return {k: WR.quantize(v) for k, v in m.items()}


def _tight_rows(M, obox, shape, nearest=False):
    """(sy0, H): the rows that the output box needs by the header's rule, over all sections -- per section, from the
    extremes of fy and fx over the box (at its corners), cut to the section: fy_min >> 8 ... (fy_max >> 8) + (1 where
    fy_max & 255), for nearest (fy + 128) >> 8; none where the section is wholly outside -- (0, 1) when none.  Every
    tap of weight above 0 lies inside them."""
    Y, X = shape
    lo, hi = [], []
    for m in M:
        fy, fx, _ = WR.positions(m, obox, shape)
        a, b = max(int(fy.min()), 0), min(int(fy.max()), 256 * (Y - 1))
        if a > b or max(int(fx.min()), 0) > min(int(fx.max()), 256 * (X - 1)):
            continue
        lo.append((a + 128) >> 8 if nearest else a >> 8)
        hi.append((b + 128) >> 8 if nearest else (b >> 8) + (1 if b & 255 else 0))
        rows = WR.tap_rows(m, obox, shape, nearest)
        assert rows.size == 0 or (lo[-1] <= rows[0] and rows[-1] <= hi[-1])
    return (min(lo), max(hi) - min(lo) + 1) if lo else (0, 1)


def _call(lib, src_ptr, D, H, W, sy0, VY, dst_ptr, odims, o0, mh, md, fill, nearest, stream):
    return lib.tem_u8_warp_affine(src_ptr, D, H, W, sy0, VY, dst_ptr, *odims, *o0, mh, md, fill, nearest, stream)


def _run(vol, M, obox=None, rows=None, fill=0, nearest=False, soff=0, doff=0):
    """One tem_u8_warp_affine call: the (y, x) box `obox` (default: the section) of every section of `vol` from the
    source rows `rows` = (sy0, H) (default: the section), the source `soff` and the output `doff` bytes into aligned
    allocations between guards of FILL; source and guards must come back untouched."""
    L, lib, stream = _env()
    D, VY, W = vol.shape
    (y0, y1), (x0, x1) = obox = ((0, VY), (0, W)) if obox is None else obox
    sy0, H = (0, VY) if rows is None else rows
    flat = np.ascontiguousarray(vol[:, sy0:sy0 + H]).reshape(-1)
    src = torch.full((flat.size + soff + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    src[GUARD + soff:GUARD + soff + flat.size] = torch.from_numpy(flat.copy()).cuda()
    odims = (D, y1 - y0, x1 - x0)
    n = int(np.prod(odims))
    dst = torch.full((n + doff + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 256 == 0 and dst.data_ptr() % 256 == 0
    mh = np.ascontiguousarray(M, np.int64)
    md = torch.from_numpy(mh).cuda()
    L.check(_call(lib, src.data_ptr() + GUARD + soff, D, H, W, sy0, VY, dst.data_ptr() + GUARD + doff, odims, (y0, x0),
                  mh.ctypes.data, md.data_ptr(), fill, int(nearest), stream), "tem_u8_warp_affine")
    got, s = dst.cpu().numpy(), src.cpu().numpy()
    assert (got[:GUARD + doff] == FILL).all() and (got[GUARD + doff + n:] == FILL).all()
    assert (s[:GUARD + soff] == FILL).all() and (s[GUARD + soff + flat.size:] == FILL).all()
    assert np.array_equal(s[GUARD + soff:GUARD + soff + flat.size], flat)
    return got[GUARD + doff:GUARD + doff + n].reshape(odims)


def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), (what, np.argwhere(got != want)[:5])


# ---------------------------------------------------------------------------------------------- tem_u8_warp_affine
@pytest.mark.parametrize("shape", [(37, 53), (5, 4), (1, 1), (40, 131)], ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_reference(shape):
    """One section per map, all maps in one launch: the whole section at the byte offsets 0...3 of source and output,
    nearest, fill 0 and 255, and an odd box off the origin."""
    Y, X = shape
    maps = _maps(Y, X)
    M = np.stack(list(maps.values()))
    vol = _data((len(maps), Y, X), "random")
    want = {(f, nr): WR.warp(vol, M, fill=f, nearest=nr) for f in (0, 255) for nr in (False, True)}
    for soff, doff in ((0, 0), (1, 3), (2, 1), (3, 2)):
        _same(_run(vol, M, soff=soff, doff=doff), want[0, False], (soff, doff))
    _same(_run(vol, M, fill=255, soff=1), want[255, False], "fill 255")
    _same(_run(vol, M, nearest=True, doff=1), want[0, True], "nearest")
    _same(_run(vol, M, fill=255, nearest=True), want[255, True], "nearest, fill 255")
    if Y > 4 and X > 4:
        box = ((2, Y - 1), (1, X - 2))                                               # oy0, ox0 > 0; OW odd or even as X is
        for off in (0, 3):
            _same(_run(vol, M, box, soff=off, doff=off), want[0, False][:, 2:Y - 1, 1:X - 2], ("box", off))
        _same(_run(vol, M, box, nearest=True, fill=255), want[255, True][:, 2:Y - 1, 1:X - 2], "box, nearest")


def test_kernel_cases_cover_what_they_claim():
    Y, X = 37, 53
    maps = _maps(Y, X)
    vol = _data((len(maps), Y, X), "random")
    names = list(maps)
    want = WR.warp(vol, np.stack(list(maps.values())), fill=7)
    inside = np.stack([WR.positions(m, ((0, Y), (0, X)), (Y, X))[2] for m in maps.values()])
    frac = dict(zip(names, inside.mean(axis=(1, 2))))
    assert frac["identity"] == 1 and np.array_equal(want[names.index("identity")], vol[names.index("identity")])
    for k in ("out_y", "out_x", "far", "just_out"):
        assert frac[k] == 0 and (want[names.index(k)] == 7).all()
    assert inside[names.index("last_row")].sum() == X and inside[names.index("last_col")].sum() == Y
    for k in ("face_y0", "face_y1", "face_x0", "face_x1"):                         # partly outside across each face
        assert 0.4 < frac[k] < 0.6
    i = inside[names.index("face_y0")]
    assert not i[0].any() and i[-1, 0]
    i = inside[names.index("face_x1")]
    assert i[-1, 0] and not i[:, -1].any()
    fy, fx, _ = WR.positions(maps["identity"], ((0, Y), (0, X)), (Y, X))           # ty = 0 on the last row, tx = 0 on the last
    assert fy[-1, 0] == 256 * (Y - 1) and fx[0, -1] == 256 * (X - 1)               # column: the clamped tap has weight 0
    fy, _, ins = WR.positions(maps["below_lsb"], ((0, Y), (0, X)), (Y, X))
    assert ins.all() and (fy & 255 == 0).all()                                     # 127 / 65536 rounds down to the grid
    limits = [k for k in names if k.startswith("limit")]
    assert len(limits) == 16 and all(0.4 < frac[k] <= 1 for k in limits)
    assert {tuple(np.sign(maps[k][[0, 1, 3, 4]] - [1 << 16, 0, 0, 1 << 16])) for k in limits} == \
        set(itertools.product((1, -1), repeat=4))
    assert all((np.abs(maps[k][[0, 1, 3, 4]] - [1 << 16, 0, 0, 1 << 16]) == 1 << 13).all() for k in limits)


def test_kernel_takes_row_cut_blocks():
    """Output rows off the origin from source blocks that hold just the rows they read: sy0 > 0, fewer rows than the
    section, bilinear and nearest; and a block one row short is refused."""
    L, lib, stream = _env()
    Y, X = 37, 53
    maps = _maps(Y, X)
    for names, box in ((("identity", "int+", "half", "sub", "lsb", "rot"), ((20, 31), (0, X))),
                       (("limit++++", "limit+-+-", "limit--++", "limit----", "rot"), ((15, 22), (5, 50))),
                       (("identity", "one", "out_y"), ((0, 3), (3, 52))), (("identity",), ((36, 37), (0, X)))):
        M = np.stack([maps[k] for k in names])
        vol = _data((len(names), Y, X), "random")
        for nearest in (False, True):
            sy0, H = rows = _tight_rows(M, box, (Y, X), nearest)
            assert H < Y and (sy0 > 0 or box[0][0] == 0)
            want = WR.warp(vol, M, (((0, len(names)),) + box), fill=9, nearest=nearest)
            for off in (0, 1):
                _same(_run(vol, M, box, rows, fill=9, nearest=nearest, soff=off, doff=3 - off), want, (names, nearest, off))
            if H > 1:                                                               # one row short, at either end
                src = torch.zeros(len(names) * H * X, dtype=torch.uint8, device="cuda")
                dst = torch.zeros(len(names) * Y * X, dtype=torch.uint8, device="cuda")
                mh = np.ascontiguousarray(M)
                md = torch.from_numpy(mh).cuda()
                od = (len(names), box[0][1] - box[0][0], box[1][1] - box[1][0])
                for r in ((sy0 + 1, H - 1), (sy0, H - 1)):
                    assert _call(lib, src.data_ptr(), len(names), r[1], X, r[0], Y, dst.data_ptr(), od,
                                 (box[0][0], box[1][0]), mh.ctypes.data, md.data_ptr(), 0, int(nearest), stream) == L.TEM_EINVAL


REAL = (2, 1001, 1731)


def test_kernel_at_the_shape_of_a_real_call():
    """A plane of 1001 x 1731: 63 x 28 tiles of 16 x 64 per plane, the last row of tiles 9 rows high and the last column
    3 columns wide; W is odd, so a row's alignment changes from row to row; one plane turns by half a degree, the other
    sits at the coefficient limits.  The whole plane, and a run of rows from the rows it reads."""
    D, Y, X = REAL
    ty, tx = WARP_TILE
    assert (-(-Y // ty), -(-X // tx), Y % ty, X % tx, X % 4) == (63, 28, 9, 3, 3)
    c = np.array([(Y - 1) / 2, (X - 1) / 2])
    L = np.array([[1.125, -0.125], [0.125, 0.875]])
    M = WR.quantize(np.stack([WR._rigid(np.deg2rad(0.5), np.array([0.37, -1.21]), c),
                              np.concatenate([L, (c - L @ c)[:, None]], axis=1)]))
    vol = _data(REAL, "random")
    want = WR.warp(vol, M, fill=3)
    assert (want[0] == 3).mean() < 0.03 and 0.02 < (want[1] == 3).mean() < 0.3
    _same(_run(vol, M, fill=3, soff=1, doff=2), want, "whole")
    box = ((500, 700), (0, X))
    rows = _tight_rows(M, box, (Y, X))
    assert rows[0] > 300 and rows[1] < 500
    _same(_run(vol, M, box, rows, fill=3), want[:, 500:700], "rows")


def test_kernel_refuses_bad_arguments():
    """TEM_EINVAL from the host-side checks, nothing launched: dst keeps its fill."""
    L, lib, stream = _env()
    D, H, W, VY = 2, 6, 8, 10
    src = torch.ones(D * H * W + 16, dtype=torch.uint8, device="cuda")
    dst = torch.full((D * 4 * 5 + 16,), FILL, dtype=torch.uint8, device="cuda")
    mh = np.ascontiguousarray(np.stack([WR.quantize(I23)] * D))
    md = torch.from_numpy(mh).cuda()
    p, q, h, m = src.data_ptr(), dst.data_ptr(), mh.ctypes.data, md.data_ptr()
    call = lambda *a: lib.tem_u8_warp_affine(*a, stream)
    # src D H W sy0 VY dst OD OH OW oy0 ox0 maps_host maps_dev fill nearest: rows 2...7 of 10, the box (3...6, 2...6)
    ok = [p, D, H, W, 2, VY, q, D, 4, 5, 3, 2, h, m, 0, 0]
    for i, v in [(0, None), (6, None), (12, None), (13, None), (1, 0), (2, 0), (3, 0), (5, 0), (7, 0), (8, 0), (9, 0),
                 (1, -1), (7, 1), (7, 3), (4, -1), (10, -1), (11, -1), (4, 5), (5, 7), (10, 7), (11, 4), (9, 7), (14, -1),
                 (14, 256), (15, 2), (15, -1), (4, 4), (2, 4), (2, 2), (10, 1), (8, 6)]:
        a = list(ok)
        a[i] = v
        assert call(*a) == L.TEM_EINVAL, (i, v)
    for j, v in [(0, (1 << 16) + (1 << 13) + 1), (0, (1 << 16) - (1 << 13) - 1), (1, (1 << 13) + 1), (1, -(1 << 13) - 1),
                 (3, (1 << 13) + 1), (3, -(1 << 13) - 1), (4, (1 << 16) + (1 << 13) + 1), (4, (1 << 16) - (1 << 13) - 1),
                 (2, 1 << 47), (2, -(1 << 47)), (5, 1 << 47), (5, -(1 << 47)), (0, 0), (2, -(1 << 63))]:
        bad = mh.copy()
        bad[1, j] = v                                                               # in the second section only
        assert call(*ok[:12], bad.ctypes.data, m, 0, 0) == L.TEM_EINVAL, (j, v)
    up = mh.copy()
    up[:, 2] = 256                                                                  # 1/256 px down: ty = 1
    ud = torch.from_numpy(up).cuda()
    assert call(*ok[:10], 4, 2, up.ctypes.data, ud.data_ptr(), 0, 0) == L.TEM_EINVAL    # rows 4...8: row 8 is not in the block
    # more workgroups than one launch holds: 2^27 rows of tiles (refused before anything is touched)
    big = 2 ** 31 - 1
    assert call(p, 1, big, 8, 0, big, q, 1, big, 8, 0, 0, h, m, 0, 0) == L.TEM_EINVAL
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == FILL).all()
    assert call(*ok[:12], up.ctypes.data, ud.data_ptr(), 0, 0) == 0                 # rows 3...7 are in the block
    assert call(*ok[:10], 4, 2, h, m, 0, 0) == 0                                    # at ty = 0 row 8 is no tap
    assert call(*ok) == 0 and call(p + 3, *ok[1:]) == 0                             # and the good call runs
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[:D * 4 * 5] == 1).all() and (got[D * 4 * 5:] == FILL).all()


# ------------------------------------------------------------------------------------------------------ volume_warp
VSHAPE = (6, 37, 53)
BUDGETS = {"whole": 6 * 37 * 53, "two_sections": 2 * 37 * 53, "ten_rows": 10 * 53, "one_row": 53}


@functools.lru_cache(maxsize=None)
def _vcase():
    Z, Y, X = VSHAPE
    vol = np.random.default_rng(29).integers(0, 256, VSHAPE, dtype=np.uint8)
    maps = _maps(Y, X)
    M = np.stack([maps[k] for k in ("rot", "sub", "limit+-+-", "out_y", "face_y1", "half")])
    want = WR.warp(vol, M, fill=11)
    vol.setflags(write=False), M.setflags(write=False), want.setflags(write=False)
    return vol, M, want


@pytest.fixture(scope="module")
def vmap(tmp_path_factory):
    path = tmp_path_factory.mktemp("warp") / "vol.u8"
    m = np.memmap(path, np.uint8, "w+", shape=VSHAPE)
    m[...] = _vcase()[0]
    m.flush()
    return np.memmap(path, np.uint8, "r", shape=VSHAPE)


@pytest.mark.parametrize("budget", list(BUDGETS), ids=list(BUDGETS))
def test_volume_warp_equals_the_reference_however_it_is_cut(vmap, budget, tmp_path):
    from transfer_em_amd.utils import volume_warp, warp_chunks
    vol, M, want = _vcase()
    out = np.memmap(tmp_path / "out.u8", np.uint8, "w+", shape=VSHAPE)
    st, n = {}, 0
    for rank in (1, 0):
        res, counts = _counted(lambda: volume_warp(vmap, M, out=out, fill=11, chunk_bytes=BUDGETS[budget], rank=rank,
                                                   world_size=2, stats=st))
        mine = len(warp_chunks(((0, 6), (0, 37), (0, 53)), VSHAPE, M, BUDGETS[budget], rank, 2))
        assert res is out and st["chunks"] == mine == counts["tem_u8_warp_affine"]  # one launch per slab
        assert st["read_s"] >= 0 and st["write_s"] >= 0
        n += mine
    _same(np.asarray(out), want, budget)
    assert {"whole": n == 1, "two_sections": n == 3, "ten_rows": n > 6 * 4, "one_row": n == 6 * 37}[budget]
    assert np.array_equal(np.asarray(vmap), vol)                                    # the input: read only


def test_volume_warp_of_an_roi_float_maps_one_image_and_nearest(vmap):
    from transfer_em_amd.utils import quantize_maps, volume_warp
    vol, M, want = _vcase()
    got = volume_warp(vmap, M, start=(5, 3, 1), size=(41, 30, 4), fill=11, chunk_bytes=7 * 53)
    _same(got, want[1:5, 3:33, 5:46], "roi")
    T = np.stack([WR._rigid(0.02 * z, np.array([0.25 * z, -0.5]), np.array([18.0, 26.0])) for z in range(6)])
    _same(volume_warp(vol, T), WR.warp(vol, quantize_maps(T)), "float maps, an ndarray, the default slab")
    _same(volume_warp(vol, T, nearest=True, fill=255), WR.warp(vol, WR.quantize(T), fill=255, nearest=True), "nearest")
    _same(volume_warp(vol[2], T[3], fill=5), WR.warp(vol[2:3], WR.quantize(T[3:4]), fill=5)[0], "one image")
    _same(volume_warp(vol[2], M[0], start=(3, 4), size=(50, 20)), WR.warp(vol[2:3], M[:1])[0, 4:24, 3:53], "one image, roi")


# ------------------------------------------------------------------------------------------------------- end to end
def test_the_rotation_is_measured_and_undone():
    """section_shift_sums -> shift_subpixel -> fit_section_maps -> section_maps -> volume_warp -> section_shift_sums
    on the fixture of rotated sections: every interior tile re-measures (0, 0), and the interior tiles' mean correlation
    is above what volume_shift by the integer medians reaches."""
    from transfer_em_amd.utils import (fit_section_maps, quantize_maps, section_maps, section_shift_sums, section_shifts,
                                       shift_counts, shift_positions, shift_scores, shift_subpixel, volume_shift,
                                       volume_warp)
    v = WR.rotated_volume()
    tile, r = WR.FIX_TILE, WR.FIX_RADIUS
    n = shift_counts(v.shape, tile, r)
    q = section_shift_sums(v, tile, r)
    sub = shift_subpixel(q, n)
    fit = fit_section_maps(sub, tile, v.shape)
    assert sub.decided.all() and fit.unresolved == []
    B = section_maps(fit.maps)
    warped = volume_warp(v, B, chunk_bytes=3 * 96 * 128)
    _same(warped, WR.warp(v, quantize_maps(B)), "the warp")
    shifted = volume_shift(v, shift_positions(section_shifts(q, n).pairs))

    def interior(vol):
        q2 = section_shift_sums(vol, tile, r)
        return shift_scores(q2, n)[:, 1, 1:3, r, r].mean(), section_shifts(q2, n).tiles[:, 1, 1:3]
    (c_raw, _), (c_shift, _), (c_warp, t_warp) = interior(v), interior(shifted), interior(warped)
    print("interior tiles' mean correlation: raw", c_raw, "shifted", c_shift, "warped", c_warp)
    assert not t_warp.any()
    assert c_warp > c_shift
