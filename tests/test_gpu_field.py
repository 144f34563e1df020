"""The warp of sections through "affine map + displacement field" on the device: tem_u8_warp_field against the integer
numpy reference (field_ref) byte for byte and against tem_u8_warp_affine where the field is zero, constant or a ramp;
volume_warp_field out of core; and the chain section_shift_sums -> shift_subpixel -> fit_section_maps ->
fit_section_fields -> section_fields -> volume_warp_field on the fixture of smoothly distorted sections.  Guards, data
and the launch counter are test_gpu_warp.py's."""
import functools

import numpy as np
import pytest
import torch

import field_ref as FR
import warp_ref as WR
from test_gpu_histogram import _counted, _env
from test_gpu_warp import WARP_TILE, _maps, _run as _run_affine, _same
from test_gpu_zcorr import FILL, GUARD, _data

pytestmark = pytest.mark.gpu

SHAPES = [(37, 53), (5, 4), (1, 1), (40, 131)]
SPACINGS = [16, (16, 64)]
MAP_NAMES = ("identity", "sub", "rot", "out_y", "face_y0", "face_y1", "face_x0", "face_x1")    # and the sixteen limits
ONE, DEV = 1 << 16, 1 << 13


def _kk(spacing):
    return FR.log2s(spacing)


@functools.lru_cache(maxsize=None)
def _cases(shape, spacing):
    """(names, M int64[n, 6], U int32[n, ny, nx, 2]): one section per (map, field) pair."""
    maps = _maps(*shape)
    mnames = list(MAP_NAMES) + [k for k in maps if k.startswith("limit")]
    fields = FR.case_fields(shape, spacing)
    pairs = [(m, f) for m in mnames for f in fields]
    return pairs, np.stack([maps[m] for m, _ in pairs]), np.stack([fields[f] for _, f in pairs])


def _call(lib, name, src_ptr, D, H, W, sy0, VY, dst_ptr, odims, o0, mh, md, uh, ud, grid, kk, fill, nearest, stream):
    return getattr(lib, name)(src_ptr, D, H, W, sy0, VY, dst_ptr, *odims, *o0, mh, md, uh, ud, *grid, *kk, fill, nearest, stream)


def _run(vol, M, U, spacing, obox=None, rows=None, fill=0, nearest=False, soff=0, doff=0, name="tem_u8_warp_field"):
    """One tem_u8_warp_field call, as test_gpu_warp._run: source and output `soff` and `doff` bytes into aligned
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
    mh, uh = np.ascontiguousarray(M, np.int64), np.ascontiguousarray(U, np.int32)
    assert uh.shape == (D,) + FR.grid((VY, W), spacing) + (2,)
    md, ud = torch.from_numpy(mh).cuda(), torch.from_numpy(uh).cuda()
    L.check(_call(lib, name, src.data_ptr() + GUARD + soff, D, H, W, sy0, VY, dst.data_ptr() + GUARD + doff, odims, (y0, x0),
                  mh.ctypes.data, md.data_ptr(), uh.ctypes.data, ud.data_ptr(), uh.shape[1:3], _kk(spacing), fill,
                  int(nearest), stream), name)
    got, s = dst.cpu().numpy(), src.cpu().numpy()
    assert (got[:GUARD + doff] == FILL).all() and (got[GUARD + doff + n:] == FILL).all()
    assert (s[:GUARD + soff] == FILL).all() and (s[GUARD + soff + flat.size:] == FILL).all()
    assert np.array_equal(s[GUARD + soff:GUARD + soff + flat.size], flat)
    return got[GUARD + doff:GUARD + doff + n].reshape(odims)


def _tight_rows(M, U, spacing, obox, shape, nearest=False):
    """(sy0, H): the rows the output box needs by the header's rule, over all sections; every real tap lies inside."""
    lo, hi = [], []
    for m, u in zip(M, U):
        r = FR.required_rows(m, u, spacing, obox, shape, nearest)
        rows = FR.tap_rows(m, u, spacing, obox, shape, nearest)
        assert rows.size == 0 or (r is not None and r[0] <= rows[0] and rows[-1] <= r[1])
        if r is not None:
            lo.append(r[0]), hi.append(r[1])
    return (min(lo), max(hi) - min(lo) + 1) if lo else (0, 1)


# ----------------------------------------------------------------------------------------------- tem_u8_warp_field
@pytest.mark.parametrize("spacing", SPACINGS, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_reference(shape, spacing):
    """One section per (map, field) pair, all in one launch: the whole section at the byte offsets 0...3 of source and
    output, nearest, fill 0 and 255, and an odd box off the origin.  With spacing 16 and (16, 64) a 16 x 64 tile of the
    larger sections straddles cell boundaries in both axes and the last cell is partial; (5, 4) and (1, 1) are smaller
    than one cell."""
    Y, X = shape
    pairs, M, U = _cases(shape, spacing)
    vol = _data((len(pairs), Y, X), "random")
    want = {(f, nr): FR.warp(vol, M, U, spacing, fill=f, nearest=nr) for f in (0, 255) for nr in (False, True)}
    for soff, doff in ((0, 0), (1, 3), (2, 1), (3, 2)):
        _same(_run(vol, M, U, spacing, soff=soff, doff=doff), want[0, False], (soff, doff))
    _same(_run(vol, M, U, spacing, fill=255, soff=1), want[255, False], "fill 255")
    _same(_run(vol, M, U, spacing, nearest=True, doff=1), want[0, True], "nearest")
    _same(_run(vol, M, U, spacing, fill=255, nearest=True), want[255, True], "nearest, fill 255")
    _same(_run(vol, M, U, spacing, fill=255, soff=3, doff=1, name="tem_u8_warp_field_direct"), want[255, False], "direct")
    _same(_run(vol, M, U, spacing, nearest=True, name="tem_u8_warp_field_direct"), want[0, True], "direct, nearest")
    if Y > 4 and X > 4:
        box = ((2, Y - 1), (1, X - 2))
        for off in (0, 3):
            _same(_run(vol, M, U, spacing, box, soff=off, doff=off), want[0, False][:, 2:Y - 1, 1:X - 2], ("box", off))
        _same(_run(vol, M, U, spacing, box, nearest=True, fill=255), want[255, True][:, 2:Y - 1, 1:X - 2], "box, nearest")


def _equivalent(shape, spacing):
    """[(field, map, the affine map that gives the same bytes)] for zero, constant and ramp fields over maps whose
    raised coefficient stays inside the limits."""
    maps, fields = _maps(*shape), FR.case_fields(shape, spacing)
    out = []
    for mname in ("identity", "sub", "half", "face_y1"):
        m = maps[mname]
        out.append((fields["zero"], m, m))
        c = fields["const"][0, 0].astype(np.int64)
        out.append((fields["const"], m, m + np.array([0, 0, c[0], 0, 0, c[1]])))
        for k, name in ((0, "yy"), (1, "yx"), (3, "xy"), (4, "xx")):
            for g in (DEV, -DEV):
                e = m.copy()
                e[k] += g
                out.append((fields[f"ramp_{name}{'+' if g > 0 else '-'}"], m, e))
    return out


@pytest.mark.parametrize("spacing", SPACINGS, ids=str)
@pytest.mark.parametrize("shape", [(37, 53), (40, 131)], ids=lambda s: "x".join(map(str, s)))
def test_zero_constant_and_ramp_fields_equal_the_affine_kernel(shape, spacing):
    """The three identities on the device, against tem_u8_warp_affine's own bytes: U = 0 is the map; a constant U the
    map with b moved by it; a ramp at the limit +-2^13 the map with that coefficient raised by it."""
    eq = _equivalent(shape, spacing)
    assert len(eq) == 4 * 10
    vol = _data((len(eq),) + shape, "random")
    U, M, E = (np.stack(v) for v in zip(*eq))
    for nearest in (False, True):
        want = _run_affine(vol, E, fill=9, nearest=nearest)
        _same(_run(vol, M, U, spacing, fill=9, nearest=nearest, soff=1, doff=2), want, nearest)
    _same(WR.warp(vol, E, fill=9), FR.warp(vol, M, U, spacing, fill=9), "the references agree")


def test_kernel_cases_cover_what_they_claim():
    shape, spacing = (40, 131), (16, 64)
    Y, X = shape
    pairs = _cases(shape, spacing)[0]
    maps, fields = _maps(*shape), FR.case_fields(shape, spacing)
    assert len(fields) == 18 and len(pairs) == 24 * 18 and {m for m, _ in pairs} >= {k for k in maps if k.startswith("limit")}
    ky, kx = _kk(spacing)
    ty, tx = WARP_TILE
    assert FR.grid(shape, spacing) == (4, 4) and Y % (1 << ky) and X % (1 << kx)      # the last cells are partial
    assert (16 >> ky) != ((16 + ty - 1) >> ky) - 1 and ((64 + tx - 1) >> kx) == 1       # the tile at (16, 64) is one cell
    assert (2 >> ky) != ((2 + ty - 1) >> ky) and (1 >> kx) != ((1 + tx - 1) >> kx)      # the box at (2, 1): its first tile
    assert FR.grid((37, 53), 16) == (4, 5) and FR.grid((1, 1), 16) == (2, 2) == FR.grid((5, 4), (16, 64))   # straddles both
    for name, f in fields.items():
        assert FR.within_limits(f, spacing), name
    dy, dx = np.abs(np.diff(fields["walk"].astype(np.int64), axis=0)), np.abs(np.diff(fields["walk"].astype(np.int64), axis=1))
    assert (dy == DEV << ky).all() and (dx == DEV << kx).all()                          # every difference at the limit
    assert np.abs(fields["max+"]).min() == FR.MAX_U == -fields["max-"].max()
    for k in ("yy", "yx", "xy", "xx"):
        r = fields[f"ramp_{k}+"].astype(np.int64)
        assert np.array_equal(r, -fields[f"ramp_{k}-"].astype(np.int64)) and max(np.abs(np.diff(r, axis=0)).max(),
                                                                                   np.abs(np.diff(r, axis=1)).max()) \
            == DEV << (ky if k[1] == "y" else kx)
    ident = maps["identity"]
    small = FR.case_fields((37, 53), 16)
    for k, axis in (("face_y0", 0), ("face_y1", 0), ("face_x0", 1), ("face_x1", 1)):     # half a section across each face
        inside = FR.positions(ident, small[k], 16, ((0, 37), (0, 53)), (37, 53))[2]
        assert 0.4 < inside.mean() < 0.6 and inside.all(axis=1 - axis).sum() in (18, 19, 26, 27)
    inside = FR.positions(ident, fields["max+"], spacing, ((0, Y), (0, X)), shape)[2]
    assert 0 < inside.mean() < 0.2                                                      # 32 px: 8 rows of 99 columns stay
    fy, _, ins = FR.positions(maps["limit+-+-"], fields["walk"], spacing, ((0, Y), (0, X)), shape)
    assert 0.3 < ins.mean() < 1
    spans = [np.ptp(fy[y:y + ty, x:x + tx] >> 8) + 2 for y in range(0, Y, ty) for x in range(0, X, tx)]
    assert 27 < max(spans) <= 37                                                        # past the affine hull, inside this one


def test_kernel_takes_row_cut_blocks():
    """Output rows off the origin from source blocks that hold just the rows the header's rule demands: sy0 > 0, fewer
    rows than the section, bilinear and nearest; a block one row short at either end is refused."""
    L, lib, stream = _env()
    shape, spacing = (40, 131), (16, 64)
    Y, X = shape
    maps, fields = _maps(*shape), FR.case_fields(shape, spacing)
    for names, box in (((("identity", "zero"), ("sub", "const"), ("rot", "walk2"), ("half", "walk")), ((20, 31), (0, X))),
                       ((("limit++++", "walk2"), ("limit+-+-", "ramp_yx-"), ("rot", "ramp_yy+")), ((33, 40), (5, 120))),
                       ((("identity", "walk2"), ("out_y", "walk")), ((36, 40), (60, 131)))):
        M, U = np.stack([maps[m] for m, _ in names]), np.stack([fields[f] for _, f in names])
        vol = _data((len(names), Y, X), "random")
        for nearest in (False, True):
            sy0, H = rows = _tight_rows(M, U, spacing, box, shape, nearest)
            assert H < Y and sy0 > 0
            want = FR.warp(vol, M, U, spacing, ((0, len(names)),) + box, fill=9, nearest=nearest)
            for off in (0, 1):
                _same(_run(vol, M, U, spacing, box, rows, fill=9, nearest=nearest, soff=off, doff=3 - off), want,
                      (names, nearest, off))
            src = torch.zeros(len(names) * H * X, dtype=torch.uint8, device="cuda")
            dst = torch.zeros(len(names) * Y * X, dtype=torch.uint8, device="cuda")
            mh, uh = np.ascontiguousarray(M), np.ascontiguousarray(U)
            md, ud = torch.from_numpy(mh).cuda(), torch.from_numpy(uh).cuda()
            od = (len(names), box[0][1] - box[0][0], box[1][1] - box[1][0])
            for r in ((sy0 + 1, H - 1), (sy0, H - 1)):
                assert _call(lib, "tem_u8_warp_field", src.data_ptr(), len(names), r[1], X, r[0], Y, dst.data_ptr(), od,
                             (box[0][0], box[1][0]), mh.ctypes.data, md.data_ptr(), uh.ctypes.data, ud.data_ptr(),
                             uh.shape[1:3], _kk(spacing), 0, int(nearest), stream) == L.TEM_EINVAL


REAL, REAL_SPACING = (2, 1001, 1731), 128


def test_kernel_at_the_shape_of_a_real_call():
    """A plane of 1001 x 1731 with spacing 128 (9 x 15 nodes, the last cells partial, W odd): one plane turns by half a
    degree under a field of up to a pixel, the other has matrix and field at their limits.  The whole plane, and a run
    of rows from the rows the rule demands."""
    _, Y, X = REAL
    c = np.array([(Y - 1) / 2, (X - 1) / 2])
    Lm = np.array([[1.125, -0.125], [0.125, 0.875]])
    M = WR.quantize(np.stack([WR._rigid(np.deg2rad(0.5), np.array([0.37, -1.21]), c),
                              np.concatenate([Lm, (c - Lm @ c)[:, None]], axis=1)]))
    nodes = FR.nodes((Y, X), REAL_SPACING)
    one_px = FR.quantize(np.stack([np.sin(np.pi * nodes[..., 1] / (X - 1)), -np.sin(np.pi * nodes[..., 0] / (Y - 1))], axis=-1))
    U = np.stack([one_px, FR.walk((Y, X), REAL_SPACING, 11)])
    assert FR.grid((Y, X), REAL_SPACING) == (9, 15) and FR.within_limits(U, REAL_SPACING) and 0.99 * FR.UNIT < np.abs(U[0]).max() <= FR.UNIT
    assert np.abs(np.diff(U[1].astype(np.int64), axis=0)).min() == DEV << 7
    vol = _data(REAL, "random")
    want = FR.warp(vol, M, U, REAL_SPACING, fill=3)
    assert (want[0] == 3).mean() < 0.03 and 0.02 < (want[1] == 3).mean() < 0.4
    _same(_run(vol, M, U, REAL_SPACING, fill=3, soff=1, doff=2), want, "whole")
    _same(_run(vol, M, U, REAL_SPACING, fill=3, name="tem_u8_warp_field_direct"), want, "direct")
    box = ((500, 700), (0, X))
    rows = _tight_rows(M, U, REAL_SPACING, box, (Y, X))
    assert rows[0] > 250 and rows[1] < 600
    _same(_run(vol, M, U, REAL_SPACING, box, rows, fill=3), want[:, 500:700], "rows")


def test_kernel_refuses_bad_arguments():
    """TEM_EINVAL from the host-side checks, nothing launched: dst keeps its fill."""
    L, lib, stream = _env()
    D, H, W, VY = 2, 6, 8, 10
    src = torch.ones(D * H * W + 16, dtype=torch.uint8, device="cuda")
    dst = torch.full((D * 4 * 5 + 16,), FILL, dtype=torch.uint8, device="cuda")
    mh = np.ascontiguousarray(np.stack([WR.quantize(WR.IDENTITY)] * D))
    uh = np.zeros((D, 2, 2, 2), np.int32)
    md, ud = torch.from_numpy(mh).cuda(), torch.from_numpy(uh).cuda()
    p, q, h, m, fh, fd = src.data_ptr(), dst.data_ptr(), mh.ctypes.data, md.data_ptr(), uh.ctypes.data, ud.data_ptr()
    for name in ("tem_u8_warp_field", "tem_u8_warp_field_direct"):
        call = lambda *a: getattr(lib, name)(*a, stream)
        # src D H W sy0 VY dst OD OH OW oy0 ox0 maps_host maps_dev field_host field_dev ny nx ky kx fill nearest
        ok = [p, D, H, W, 2, VY, q, D, 4, 5, 3, 2, h, m, fh, fd, 2, 2, 4, 4, 0, 0]
        for i, v in [(0, None), (6, None), (12, None), (13, None), (14, None), (15, None), (1, 0), (2, 0), (3, 0), (5, 0),
                     (7, 0), (8, 0), (9, 0), (1, -1), (7, 1), (7, 3), (4, -1), (10, -1), (11, -1), (4, 5), (5, 7), (10, 7),
                     (11, 4), (9, 7), (20, -1), (20, 256), (21, 2), (21, -1), (4, 4), (2, 4), (2, 2), (10, 1), (8, 6),
                     (16, 1), (16, 3), (17, 1), (17, 3), (18, 3), (18, 11), (19, 3), (19, 11)]:
            a = list(ok)
            a[i] = v
            assert call(*a) == L.TEM_EINVAL, (i, v)
        for j, v in [(0, ONE + DEV + 1), (1, -DEV - 1), (3, DEV + 1), (4, ONE - DEV - 1), (2, 1 << 47), (5, -(1 << 47))]:
            bad = mh.copy()
            bad[1, j] = v                                                               # in the second section only
            assert call(*ok[:12], bad.ctypes.data, *ok[13:]) == L.TEM_EINVAL, (j, v)
        for idx, v in [((1, 0, 0, 0), FR.MAX_U + 1), ((1, 1, 1, 1), -FR.MAX_U - 1), ((1, 0, 0, 0), (DEV << 4) + 1),
                       ((1, 0, 1, 1), -(DEV << 4) - 1), ((0, 1, 1, 0), (DEV << 4) + 1)]:
            bad = uh.copy()
            bad[idx] = v
            assert call(*ok[:14], bad.ctypes.data, *ok[15:]) == L.TEM_EINVAL, (idx, v)
        up = uh.copy()
        up[...] = 256                                                                   # 1/256 px down: ty = 1
        upd = torch.from_numpy(up).cuda()
        moved = ok[:10] + [4, 2] + ok[12:14] + [up.ctypes.data, upd.data_ptr()] + ok[16:]
        assert call(*moved) == L.TEM_EINVAL                                             # rows 4...8: row 8 is not in the block
        torch.cuda.synchronize()
        assert (dst.cpu().numpy() == FILL).all()
        assert call(*(ok[:14] + [up.ctypes.data, upd.data_ptr()] + ok[16:])) == 0       # rows 3...7 are in the block
        assert call(*(ok[:10] + [4, 2] + ok[12:])) == 0                                 # at ty = 0 row 8 is no tap
        at = uh.copy()
        at[1, 0, :, 1], at[1, 1, :, 1] = DEV << 4, 0                                    # a difference at the limit passes
        atd = torch.from_numpy(at).cuda()
        assert call(*(ok[:14] + [at.ctypes.data, atd.data_ptr()] + ok[16:])) == 0
        assert call(*ok) == 0 and call(p + 3, *ok[1:]) == 0                             # and the good call runs
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert (got[:D * 4 * 5] == 1).all() and (got[D * 4 * 5:] == FILL).all()
        dst.fill_(FILL)


# ------------------------------------------------------------------------------------------------ volume_warp_field
VSHAPE, VSPACING = (6, 37, 53), 16
BUDGETS = {"whole": 6 * 37 * 53, "two_sections": 2 * 37 * 53, "ten_rows": 10 * 53, "one_row": 53}


@functools.lru_cache(maxsize=None)
def _vcase():
    _, Y, X = VSHAPE
    vol = np.random.default_rng(29).integers(0, 256, VSHAPE, dtype=np.uint8)
    maps, fields = _maps(Y, X), FR.case_fields((Y, X), VSPACING)
    M = np.stack([maps[k] for k in ("rot", "sub", "limit+-+-", "out_y", "face_y1", "half")])
    U = np.stack([fields[k] for k in ("walk", "ramp_yx-", "walk2", "walk", "const", "face_x0")])
    want = FR.warp(vol, M, U, VSPACING, fill=11)
    vol.setflags(write=False), M.setflags(write=False), U.setflags(write=False), want.setflags(write=False)
    return vol, M, U, want


@pytest.fixture(scope="module")
def vmap(tmp_path_factory):
    path = tmp_path_factory.mktemp("field") / "vol.u8"
    m = np.memmap(path, np.uint8, "w+", shape=VSHAPE)
    m[...] = _vcase()[0]
    m.flush()
    return np.memmap(path, np.uint8, "r", shape=VSHAPE)


@pytest.mark.parametrize("budget", list(BUDGETS), ids=list(BUDGETS))
def test_volume_warp_field_equals_the_reference_however_it_is_cut(vmap, budget, tmp_path):
    from transfer_em_amd.utils import field_chunks, volume_warp_field
    vol, M, U, want = _vcase()
    out = np.memmap(tmp_path / "out.u8", np.uint8, "w+", shape=VSHAPE)
    st, n = {}, 0
    for rank in (1, 0):
        res, counts = _counted(lambda: volume_warp_field(vmap, M, U, VSPACING, out=out, fill=11, chunk_bytes=BUDGETS[budget],
                                                         rank=rank, world_size=2, stats=st))
        mine = len(field_chunks(((0, 6), (0, 37), (0, 53)), VSHAPE, M, U, VSPACING, BUDGETS[budget], rank, 2))
        assert res is out and st["chunks"] == mine == counts["tem_u8_warp_field"]       # one launch per slab
        assert st["read_s"] >= 0 and st["write_s"] >= 0
        n += mine
    _same(np.asarray(out), want, budget)
    assert {"whole": n == 1, "two_sections": n == 3, "ten_rows": n > 6 * 4, "one_row": n == 6 * 37}[budget]
    assert np.array_equal(np.asarray(vmap), vol)                                        # the input: read only


def test_volume_warp_field_of_an_roi_float_inputs_one_image_and_nearest(vmap):
    from transfer_em_amd.utils import quantize_field, quantize_maps, volume_warp, volume_warp_field
    vol, M, U, want = _vcase()
    got = volume_warp_field(vmap, M, U, VSPACING, start=(5, 3, 1), size=(41, 30, 4), fill=11, chunk_bytes=7 * 53)
    _same(got, want[1:5, 3:33, 5:46], "roi")
    T = np.stack([WR._rigid(0.02 * z, np.array([0.25 * z, -0.5]), np.array([18.0, 26.0])) for z in range(6)])
    nodes = FR.nodes(VSHAPE, VSPACING)
    F = np.stack([np.stack([0.3 * z * np.sin(nodes[..., 1] / 17.0), np.cos(nodes[..., 0] / 12.0 + z)], axis=-1)
                  for z in range(6)])
    qm, qf = quantize_maps(T), quantize_field(F, VSPACING)
    assert np.array_equal(qf, FR.quantize(F)) and qf.dtype == np.int32
    _same(volume_warp_field(vol, T, F, VSPACING), FR.warp(vol, qm, qf, VSPACING), "float inputs, an ndarray, the default slab")
    _same(volume_warp_field(vol, T, F, VSPACING, nearest=True, fill=255), FR.warp(vol, qm, qf, VSPACING, fill=255, nearest=True),
          "nearest")
    _same(volume_warp_field(vol[2], T[3], F[4], VSPACING, fill=5), FR.warp(vol[2:3], qm[3:4], qf[4:5], VSPACING, fill=5)[0],
          "one image")
    _same(volume_warp_field(vol[2], M[0], U[0], VSPACING, start=(3, 4), size=(50, 20)),
          FR.warp(vol[2:3], M[:1], U[:1], VSPACING)[0, 4:24, 3:53], "one image, roi")
    _same(volume_warp_field(vol, T, np.zeros_like(F), VSPACING, fill=7), volume_warp(vol, T, fill=7), "zero fields: volume_warp")


# ------------------------------------------------------------------------------------------------------- end to end
def test_the_distortion_is_measured_and_undone():
    """section_shift_sums -> shift_subpixel -> fit_section_maps -> fit_section_fields -> section_fields ->
    volume_warp_field -> section_shift_sums on the fixture of smoothly distorted sections: the result is the reference's
    byte for byte, every interior tile re-measures (0, 0), and the interior tiles' mean correlation is above what
    volume_warp with the affine maps alone reaches."""
    from transfer_em_amd.utils import (fit_section_fields, fit_section_maps, quantize_field, quantize_maps, section_fields,
                                       section_shift_sums, section_shifts, shift_counts, shift_scores, shift_subpixel,
                                       volume_warp, volume_warp_field)
    v = FR.distorted_volume()
    tile, r, S = FR.FIX_TILE, FR.FIX_RADIUS, FR.FIX_SPACING
    n = shift_counts(v.shape, tile, r)
    sub = shift_subpixel(section_shift_sums(v, tile, r), n)
    fit = fit_section_maps(sub, tile, v.shape)
    ff = fit_section_fields(sub, fit, tile, v.shape, S)
    assert sub.decided.all() and fit.unresolved == []
    B, F = section_fields(fit.maps, ff.fields, S, v.shape)
    warped = volume_warp_field(v, B, F, S, chunk_bytes=3 * 192 * 256)
    _same(warped, FR.warp(v, quantize_maps(B), quantize_field(F, S), S), "the warp")
    affine = volume_warp(v, B)

    def interior(vol):
        q2 = section_shift_sums(vol, tile, r)
        return shift_scores(q2, n)[:, 1:-1, 1:-1, r, r].mean(), section_shifts(q2, n).tiles[:, 1:-1, 1:-1]
    (c_raw, _), (c_affine, t_affine), (c_field, t_field) = interior(v), interior(affine), interior(warped)
    print("interior tiles' mean correlation: raw", c_raw, "affine", c_affine, "field", c_field,
          "; interior tiles off (0, 0) after the affine warp:", int(t_affine.any(axis=-1).sum()))
    assert not t_field.any()
    assert c_field > c_affine
