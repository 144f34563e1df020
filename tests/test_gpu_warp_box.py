"""tem_u8_warp_box on the device: tem_u8_warp_affine's and tem_u8_warp_field's bytes from a source block that is cut in y
and in x.  Every call is held against the existing entry on the whole rows and against the numpy references, byte for
byte; the source box sits between guards at every alignment and must come back untouched with them; a box one row or
one column short of what utils.warp_source_box plans is refused without a launch.  Guards, data and the runners of the
existing entries are test_gpu_warp.py's and test_gpu_field.py's."""
import functools

import numpy as np
import pytest
import torch

import field_ref as FR
import warp_box_cases as C
import warp_ref as WR
from test_gpu_field import _run as _run_field
from test_gpu_histogram import _env
from test_gpu_warp import _maps, _run as _run_affine, _same
from test_gpu_zcorr import FILL, GUARD, _data

pytestmark = pytest.mark.gpu

Y, X = SEC = (110, 150)
GENTLE = ("identity", "sub", "half", "rot", "lsb", "limit++++", "limit+-+-", "limit-++-", "limit----")
WILD = ("face_y0", "face_y1", "face_x0", "face_x1", "out_y", "out_x", "just_out", "last_row", "last_col", "far", "rot")
FORMS = [(f, n) for f in (False, True) for n in (False, True)]
IDS = ["affine", "affine-nearest", "field", "field-nearest"]


@functools.lru_cache(maxsize=None)
def _group(names, field):
    """(vol, M, U): one section per named map of test_gpu_warp._maps, with warp_box_cases' random 2 px fields or none."""
    maps = _maps(Y, X)
    M = np.stack([maps[k] for k in names])
    U = C.stack((len(names), Y, X), seed=len(names))[1] if field else None
    return _data((len(names), Y, X), "random"), M, U


def _plan(M, U, obox, nearest):
    from transfer_em_amd.utils import Warp, warp_source_box
    W = Warp(M, U, C.SPACING if U is not None else None)
    return warp_source_box(((0, len(M)),) + tuple(obox), W, (len(M), Y, X), nearest=nearest)


def _call(vol, M, U, obox, sbox, fill, nearest, soff, doff):
    """One tem_u8_warp_box call: (its return code, the output block).  The source box `sbox` of every section sits `soff` bytes
    into an aligned allocation between guards of FILL, the output box `doff` bytes into another."""
    L, lib, stream = _env()
    D, VY, VX = vol.shape
    (y0, y1), (x0, x1) = obox
    (sy0, sy1), (sx0, sx1) = sbox
    flat = np.ascontiguousarray(vol[:, sy0:sy1, sx0:sx1]).reshape(-1)
    src = torch.full((flat.size + soff + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    src[GUARD + soff:GUARD + soff + flat.size] = torch.from_numpy(flat.copy()).cuda()
    odims = (D, y1 - y0, x1 - x0)
    n = int(np.prod(odims))
    dst = torch.full((n + doff + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 256 == 0 and dst.data_ptr() % 256 == 0
    mh = np.ascontiguousarray(M, np.int64)
    md = torch.from_numpy(mh).cuda()
    if U is None:
        fld = (None, None, 0, 0, 0, 0)
    else:
        uh = np.ascontiguousarray(U, np.int32)
        ud = torch.from_numpy(uh).cuda()
        k = C.SPACING.bit_length() - 1
        fld = (uh.ctypes.data, ud.data_ptr(), uh.shape[1], uh.shape[2], k, k)
    rc = lib.tem_u8_warp_box(src.data_ptr() + GUARD + soff, D, sy1 - sy0, sx1 - sx0, sy0, sx0, VY, VX,
                             dst.data_ptr() + GUARD + doff, *odims, y0, x0, mh.ctypes.data, md.data_ptr(), *fld, fill,
                             int(nearest), stream)
    got, s = dst.cpu().numpy(), src.cpu().numpy()
    assert (got[:GUARD + doff] == FILL).all() and (got[GUARD + doff + n:] == FILL).all()
    assert (s[:GUARD + soff] == FILL).all() and (s[GUARD + soff + flat.size:] == FILL).all()
    assert np.array_equal(s[GUARD + soff:GUARD + soff + flat.size], flat)
    return rc, got[GUARD + doff:GUARD + doff + n].reshape(odims)


def _run(vol, M, U, obox, sbox, fill=0, nearest=False, soff=0, doff=0):
    L = _env()[0]
    rc, got = _call(vol, M, U, obox, sbox, fill, nearest, soff, doff)
    L.check(rc, "tem_u8_warp_box")
    return got


def _existing(vol, M, U, obox, fill, nearest):
    """The existing entry's bytes for the same output box, from whole rows of the whole section."""
    if U is None:
        return _run_affine(vol, M, obox, fill=fill, nearest=nearest)
    return _run_field(vol, M, U, C.SPACING, obox, fill=fill, nearest=nearest)


def _want(vol, M, U, obox, fill, nearest):
    """... which are the numpy reference's."""
    want = _existing(vol, M, U, obox, fill, nearest)
    _same(want, C.warp(vol, M, U, ((0, len(M)),) + tuple(obox), fill, nearest), "the existing entry against numpy")
    return want


# ----------------------------------------------------------------------------------------------------------- sweep
@pytest.mark.parametrize("field,nearest", FORMS, ids=IDS)
def test_box_cut_on_both_sides_at_every_alignment(field, nearest):
    """An output box of 55 x 100 off the tile grid (4 x 2 workgroups per plane, the last ones 7 rows and 36 columns) of
    nine sections under gentle maps and the maps at the +-1/8 limits.  The planner's box is cut on all four sides; it is
    widened by 0...3 columns on the left, so that sx0 takes every residue mod 4, and by 0 or 1 on the right, so that BW
    is even and odd -- an odd BW makes a row's alignment change from row to row --, at the four alignments of the source
    pointer and with the output off alignment."""
    vol, M, U = _group(GENTLE, field)
    obox = ((20, 75), (30, 130))
    (ty0, ty1), (tx0, tx1) = tight = _plan(M, U, obox, nearest)
    assert 0 < ty0 and ty1 < Y and 3 <= tx0 and tx1 + 1 < X                   # cut on all four sides, with room to widen
    want = _want(vol, M, U, obox, 7, nearest)
    assert (want == 7).mean() < 0.02 and len(np.unique(want)) > 100
    seen = set()
    for e in range(4):
        sbox = ((ty0, ty1), (tx0 - e, tx1 + (e >> 1)))
        for soff in range(4):
            _same(_run(vol, M, U, obox, sbox, 7, nearest, soff, (soff + e) % 4), want, (sbox, soff))
            seen.add(((tx0 - e) % 4, (sbox[1][1] - sbox[1][0]) % 2, soff))
    assert len({s[0] for s in seen}) == 4 and len({s[1] for s in seen}) == 2
    _same(_run(vol, M, U, obox, ((ty0 - 1, ty1 + 2), tight[1]), 7, nearest), want, "more rows than needed")


@pytest.mark.parametrize("field,nearest", FORMS, ids=IDS)
def test_box_flush_with_each_face(field, nearest):
    """Output boxes at each face of the section under the gentle maps: the planner's box is flush with that face and cut
    on the opposite side.  And the whole section under maps that move it half a section across each face, wholly
    outside, or by far: the box is the section, sx0 = 0 and BW = VX, and the bytes are the existing entries'."""
    vol, M, U = _group(GENTLE, field)
    faces = {"y0": ((0, 30), (40, 101)), "y1": ((80, Y), (40, 101)), "x0": ((40, 71), (0, 50)), "x1": ((40, 71), (99, X))}
    for face, obox in faces.items():
        sbox = _plan(M, U, obox, nearest)
        flush = {"y0": sbox[0][0] == 0, "y1": sbox[0][1] == Y, "x0": sbox[1][0] == 0, "x1": sbox[1][1] == X}
        assert flush[face] and sum(flush.values()) == 1, (face, sbox)
        _same(_run(vol, M, U, obox, sbox, 200, nearest, 1, 2), _want(vol, M, U, obox, 200, nearest), face)
    vol, M, U = _group(WILD, field)
    whole = ((0, Y), (0, X))
    assert _plan(M, U, whole, nearest) == whole
    want = _want(vol, M, U, whole, 3, nearest)
    for soff in (0, 3):
        _same(_run(vol, M, U, whole, whole, 3, nearest, soff, 1), want, ("whole", soff))


@pytest.mark.parametrize("field,nearest", FORMS, ids=IDS)
def test_block_with_tiles_wholly_outside(field, nearest):
    """Sections moved by about 100 columns, and one also by 70 rows: of the 7 x 3 workgroups per plane the right column
    (and under the second map the lower rows) writes fill without staging anything, the middle column straddles the
    section's face, and the source box is the section's right 50-odd columns -- a third of its width."""
    maps = np.stack([WR.quantize(np.array([[1.0, 0.0, dy], [0.0, 1.0, dx]])) for dy, dx in ((0.0, 100.0), (70.4, 97.5),
                                                                                          (-1.25, 110.0), (3.0, 99.75))])
    vol = _data((4, Y, X), "random")
    U = C.stack((4, Y, X), seed=11)[1] if field else None
    obox = ((5, Y), (0, X))
    sbox = _plan(maps, U, obox, nearest)
    assert sbox[1][1] == X and 90 <= sbox[1][0] <= 100 and sbox[0][0] > 0
    want = _want(vol, maps, U, obox, 99, nearest)
    assert (want[:, :, 64:] == 99).all() and (want[1, 48:] == 99).all() and (want[:, :, :40] != 99).any()
    for soff in (0, 2):
        _same(_run(vol, maps, U, obox, sbox, 99, nearest, soff, 3 - soff), want, soff)


def test_box_at_the_shape_of_a_real_call():
    """Two planes of 301 x 1731 (odd: a row's alignment changes from row to row in the section, and with BW = 331 in the
    box too), an output box of 200 x 326 in the middle -- a chunk's footprint inside a section five times as wide --
    turned by half a degree and moved by a sub-pixel, with and without a field of a pixel at spacing 32."""
    D, VY, VX = shape = (2, 301, 1731)
    vol = _data(shape, "random")
    c = np.array([(VY - 1) / 2, (VX - 1) / 2])
    M = WR.quantize(np.stack([WR._rigid(np.deg2rad(0.5), np.array([0.3, -0.7]), c), WR._rigid(-np.deg2rad(0.5), np.array([-1.6, 2.2]), c)]))
    rng = np.random.default_rng(3)
    U = FR.quantize(rng.uniform(-1, 1, (D,) + FR.grid((VY, VX), C.SPACING) + (2,)))
    obox = ((50, 250), (700, 1026))
    from transfer_em_amd.utils import Warp, warp_source_box
    for u in (None, U):
        sbox = warp_source_box(((0, D),) + obox, Warp(M, u, None if u is None else C.SPACING), shape)
        bw = sbox[1][1] - sbox[1][0]
        assert 326 < bw < 345 and sbox[1][0] > 600 and sbox[0][0] > 30 and sbox[0][1] < 270
        want = C.warp(vol, M, u, ((0, D),) + obox, 5)
        assert (want == 5).mean() < 0.02                                        # every voxel is inside: no fill
        for widen in (0, 1):                                                    # BW of either parity
            box = (sbox[0], (sbox[1][0], sbox[1][1] + widen))
            _same(_run(vol, M, u, obox, box, 5, False, 1, 2), want, (u is None, widen))


# -------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("field,nearest", FORMS, ids=IDS)
def test_a_box_one_row_or_one_column_short_is_refused(field, nearest):
    """The planner's box is exactly what the entry demands: it runs, and with one row or one column fewer on any of its
    four sides the call is TEM_EINVAL and dst keeps its fill."""
    L = _env()[0]
    vol, M, U = _group(GENTLE, field)
    obox = ((20, 75), (30, 130))
    (ty0, ty1), (tx0, tx1) = _plan(M, U, obox, nearest)
    for sbox in (((ty0 + 1, ty1), (tx0, tx1)), ((ty0, ty1 - 1), (tx0, tx1)), ((ty0, ty1), (tx0 + 1, tx1)),
                 ((ty0, ty1), (tx0, tx1 - 1))):
        rc, got = _call(vol, M, U, obox, sbox, 0, nearest, 0, 0)
        assert rc == L.TEM_EINVAL and (got == FILL).all(), sbox
    rc, got = _call(vol, M, U, obox, ((ty0, ty1), (tx0, tx1)), 0, nearest, 0, 0)
    assert rc == 0 and not (got == FILL).all()


def test_entry_refuses_bad_arguments():
    """TEM_EINVAL from the host-side checks, nothing launched: what the existing entries refuse, a box that leaves the
    section, and one field pointer without the other."""
    L, lib, stream = _env()
    D, BH, BW, VY, VX = 2, 6, 9, 10, 40
    src = torch.ones(D * BH * BW + 16, dtype=torch.uint8, device="cuda")
    dst = torch.full((D * 4 * 5 + 16,), FILL, dtype=torch.uint8, device="cuda")
    mh = np.ascontiguousarray(np.stack([WR.quantize(WR.IDENTITY)] * D))
    md = torch.from_numpy(mh).cuda()
    uh = np.zeros((D, 2, 4, 2), np.int32)                                    # the lattice of (10, 40) at spacing 16
    ud = torch.from_numpy(uh).cuda()
    p, q, h, m = src.data_ptr(), dst.data_ptr(), mh.ctypes.data, md.data_ptr()
    call = lambda *a: lib.tem_u8_warp_box(*a, stream)
    # 0 src, 1 D, 2 BH, 3 BW, 4 sy0, 5 sx0, 6 VY, 7 VX, 8 dst, 9 OD, 10 OH, 11 OW, 12 oy0, 13 ox0, 14 maps_host, 15 maps_dev,
    # 16 field_host, 17 field_dev, 18 ny, 19 nx, 20 ky, 21 kx, 22 fill, 23 nearest: rows 2...7, columns 20...28; box (3...6, 22...26)
    ok = [p, D, BH, BW, 2, 20, VY, VX, q, D, 4, 5, 3, 22, h, m, None, None, 0, 0, 0, 0, 0, 0]
    okf = ok[:16] + [uh.ctypes.data, ud.data_ptr(), 2, 4, 4, 4, 0, 0]
    bad = [(0, None), (8, None), (14, None), (15, None), (1, 0), (2, 0), (3, 0), (6, 0), (7, 0), (9, 1), (9, 3), (10, 0),
           (11, 0), (4, -1), (5, -1), (12, -1), (13, -1), (22, -1), (22, 256), (23, 2), (23, -1),
           (4, 5), (6, 7), (5, 32), (7, 28), (12, 7), (13, 36), (11, 19),                           # a box that leaves the section
           (4, 4), (2, 4), (2, 2), (12, 1), (10, 6),                                                  # rows that are not there
           (5, 23), (3, 6), (3, 2), (13, 19), (11, 8)]                                                # columns that are not there
    for i, v in bad:
        for base in (ok, okf):
            a = list(base)
            a[i] = v
            assert call(*a) == L.TEM_EINVAL, (i, v, base is okf)
    for i, v in [(16, None), (17, None), (18, 3), (19, 3), (20, 3), (21, 11), (21, 5)]:               # the field's own
        a = list(okf)
        a[i] = v
        assert call(*a) == L.TEM_EINVAL, (i, v)
    assert call(*ok[:16], uh.ctypes.data, None, 2, 4, 4, 4, 0, 0) == L.TEM_EINVAL
    right = mh.copy()
    right[:, 5] = 256                                                         # 1/256 px to the right: tx = 1
    rd = torch.from_numpy(right).cuda()
    assert call(*ok[:13], 24, right.ctypes.data, rd.data_ptr(), *ok[16:]) == L.TEM_EINVAL            # columns 24...29: 29 is not there
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == FILL).all()
    assert call(*ok[:13], 24, h, m, *ok[16:]) == 0                           # at tx = 0 column 29 is no tap
    assert call(*ok[:14], right.ctypes.data, rd.data_ptr(), *ok[16:]) == 0   # columns 22...27 are there
    assert call(*ok) == 0 and call(*okf) == 0 and call(p + 3, *okf[1:]) == 0
    assert call(*ok[:16], None, None, -1, -1, 99, 99, 0, 0) == 0             # no field: the lattice is not looked at
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[:D * 4 * 5] == 1).all() and (got[D * 4 * 5:] == FILL).all()
