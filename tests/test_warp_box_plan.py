"""The host side of the warp= keyword of predict_cube / predict_volume, without a GPU: utils.warp_source_box against the
taps that the numpy references (warp_ref, field_ref) compute by brute force, its exact identities, utils.Warp's
validation, the binding of tem_u8_warp_box, and the frames rule -- what lives in the raw frame and what in the aligned
one -- on a small case, with numpy standing in for the device leg of predict_volume's chunks."""
import types

import numpy as np
import pytest

import repair_ref as RR
import warp_box_cases as C
import warp_ref as WR
from transfer_em_amd import utils
from transfer_em_amd.utils import Warp, chunk_plan, warp_source_box

SHAPE = (6, 110, 150)
IDENT = np.array([1 << 16, 0, 0, 0, 1 << 16, 0], np.int64)


def _boxes(shape, n, seed):
    """n random non-empty (z, y, x) boxes of the volume, the first few flush with its faces."""
    rng = np.random.default_rng(seed)
    Z, Y, X = shape
    out = [((0, Z), (0, Y), (0, X)), ((0, 1), (0, 1), (0, 1)), ((Z - 1, Z), (Y - 1, Y), (X - 1, X)), ((1, 3), (0, 40), (90, X)),
           ((2, 5), (60, Y), (0, 33))]
    while len(out) < n:
        lo = [int(rng.integers(0, m)) for m in shape]
        out.append(tuple((a, int(rng.integers(a + 1, min(a + 80, m) + 1))) for a, m in zip(lo, shape)))
    return out


@pytest.mark.parametrize("field", [True, False], ids=["field", "affine"])
@pytest.mark.parametrize("nearest", [False, True], ids=["bilinear", "nearest"])
def test_planned_box_holds_every_tap(field, nearest):
    """Sections turned by up to +-0.012 rad, moved by up to +-3 px and bent by a 2 px field at spacing 32: every tap of
    weight above 0 that the references find, voxel by voxel, lies in the box the planner returns; the box lies in the
    volume; and where every voxel of the output box is inside its section the planner's box is at most the field's range
    (4 px) and one tap wider than the hull of the taps on any side."""
    M, U = C.stack(SHAPE, field=field)
    W = Warp(M, U, C.SPACING if field else None)
    tight = 0
    for box in _boxes(SHAPE, 40, 3):
        got = warp_source_box(box, W, SHAPE, nearest=nearest)
        hull = C.tap_hull(M, U, box, SHAPE, nearest)
        if hull is None:
            continue
        assert got is not None, box
        for (a, b), (lo, hi), n in zip(got, hull, SHAPE[1:]):
            assert 0 <= a <= lo and hi <= b <= n, (box, got, hull)
        if all(C.positions(M[z], None if U is None else U[z], box[1:], SHAPE[1:])[2].all() for z in range(*box[0])):
            tight += 1
            slack = 5 if field else 0                # the affine rule is exact: the extremes sit at the corners
            for (a, b), (lo, hi) in zip(got, hull):
                assert lo - a <= slack and b - hi <= slack, (box, got, hull)
    assert tight >= 10


def test_identity_maps_and_a_zero_field_give_the_box_itself():
    Z, Y, X = SHAPE
    M = np.tile(IDENT, (Z, 1))
    zero = np.zeros((Z,) + utils.field_grid(SHAPE, 32) + (2,), np.int32)
    for W in (Warp(M), Warp(M, zero, 32), Warp(np.tile(WR.IDENTITY, (Z, 1, 1)), zero.astype(np.float64), (32, 32))):
        for box in _boxes(SHAPE, 25, 4):
            for nearest in (False, True):
                assert warp_source_box(box, W, SHAPE, nearest=nearest) == tuple(box[1:]), (box, nearest)


def test_a_box_wholly_outside_needs_nothing():
    Z, Y, X = SHAPE
    box = ((1, 4), (10, 50), (20, 90))
    for col, by in ((2, Y + 5), (2, -60), (5, X), (5, -95)):      # b_y or b_x moves every voxel of the box past a face
        M = np.tile(IDENT, (Z, 1))
        M[:, col] = by << 16
        assert warp_source_box(box, Warp(M), SHAPE) is None
        assert warp_source_box(box, Warp(M), SHAPE, nearest=True) is None
        M[2] = IDENT                                            # one section of the box comes back: its rows and columns alone
        assert warp_source_box(box, Warp(M), SHAPE) == ((10, 50), (20, 90))
        assert warp_source_box(((3, 4),) + box[1:], Warp(M), SHAPE) is None
    M = np.tile(IDENT, (Z, 1))
    M[:, 2] = ((Y - 1) << 16) - (10 << 16) + 128 * 256           # fy = 256 (Y - 1) + 128 at y = 10: outside by half a pixel
    assert warp_source_box(((0, Z), (10, 11), (0, X)), Warp(M), SHAPE) is None
    M[:, 2] -= 128 * 256                                          # ... and exactly the last row
    assert warp_source_box(((0, Z), (10, 11), (0, X)), Warp(M), SHAPE) == ((Y - 1, Y), (0, X))


def test_half_a_pixel_adds_the_next_row_and_column():
    Z, Y, X = SHAPE
    M = np.tile(IDENT, (Z, 1))
    M[:, 2], M[:, 5] = 1 << 15, -(1 << 15)                       # +0.5 px in y, -0.5 px in x
    box = ((0, Z), (10, 20), (30, 40))
    assert warp_source_box(box, Warp(M), SHAPE) == ((10, 21), (29, 40))
    assert warp_source_box(box, Warp(M), SHAPE, nearest=True) == ((11, 21), (30, 40))      # half up in both
    assert warp_source_box(((0, Z), (0, 5), (0, 5)), Warp(M), SHAPE) == ((0, 6), (0, 5))    # fx < 0 is outside, not a tap


def test_planner_refuses_what_it_cannot_plan():
    M = np.tile(IDENT, (SHAPE[0], 1))
    for box in (((0, 1), (0, 1), (0, SHAPE[2] + 1)), ((0, 1), (5, 5), (0, 1)), ((-1, 1), (0, 1), (0, 1))):
        with pytest.raises(ValueError, match="empty or reaches outside"):
            warp_source_box(box, Warp(M), SHAPE)
    with pytest.raises(ValueError, match="needs a Warp"):
        warp_source_box(((0, 1), (0, 1), (0, 1)), None, SHAPE)
    with pytest.raises(ValueError, match=r"\[z, y, x\]"):
        warp_source_box(((0, 1), (0, 1), (0, 1)), Warp(M), SHAPE[1:])


def _bad_warps():
    Z, Y, X = SHAPE
    M, U = C.stack(SHAPE)
    far, steep, big = M.copy(), U.copy(), U.copy()
    far[3, 1] = (1 << 13) + 1
    steep[2, 1, 1, 0], steep[2, 1, 2, 0] = 0, (32 << 13) + 1
    big[4, 0, 0, 1] = (1 << 21) + 1
    return [(Warp(M[1:]), "maps must be floats of shape"), (Warp(M.astype(np.int32)), "maps must be floats of shape"),
            (Warp(far), "outside the limits"), (Warp(np.full((Z, 2, 3), np.nan)), "maps must be finite"),
            (Warp(M, U), "go together"), (Warp(M, None, 32), "go together"), (Warp(M, U, 48), "power of two"),
            (Warp(M, U, 8), "power of two"), (Warp(M, U[:, 1:], 32), "fields must be floats or int32 of shape"),
            (Warp(M, steep, 32), "above the limit of 1/8 of the spacing"), (Warp(M, big, 32), "outside the limit of 32 px"),
            (Warp(M, fill=256), "fill must lie in 0...255"), (Warp(M, fill=-1), "fill must lie in 0...255"),
            (Warp(M, fill=1.5), "fill must be an integer"), ((M,), "warp must be None or a Warp"), (7, "warp must be None or a Warp")]


def test_warp_raises_the_existing_errors_before_any_gpu_work(monkeypatch):
    """Every refusal is a ValueError with the text that volume_warp / volume_warp_field give, from the planner and from
    predict_cube / predict_volume ahead of the first touch of the GPU."""
    from transfer_em_amd import hip_ops

    def no_gpu():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(hip_ops, "require_gpu", no_gpu)
    vol = np.zeros(SHAPE, np.uint8)
    models = [types.SimpleNamespace(generator_g=types.SimpleNamespace(is3d=d, plan=None), outdimsize=36, buffer=19)
              for d in (True, False)]
    for warp, text in _bad_warps():
        with pytest.raises(ValueError, match=text):
            warp_source_box(((0, 1), (0, 8), (0, 8)), warp, SHAPE)
        for model in models:
            for fn in (utils.predict_cube, utils.predict_volume):
                with pytest.raises(ValueError, match=text):
                    fn(vol, (0, 0, 0), (36, 36, 2), model, (0.0, 1.0), (0.0, 1.0), warp=warp)
    M = C.stack(SHAPE)[0]
    for fn in (utils.predict_cube, utils.predict_volume):
        with pytest.raises(ValueError, match="uint8"):
            fn(vol.astype(np.int16), (0, 0, 0), (36, 36, 2), models[0], (0.0, 1.0), (0.0, 1.0), warp=Warp(M))
        with pytest.raises(ValueError, match="maps must be floats of shape"):      # one image takes one map
            fn(vol[0], (0, 0), (36, 36), models[1], (0.0, 1.0), (0.0, 1.0), warp=Warp(M))


def test_warp_takes_what_volume_warp_takes():
    M, U = C.stack(SHAPE)
    w = utils._check_warp(Warp(M, U, 32, fill=9), SHAPE)
    assert np.array_equal(w.M, M) and np.array_equal(w.U, U) and (w.ny, w.nx, w.ky, w.kx, w.fill) == (5, 6, 5, 5, 9)
    assert w.M.flags.c_contiguous and w.U.flags.c_contiguous and w.M.dtype == np.int64 and w.U.dtype == np.int32
    f = utils._check_warp(Warp(M.reshape(-1, 2, 3) / 65536.0, U / 65536.0, (32, 32)), SHAPE)      # floats are quantised
    assert np.array_equal(f.M, M) and np.array_equal(f.U, U)
    a = utils._check_warp(Warp(M), SHAPE)
    assert a.U is None and (a.ny, a.nx, a.ky, a.kx, a.fill) == (0, 0, 0, 0, 0)
    one = utils._check_warp(Warp(M[1], U[1], 32), SHAPE[1:])                                       # one image, one map, one field
    assert one.M.shape == (1, 6) and one.U.shape == (1, 5, 6, 2)
    assert utils._check_warp(None, SHAPE) is None and utils._check_warp(w, SHAPE) is w
    assert Warp(M) == (M, None, None, 0) and Warp._fields == ("maps", "fields", "spacing", "fill")


def test_the_entry_is_declared_and_bound():
    import ctypes as C_
    import inspect
    from transfer_em_amd import _lib
    sig = _lib._SIGS["tem_u8_warp_box"]
    assert len(sig) == 25 and [i for i, t in enumerate(sig) if t is C_.c_void_p] == [0, 8, 14, 15, 16, 17, 24]
    for fn in (utils.predict_cube, utils.predict_volume):
        assert inspect.signature(fn).parameters["warp"].default is None
    for fn in (utils.predict_ng_cube, utils.predict_cube_from_saved_model):      # the reference's signatures stay
        assert "warp" not in inspect.signature(fn).parameters


# ------------------------------------------------------------------------------------------------- the frames rule
F_SHAPE, F_START, F_SIZE, F_GAP, F_FILL = (20, 60, 120), (-5, 3, -2), (110, 50, 20), 3, 37
F_SECTIONS = [0, 7, 8, 19]


def test_frames_rule_with_a_host_stand_in_for_the_device_leg():
    """predict_volume's reads under warp + repair, chunk by chunk, with the numpy references standing in for
    tem_u8_warp_box and tem_u8_repair_z.  The raw volume and the raw mask are seen only through the boxes that
    _warp_footprints plans (everything else is scrambled); the footprint each chunk then holds equals the same box of
    repair(A, sections, mask moved with nearest), A the aligned volume: the mask lives in the raw frame, the sections in
    the aligned one, and the z halo of the repair is part of what is aligned.  The chunks are a 2-D model's: runs of sections without a halo of their own along z."""
    M, U = C.stack(F_SHAPE, seed=9)
    vol = C.smooth_volume(F_SHAPE, 1)
    mask = np.zeros(F_SHAPE, np.uint8)
    mask[5:14, 20:45, 30:60] = 3
    mask[:, 2, 117] = 1
    W = Warp(M, U, C.SPACING, fill=F_FILL)
    A, mA = C.warp(vol, M, U, fill=F_FILL), C.warp(mask, M, U, fill=0, nearest=True)
    want = RR.repair(A, sections=F_SECTIONS, mask=mA, max_gap=F_GAP)
    assert (mA != mask).mean() > 0.005 and (A == F_FILL).sum() > 50 and (want != A).mean() > 0.1
    assert not np.array_equal(RR.repair(A, sections=F_SECTIONS, mask=mask, max_gap=F_GAP), want)     # the other rule differs
    chunks = chunk_plan(F_START, F_SIZE, 36, 19, F_SHAPE, (4, 1, 1), is3d=False)    # runs of four sections, one tile each
    foot, sbox, mbox = utils._warp_footprints(chunks, F_GAP, utils._check_warp(W, F_SHAPE), F_SHAPE, True)
    assert len(chunks) == 5 * 2 * 4 and sum(f is None for f in foot) == 0

    def leg(src, f, b, nearest, fill):                  # what the launch computes from the box that was read
        (z0, z1), (y0, y1), (x0, x1) = f
        if b is None:
            return np.full((z1 - z0, y1 - y0, x1 - x0), fill, np.uint8)
        seen = src ^ 0x5A                                                                           # never read: scrambled
        seen[z0:z1, b[0][0]:b[0][1], b[1][0]:b[1][1]] = src[z0:z1, b[0][0]:b[0][1], b[1][0]:b[1][1]]
        return C.warp(seen, M, U, f, fill, nearest)

    cut = cut_x = 0
    for c, f, sb, mb in zip(chunks, foot, sbox, mbox):
        (z0, z1), (y0, y1), (x0, x1) = f
        assert (z0, z1) == (max(c.read[0][0] - F_GAP, 0), min(c.read[0][1] + F_GAP, F_SHAPE[0])) and f[1:] == c.read[1:]
        blk, mblk = leg(vol, f, sb, False, F_FILL), leg(mask, f, mb, True, 0)
        assert np.array_equal(blk, A[z0:z1, y0:y1, x0:x1]) and np.array_equal(mblk, mA[z0:z1, y0:y1, x0:x1])
        local = [s - z0 for s in F_SECTIONS if z0 <= s < z1]
        fixed = RR.repair(blk, sections=local or None, mask=mblk, max_gap=F_GAP)
        c0, (a, b) = c.read[0][0] - z0, c.read[0]
        assert np.array_equal(fixed[c0:c0 + c.block[0]], want[a:b, y0:y1, x0:x1])
        cut += (z0, z1) != tuple(c.read[0])
        cut_x += sb[1][0] > 0 and sb[1][1] < F_SHAPE[2]
    assert cut >= 1 and cut_x >= 1                       # a halo along z was aligned; a box was cut on both sides in x
