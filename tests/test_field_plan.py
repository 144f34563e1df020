"""The host side of the elastic alignment of sections, without a GPU: the numpy reference field_ref against warp_ref
where the field is zero, constant or a ramp; field_grid, quantize_field, the slab plan field_chunks, fit_section_fields,
section_fields, every ValueError, the signatures, and the numbers of the fixture of smoothly distorted sections from the
references alone."""
import functools
import inspect

import numpy as np
import pytest

import field_ref as FR
import warp_ref as WR
import zshift_ref as SR
from transfer_em_amd.utils import (HIST_CHUNK_BYTES, FieldFits, SectionFits, SubShifts, field_chunks, field_grid,
                                   fit_section_fields, fit_section_maps, quantize_field, quantize_maps, section_fields,
                                   section_maps, section_shifts, shift_counts, shift_scores, shift_subpixel, volume_warp,
                                   volume_warp_field, warp_chunks)

I23 = WR.IDENTITY
ONE, DEV, MAXU = 1 << 16, 1 << 13, 1 << 21


# ---------------------------------------------------------------------------------------- the reference's identities
@pytest.mark.parametrize("spacing", [16, (16, 64), (32, 16)], ids=str)
def test_zero_constant_and_ramp_fields_are_affine_maps(spacing):
    """U = 0 gives warp_ref's bytes; a constant U those of the map with b moved by it; a ramp of slope g in one
    component along one axis those of the map with that coefficient raised by g -- exactly, bilinear and nearest."""
    shape = (40, 131)
    rng = np.random.default_rng(1)
    vol = rng.integers(0, 256, (3,) + shape, dtype=np.uint8)
    c = np.array([19.5, 65.0])
    M = WR.quantize(np.stack([I23, WR._rigid(0.01, np.array([-1.37, 2.71]), c), WR._rigid(-0.004, np.array([6.5, -0.25]), c)]))
    zero = np.zeros((3,) + FR.grid(shape, spacing) + (2,), np.int32)
    const = np.stack([FR.constant(shape, spacing, 89784, -177603)] * 3)
    moved = M + np.array([0, 0, 89784, 0, 0, -177603])
    for nearest in (False, True):
        want = WR.warp(vol, M, fill=7, nearest=nearest)
        assert np.array_equal(FR.warp(vol, M, zero, spacing, fill=7, nearest=nearest), want)
        assert np.array_equal(FR.warp(vol, M, const, spacing, fill=7, nearest=nearest), WR.warp(vol, moved, fill=7, nearest=nearest))
        for k, comp, axis in ((0, 0, 0), (1, 0, 1), (3, 1, 0), (4, 1, 1)):
            for g in (DEV, -DEV, 4097, -1):
                E = M.copy()
                E[:, k] += g
                U = np.stack([FR.ramp(shape, spacing, comp, axis, g)] * 3)
                got = FR.warp(vol, M, U, spacing, fill=7, nearest=nearest)
                assert np.array_equal(got, WR.warp(vol, E, fill=7, nearest=nearest)), (k, g)
                assert g == -1 or not np.array_equal(got, want)
    box = ((1, 3), (3, 30), (7, 120))                                                # a box reads the same voxels
    U = np.stack([FR.walk(shape, spacing, s) for s in range(3)])
    assert np.array_equal(FR.warp(vol, M, U, spacing, box), FR.warp(vol, M, U, spacing)[1:3, 3:30, 7:120])


def test_the_required_rows_hold_every_tap():
    shape = (40, 131)
    for spacing in (16, (16, 64)):
        fields = FR.case_fields(shape, spacing)
        for name, U in fields.items():
            for m in WR.quantize(np.stack([I23, WR._rigid(0.05, np.array([0.4, -0.6]), np.array([19.5, 65.0])),
                                           np.array([[1.125, -0.125, -3.0], [0.125, 0.875, 4.0]])])):
                for box in (((0, 40), (0, 131)), ((17, 24), (5, 120)), ((39, 40), (130, 131)), ((3, 19), (60, 70))):
                    for nearest in (False, True):
                        rows = FR.tap_rows(m, U, spacing, box, shape, nearest)
                        need = FR.required_rows(m, U, spacing, box, shape, nearest)
                        assert rows.size == 0 or (need is not None and need[0] <= rows[0] and rows[-1] <= need[1]), (name, box)
                        assert need is None or 0 <= need[0] <= need[1] <= shape[0] - 1


# --------------------------------------------------------------------------------------- field_grid, quantize_field
def test_field_grid_at_the_spacing_one_past_it_and_one_pixel():
    for S in (16, 64, 1024):
        assert field_grid((3, S, S + 1), S) == (2, 3) == FR.grid((S, S + 1), S)      # S pixels: one cell; S + 1: two
        assert field_grid((1, 1), S) == (2, 2) and field_grid((S - 1, 2 * S), S) == (2, 3)
        assert field_grid((2 * S + 1, 1), (S, 16)) == (4, 2)
    assert field_grid((7, 100, 1000), (32, 256)) == (5, 5) == FR.grid((100, 1000), (32, 256))
    Y, X, (ky, kx) = 100, 1000, (5, 8)                                                # every pixel has its four nodes
    assert ((Y - 1) >> ky) + 1 <= field_grid((Y, X), (32, 256))[0] - 1 and ((X - 1) >> kx) + 1 <= 5 - 1
    for bad in (8, 2048, 48, 0, -16, 16.0, True, (16,), (16, 16, 16), (16, 24), "16", None):
        with pytest.raises(ValueError):
            field_grid((4, 50, 50), bad)
    for shape in ((50,), (1, 2, 3, 4), (0, 5, 5)):
        with pytest.raises(ValueError):
            field_grid(shape, 16)


def test_quantize_field_at_and_just_past_each_limit():
    S = (16, 64)
    f = np.zeros((2, 4, 4, 2))
    f[1] = (1.37, -2.71)
    f[0, 2, 2] = (0.5 / ONE, 1.49 / ONE)
    q = quantize_field(f, S)
    assert q.dtype == np.int32 and q.shape == f.shape and np.array_equal(q, FR.quantize(f))
    assert q[1, 2, 3].tolist() == [89784, -177603] and q[0, 2, 2].tolist() == [0, 1]  # rint: half to even, 1.49 down
    assert np.array_equal(quantize_field(f.astype(np.float32), S), FR.quantize(f.astype(np.float32)))
    at = np.full((1, 4, 4, 2), 32.0)                                                  # |U| = 2^21 passes, one lsb more does not
    assert quantize_field(at, S).max() == MAXU == -quantize_field(-at, S).min()
    at[0, 1, 2, 1] += 1.0 / ONE
    with pytest.raises(ValueError, match=r"section 0, node \(1, 2\).*32 px"):
        quantize_field(at, S)
    for axis, k, name in ((1, 4, "y"), (2, 6, "x")):
        step = np.zeros((3, 4, 4, 2))
        sl = [2, slice(None), slice(None), 0]
        sl[axis] = slice(2, None)
        step[tuple(sl)] = (1 << k) / 8                                                # S / 8 px from node 1 to node 2: the limit
        assert np.abs(np.diff(quantize_field(step, S).astype(np.int64), axis=axis)).max() == DEV << k
        assert np.array_equal(quantize_field(-step, S), -quantize_field(step, S))
        step[tuple(sl)] += 1.0 / ONE
        node = "1, 0" if axis == 1 else "0, 1"
        with pytest.raises(ValueError, match=rf"section 2, node \({node}\).*along {name}.*{(1 << k) / 8:g} px"):
            quantize_field(step, S)
    for bad in (f[0], f[..., :1], f[:, :1], f.astype(np.int32), f * np.nan, np.where(f > 1, np.inf, f), f * 1e300):
        with pytest.raises(ValueError):
            quantize_field(bad, S)
    with pytest.raises(ValueError):
        quantize_field(f, 24)


# ----------------------------------------------------------------------------------------------------- field_chunks
def _size(box):
    return int(np.prod([hi - lo for lo, hi in box]))


def _tables(Z, kind, shape, spacing):
    rng = np.random.default_rng(Z + len(kind))
    T = np.tile(I23, (Z, 1, 1))
    U = np.zeros((Z,) + FR.grid(shape, spacing) + (2,), np.int32)
    if kind == "walks":
        for z in range(Z):
            T[z] = WR._rigid(rng.uniform(-0.1, 0.1), rng.uniform(-6, 6, 2), np.array(shape[1:]) / 2)
            U[z] = FR.walk(shape[1:], spacing, z)
    elif kind == "limits":
        T[:, :, :2] += rng.choice([-0.125, 0.125], (Z, 2, 2))
        T[:, :, 2] = rng.uniform(-9, 9, (Z, 2))
        U[...] = np.stack([FR.walk(shape[1:], spacing, 10 + z) for z in range(Z)])
    elif kind == "outside":
        U[...] = np.where(np.arange(Z) % 2 == 0, MAXU, -MAXU)[:, None, None, None]
    return quantize_maps(T), U


@pytest.mark.parametrize("kind", ["zero", "walks", "limits", "outside"])
def test_chunks_partition_the_box_and_hold_every_tap_within_the_budget(kind):
    shape, spacing = (5, 23, 17), 16
    Z, Y, X = shape
    M, U = _tables(Z, kind, shape, spacing)
    for box in (((0, Z), (0, Y), (0, X)), ((1, 4), (3, 20), (2, 11))):
        for budget in (None, Z * Y * X, 2 * Y * X, Y * X, Y * X - 1, 12 * X, 6 * X, 2 * X, X, 1):
            chunks = field_chunks(box, shape, M, U, spacing, budget)
            seen = np.zeros(shape, np.int32)
            b = HIST_CHUNK_BYTES if budget is None else budget
            for (oz, oy, ox), (rz, ry, rx) in chunks:
                seen[oz[0]:oz[1], oy[0]:oy[1], ox[0]:ox[1]] += 1
                assert oz[0] < oz[1] and oy[0] < oy[1] and ox == box[2] and rx == (0, X) and rz == oz
                assert oy == box[1] or oz[1] - oz[0] == 1                           # whole sections, or rows of one
                assert 0 <= ry[0] < ry[1] <= Y
                assert (_size((oz, oy, ox)) <= b and _size((rz, ry, rx)) <= b) or oy[1] - oy[0] == 1
                for z in range(*oz):
                    for nearest in (False, True):
                        rows = FR.tap_rows(M[z], U[z], spacing, (oy, ox), (Y, X), nearest)
                        assert rows.size == 0 or (ry[0] <= rows[0] and rows[-1] < ry[1])   # every tap of weight above 0
                        need = FR.required_rows(M[z], U[z], spacing, (oy, ox), (Y, X), nearest)
                        assert need is None or (ry[0] <= need[0] and need[1] < ry[1])     # and what the launch demands
            assert (seen[box[0][0]:box[0][1], box[1][0]:box[1][1], box[2][0]:box[2][1]] == 1).all() and seen.sum() == _size(box)
            order = [(c[0][0], c[1][0]) for c, _ in chunks]
            assert order == sorted(order)
            if budget == 1:
                assert len(chunks) == (box[0][1] - box[0][0]) * (box[1][1] - box[1][0])   # down to one row
            if kind == "zero":
                assert chunks == warp_chunks(box, shape, M, budget)


def test_chunks_with_a_zero_field_are_warp_chunks_and_go_round_robin():
    shape, spacing = (6, 40, 30), (16, 32)
    Z, Y, X = shape
    whole = ((0, Z), (0, Y), (0, X))
    T = np.stack([WR._rigid(0.03 * (z - 2.5), np.array([0.3 * z, -0.2 * z]), np.array([20.0, 15.0])) for z in range(Z)])
    M = quantize_maps(T)
    zero = np.zeros((Z,) + field_grid(shape, spacing) + (2,), np.int32)
    for box in (whole, ((0, Z), (8, 30), (6, 22))):
        for budget in (None, 2 * Y * X, 7 * X, X):
            for rank, world in ((0, 1), (0, 2), (1, 2)):
                assert field_chunks(box, shape, M, zero, spacing, budget, rank, world) == \
                    warp_chunks(box, shape, M, budget, rank, world)
    down = zero.copy()
    down[..., 0] = 3 * ONE                                                          # three rows down: the read rows follow
    a, b = field_chunks(whole, shape, quantize_maps(np.tile(I23, (Z, 1, 1))), down, spacing, 10 * X), \
        warp_chunks(whole, shape, quantize_maps(np.tile(I23, (Z, 1, 1))), 10 * X)
    assert a[0] == (b[0][0], ((0, 1), (3, 13), (0, X))) and [o for o, _ in a[:3]] == [o for o, _ in b[:3]]
    U = np.stack([FR.walk(shape[1:], spacing, z) for z in range(Z)])
    both = [field_chunks(whole, shape, M, U, spacing, 2 * Y * X, rank=r, world_size=2) for r in (0, 1)]
    allc = field_chunks(whole, shape, M, U, spacing, 2 * Y * X)
    assert both[0] == allc[0::2] and both[1] == allc[1::2] and len(allc) >= 3
    assert field_chunks(((2, 2), (0, Y), (0, X)), shape, M, U, spacing) == []


def test_chunks_refuse_bad_arguments():
    shape, S = (4, 6, 8), 16
    M, U = _tables(4, "zero", shape, S)
    whole = ((0, 4), (0, 6), (0, 8))
    badm, badu, steep = M.copy(), U.copy(), U.copy()
    badm[2, 1] = DEV + 1
    badu[1, 0, 1, 0] = MAXU + 1
    steep[3, 1, 1, 1] = (DEV << 4) + 1
    for a, kw in (((whole, shape, M, U, S), dict(chunk_bytes=0)), ((whole, shape, M, U, S), dict(rank=1)),
                  ((whole, shape, M, U, S), dict(rank=0, world_size=0)), ((whole, (6, 8), M, U, S), {}),
                  ((whole, shape, M[:3], U, S), {}), ((whole, shape, M.astype(np.float64), U, S), {}),
                  ((whole, shape, badm, U, S), {}), ((whole, shape, M, U[:3], S), {}), ((whole, shape, M, U[:, :1], S), {}),
                  ((whole, shape, M, U.astype(np.int64), S), {}), ((whole, shape, M, U.astype(np.float64), S), {}),
                  ((whole, shape, M, badu, S), {}), ((whole, shape, M, steep, S), {}), ((whole, shape, M, U, 8), {}),
                  ((whole, shape, M, U, (16, 48)), {}), ((((0, 5), (0, 6), (0, 8)), shape, M, U, S), {}),
                  ((((0, 4), (-1, 6), (0, 8)), shape, M, U, S), {}), ((((0, 4), (0, 6), (0, 9)), shape, M, U, S), {})):
        with pytest.raises(ValueError):
            field_chunks(*a, **kw)


# ----------------------------------------------------------------------------------------------- fit_section_fields
SHAPE, TILE, SPACING = (3, 150, 200), 32, (16, 32)   # 5 x 7 tiles, the last row and column partial


def _points(shape=SHAPE, tile=TILE):
    Y, X = shape[1:]
    c = lambda n: np.array([(k * tile + min((k + 1) * tile, n) - 1) / 2 for k in range(-(-n // tile))])
    return np.stack(np.meshgrid(c(Y), c(X), indexing="ij"), axis=-1)


MAPS = np.array([[[1.01, -0.02, 1.25], [0.015, 0.99, -2.5]], [[0.999, 0.03, -0.75], [-0.03, 1.002, 0.5]]])
BILIN = np.array([[[2e-4, -1e-4], [0.3, -0.2]], [[-1.5e-4, 2.5e-4], [-0.4, 0.1]]])   # per pair: (y x coefficient, constant)


def _true(z, p):
    """The pair function with a bilinear term: T_z p + c_z y x / 1 + d_z."""
    return WR.apply(MAPS[z], p) + BILIN[z, 0] * (p[..., :1] * p[..., 1:]) + BILIN[z, 1]


def _exact_offsets():
    pts = _points()
    return np.stack([_true(z, pts) - pts for z in range(2)])


def _inner_nodes(shape=SHAPE, spacing=SPACING, tile=TILE):
    """The nodes inside the hull of the tile points."""
    pts, nodes = _points(shape, tile), FR.nodes(shape, spacing)
    return nodes, (nodes[..., 0] >= pts[0, 0, 0]) & (nodes[..., 0] <= pts[-1, 0, 0]) & \
        (nodes[..., 1] >= pts[0, 0, 1]) & (nodes[..., 1] <= pts[0, -1, 1])


def test_fit_recovers_an_exactly_bilinear_residual():
    off, dec = _exact_offsets(), np.ones((2, 5, 7), bool)
    sub = SubShifts(off, dec, np.ones((2, 5, 7)))
    fit = fit_section_maps(sub, TILE, SHAPE, max_residual=10.0)
    assert fit.kept.all() and 0.5 < fit.residual.max() < 10.0                       # the maps alone do not explain it
    ff = fit_section_fields(sub, fit, TILE, SHAPE, SPACING, smooth=0)
    assert isinstance(ff, FieldFits) and ff.fields.shape == (2, 11, 8, 2) and ff.fields.dtype == np.float64
    # (the misfit at the tile points is not 0: outside the outermost points the value is held, and the lattice cannot
    # follow that bend inside one cell)
    assert ff.used.all() and ff.used.dtype == np.bool_ and ff.residual.shape == (2,) and ff.residual.max() < 0.25
    nodes, inner = _inner_nodes()
    assert inner.sum() > 30
    for z in range(2):                                       # map + field is the truth at every node between the points
        got = WR.apply(fit.maps[z], nodes) + ff.fields[z]
        assert np.abs(got - _true(z, nodes))[inner].max() < 1e-9
        assert np.array_equal(ff.fields[z][0], ff.fields[z][1]) or nodes[1, 0, 0] > _points()[0, 0, 0]   # held outside
    pts = _points()
    for z in range(2):                                       # and, interpolated on the lattice, at points between them
        p = np.stack(np.meshgrid(np.linspace(pts[0, 0, 0], pts[-1, 0, 0], 9)[1:-1],
                                 np.linspace(pts[0, 0, 1], pts[0, -1, 1], 9)[1:-1], indexing="ij"), axis=-1)
        got = WR.apply(fit.maps[z], p) + FR.interp(ff.fields[z], SPACING, p)
        assert np.abs(got - _true(z, p)).max() < 0.02                                # the lattice cuts the tiles' cells: y x is not linear there
    again = fit_section_fields(sub, fit, TILE, SHAPE, SPACING, smooth=0)
    assert again.fields.tobytes() == ff.fields.tobytes() and again.residual.tobytes() == ff.residual.tobytes()
    sm = fit_section_fields(sub, fit, TILE, SHAPE, SPACING)                          # one pass: exact inside, biased on the rim
    for z in range(2):
        e = np.abs(WR.apply(fit.maps[z], nodes) + sm.fields[z] - _true(z, nodes))
        core = inner & (nodes[..., 0] >= pts[1, 0, 0]) & (nodes[..., 0] <= pts[-3, 0, 0]) & (nodes[..., 1] >= pts[0, 1, 1]) & \
            (nodes[..., 1] <= pts[0, -3, 1])
        assert core.sum() == 6 and e[core].max() < 1e-9 and e[inner].max() < 0.5


def _spread3(off, fit):
    """The largest spread of the true residual over a 3 x 3 neighbourhood of tiles."""
    pts = _points()
    e = np.stack([pts + off[z] - WR.apply(fit.maps[z], pts) for z in range(2)])
    return max(np.ptp(e[z, max(i - 1, 0):i + 2, max(j - 1, 0):j + 2], axis=(0, 1)).max() for z in range(2) for i in range(5)
               for j in range(7))


def test_fit_drops_one_tile_of_nonsense_and_its_neighbours_keep_their_values():
    """With the tile gone, a smoothed value loses one member of its normalised 3 x 3 average, whose weight is at most 4 of
    9 (a corner tile's own), so it -- and every node, an interpolation of tile values -- moves by at most 4 / 9 of the
    largest spread of the true residual over a 3 x 3 neighbourhood, never by the nonsense itself."""
    off, dec = _exact_offsets(), np.ones((2, 5, 7), bool)
    fit = fit_section_maps((off, dec), TILE, SHAPE, max_residual=10.0)
    clean = fit_section_fields((off, dec), fit, TILE, SHAPE, SPACING)
    spread = _spread3(off, fit)
    bad = off.copy()
    bad[0, 2, 3] += (3.0, -3.0)
    bad[1, 0, 6] += (0.0, 2.5)
    ff = fit_section_fields((bad, dec), fit, TILE, SHAPE, SPACING)
    want = np.ones((2, 5, 7), bool)
    want[0, 2, 3] = want[1, 0, 6] = False
    moved = np.abs(ff.fields - clean.fields).max()
    print("nodes moved by at most", moved, "px; 4 / 9 of the residual's spread over 3 x 3 tiles", 4 / 9 * spread, "px")
    assert np.array_equal(ff.used, want) and 0 < moved <= 4 / 9 * spread < 1.0
    assert np.abs(ff.fields - clean.fields)[0].max() < 0.05                        # an interior tile: its neighbours are symmetric
    loose = fit_section_fields((bad, dec), fit, TILE, SHAPE, SPACING, max_residual=10.0)
    assert loose.used.all() and np.abs(loose.fields - clean.fields).max() > 0.5     # kept, it pulls the nodes along
    assert loose.residual[0] > 1.0 > ff.residual[0]


def test_fit_fills_an_undecided_tile_and_gives_an_unresolved_pair_zero():
    off, dec = _exact_offsets(), np.ones((2, 5, 7), bool)
    fit = fit_section_maps((off, dec), TILE, SHAPE, max_residual=10.0)
    clean = fit_section_fields((off, dec), fit, TILE, SHAPE, SPACING)
    hole = dec.copy()
    hole[0, 1, 1] = False
    off2 = off.copy()
    off2[0, 1, 1] = (99.0, -99.0)                                                   # an undecided tile's offset is not read
    ff = fit_section_fields((off2, hole), fit, TILE, SHAPE, SPACING)
    assert np.array_equal(ff.used, hole) and np.abs(ff.fields - clean.fields).max() <= 4 / 9 * _spread3(off, fit)   # as above
    raw = fit_section_fields((off2, hole), fit, TILE, SHAPE, SPACING, smooth=0)     # without a pass it gets 0
    pts = _points()
    e = pts[1, 1] + off[0, 1, 1] - WR.apply(fit.maps[0], pts[1, 1])
    full = fit_section_fields((off, dec), fit, TILE, SHAPE, SPACING, smooth=0)
    assert np.abs(e).max() > 0.3 and np.abs(raw.fields[0] - full.fields[0]).max() > 0.15 and not raw.used[0, 1, 1]
    lone = np.zeros_like(dec)
    lone[0, 4, 6] = True                                                            # one tile: one pass reaches its neighbours only
    one = fit_section_fields((off, lone), fit, TILE, SHAPE, SPACING)
    assert one.used.sum() == 1 and not one.fields[1].any() and one.fields[0][0, 0].tolist() == [0.0, 0.0]
    assert np.abs(one.fields[0][-1, -1] - (pts[4, 6] + off[0, 4, 6] - WR.apply(fit.maps[0], pts[4, 6]))).max() < 1e-9
    unres = SectionFits(fit.maps, fit.kept, fit.residual, [1])
    z = fit_section_fields((off, dec), unres, TILE, SHAPE, SPACING)
    assert not z.fields[1].any() and not z.used[1].any() and z.residual[1] == 0 and np.array_equal(z.fields[0], clean.fields[0])


def test_fit_refuses_bad_arguments():
    off, dec = _exact_offsets(), np.ones((2, 5, 7), bool)
    fit = fit_section_maps((off, dec), TILE, SHAPE, max_residual=10.0)
    ok = dict(sub=(off, dec), fits=fit, tile=TILE, vol_shape=SHAPE, spacing=SPACING)
    for kw in (dict(sub=(off[:, :4], dec)), dict(sub=(off, dec[:1])), dict(sub=(off, dec.astype(np.uint8))),
               dict(sub=(off.astype(complex), dec)), dict(fits=(fit.maps[:1], fit.kept, fit.residual, [])),
               dict(fits=(fit.maps * np.nan, fit.kept, fit.residual, [])), dict(tile=0), dict(vol_shape=(150, 200, 3, 1)),
               dict(spacing=8), dict(spacing=(16, 20)), dict(smooth=-1), dict(smooth=1.5), dict(smooth=True),
               dict(max_residual=0), dict(max_residual=np.inf), dict(max_residual="1")):
        with pytest.raises(ValueError):
            fit_section_fields(**{**ok, **kw})


# --------------------------------------------------------------------------------------------------- section_fields
def test_section_fields_with_zero_fields_are_section_maps():
    rng = np.random.default_rng(4)
    shape, S = (9, 100, 140), (32, 64)
    T = np.stack([WR._rigid(rng.uniform(-0.02, 0.02), rng.uniform(-2, 2, 2), np.array([49.5, 69.5])) for _ in range(8)])
    zero = np.zeros((8,) + field_grid(shape, S) + (2,))
    for window in (None, 3, 5):
        maps, fields = section_fields(T, zero, S, shape, window)
        assert maps.tobytes() == section_maps(T, window).tobytes()
        assert fields.shape == (9,) + field_grid(shape, S) + (2,) and fields.dtype == np.float64 and not fields.any()
    assert not quantize_field(section_fields(T, zero, S, shape)[1], S).any()


def test_section_fields_compose_two_known_pair_fields_pointwise():
    shape, S = (3, 100, 140), (32, 64)
    nodes = FR.nodes(shape, S)
    c = np.array([49.5, 69.5])
    T = np.stack([WR._rigid(0.01, np.array([0.5, -1.0]), c), WR._rigid(-0.02, np.array([-1.5, 0.25]), c)])
    R = np.stack([np.stack([0.8 * np.sin(nodes[..., 1] / 50.0), 0.5 * np.cos(nodes[..., 0] / 40.0)], axis=-1),
                  np.stack([-0.6 * np.cos(nodes[..., 0] / 30.0), 0.9 * np.sin(nodes[..., 1] / 60.0 + 1.0)], axis=-1)])
    F = lambda z, q: WR.apply(T[z], q) + FR.interp(R[z], S, q)
    maps, fields = section_fields(T, R, S, shape)
    assert np.array_equal(maps, section_maps(T)) and not fields[0].any()
    G1, G2 = F(0, nodes), F(1, F(0, nodes))
    assert np.abs(WR.apply(maps[1], nodes) + fields[1] - G1).max() < 1e-9
    assert np.abs(WR.apply(maps[2], nodes) + fields[2] - G2).max() < 1e-9
    assert np.abs(fields[1] - R[0]).max() < 1e-9 and np.abs(fields[2]).max() > 0.5
    # a window: the maps are section_maps', the field is D_z read at the node carried through the inverse trend, less
    # the running lower median of the three sections
    wm, wf = section_fields(T, R, S, shape, window=3)
    assert np.array_equal(wm, section_maps(T, 3))
    B = section_maps(T)
    moved = np.stack([FR.interp(fields[z], S, WR.apply(WR.compose(WR.invert(B[z]), wm[z]), nodes)) for z in range(3)])
    med = np.stack([np.sort(moved[max(z - 1, 0):z + 2], axis=0)[(min(z + 2, 3) - max(z - 1, 0) - 1) // 2] for z in range(3)])
    assert np.abs(wf - (moved - med)).max() < 1e-9 and np.abs(wf).max() > 0.1
    for a in ((T, R[:1], S, shape), (T, R.astype(np.int32), S, shape), (T, R * np.nan, S, shape), (T, R, 24, shape),
              (T, R, S, (3, 100, 300)), (T[:, :, :2], R, S, shape), (T, R[:, :3], S, shape)):
        with pytest.raises(ValueError):
            section_fields(*a)
    with pytest.raises(ValueError):
        section_fields(T, R, S, shape, window=2)


# ------------------------------------------------------------------- volume_warp_field: refused before any GPU work
def test_volume_warp_field_refuses_bad_arguments_on_the_host(monkeypatch):
    from transfer_em_amd import hip_ops

    def no_gpu():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(hip_ops, "require_gpu", no_gpu)
    v, S = np.zeros((4, 6, 8), np.uint8), 16
    T, F = np.tile(I23, (4, 1, 1)), np.zeros((4, 2, 2, 2))
    far, high, steep = T.copy(), F.copy(), F.copy()
    far[1, 0, 1] = 0.126
    high[2, 1, 1, 0] = 32.001
    steep[3, 0, 1, 1] = 2.001
    for a, kw in (((v.astype(np.int16), T, F, S), {}), ((v[0, 0], T, F, S), {}), ((v[None], T, F, S), {}), ((v, T[:3], F, S), {}),
                  ((v, far, F, S), {}), ((v, T, F[:3], S), {}), ((v, T, F[:, :1], S), {}), ((v, T, F[0], S), {}),
                  ((v, T, F.astype(np.int64), S), {}), ((v, T, F * np.nan, S), {}), ((v, T, high, S), {}),
                  ((v, T, steep, S), {}), ((v, T, F, 8), {}), ((v, T, F, (16, 2048)), {}), ((v, T, F, 32.0), {}),
                  ((v, T, np.zeros((4, 3, 2, 2)), S), {}), ((v, T, F, S), dict(fill=256)), ((v, T, F, S), dict(fill=1.5)),
                  ((v, T, F, S), dict(start=(0, 0, 0), size=(9, 6, 4))), ((v, T, F, S), dict(out=np.zeros((4, 6, 8), np.int8))),
                  ((v, T, F, S), dict(out=np.zeros((4, 6, 9), np.uint8))), ((v, T, F, S), dict(chunk_bytes=0)),
                  ((v, T, F, S), dict(rank=2, world_size=2)), ((v[0], T, F, S), {}), ((v[0], T[0], F, S), {})):
        with pytest.raises(ValueError):
            volume_warp_field(*a, **kw)
    with pytest.raises(AssertionError, match="the GPU was asked for"):                 # and a good call gets that far
        volume_warp_field(v, T, F, S)
    with pytest.raises(AssertionError, match="the GPU was asked for"):
        volume_warp_field(v[0], quantize_maps(T)[0], quantize_field(F, S)[0], S, nearest=True, fill=255)


def test_signatures_and_the_reference_alias():
    import transfer_em.utils as alias
    from transfer_em_amd import _lib, utils
    for name in ("field_grid", "fit_section_fields", "section_fields", "quantize_field", "field_chunks", "volume_warp_field",
                 "FieldFits"):
        assert getattr(alias, name) is getattr(utils, name)
    sig = lambda f: list(inspect.signature(f).parameters)
    dflt = lambda f, p: inspect.signature(f).parameters[p].default
    assert sig(field_grid) == ["vol_shape", "spacing"] and sig(quantize_field) == ["fields", "spacing"]
    assert sig(fit_section_fields) == ["sub", "fits", "tile", "vol_shape", "spacing", "smooth", "max_residual"]
    assert dflt(fit_section_fields, "smooth") == 1 and dflt(fit_section_fields, "max_residual") == 1.0
    assert sig(section_fields) == ["pair_maps", "pair_fields", "spacing", "vol_shape", "window"]
    assert dflt(section_fields, "window") is None
    assert sig(field_chunks) == ["out_box", "vol_shape", "M", "U", "spacing", "chunk_bytes", "rank", "world_size"]
    assert sig(volume_warp_field) == ["volume", "maps", "fields", "spacing", "out", "start", "size", "fill", "nearest",
                                      "chunk_bytes", "rank", "world_size", "device", "stats"]
    assert sig(volume_warp_field)[4:] == sig(volume_warp)[2:]                       # volume_warp's, from `out` on
    assert dflt(volume_warp_field, "fill") == 0 and dflt(volume_warp_field, "nearest") is False
    assert FieldFits._fields == ("fields", "used", "residual")
    assert len(_lib._SIGS["tem_u8_warp_field"]) == 23 == len(_lib._SIGS["tem_u8_warp_field_direct"])
    assert "volume_warp_field" in inspect.getdoc(volume_warp) and "fit_section_fields" in inspect.getdoc(fit_section_maps)


# ------------------------------------------------------------------------ the fixture's own numbers, references only
@functools.lru_cache(maxsize=None)
def _fixture_fit():
    v = FR.distorted_volume()
    tile, r = FR.FIX_TILE, FR.FIX_RADIUS
    q = SR.volume_sums(v, (tile, tile), r)
    n = shift_counts(v.shape, tile, r)
    sub = shift_subpixel(q, n)
    fit = fit_section_maps(sub, tile, v.shape)
    return v, q, n, sub, fit, fit_section_fields(sub, fit, tile, v.shape, FR.FIX_SPACING)


def test_the_fixture_is_what_it_says():
    """This fixture's own values: all 336 tiles decide, the smallest peak 0.881, the largest offset 3 of radius 4; the
    affine fit leaves 0.87 to 1.00 px at a kept tile per pair (after dropping 13 tiles above 1 px); map + field is within
    0.21 to 0.28 px of the true pair function at the 35 nodes between the tile points, the map alone 0.62 to 1.12 px
    off; the field rests on 335 tiles and misses a used tile by at most 0.67 px (on the rim, where the value is held)."""
    v, q, n, sub, fit, ff = _fixture_fit()
    assert v.shape == FR.FIX_SHAPE == (8, 192, 256) and v.dtype == np.uint8 and not v.flags.writeable
    assert shift_counts(v.shape, FR.FIX_TILE, FR.FIX_RADIUS).shape[:2] == (6, 8)
    T = FR.true_pair_functions()
    nodes, inner = _inner_nodes(v.shape, FR.FIX_SPACING, FR.FIX_TILE)
    assert FR.grid(v.shape, FR.FIX_SPACING) == (7, 9) and inner.sum() == 5 * 7
    tiles = section_shifts(q, n).tiles
    print("decided", int(sub.decided.sum()), "of", sub.decided.size, "; smallest peak", sub.peak.min(), "; largest offset",
          np.abs(tiles).max())
    assert sub.decided.all() and np.abs(tiles).max() < FR.FIX_RADIUS and fit.unresolved == []   # every tile decides off the rim
    print("affine fit: largest kept residual per pair", np.round(fit.residual, 3), "; tiles dropped", int((~fit.kept).sum()))
    assert fit.residual.min() > 0.75                                                # clearly above the bar of 0.5 px
    err_field, err_map = [], []
    for z in range(v.shape[0] - 1):
        truth = T[z](nodes)
        err_field.append(np.abs(WR.apply(fit.maps[z], nodes) + ff.fields[z] - truth).max(axis=-1)[inner].max())
        err_map.append(np.abs(WR.apply(fit.maps[z], nodes) - truth).max(axis=-1)[inner].max())
    print("map + field against the truth at the inner nodes, px", np.round(err_field, 3), "; the map alone", np.round(err_map, 3))
    print("field fit: tiles used", int(ff.used.sum()), "of", ff.used.size, "; largest misfit per pair", np.round(ff.residual, 3))
    assert max(err_field) < 0.5 < min(err_map)
    fields = section_fields(fit.maps, ff.fields, FR.FIX_SPACING, v.shape)[1]
    U = quantize_field(fields, FR.FIX_SPACING)                                       # inside the limits
    assert FR.within_limits(U, FR.FIX_SPACING) and 1.0 < np.abs(fields).max() < 8.0


def _interior(vol, n):
    tile, r = FR.FIX_TILE, FR.FIX_RADIUS
    q = SR.volume_sums(vol, (tile, tile), r)
    return shift_scores(q, n)[:, 1:-1, 1:-1, r, r].mean(), section_shifts(q, n).tiles[:, 1:-1, 1:-1]


def test_the_reference_field_warp_aligns_the_fixture_better_than_the_affine_warp():
    """This fixture's own values: the interior tiles' mean correlation is 0.711 raw, 0.941 after the affine warp and
    0.958 after the warp through map + field; after that every interior tile re-measures (0, 0), after the affine warp
    91 of 168 do not."""
    v, q, n, sub, fit, ff = _fixture_fit()
    maps, fields = section_fields(fit.maps, ff.fields, FR.FIX_SPACING, v.shape)
    M = quantize_maps(maps)
    (c_raw, _), (c_affine, t_affine) = _interior(v, n), _interior(WR.warp(v, M), n)
    c_field, t_field = _interior(FR.warp(v, M, quantize_field(fields, FR.FIX_SPACING), FR.FIX_SPACING), n)
    print("interior tiles' mean correlation: raw", c_raw, "affine", c_affine, "field", c_field,
          "; interior tiles off (0, 0) after the affine warp:", int(t_affine.any(axis=-1).sum()), "of", t_affine.shape[0] * 24)
    assert not t_field.any() and t_affine.any()
    assert c_raw < c_affine < c_field
