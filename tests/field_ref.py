"""The numpy reference of the warp of sections through "affine map + displacement field" (include/tem_hip.h:
tem_u8_warp_field), independent of transfer_em_amd.utils, and the seeded fixture of smoothly distorted sections that the
field tests share.

The lattice of a section of Y x X pixels with the spacings Sy = 2^ky, Sx = 2^kx has ny = ((Y - 1) >> ky) + 2 by
nx = ((X - 1) >> kx) + 2 nodes, node (i, j) at pixel (i Sy, j Sx); U[i, j] = (u_y, u_x) are int32 in units of 2^-16 px.
For the output voxel (y, x), in int64:
  i = y >> ky, ry = y & (Sy - 1); j = x >> kx, rx = x & (Sx - 1)
  u = ((Sy - ry) ((Sx - rx) U[i, j] + rx U[i, j + 1]) + ry ((Sx - rx) U[i + 1, j] + rx U[i + 1, j + 1])) >> (ky + kx)
  sy = a_yy y + a_yx x + b_y + u_y,  sx = a_xy y + a_xx x + b_x + u_x
and from there on warp_ref's definition: fy = (sy + 128) >> 8, inside, taps, one rounding, nearest."""
import functools

import numpy as np

import warp_ref as WR
from zcorr_ref import _box_blur

UNIT, MAX_U, MAX_SLOPE = 1 << 16, 1 << 21, 1 << 13


def log2s(spacing):
    """(ky, kx) of a spacing, an int or (Sy, Sx)."""
    sy, sx = (spacing, spacing) if np.isscalar(spacing) else spacing
    ky, kx = int(sy).bit_length() - 1, int(sx).bit_length() - 1
    assert (1 << ky, 1 << kx) == (sy, sx) and 4 <= ky <= 10 and 4 <= kx <= 10
    return ky, kx


def grid(shape, spacing):
    """(ny, nx) of the lattice over a section of shape[-2:]."""
    ky, kx = log2s(spacing)
    return ((shape[-2] - 1) >> ky) + 2, ((shape[-1] - 1) >> kx) + 2


def quantize(fields):
    """int32 of float fields in pixels: rint(u 2^16)."""
    return np.rint(np.asarray(fields, np.float64) * UNIT).astype(np.int32)


def within_limits(U, spacing):
    """Whether the int field U [..., ny, nx, 2] keeps |U| <= 2^21 and the differences of adjacent nodes S 2^13."""
    ky, kx = log2s(spacing)
    U = np.asarray(U).astype(np.int64)
    return bool((np.abs(U) <= MAX_U).all() and (np.abs(np.diff(U, axis=-3)) <= MAX_SLOPE << ky).all()
                and (np.abs(np.diff(U, axis=-2)) <= MAX_SLOPE << kx).all())


def displacement(U, spacing, box):
    """int64 [y1 - y0, x1 - x0, 2]: the field of the voxels of the (y, x) (lo, hi) box."""
    ky, kx = log2s(spacing)
    (y0, y1), (x0, x1) = box
    U = np.asarray(U).astype(np.int64)
    y, x = np.arange(y0, y1, dtype=np.int64)[:, None, None], np.arange(x0, x1, dtype=np.int64)[None, :, None]
    i, ry, j, rx = y >> ky, y & ((1 << ky) - 1), x >> kx, x & ((1 << kx) - 1)
    i, j = i[..., 0], j[..., 0]
    wy, wx = (1 << ky) - ry, (1 << kx) - rx
    return (wy * (wx * U[i, j] + rx * U[i, j + 1]) + ry * (wx * U[i + 1, j] + rx * U[i + 1, j + 1])) >> (ky + kx)


def positions(m, U, spacing, box, shape):
    """(fy, fx, inside) of the output voxels of the (y, x) (lo, hi) `box` of a section of `shape`."""
    (Y, X), ((y0, y1), (x0, x1)) = shape, box
    y, x = np.arange(y0, y1, dtype=np.int64)[:, None], np.arange(x0, x1, dtype=np.int64)[None]
    ayy, ayx, by, axy, axx, bx = (int(v) for v in m)
    u = displacement(U, spacing, box)
    fy, fx = (ayy * y + ayx * x + by + u[..., 0] + 128) >> 8, (axy * y + axx * x + bx + u[..., 1] + 128) >> 8
    return fy, fx, (fy >= 0) & (fy <= 256 * (Y - 1)) & (fx >= 0) & (fx <= 256 * (X - 1))


def warp_section(V, m, U, spacing, box=None, fill=0, nearest=False):
    """uint8 [y1 - y0, x1 - x0]: the box (default: the whole section) of section `V` [Y, X] under map `m` and field `U`."""
    V = np.asarray(V)
    Y, X = V.shape
    fy, fx, inside = positions(m, U, spacing, ((0, Y), (0, X)) if box is None else box, V.shape)
    fy, fx = np.where(inside, fy, 0), np.where(inside, fx, 0)
    if nearest:
        v = V[(fy + 128) >> 8, (fx + 128) >> 8].astype(np.int64)
    else:
        iy, ty, ix, tx = fy >> 8, fy & 255, fx >> 8, fx & 255
        jy, jx, W = np.minimum(iy + 1, Y - 1), np.minimum(ix + 1, X - 1), V.astype(np.int64)
        v = ((256 - ty) * ((256 - tx) * W[iy, ix] + tx * W[iy, jx]) + ty * ((256 - tx) * W[jy, ix] + tx * W[jy, jx])
             + (1 << 15)) >> 16
    return np.where(inside, v, fill).astype(np.uint8)


def warp(vol, maps, fields, spacing, box=None, fill=0, nearest=False):
    """uint8: the (z, y, x) (lo, hi) `box` (default: all) of `vol` [Z, Y, X], section z under maps[z] and fields[z]."""
    Z, Y, X = vol.shape
    (z0, z1), yx = ((0, Z), ((0, Y), (0, X))) if box is None else (box[0], tuple(box[1:]))
    return np.stack([warp_section(vol[z], maps[z], fields[z], spacing, yx, fill, nearest) for z in range(z0, z1)])


def tap_rows(m, U, spacing, box, shape, nearest=False):
    """The sorted rows that the inside voxels of the (y, x) box read with a weight above 0."""
    fy, _, inside = positions(m, U, spacing, box, shape)
    fy = fy[inside]
    if nearest:
        return np.unique((fy + 128) >> 8)
    return np.unique(np.concatenate([fy >> 8, (fy >> 8)[(fy & 255) != 0] + 1]))


def required_rows(m, U, spacing, box, shape, nearest=False):
    """The header's rule: (first, last) row that the source block must hold for the (y, x) box of one plane, or None
    where the plane is wholly outside by the same bounds.  The extremes of the affine sy, sx over the box's corners plus
    the least and largest node of the cells the box meets; fy cut to the section."""
    ky, kx = log2s(spacing)
    (Y, X), ((y0, y1), (x0, x1)) = shape, box
    U = np.asarray(U).astype(np.int64)
    sub = U[y0 >> ky:((y1 - 1) >> ky) + 2, x0 >> kx:((x1 - 1) >> kx) + 2]
    ayy, ayx, by, axy, axx, bx = (int(v) for v in m)
    cs = [(y, x) for y in (y0, y1 - 1) for x in (x0, x1 - 1)]
    sy, sx = [ayy * y + ayx * x + by for y, x in cs], [axy * y + axx * x + bx for y, x in cs]
    (uylo, uxlo), (uyhi, uxhi) = (int(v) for v in sub.min(axis=(0, 1))), (int(v) for v in sub.max(axis=(0, 1)))
    fylo, fyhi = max((min(sy) + uylo + 128) >> 8, 0), min((max(sy) + uyhi + 128) >> 8, 256 * (Y - 1))
    fxlo, fxhi = max((min(sx) + uxlo + 128) >> 8, 0), min((max(sx) + uxhi + 128) >> 8, 256 * (X - 1))
    if fylo > fyhi or fxlo > fxhi:
        return None
    if nearest:
        return (fylo + 128) >> 8, (fyhi + 128) >> 8
    return fylo >> 8, (fyhi >> 8) + (1 if fyhi & 255 else 0)


def interp(F, spacing, p):
    """Float: the field F [ny, nx, 2] (pixels) interpolated bilinearly at the points p [..., 2] = (y, x), clamped to the
    lattice."""
    ky, kx = log2s(spacing)
    F = np.asarray(F, np.float64)
    ny, nx = F.shape[:2]
    p = np.asarray(p, np.float64)
    gy, gx = np.clip(p[..., 0] / (1 << ky), 0, ny - 1), np.clip(p[..., 1] / (1 << kx), 0, nx - 1)
    i, j = np.minimum(np.floor(gy).astype(np.int64), ny - 2), np.minimum(np.floor(gx).astype(np.int64), nx - 2)
    ty, tx = (gy - i)[..., None], (gx - j)[..., None]
    return (1 - ty) * ((1 - tx) * F[i, j] + tx * F[i, j + 1]) + ty * ((1 - tx) * F[i + 1, j] + tx * F[i + 1, j + 1])


def nodes(shape, spacing):
    """float64 [ny, nx, 2]: the nodes' pixel positions."""
    ky, kx = log2s(spacing)
    ny, nx = grid(shape, spacing)
    return np.stack(np.meshgrid(np.arange(ny, dtype=np.float64) * (1 << ky), np.arange(nx, dtype=np.float64) * (1 << kx),
                                indexing="ij"), axis=-1)


# --------------------------------------------------------------------------------------------------------- the cases
def ramp(shape, spacing, comp, axis, g):
    """int32 [ny, nx, 2]: U[i, j, comp] = (i Sy if axis == 0 else j Sx) g -- the affine map with the coefficient that
    takes component `comp` from `axis` raised by g."""
    ky, kx = log2s(spacing)
    ny, nx = grid(shape, spacing)
    U = np.zeros((ny, nx, 2), np.int64)
    U[..., comp] = (np.arange(ny)[:, None] << ky) * g if axis == 0 else (np.arange(nx)[None, :] << kx) * g
    assert np.abs(U).max() <= MAX_U
    return U.astype(np.int32)


def constant(shape, spacing, uy, ux):
    """int32 [ny, nx, 2]: every node (uy, ux), in 2^-16 px."""
    U = np.empty(grid(shape, spacing) + (2,), np.int32)
    U[...] = (uy, ux)
    return U


def walk(shape, spacing, seed, step=1.0):
    """int32 [ny, nx, 2]: a field whose every difference of adjacent nodes is within `step` of the limit S 2^13, most of
    them at +-step times it: per component a random walk of +-step Sy 2^13 along y plus one of +-step Sx 2^13 along x,
    each reflected into [-2^20, 2^20]."""
    ky, kx = log2s(spacing)
    ny, nx = grid(shape, spacing)
    rng = np.random.default_rng(seed)

    def line(n, d):
        v, out = int(rng.integers(-MAX_U // 4, MAX_U // 4)), []
        for _ in range(n):
            out.append(v)
            s = d if rng.integers(2) else -d
            v = v + s if abs(v + s) <= MAX_U // 2 else v - s
        return np.array(out, np.int64)
    U = np.stack([line(ny, int(step * (MAX_SLOPE << ky)))[:, None] + line(nx, int(step * (MAX_SLOPE << kx)))[None, :]
                  for _ in range(2)], axis=-1)
    assert within_limits(U, spacing)
    return U.astype(np.int32)


def case_fields(shape, spacing):
    """{name: int32 [ny, nx, 2]}: the fields of the kernel tests for a section of `shape` (small enough for a ramp at the
    limit to stay below 32 px)."""
    Y, X = shape
    half = lambda n: min(n * UNIT // 2, MAX_U)
    f = {"zero": constant(shape, spacing, 0, 0), "const": constant(shape, spacing, int(1.37 * UNIT), int(-2.71 * UNIT)),
         "max+": constant(shape, spacing, MAX_U, MAX_U), "max-": constant(shape, spacing, -MAX_U, -MAX_U),
         "face_y0": constant(shape, spacing, -half(Y), 0), "face_y1": constant(shape, spacing, half(Y), 0),
         "face_x0": constant(shape, spacing, 0, -half(X)), "face_x1": constant(shape, spacing, 0, half(X)),
         "walk": walk(shape, spacing, 5), "walk2": walk(shape, spacing, 6, 0.37)}
    for comp, axis, name in ((0, 0, "yy"), (0, 1, "yx"), (1, 0, "xy"), (1, 1, "xx")):
        for g in (MAX_SLOPE, -MAX_SLOPE):
            f[f"ramp_{name}{'+' if g > 0 else '-'}"] = ramp(shape, spacing, comp, axis, g)
    return f


# ------------------------------------------------------------------------------------------------------- the fixture
FIX_SHAPE, FIX_TILE, FIX_RADIUS, FIX_MARGIN, FIX_SPACING = (8, 192, 256), 32, 4, 24, 32
FIX_ROT, FIX_SHIFT, FIX_AMP = 0.003, 0.5, (1.5, 2.0)     # per pair: rotation step, shift, and the sine's amplitude (px)


def _pair_function(theta, t, amp, centre, shape):
    """p -> T(p): a rotation about the centre and a shift, plus a half-period sine across the section: u_y = amp_y
    sin(pi x / (X - 1)), u_x = amp_x sin(pi y / (Y - 1)); gradient at most amp pi / (n - 1), far below 1 / 8."""
    rigid = WR._rigid(theta, t, centre)
    Y, X = shape

    def T(p):
        p = np.asarray(p, np.float64)
        s = np.stack([amp[0] * np.sin(np.pi * p[..., 1] / (X - 1)), amp[1] * np.sin(np.pi * p[..., 0] / (Y - 1))], axis=-1)
        return WR.apply(rigid, p) + s
    return T


@functools.lru_cache(maxsize=None)
def _fixture(seed=47):
    Z, Y, X = FIX_SHAPE
    rng = np.random.default_rng(seed)
    dtheta = rng.uniform(-FIX_ROT, FIX_ROT, Z - 1)
    dt = rng.uniform(-FIX_SHIFT, FIX_SHIFT, (Z - 1, 2))
    amp = rng.uniform(*FIX_AMP, (Z - 1, 2)) * rng.choice([-1.0, 1.0], (Z - 1, 2))
    centre = np.array([(Y - 1) / 2, (X - 1) / 2])
    T = [_pair_function(dtheta[z], dt[z], amp[z], centre, (Y, X)) for z in range(Z - 1)]
    M = FIX_MARGIN
    a = rng.standard_normal((Z, Y + 2 * M, X + 2 * M))
    for _ in range(2):
        for axis in range(3):
            a = _box_blur(a, axis)
    a = 128.0 + 40.0 * a / a.std()
    yx = np.stack(np.meshgrid(np.arange(Y, dtype=np.float64), np.arange(X, dtype=np.float64), indexing="ij"), axis=-1)
    vol = np.empty(FIX_SHAPE, np.uint8)
    for z in range(Z):
        q = yx                                   # section z shows at p the tissue at G_z(p) = T_{Z - 2} o ... o T_z (p)
        for k in range(z, Z - 1):
            q = T[k](q)
        q = q + M
        assert q.min() >= 0 and q[..., 0].max() <= Y + 2 * M - 1 and q[..., 1].max() <= X + 2 * M - 1
        i = np.minimum(np.floor(q).astype(np.int64), [Y + 2 * M - 2, X + 2 * M - 2])
        f = q - i
        s = a[z]
        v = (1 - f[..., 0]) * ((1 - f[..., 1]) * s[i[..., 0], i[..., 1]] + f[..., 1] * s[i[..., 0], i[..., 1] + 1]) + \
            f[..., 0] * ((1 - f[..., 1]) * s[i[..., 0] + 1, i[..., 1]] + f[..., 1] * s[i[..., 0] + 1, i[..., 1] + 1])
        vol[z] = np.clip(np.rint(v).astype(np.int64) + rng.integers(-6, 7, (Y, X)), 0, 255)
    vol.setflags(write=False)
    return vol, tuple(T)


def distorted_volume():
    """A (8, 192, 256) uint8 volume of warp_ref's smooth recipe, generated with a margin of 24: section z shows at p the
    tissue at G_z(p), G_7 = id and G_z = G_{z + 1} o T_z, where the pair function T_z is a rotation about the centre
    within +-0.003 rad and a shift within +-0.5 px plus a half-period sine of 1.5 to 2 px across the section in each
    component, of either sign; sampled bilinearly in float64, integer noise in [-6, 6] added after.  Read-only."""
    return _fixture()[0]


def true_pair_functions():
    """The Z - 1 functions T_z: section z + 1 shows at T_z(p) what section z shows at p, for points p [..., 2]."""
    return _fixture()[1]
