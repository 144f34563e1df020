"""The numpy reference of the affine warp of sections (include/tem_hip.h: tem_u8_warp_affine), independent of
transfer_em_amd.utils, and the seeded fixture of rotated and translated sections that the warp tests share.

A section's map is six integers in units of 2^-16, (a_yy, a_yx, b_y, a_xy, a_xx, b_x).  For the output voxel (y, x), in
volume coordinates, in int64:
  sy = a_yy y + a_yx x + b_y,  sx = a_xy y + a_xx x + b_x;   fy = (sy + 128) >> 8,  fx = (sx + 128) >> 8
  inside iff 0 <= fy <= 256 (Y - 1) and 0 <= fx <= 256 (X - 1), else `fill`
  iy = fy >> 8, ty = fy & 255, rows iy and min(iy + 1, Y - 1); ix, tx likewise
  v = ((256 - ty) ((256 - tx) v00 + tx v01) + ty ((256 - tx) v10 + tx v11) + 2^15) >> 16;   nearest: V[(fy + 128) >> 8,
  (fx + 128) >> 8].
Float maps are [2, 3]: rows (y, x), columns (from y, from x, constant): T(p) = L p + b with p = (y, x)."""
import functools

import numpy as np

from zcorr_ref import _box_blur

UNIT = 1 << 16


def quantize(maps):
    """int64[..., 6] of float maps [..., 2, 3]: rint(m 2^16), in the order (a_yy, a_yx, b_y, a_xy, a_xx, b_x)."""
    m = np.asarray(maps, np.float64)
    return np.rint(m * UNIT).astype(np.int64).reshape(m.shape[:-2] + (6,))


def positions(m, box, shape):
    """(fy, fx, inside) of the output voxels of the (y, x) (lo, hi) `box` of a section of `shape` under the map `m`."""
    (Y, X), ((y0, y1), (x0, x1)) = shape, box
    y, x = np.arange(y0, y1, dtype=np.int64)[:, None], np.arange(x0, x1, dtype=np.int64)[None]
    ayy, ayx, by, axy, axx, bx = (int(v) for v in m)
    fy, fx = (ayy * y + ayx * x + by + 128) >> 8, (axy * y + axx * x + bx + 128) >> 8
    return fy, fx, (fy >= 0) & (fy <= 256 * (Y - 1)) & (fx >= 0) & (fx <= 256 * (X - 1))


def warp_section(V, m, box=None, fill=0, nearest=False):
    """uint8 [y1 - y0, x1 - x0]: the box (default: the whole section) of section `V` [Y, X] warped by the map `m`."""
    V = np.asarray(V)
    Y, X = V.shape
    fy, fx, inside = positions(m, ((0, Y), (0, X)) if box is None else box, V.shape)
    fy, fx = np.where(inside, fy, 0), np.where(inside, fx, 0)
    if nearest:
        v = V[(fy + 128) >> 8, (fx + 128) >> 8].astype(np.int64)
    else:
        iy, ty, ix, tx = fy >> 8, fy & 255, fx >> 8, fx & 255
        jy, jx, W = np.minimum(iy + 1, Y - 1), np.minimum(ix + 1, X - 1), V.astype(np.int64)
        v = ((256 - ty) * ((256 - tx) * W[iy, ix] + tx * W[iy, jx]) + ty * ((256 - tx) * W[jy, ix] + tx * W[jy, jx])
             + (1 << 15)) >> 16
    return np.where(inside, v, fill).astype(np.uint8)


def warp(vol, maps, box=None, fill=0, nearest=False):
    """uint8: the (z, y, x) (lo, hi) `box` (default: all) of `vol` [Z, Y, X] with section z warped by maps[z] (int64[Z, 6])."""
    Z, Y, X = vol.shape
    (z0, z1), yx = ((0, Z), ((0, Y), (0, X))) if box is None else (box[0], tuple(box[1:]))
    return np.stack([warp_section(vol[z], maps[z], yx, fill, nearest) for z in range(z0, z1)])


def tap_rows(m, box, shape, nearest=False):
    """The sorted rows that the inside voxels of the (y, x) box read with a weight above 0."""
    fy, _, inside = positions(m, box, shape)
    fy = fy[inside]
    if nearest:
        return np.unique((fy + 128) >> 8)
    return np.unique(np.concatenate([fy >> 8, (fy >> 8)[(fy & 255) != 0] + 1]))


def compose(a, b):
    """The float map a o b: p -> a(b(p))."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.concatenate([a[:, :2] @ b[:, :2], (a[:, :2] @ b[:, 2] + a[:, 2])[:, None]], axis=1)


def invert(a):
    a = np.asarray(a, np.float64)
    Li = np.linalg.inv(a[:, :2])
    return np.concatenate([Li, (-Li @ a[:, 2])[:, None]], axis=1)


def apply(a, p):
    """a(p) for points p [..., 2] = (y, x)."""
    a = np.asarray(a, np.float64)
    return np.asarray(p, np.float64) @ a[:, :2].T + a[:, 2]


IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


# ------------------------------------------------------------------------------------------------------- the fixture
FIX_SHAPE, FIX_TILE, FIX_RADIUS, FIX_MARGIN = (16, 96, 128), 32, 4, 24
FIX_ROT, FIX_SHIFT = 0.012, 1.5                  # per pair: a rotation step within +-FIX_ROT rad, a shift within +-FIX_SHIFT px
FIX_PLANTED = {9: 0.03}                          # pair z: its rotation step, 2.4 px at the corners


def _rigid(theta, t, centre):
    """The map p -> R(theta) (p - centre) + centre + t."""
    c, s = np.cos(theta), np.sin(theta)
    L = np.array([[c, -s], [s, c]])
    return np.concatenate([L, (centre - L @ centre + t)[:, None]], axis=1)


@functools.lru_cache(maxsize=None)
def _fixture(seed=31):
    Z, Y, X = FIX_SHAPE
    rng = np.random.default_rng(seed)
    dtheta = rng.uniform(-FIX_ROT, FIX_ROT, Z - 1)
    for z, step in FIX_PLANTED.items():
        dtheta[z] = step
    dt = rng.uniform(-FIX_SHIFT, FIX_SHIFT, (Z - 1, 2))
    theta, t = np.concatenate([[0.0], np.cumsum(dtheta)]), np.concatenate([np.zeros((1, 2)), np.cumsum(dt, axis=0)])
    centre = np.array([(Y - 1) / 2, (X - 1) / 2])
    G = [_rigid(theta[z], t[z], centre) for z in range(Z)]       # section z shows at p the tissue at G[z](p)
    M = FIX_MARGIN
    a = rng.standard_normal((Z, Y + 2 * M, X + 2 * M))
    for _ in range(2):
        for axis in range(3):
            a = _box_blur(a, axis)
    a = 128.0 + 40.0 * a / a.std()
    yx = np.stack(np.meshgrid(np.arange(Y, dtype=np.float64), np.arange(X, dtype=np.float64), indexing="ij"), axis=-1)
    vol = np.empty(FIX_SHAPE, np.uint8)
    for z in range(Z):
        q = apply(G[z], yx) + M
        assert q.min() >= 0 and q[..., 0].max() <= Y + 2 * M - 1 and q[..., 1].max() <= X + 2 * M - 1
        i = np.minimum(np.floor(q).astype(np.int64), [Y + 2 * M - 2, X + 2 * M - 2])
        f = q - i
        s = a[z]
        v = (1 - f[..., 0]) * ((1 - f[..., 1]) * s[i[..., 0], i[..., 1]] + f[..., 1] * s[i[..., 0], i[..., 1] + 1]) + \
            f[..., 0] * ((1 - f[..., 1]) * s[i[..., 0] + 1, i[..., 1]] + f[..., 1] * s[i[..., 0] + 1, i[..., 1] + 1])
        vol[z] = np.clip(np.rint(v).astype(np.int64) + rng.integers(-6, 7, (Y, X)), 0, 255)
    pairs = np.stack([compose(invert(G[z + 1]), G[z]) for z in range(Z - 1)])
    sections = np.stack([compose(invert(G[z]), G[0]) for z in range(Z)])
    for arr in (vol, pairs, sections):
        arr.setflags(write=False)
    return vol, pairs, sections


def rotated_volume():
    """A (16, 96, 128) uint8 volume of zcorr_ref.defect_volume's smooth recipe -- standard normal noise, box-blurred with
    width 5 twice along every axis, scaled to 128 + 40 sigma -- generated with a margin of 24 and every section sampled
    bilinearly in float64 through its own rotation about the centre plus translation, then given integer noise in
    [-6, 6]: no fill enters.  Consecutive sections differ by a rotation step within +-0.012 rad (pair 9: 0.03 rad) and a
    shift within +-1.5 px per axis.  Read-only."""
    return _fixture()[0]


def true_pair_maps():
    """float64[15, 2, 3]: T_z, section z + 1 shows at T_z(p) what section z shows at p.  Read-only."""
    return _fixture()[1]


def true_section_maps():
    """float64[16, 2, 3]: B_0 = I, B_{z + 1} = T_z o B_z: volume[z](B_z p) shows what section 0 shows at p.  Read-only."""
    return _fixture()[2]
