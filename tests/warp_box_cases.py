"""What the tests of tem_u8_warp_box, utils.warp_source_box and the warp= keyword share: a seeded stack whose sections are
turned, moved and bent, as quantised tables; the taps of an output box by brute force from the numpy references
(warp_ref, field_ref), independent of transfer_em_amd.utils; and the reference of a box-cut call."""
import functools

import numpy as np

import field_ref as FR
import warp_ref as WR

ROT, SHIFT, AMP, SPACING = 0.012, 3.0, 2.0, 32       # per section: +-rad about the centre, +-px, the field's +-px, its lattice


@functools.lru_cache(maxsize=None)
def stack(shape, seed=5, field=True):
    """(M int64[Z, 6], U int32[Z, ny, nx, 2] or None): per section a rotation within +-ROT rad about the centre and a
    shift within +-SHIFT px, and on the lattice of SPACING a field of independent node values within +-AMP px -- adjacent
    nodes differ by at most 2 AMP = 4 px, the limit of SPACING / 8.  Section 0 is the identity with a zero field.
    Read-only."""
    Z, Y, X = shape
    rng = np.random.default_rng(seed)
    c = np.array([(Y - 1) / 2, (X - 1) / 2])
    maps = [WR.IDENTITY] + [WR._rigid(rng.uniform(-ROT, ROT), rng.uniform(-SHIFT, SHIFT, 2), c) for _ in range(Z - 1)]
    M = WR.quantize(np.stack(maps))
    U = None
    if field:
        U = FR.quantize(rng.uniform(-AMP, AMP, (Z,) + FR.grid((Y, X), SPACING) + (2,)))
        U[0] = 0
        assert FR.within_limits(U, SPACING)
        U.setflags(write=False)
    M.setflags(write=False)
    return M, U


def positions(m, u, box, shape):
    """(fy, fx, inside) of the output voxels of the (y, x) box of one section: field_ref's with a field, else warp_ref's."""
    return WR.positions(m, box, shape) if u is None else FR.positions(m, u, SPACING, box, shape)


def taps(m, u, box, shape, nearest=False):
    """(rows, columns): the sorted rows and columns that the inside voxels of the (y, x) box of one section read with a
    weight above 0, by brute force over every voxel."""
    fy, fx, inside = positions(m, u, box, shape)
    out = []
    for f in (fy[inside], fx[inside]):
        out.append(np.unique((f + 128) >> 8) if nearest else np.unique(np.concatenate([f >> 8, (f >> 8)[(f & 255) != 0] + 1])))
    return tuple(out)


def tap_hull(M, U, box, shape, nearest=False):
    """((y0, y1), (x0, x1)) half open: the hull of every tap of the (z, y, x) box, or None where there is none."""
    (z0, z1), yx = box[0], tuple(box[1:])
    rows, cols = zip(*(taps(M[z], None if U is None else U[z], yx, shape[1:], nearest) for z in range(z0, z1)))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    if rows.size == 0:
        return None
    return (int(rows.min()), int(rows.max()) + 1), (int(cols.min()), int(cols.max()) + 1)


def warp(vol, M, U, box=None, fill=0, nearest=False):
    """The aligned volume (or its (z, y, x) box) by the numpy references."""
    return WR.warp(vol, M, box, fill, nearest) if U is None else FR.warp(vol, M, U, SPACING, box, fill, nearest)


def smooth_volume(shape, seed):
    """uint8: a smooth texture plus noise -- a voxel differs from its neighbours, so a tap one pixel off shows."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    v = 128 + 60 * np.sin(0.31 * y + 0.05 * z) * np.cos(0.23 * x - 0.07 * z) + rng.integers(-20, 21, shape)
    a = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    a.setflags(write=False)
    return a
