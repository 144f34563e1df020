"""The numpy reference of the CENTRED shifted tile sums (include/tem_hip.h: tem_u8_zshift_tiles_at), independent of
transfer_em_amd.utils: per plane, tile and local offset plain slicing with the total offset (cy + dy, cx + dx), the
counts by brute force, the coarse-to-fine driver run on the host with these sums, and the seeded fixture of sections
with large planted jumps that the tests share.

For a block [D, H, W] of whole rows whose row 0 sits at row y_org of a section of Y rows, tiles of (th, tw) pixels
anchored at the volume's (0, 0) on a grid of gy x gx, a radius r (R = 2 r + 1), core planes [c0, c1), core rows
[r0, r1) and centres C[plane - c0, i, j] = (cy, cx):
  sums[d - c0, i, j, dy + r, dx + r] = (sum v, sum v v, sum w, sum w w, sum v w) over the core voxels v = (d, y, x) of
  tile (i, j) whose partner w = (d + 1, y + cy + dy, x + cx + dx) lies in the section; all zero for d = D - 1."""
import functools

import numpy as np

from zcorr_ref import _box_blur
from zshift_ref import _five


def tile_sums_at(block, centers, c0, c1, r0, r1, y_org, Y, th, tw, gy, gx, r):
    """np.int64[c1 - c0, gy, gx, R, R, 5]: a loop over planes, tiles and local offsets with plain slicing.  `centers` is
    integers [c1 - c0, gy, gx, 2] (a row of the table per core plane, from plane c0 on)."""
    block, centers = np.asarray(block), np.asarray(centers)
    D, H, W = block.shape
    R = 2 * r + 1
    out = np.zeros((c1 - c0, gy, gx, R, R, 5), np.int64)
    for d in range(c0, min(c1, D - 1)):
        for i in range(gy):
            ya, yb = max(i * th - y_org, r0), min((i + 1) * th - y_org, r1)
            for j in range(gx):
                xa, xb = j * tw, min((j + 1) * tw, W)
                cy, cx = (int(v) for v in centers[d - c0, i, j])
                for dy in range(-r, r + 1):
                    ty = cy + dy
                    yl, yh = max(ya, -y_org - ty), min(yb, Y - y_org - ty)
                    for dx in range(-r, r + 1):
                        tx = cx + dx
                        xl, xh = max(xa, -tx), min(xb, W - tx)
                        if yl >= yh or xl >= xh:
                            continue
                        assert 0 <= yl + ty and yh + ty <= H, "the block lacks a partner row that the volume has"
                        five = _five(block[d, yl:yh, xl:xh], block[d + 1, yl + ty:yh + ty, xl + tx:xh + tx])
                        out[d - c0, i, j, dy + r, dx + r] = [int(a.sum()) for a in five]
    return out


def grid(shape, tile):
    return -(-shape[-2] // tile[0]), -(-shape[-1] // tile[1])


def volume_sums_at(vol, centers, tile, r):
    """np.int64[Z, gy, gx, R, R, 5] of a whole volume [Z, Y, X] on tiles (th, tw) with centres [Z - 1, gy, gx, 2]."""
    Z, Y, X = vol.shape
    gy, gx = grid(vol.shape, tile)
    table = np.zeros((Z, gy, gx, 2), np.int64)
    table[:Z - 1] = centers
    return tile_sums_at(vol, table, 0, Z, 0, Y, 0, Y, *tile, gy, gx, r)


def counts_at_brute(shape, tile, r, centers):
    """np.int64[P, gy, gx, R, R]: the number of terms of every entry, by counting voxels one by one."""
    (Y, X), (th, tw) = shape[-2:], tile
    centers = np.asarray(centers)
    P, gy, gx = centers.shape[:3]
    n = np.zeros((P, gy, gx, 2 * r + 1, 2 * r + 1), np.int64)
    for z in range(P):
        for y in range(Y):
            for x in range(X):
                cy, cx = centers[z, y // th, x // tw]
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        if 0 <= y + cy + dy < Y and 0 <= x + cx + dx < X:
                            n[z, y // th, x // tw, dy + r, dx + r] += 1
    return n


# ------------------------------------------------------------------------------------------------------- the fixture
BIG_SHAPE, BIG_TILE, BIG_RADIUS, BIG_LEVELS = (10, 160, 192), 32, 4, 3
BIG_PLANTED = {2: (11, -9), 5: (-22, 17), 7: (6, 27), 8: (44, 0)}       # pair z: (dy, dx); (44, 0) is beyond 3 x 2^3


@functools.lru_cache(maxsize=None)
def big_pairs():
    """int64[9, 2]: the displacement (dy, dx) of section z + 1 against section z: steps in [-1, 1] per axis, and the
    planted jumps.  Read-only."""
    pairs = np.random.default_rng(31).integers(-1, 2, (BIG_SHAPE[0] - 1, 2)).astype(np.int64)
    for z, step in BIG_PLANTED.items():
        pairs[z] = step
    pairs.setflags(write=False)
    return pairs


def big_positions():
    return np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(big_pairs(), axis=0)])


@functools.lru_cache(maxsize=None)
def big_jump_volume():
    """A (10, 160, 192) uint8 volume of zshift_ref's recipe -- standard normal noise, box-blurred twice along every
    axis, scaled to 128 + 40 sigma, plus integer noise in [-6, 6] -- generated with a margin and every section cut out
    at its own origin first - P[z], so that section z + 1 shows at (y + dy, x + dx) what section z shows at (y, x),
    (dy, dx) = big_pairs()[z], and no fill enters.  Read-only."""
    P = big_positions()
    first = P.max(axis=0)
    span = P.max(axis=0) - P.min(axis=0)
    shape = (BIG_SHAPE[0], BIG_SHAPE[1] + int(span[0]), BIG_SHAPE[2] + int(span[1]))
    rng = np.random.default_rng(32)
    a = rng.standard_normal(shape)
    for _ in range(2):
        for axis in range(3):
            a = _box_blur(a, axis)
    a = 128.0 + 40.0 * a / a.std()
    base = np.clip(np.rint(a).astype(np.int64) + rng.integers(-6, 7, shape), 0, 255).astype(np.uint8)
    (_, Y, X), org = BIG_SHAPE, first[None] - P
    vol = np.stack([base[z, org[z, 0]:org[z, 0] + Y, org[z, 1]:org[z, 1] + X] for z in range(shape[0])])
    vol.setflags(write=False)
    return vol


def halve(vol):
    """(S + 2) // 4 over 2 x 2 pixels of every section: volume_rescale's rule at step (2, 2, 1) for even Y and X."""
    v = vol.astype(np.int64)
    return ((v[:, 0::2, 0::2] + v[:, 0::2, 1::2] + v[:, 1::2, 0::2] + v[:, 1::2, 1::2] + 2) // 4).astype(np.uint8)


def host_rescale(volume, step, out=None, **kw):
    """volume_rescale's stand-in for the driver run on the host."""
    assert tuple(step) == (2, 2, 1) and volume.shape[1] % 2 == 0 and volume.shape[2] % 2 == 0
    got = halve(np.asarray(volume))
    if out is None:
        return got
    out[...] = got
    return out


def host_sums_at(volume, centers, tile=128, radius=4, **kw):
    """section_shift_sums_at's stand-in for the driver run on the host."""
    tile = (tile, tile) if isinstance(tile, int) else tuple(tile)
    return volume_sums_at(np.asarray(volume), centers, tile, radius)


@functools.lru_cache(maxsize=None)
def host_driver(levels=BIG_LEVELS):
    """section_shifts_coarse_to_fine on big_jump_volume() with the device passes replaced by this module's numpy:
    the driver's own logic with the reference's sums.  Read-only by convention."""
    import pytest
    from transfer_em_amd import utils
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(utils, "volume_rescale", host_rescale)
        mp.setattr(utils, "section_shift_sums_at", host_sums_at)
        return utils.section_shifts_coarse_to_fine(big_jump_volume(), BIG_TILE, BIG_RADIUS, levels)
