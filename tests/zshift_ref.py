"""The numpy reference of the shifted tile sums along z (include/tem_hip.h: tem_u8_zshift_tiles), independent of
transfer_em_amd.utils: per plane, tile and offset plain slicing (tile_sums_direct), the same per plane and offset with
the tiles summed by np.add.reduceat (tile_sums, which the kernel's tests can afford on 1 x 1 tiles), and the closed-form
counts.  Also the seeded fixture of jittered sections that the shift tests share.

For a block [D, H, W] of whole rows whose row 0 sits at row y_org of a section of Y rows, tiles of (th, tw) pixels
anchored at the volume's (0, 0) on a grid of gy x gx, a radius r (R = 2 r + 1), core planes [c0, c1), core rows [r0, r1):
  sums[d - c0, i, j, dy + r, dx + r] = (sum v, sum v v, sum w, sum w w, sum v w) over the core voxels v = (d, y, x) of
  tile (i, j) whose partner w = (d + 1, y + dy, x + dx) lies in the section; all zero for d = D - 1."""
import functools

import numpy as np

from zcorr_ref import _box_blur


def _five(v, w):
    v, w = v.astype(np.int64), w.astype(np.int64)
    return v, v * v, w, w * w, v * w


def tile_sums_direct(block, c0, c1, r0, r1, y_org, Y, th, tw, gy, gx, r):
    """np.int64[c1 - c0, gy, gx, R, R, 5]: a loop over planes, tiles and offsets with plain slicing."""
    block = np.asarray(block)
    D, H, W = block.shape
    R = 2 * r + 1
    out = np.zeros((c1 - c0, gy, gx, R, R, 5), np.int64)
    for d in range(c0, min(c1, D - 1)):
        for i in range(gy):
            ya, yb = max(i * th - y_org, r0), min((i + 1) * th - y_org, r1)
            for j in range(gx):
                xa, xb = j * tw, min((j + 1) * tw, W)
                for dy in range(-r, r + 1):
                    yl, yh = max(ya, -y_org - dy), min(yb, Y - y_org - dy)
                    for dx in range(-r, r + 1):
                        xl, xh = max(xa, -dx), min(xb, W - dx)
                        if yl >= yh or xl >= xh:
                            continue
                        assert 0 <= yl + dy and yh + dy <= H, "the block lacks a partner row that the volume has"
                        five = _five(block[d, yl:yh, xl:xh], block[d + 1, yl + dy:yh + dy, xl + dx:xh + dx])
                        out[d - c0, i, j, dy + r, dx + r] = [int(a.sum()) for a in five]
    return out


def tile_sums(block, c0, c1, r0, r1, y_org, Y, th, tw, gy, gx, r):
    """The same array: per plane and offset the five products over the voxels that have a partner, as whole images with
    zeros elsewhere, summed over the tiles with np.add.reduceat."""
    block = np.asarray(block)
    D, H, W = block.shape
    R = 2 * r + 1
    out = np.zeros((c1 - c0, gy, gx, R, R, 5), np.int64)
    if r0 >= r1:
        return out
    i0, j0 = (y_org + r0) // th, 0
    ycuts = [max(i * th - y_org, r0) - r0 for i in range(i0, (y_org + r1 - 1) // th + 1)]
    xcuts = [j * tw for j in range(j0, (W - 1) // tw + 1)]
    for d in range(c0, min(c1, D - 1)):
        for dy in range(-r, r + 1):
            yl, yh = max(r0, -y_org - dy), min(r1, Y - y_org - dy)
            for dx in range(-r, r + 1):
                xl, xh = max(0, -dx), min(W, W - dx)
                if yl >= yh or xl >= xh:
                    continue
                assert 0 <= yl + dy and yh + dy <= H, "the block lacks a partner row that the volume has"
                img = np.zeros((5, r1 - r0, W), np.int64)
                img[:, yl - r0:yh - r0, xl:xh] = _five(block[d, yl:yh, xl:xh],
                                                       block[d + 1, yl + dy:yh + dy, xl + dx:xh + dx])
                t = np.add.reduceat(np.add.reduceat(img, ycuts, axis=1), xcuts, axis=2)
                out[d - c0, i0:i0 + len(ycuts), :len(xcuts), dy + r, dx + r] = np.moveaxis(t, 0, -1)
    return out


def volume_sums(vol, tile, r):
    """np.int64[Z, gy, gx, R, R, 5] of a whole volume [Z, Y, X] on tiles (th, tw)."""
    th, tw = tile
    Z, Y, X = vol.shape
    return tile_sums(vol, 0, Z, 0, Y, 0, Y, th, tw, -(-Y // th), -(-X // tw), r)


def counts(shape, tile, r):
    """np.int64[gy, gx, R, R]: the number of terms of every entry, in closed form: rows x columns."""
    (Y, X), (th, tw) = shape[-2:], tile
    gy, gx = -(-Y // th), -(-X // tw)
    n = np.zeros((gy, gx, 2 * r + 1, 2 * r + 1), np.int64)
    for i in range(gy):
        for j in range(gx):
            for dy in range(-r, r + 1):
                rows = min((i + 1) * th, Y, Y - dy) - max(i * th, -dy)
                for dx in range(-r, r + 1):
                    cols = min((j + 1) * tw, X, X - dx) - max(j * tw, -dx)
                    n[i, j, dy + r, dx + r] = max(rows, 0) * max(cols, 0)
    return n


def counts_brute(shape, tile, r):
    """The same by counting voxels one by one."""
    (Y, X), (th, tw) = shape[-2:], tile
    gy, gx = -(-Y // th), -(-X // tw)
    n = np.zeros((gy, gx, 2 * r + 1, 2 * r + 1), np.int64)
    for y in range(Y):
        for x in range(X):
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    if 0 <= y + dy < Y and 0 <= x + dx < X:
                        n[y // th, x // tw, dy + r, dx + r] += 1
    return n


def shifted_corr(vol, tile, r):
    """float64[Z - 1, gy, gx, R, R]: np.corrcoef of every tile's voxels that have a partner with those partners, 0.0
    where either side is constant."""
    th, tw = tile
    Z, Y, X = vol.shape
    gy, gx = -(-Y // th), -(-X // tw)
    c = np.zeros((Z - 1, gy, gx, 2 * r + 1, 2 * r + 1))
    for z in range(Z - 1):
        for i in range(gy):
            for j in range(gx):
                for dy in range(-r, r + 1):
                    yl, yh = max(i * th, -dy), min((i + 1) * th, Y, Y - dy)
                    for dx in range(-r, r + 1):
                        xl, xh = max(j * tw, -dx), min((j + 1) * tw, X, X - dx)
                        if yl >= yh or xl >= xh:
                            continue
                        a = vol[z, yl:yh, xl:xh].reshape(-1).astype(np.float64)
                        b = vol[z + 1, yl + dy:yh + dy, xl + dx:xh + dx].reshape(-1).astype(np.float64)
                        if a.min() != a.max() and b.min() != b.max():
                            c[z, i, j, dy + r, dx + r] = np.corrcoef(a, b)[0, 1]
    return c


# ------------------------------------------------------------------------------------------------------- the fixture
FIX_SHAPE, FIX_TILE, FIX_RADIUS = (24, 90, 120), 32, 4
FIX_PLANTED = {7: (4, -1), 15: (-2, 6)}          # pair z: (dy, dx); one component equal to the radius, one past it


@functools.lru_cache(maxsize=None)
def fixture_pairs(seed=23):
    """int64[23, 2]: the displacement (dy, dx) of section z + 1 against section z: steps in [-1, 1] per axis, and the
    two planted pairs.  Read-only."""
    rng = np.random.default_rng(seed)
    pairs = rng.integers(-1, 2, (FIX_SHAPE[0] - 1, 2)).astype(np.int64)
    for z, step in FIX_PLANTED.items():
        pairs[z] = step
    pairs.setflags(write=False)
    return pairs


def fixture_positions():
    """int64[24, 2]: P[0] = 0, P[z + 1] = P[z] + pairs[z]."""
    return np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(fixture_pairs(), axis=0)])


@functools.lru_cache(maxsize=None)
def _fixture(seed=23):
    P = fixture_positions()
    first = P.max(axis=0)                                        # where section 0 is cut: every origin stays >= 0
    span = P.max(axis=0) - P.min(axis=0)
    shape = (FIX_SHAPE[0], FIX_SHAPE[1] + int(span[0]), FIX_SHAPE[2] + int(span[1]))
    rng = np.random.default_rng(seed + 1)
    a = rng.standard_normal(shape)
    for _ in range(2):
        for axis in range(3):
            a = _box_blur(a, axis)
    a = 128.0 + 40.0 * a / a.std()
    base = np.clip(np.rint(a).astype(np.int64) + rng.integers(-6, 7, shape), 0, 255).astype(np.uint8)
    (_, Y, X), org = FIX_SHAPE, first[None] - P                  # section z is cut at org[z]
    vol = np.stack([base[z, org[z, 0]:org[z, 0] + Y, org[z, 1]:org[z, 1] + X] for z in range(shape[0])])
    flat = np.ascontiguousarray(base[:, first[0]:first[0] + Y, first[1]:first[1] + X])
    vol.setflags(write=False), flat.setflags(write=False)
    return vol, flat


def jitter_volume():
    """A (24, 90, 120) uint8 volume of zcorr_ref.defect_volume's smooth recipe -- standard normal noise, box-blurred with
    width 5 twice along every axis, scaled to 128 + 40 sigma, plus integer noise in [-6, 6] -- generated with a margin
    and every section cut out at its own origin, so that section z + 1 shows at (y + dy, x + dx) what section z shows at
    (y, x), (dy, dx) = fixture_pairs()[z], and no fill enters.  Read-only."""
    return _fixture()[0]


def flat_volume():
    """The same sections all cut at section 0's origin: what volume_shift(jitter_volume(), fixture_positions()) gives
    wherever no fill enters.  Read-only."""
    return _fixture()[1]


@functools.lru_cache(maxsize=None)
def fixture_sums():
    """volume_sums of the jittered fixture at its tile and radius.  Read-only."""
    q = volume_sums(jitter_volume(), (FIX_TILE, FIX_TILE), FIX_RADIUS)
    q.setflags(write=False)
    return q
