"""The numpy reference of the tile sums along z (include/tem_hip.h: tem_u8_zcorr_tiles), independent of
transfer_em_amd.utils: a loop over sections and tiles with plain slicing, in Python integers.  Also the seeded fixture
with planted defects that the detector's tests share.

For a block [D, H, W] whose voxel (d, y, x) sits at in-plane volume coordinates (y_org + y, x_org + x), tiles of
(th, tw) pixels anchored at the volume's (0, 0) on a grid of gy x gx, and core planes [c0, c1):
  sums[d - c0, i, j] = (sum v, sum v v, sum v v+ (0 for d = D - 1), count) over the block's voxels in tile (i, j)."""
import functools

import numpy as np


def tile_sums(block, c0, c1, y_org, x_org, th, tw, gy, gx):
    """np.int64[c1 - c0, gy, gx, 4] of the block's core planes."""
    block = np.asarray(block)
    D, H, W = block.shape
    out = np.zeros((c1 - c0, gy, gx, 4), np.int64)
    for d in range(c0, c1):
        for i in range(gy):
            ya, yb = max(i * th - y_org, 0), min((i + 1) * th - y_org, H)
            if ya >= yb:
                continue
            for j in range(gx):
                xa, xb = max(j * tw - x_org, 0), min((j + 1) * tw - x_org, W)
                if xa >= xb:
                    continue
                v = block[d, ya:yb, xa:xb].astype(np.int64)
                s12 = int((v * block[d + 1, ya:yb, xa:xb].astype(np.int64)).sum()) if d + 1 < D else 0
                out[d - c0, i, j] = (int(v.sum()), int((v * v).sum()), s12, v.size)
    return out


def volume_sums(vol, tile):
    """np.int64[Z, gy, gx, 4] of a whole volume [Z, Y, X] on tiles (th, tw)."""
    th, tw = tile
    Z, Y, X = vol.shape
    return tile_sums(vol, 0, Z, 0, 0, th, tw, -(-Y // th), -(-X // tw))


def tile_corr(vol, tile):
    """float64[Z - 1, gy, gx]: np.corrcoef of every tile with the same tile one section up, 0.0 where either is constant."""
    th, tw = tile
    Z, Y, X = vol.shape
    gy, gx = -(-Y // th), -(-X // tw)
    c = np.zeros((Z - 1, gy, gx))
    for z in range(Z - 1):
        for i in range(gy):
            for j in range(gx):
                a = vol[z, i * th:(i + 1) * th, j * tw:(j + 1) * tw].reshape(-1).astype(np.float64)
                b = vol[z + 1, i * th:(i + 1) * th, j * tw:(j + 1) * tw].reshape(-1).astype(np.float64)
                if a.min() != a.max() and b.min() != b.max():
                    c[z, i, j] = np.corrcoef(a, b)[0, 1]
    return c


# ------------------------------------------------------------------------------------------------------- the fixture
FIX_SHAPE, FIX_TILE = (48, 96, 128), 32
FIX_SECTIONS = [10, 20, 30, 31]
FIX_TILES = [(40, 1, 2)]


def _box_blur(a, axis, width=5):
    k = np.ones(width) / width
    return np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), axis, a)


@functools.lru_cache(maxsize=None)
def defect_volume(seed=11):
    """A (48, 96, 128) uint8 volume that varies smoothly along every axis -- standard normal noise, box-blurred with
    width 5 twice along every axis, scaled to 128 + 40 sigma, plus integer noise in [-6, 6] -- with planted defects:
    section 10 black, section 20 uniform random bytes, sections 30 and 31 white, and tile (z 40, i 1, j 2) of the 32 x 32
    grid replaced by v[5, 0:32, 0:32].  Read-only."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(FIX_SHAPE)
    for _ in range(2):
        for axis in range(3):
            a = _box_blur(a, axis)
    a = 128.0 + 40.0 * a / a.std()
    v = np.clip(np.rint(a).astype(np.int64) + rng.integers(-6, 7, FIX_SHAPE), 0, 255).astype(np.uint8)
    v[10] = 0
    v[20] = rng.integers(0, 256, FIX_SHAPE[1:], dtype=np.uint8)
    v[30:32] = 255
    v[40, 32:64, 64:96] = v[5, 0:32, 0:32]
    v.setflags(write=False)
    return v
