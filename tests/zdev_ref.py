"""The numpy reference of the z-median outliers (include/tem_hip.h: tem_u8_zdev_tiles, tem_u8_zdev_mask), independent of
transfer_em_amd.utils: plain loops and slicing, as zcorr_ref.  Also the seeded fixture with planted particles that the
detector's tests share.

With nbr[Z, 2] = (lo, hi) per section ((-1, -1): no verdict), a = V[lo], v = V[z], b = V[hi]:
  e = |v - median(a, v, b)|  (0 without a verdict)
  tile sums  t[z, i, j] = (sum e, n) over tile (i, j); n = 0 without a verdict
  mask       1 iff 256 Ws > thr[i, j] c: Ws the sum of e over the (2 r + 1)^2 window cut to the section, c its voxels;
             or where tiles[z, i, j] is set."""
import functools
from typing import NamedTuple

import numpy as np


def neighbours(Z, skip=(), max_lag=4):
    """np.int32[Z, 2]: the nearest good sections below and above, (-1, -1) for a skipped section, the first and last
    good one, and where either neighbour is further than max_lag."""
    bad = set(int(z) for z in skip)
    nbr = np.full((Z, 2), -1, np.int32)
    for z in range(Z):
        if z in bad:
            continue
        below = [k for k in range(z - 1, -1, -1) if k not in bad]
        above = [k for k in range(z + 1, Z) if k not in bad]
        if below and above and z - below[0] <= max_lag and above[0] - z <= max_lag:
            nbr[z] = (below[0], above[0])
    return nbr


def deviation(vol, nbr):
    """np.uint8[Z, Y, X]: e of every voxel."""
    vol = np.asarray(vol)
    e = np.zeros(vol.shape, np.uint8)
    for z in range(vol.shape[0]):
        lo, hi = int(nbr[z][0]), int(nbr[z][1])
        if lo < 0:
            continue
        a, v, b = (vol[k].astype(np.int64) for k in (lo, z, hi))
        m = np.median(np.stack([a, v, b]), axis=0).astype(np.int64)
        e[z] = np.abs(v - m).astype(np.uint8)
    return e


def tile_sums(e, verdict, y_org, x_org, th, tw, gy, gx):
    """np.int64[D, gy, gx, 2] of a block e[D, H, W] of deviations whose voxel (d, y, x) sits at in-plane volume
    coordinates (y_org + y, x_org + x); verdict[d]: whether plane d's section has one."""
    D, H, W = e.shape
    out = np.zeros((D, gy, gx, 2), np.int64)
    for d in range(D):
        if not verdict[d]:
            continue
        for i in range(gy):
            ya, yb = max(i * th - y_org, 0), min((i + 1) * th - y_org, H)
            if ya >= yb:
                continue
            for j in range(gx):
                xa, xb = max(j * tw - x_org, 0), min((j + 1) * tw - x_org, W)
                if xa >= xb:
                    continue
                t = e[d, ya:yb, xa:xb]
                out[d, i, j] = (int(t.astype(np.int64).sum()), t.size)
    return out


def volume_sums(vol, nbr, tile):
    """np.int64[Z, gy, gx, 2] of a whole volume on tiles (th, tw)."""
    th, tw = tile
    Z, Y, X = vol.shape
    return tile_sums(deviation(vol, nbr), [int(nbr[z][0]) >= 0 for z in range(Z)], 0, 0, th, tw, -(-Y // th), -(-X // tw))


def window_sums(e, r):
    """(Ws int64[Z, Y, X], c int64[Y, X]): the sums of e over the (2 r + 1)^2 windows cut to the section, and the cut
    windows' voxel counts.  One shifted add per offset."""
    Z, Y, X = e.shape
    pad = np.zeros((Z, Y + 2 * r, X + 2 * r), np.int64)
    pad[:, r:r + Y, r:r + X] = e
    one = np.zeros((Y + 2 * r, X + 2 * r), np.int64)
    one[r:r + Y, r:r + X] = 1
    Ws, c = np.zeros((Z, Y, X), np.int64), np.zeros((Y, X), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            Ws += pad[:, dy:dy + Y, dx:dx + X]
            c += one[dy:dy + Y, dx:dx + X]
    return Ws, c


def mask(vol, nbr, thr, tile, r, tiles=None):
    """np.uint8[Z, Y, X]: the mask of a whole volume.  thr int[gy, gx]; tiles [Z, gy, gx] or None."""
    th, tw = tile
    Z, Y, X = vol.shape
    Ws, c = window_sums(deviation(vol, nbr), r)
    T = np.repeat(np.repeat(np.asarray(thr, np.int64), th, axis=0), tw, axis=1)[:Y, :X]
    m = 256 * Ws > (T * c)[None]
    if tiles is not None:
        m |= np.repeat(np.repeat(np.asarray(tiles) != 0, th, axis=1), tw, axis=2)[:, :Y, :X]
    return m.astype(np.uint8)


def thresholds(s, ratio=12.0, min_dev=16.0):
    """(thr int32[gy, gx], scale float64[gy, gx]) from tile sums s[Z, gy, gx, 2]."""
    Z, gy, gx, _ = s.shape
    thr, scale = np.zeros((gy, gx), np.int32), np.zeros((gy, gx))
    for i in range(gy):
        for j in range(gx):
            means = [int(s[z, i, j, 0]) / int(s[z, i, j, 1]) for z in range(Z) if s[z, i, j, 1] > 0]
            scale[i, j] = float(np.median(means)) if means else 0.0
            thr[i, j] = min(int(np.ceil(256.0 * max(ratio * scale[i, j], min_dev))), 65280)
    return thr, scale


# ------------------------------------------------------------------------------------------------------- the fixture
FIX_SHAPE, FIX_TILE, FIX_SKIP, FIX_WINDOW = (32, 128, 192), 64, [12], 9
FIX_BLOBS = [(4, 20, 30, 10, 10, 15), (9, 70, 100, 12, 8, 240), (9, 5, 150, 6, 20, 20), (15, 100, 60, 14, 14, 30),
             (22, 60, 170, 9, 9, 235), (27, 118, 2, 10, 10, 10), (1, 40, 90, 8, 8, 25), (30, 0, 0, 12, 12, 250)]
FIX_THICK = ((18, 20), (50, 60), (20, 30), 15)          # two sections thick: resembles a neighbour, not flagged


class Fixture(NamedTuple):
    volume: np.ndarray      # with the particles, the thick blob and the black section 12
    clean: np.ndarray       # before any of them
    planted: np.ndarray     # bool: the single-section particles' voxels
    labels: np.ndarray      # int: 1 + the particle's index in FIX_BLOBS, 0 elsewhere
    thick: np.ndarray       # bool: the thick blob's voxels


def _box_blur(a, axis, width=5):
    k = np.ones(width) / width
    return np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), axis, a)


@functools.lru_cache(maxsize=None)
def fixture():
    """zcorr_ref.defect_volume's recipe without its defects at (32, 128, 192), default_rng(5): standard normal noise,
    box-blurred with width 5 twice along every axis, 128 + 40 a / std, rounded, plus integers(-6, 7), clipped; then
    constant particles FIX_BLOBS = (z, y, x, h, w, value), the thick blob and the black section 12.  Read-only."""
    rng = np.random.default_rng(5)
    a = rng.standard_normal(FIX_SHAPE)
    for _ in range(2):
        for axis in range(3):
            a = _box_blur(a, axis)
    a = 128.0 + 40.0 * a / a.std()
    clean = np.clip(np.rint(a).astype(np.int64) + rng.integers(-6, 7, FIX_SHAPE), 0, 255).astype(np.uint8)
    v = clean.copy()
    planted, labels = np.zeros(FIX_SHAPE, bool), np.zeros(FIX_SHAPE, np.int64)
    for k, (z, y, x, h, w, val) in enumerate(FIX_BLOBS):
        v[z, y:y + h, x:x + w] = val
        planted[z, y:y + h, x:x + w] = True
        labels[z, y:y + h, x:x + w] = k + 1
    v[12] = 0
    (tz0, tz1), (ty0, ty1), (tx0, tx1), val = FIX_THICK
    v[tz0:tz1, ty0:ty1, tx0:tx1] = val
    thick = np.zeros(FIX_SHAPE, bool)
    thick[tz0:tz1, ty0:ty1, tx0:tx1] = True
    for arr in (v, clean, planted, labels, thick):
        arr.setflags(write=False)
    return Fixture(v, clean, planted, labels, thick)


class Verdict(NamedTuple):
    thr: np.ndarray         # the thresholds
    mask: np.ndarray        # the reference's mask of the fixture
    flagged: int            # its ones
    hits: int               # planted voxels flagged
    recall: list            # per particle
    far: int                # flagged voxels further than the radius (Chebyshev, in the section) from a planted voxel
    ratio_away: float       # the largest 256 Ws / (thr c) at voxels further than the radius from any planted or thick voxel
    thick_hits: int         # voxels of the thick blob flagged


@functools.lru_cache(maxsize=None)
def check_fixture():
    """The reference's verdict on the fixture at the defaults (tile 64, window 9, ratio 12, min_dev 16, skip [12])."""
    fx = fixture()
    tile, r = (FIX_TILE, FIX_TILE), FIX_WINDOW // 2
    nbr = neighbours(FIX_SHAPE[0], FIX_SKIP)
    thr, _ = thresholds(volume_sums(fx.volume, nbr, tile))
    m = mask(fx.volume, nbr, thr, tile, r)
    near = window_sums(fx.planted.astype(np.uint8), r)[0] > 0            # within the radius of a planted voxel
    near_any = window_sums((fx.planted | fx.thick).astype(np.uint8), r)[0] > 0
    Ws, c = window_sums(deviation(fx.volume, nbr), r)
    T = np.repeat(np.repeat(thr.astype(np.int64), FIX_TILE, axis=0), FIX_TILE, axis=1)[:FIX_SHAPE[1], :FIX_SHAPE[2]]
    ratio = 256.0 * Ws / (T * c)[None]
    recall = [float(m[fx.labels == k + 1].mean()) for k in range(len(FIX_BLOBS))]
    m.setflags(write=False)
    return Verdict(thr, m, int(m.sum()), int(m[fx.planted].sum()), recall, int((m != 0)[~near].sum()),
                   float(ratio[~near_any].max()), int(m[fx.thick].sum()))
