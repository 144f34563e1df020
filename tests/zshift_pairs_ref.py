"""The numpy reference of the shifted tile sums of an explicit list of section PAIRS (include/tem_hip.h:
tem_u8_zshift_tiles_pairs), independent of transfer_em_amd.utils: per pair, tile and local offset plain slicing, the
pair-list driver run on the host with these sums, and the seeded fixture of drifting sections with bad sections among
them that the tests share.

For a block [D, H, W] of whole rows whose plane 0 is volume section z_org and whose row 0 sits at row y_org of a
section of Y rows, tiles of (th, tw) pixels anchored at the volume's (0, 0) on a grid of gy x gx, a radius r
(R = 2 r + 1), core rows [r0, r1), pairs[k] = (a, b) and centres C[k, i, j] = (cy, cx):
  sums[k, i, j, dy + r, dx + r] = (sum v, sum v v, sum w, sum w w, sum v w) over the core voxels v = (a - z_org, y, x)
  of tile (i, j) whose partner w = (b - z_org, y + cy + dy, x + cx + dx) lies in the section.

The fixture (BAD_*): zshift_ref's recipe at 12 x 160 x 192 -- its two box blurs of width 5 along z are enough for
sections three apart to resemble each other, so it is blurred no further --, every section cut at its own origin:
steps in [-1, 1] per axis plus a steady drift of (3, -2) per section, and a jump of (13, -17) planted on pair 3,
across a bad section.  Then section 3 is made black and sections 7 and 8 uniform noise; the good sections on either
side are bridged by the pairs (2, 4), lag 2, and (6, 9), lag 3.  Checked on the CPU with the driver run on the host
(host_bridged; tile 32, radius 4, levels 3, min_corr 0.1, min_decided 0.5) -- this fixture's own values, not bars of
any test:
  every pair of the chain resolved; every good section's position exact
  decided tiles of 30: 30 for each of the six lag-1 pairs, 30 for the bridge (2, 4), 30 for the bridge (6, 9)
  smallest peak among decided tiles: lag 1 0.888, (2, 4) 0.700, (6, 9) 0.433
  the bridges measure (16, -18) and (9, -7)
section_shifts_coarse_to_fine on the same volume leaves the pairs 2, 3, 6, 7, 8 unresolved (suspect_sections: 3, 7, 8),
and the sections from 4 on sit off by (-16, 18), growing to (-25, 25) from section 9 on: the displacements that those
pairs carry."""
import functools

import numpy as np

from zcorr_ref import _box_blur
from zshift_ref import _five


def tile_sums_pairs(block, pairs, centers, z_org, r0, r1, y_org, Y, th, tw, gy, gx, r):
    """np.int64[P, gy, gx, R, R, 5]: a loop over pairs, tiles and local offsets with plain slicing.  `pairs` is integers
    [P, 2] of volume sections, `centers` integers [P, gy, gx, 2]."""
    block, pairs, centers = np.asarray(block), np.asarray(pairs), np.asarray(centers)
    D, H, W = block.shape
    R = 2 * r + 1
    out = np.zeros((len(pairs), gy, gx, R, R, 5), np.int64)
    for k, (a, b) in enumerate(pairs.tolist()):
        assert 0 <= a - z_org < D and 0 <= b - z_org < D, "the block lacks a section of the pair"
        va, vb = block[a - z_org], block[b - z_org]
        for i in range(gy):
            ya, yb = max(i * th - y_org, r0), min((i + 1) * th - y_org, r1)
            for j in range(gx):
                xa, xb = j * tw, min((j + 1) * tw, W)
                cy, cx = (int(v) for v in centers[k, i, j])
                for dy in range(-r, r + 1):
                    ty = cy + dy
                    yl, yh = max(ya, -y_org - ty), min(yb, Y - y_org - ty)
                    for dx in range(-r, r + 1):
                        tx = cx + dx
                        xl, xh = max(xa, -tx), min(xb, W - tx)
                        if yl >= yh or xl >= xh:
                            continue
                        assert 0 <= yl + ty and yh + ty <= H, "the block lacks a partner row that the volume has"
                        five = _five(va[yl:yh, xl:xh], vb[yl + ty:yh + ty, xl + tx:xh + tx])
                        out[k, i, j, dy + r, dx + r] = [int(s.sum()) for s in five]
    return out


def grid(shape, tile):
    return -(-shape[-2] // tile[0]), -(-shape[-1] // tile[1])


def volume_sums_pairs(vol, pairs, centers, tile, r):
    """np.int64[P, gy, gx, R, R, 5] of a whole volume [Z, Y, X] on tiles (th, tw) with centres [P, gy, gx, 2]."""
    Z, Y, X = vol.shape
    return tile_sums_pairs(vol, pairs, centers, 0, 0, Y, 0, Y, *tile, *grid(vol.shape, tile), r)


# ------------------------------------------------------------------------------------------------------- the fixture
BAD_SHAPE, BAD_TILE, BAD_RADIUS, BAD_LEVELS = (12, 160, 192), 32, 4, 3
BAD_DRIFT, BAD_JUMP = (3, -2), {3: (13, -17)}                    # per section; pair z: (dy, dx), planted
BAD_BLACK, BAD_NOISE = 3, (7, 8)
BAD_SKIP = (3, 7, 8)
BAD_BRIDGES = ((2, 4), (6, 9))


@functools.lru_cache(maxsize=None)
def bad_pairs():
    """int64[11, 2]: the displacement (dy, dx) of section z + 1 against section z: steps in [-1, 1] per axis plus the
    drift, and the planted jump.  Read-only."""
    pairs = np.random.default_rng(71).integers(-1, 2, (BAD_SHAPE[0] - 1, 2)).astype(np.int64) + np.array(BAD_DRIFT)
    for z, step in BAD_JUMP.items():
        pairs[z] = step
    pairs.setflags(write=False)
    return pairs


def bad_positions():
    """int64[12, 2]: where every section truly sits, P[0] = 0, P[z + 1] = P[z] + pairs[z]."""
    return np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(bad_pairs(), axis=0)])


@functools.lru_cache(maxsize=None)
def bad_volume():
    """The (12, 160, 192) uint8 fixture: standard normal noise, box-blurred with width 5 twice along every axis, scaled
    to 128 + 40 sigma, plus integer noise in [-6, 6], generated with a margin and every section cut out at its own
    origin first - P[z]; then section 3 black, sections 7 and 8 uniform random bytes.  Read-only."""
    P = bad_positions()
    first = P.max(axis=0)
    span = P.max(axis=0) - P.min(axis=0)
    shape = (BAD_SHAPE[0], BAD_SHAPE[1] + int(span[0]), BAD_SHAPE[2] + int(span[1]))
    rng = np.random.default_rng(72)
    a = rng.standard_normal(shape)
    for _ in range(2):
        for axis in range(3):
            a = _box_blur(a, axis)
    a = 128.0 + 40.0 * a / a.std()
    base = np.clip(np.rint(a).astype(np.int64) + rng.integers(-6, 7, shape), 0, 255).astype(np.uint8)
    (_, Y, X), org = BAD_SHAPE, first[None] - P
    vol = np.stack([base[z, org[z, 0]:org[z, 0] + Y, org[z, 1]:org[z, 1] + X] for z in range(shape[0])])
    vol[BAD_BLACK] = 0
    for z in BAD_NOISE:
        vol[z] = rng.integers(0, 256, (Y, X), dtype=np.uint8)
    vol.setflags(write=False)
    return vol


def halve(vol):
    """(S + 2) // 4 over 2 x 2 pixels of every section: volume_rescale's rule at step (2, 2, 1) for even Y and X."""
    v = vol.astype(np.int64)
    return ((v[:, 0::2, 0::2] + v[:, 0::2, 1::2] + v[:, 1::2, 0::2] + v[:, 1::2, 1::2] + 2) // 4).astype(np.uint8)


def host_rescale(volume, step, out=None, start=None, size=None, **kw):
    """volume_rescale's stand-in for the drivers run on the host: whole sections [z0, z0 + n) of the output grid."""
    assert tuple(step) == (2, 2, 1) and volume.shape[1] % 2 == 0 and volume.shape[2] % 2 == 0
    z0, n = (0, volume.shape[0]) if start is None else (start[2], size[2])
    assert start is None or (tuple(start[:2]) == (0, 0) and tuple(size[:2]) == (volume.shape[2] // 2, volume.shape[1] // 2))
    got = halve(np.asarray(volume[z0:z0 + n]))
    if out is None:
        return got
    out[...] = got
    return out


def host_sums_pairs(volume, pairs, centers=None, tile=128, radius=4, **kw):
    """section_shift_sums_pairs' stand-in for the driver run on the host."""
    tile = (tile, tile) if isinstance(tile, int) else tuple(tile)
    return volume_sums_pairs(np.asarray(volume), pairs, centers, tile, radius)


def host_sums_at(volume, centers, tile=128, radius=4, **kw):
    """section_shift_sums_at's stand-in: the pairs (z, z + 1) and a row of zeros for the last section."""
    Z = volume.shape[0]
    q = host_sums_pairs(volume, [(z, z + 1) for z in range(Z - 1)], centers, tile, radius)
    return np.concatenate([q, np.zeros_like(q[:1])])


def host_run(fn, *a, **kw):
    """fn(*a, **kw) with utils' device passes replaced by this module's numpy."""
    import pytest
    from transfer_em_amd import utils
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(utils, "volume_rescale", host_rescale)
        mp.setattr(utils, "section_shift_sums_at", host_sums_at)
        mp.setattr(utils, "section_shift_sums_pairs", host_sums_pairs)
        return fn(*a, **kw)


@functools.lru_cache(maxsize=None)
def chain_list():
    """section_pairs' list for the fixture: the good sections' chain, bridges included."""
    from transfer_em_amd import utils
    got = utils.section_pairs(BAD_SHAPE[0], BAD_SKIP)
    assert not got.broken
    got.pairs.setflags(write=False)
    return got.pairs


@functools.lru_cache(maxsize=None)
def host_bridged(bridges_only=False):
    """section_shifts_bridged on bad_volume(), over the whole chain or the two bridges alone, run on the host: the
    driver's own logic with the reference's sums.  Read-only by convention."""
    from transfer_em_amd import utils
    pairs = np.array(BAD_BRIDGES, np.int64) if bridges_only else chain_list()
    return host_run(utils.section_shifts_bridged, bad_volume(), pairs, BAD_TILE, BAD_RADIUS, BAD_LEVELS)


@functools.lru_cache(maxsize=None)
def host_plain():
    """section_shifts_coarse_to_fine on bad_volume(), run on the host: what the chain gives without bridges."""
    from transfer_em_amd import utils
    return host_run(utils.section_shifts_coarse_to_fine, bad_volume(), BAD_TILE, BAD_RADIUS, BAD_LEVELS)
