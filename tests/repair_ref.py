"""The numpy reference of the repair along z (include/tem_hip.h: tem_u8_repair_z), independent of transfer_em_amd.utils
and the one numpy statement of the rule: vectorised over a whole volume [Z, Y, X], one pass per distance d = 1 ... R.

A voxel is bad if any given source says so (`sections`: whole sections; `mask`: non-zero bytes; `missing_value`: one grey
level).  A bad voxel takes the nearest good voxel of its column at most R = max_gap below (a, at distance d0) and above
(b, d1): (2 (a d1 + b d0) + n) // (2 n) with n = d0 + d1 where both exist, the one that exists, or stays as it is."""
import numpy as np


def bad_voxels(vol, sections=None, mask=None, missing_value=None):
    """The bool [Z, Y, X] map of bad voxels."""
    vol = np.asarray(vol)
    bad = np.zeros(vol.shape, bool)
    if sections is not None:
        bad[[int(z) for z in sections]] = True
    if mask is not None:
        bad |= np.asarray(mask) != 0
    if missing_value is not None:
        bad |= vol == missing_value
    return bad


def _nearest_good(vol, bad, R, up):
    """(value, distance) of the nearest good voxel at most R planes below (up=False) or above (up=True); distance 0
    where there is none."""
    Z = vol.shape[0]
    val = np.zeros(vol.shape, np.int64)
    dist = np.zeros(vol.shape, np.int64)
    for d in range(1, min(R, Z - 1) + 1):
        here, there = (slice(0, Z - d), slice(d, Z)) if up else (slice(d, Z), slice(0, Z - d))
        take = ~bad[there] & (dist[here] == 0)
        val[here][take] = vol[there][take]
        dist[here][take] = d
    return val, dist


def filled(vol, sections=None, mask=None, missing_value=None, max_gap=8):
    """The bool [Z, Y, X] map of the bad voxels that have a good voxel within max_gap: those `repair` fills (whether or
    not the byte changes).  The bad voxels outside it stay as they are."""
    vol = np.asarray(vol)
    bad = bad_voxels(vol, sections, mask, missing_value)
    return bad & ((_nearest_good(vol, bad, max_gap, False)[1] > 0) | (_nearest_good(vol, bad, max_gap, True)[1] > 0))


def repair(vol, sections=None, mask=None, missing_value=None, max_gap=8, counts=False):
    """The repaired copy of the uint8 volume `vol` [Z, Y, X]; with counts=True, (copy, repaired, unrepaired): the bad
    voxels that were filled and those left as they are."""
    vol = np.asarray(vol)
    assert vol.dtype == np.uint8 and vol.ndim == 3 and 1 <= max_gap <= 32
    bad = bad_voxels(vol, sections, mask, missing_value)
    a, d0 = _nearest_good(vol, bad, max_gap, False)
    b, d1 = _nearest_good(vol, bad, max_gap, True)
    n = d0 + d1
    both = bad & (d0 > 0) & (d1 > 0)
    below = bad & (d0 > 0) & (d1 == 0)
    above = bad & (d0 == 0) & (d1 > 0)
    out = vol.copy()
    out[both] = ((2 * (a * d1 + b * d0) + n)[both] // (2 * n[both])).astype(np.uint8)
    out[below] = a[below].astype(np.uint8)
    out[above] = b[above].astype(np.uint8)
    if counts:
        rep = int(both.sum() + below.sum() + above.sum())
        return out, rep, int(bad.sum()) - rep
    return out
