"""The numpy references of the spacing measurement along z, independent of transfer_em_amd.utils: the lag sums
(include/tem_hip.h: tem_u8_zcorr_lags) as loops over sections and tiles in Python integers, the taps and the blend of
tem_u8_resample_z, and the estimator of utils.section_spacing with a dense least-squares solve.  Also the seeded
fixture with planted section positions that the tests share.

The fixture (fixture()): a random field smoothed separably (Gaussian, sigma 2 sections along z on a grid 8 x finer than
a section and padded by 4 sigma at both ends, sigma 1.5 pixels in plane -- a tile of 32 x 32 then holds enough
independent samples for its correlations --), sampled linearly at 40 planted positions of 64 x 96 pixels -- spacings
drawn in [0.6, 1.5], one gap of 2.6, then scaled so that the positions run from 0 to 39 (the gap: 2.42) --, scaled to
128 + 40 sigma, plus integer noise in [-2, 2], as uint8; section FIX_SKIP is black.  The ground truth is the same field
sampled at 0, 1, ..., 39.  The conditions, computed by check_fixture() from this file alone on tiles of 32 and lags
1...4 (values recorded from it):
  the curve decreases strictly                      1, 0.9449, 0.7992, 0.5974, 0.4187
  every tile column is decided                      6 of 6
  the largest spacing error of good neighbours      0.1477 sections (bar: 0.25) where even spacing is off by 1.4186 (>= 1.0)
  the largest position error                        0.3714 sections, against 1.5159 for even spacing
  RMSE against the ground truth, grey levels        raw 11.9121, resampled 2.4943 (bar: half of raw); true positions 1.8857
  clipped and unresolved                            empty
The RMSE is taken over the output sections that are not FIX_SKIP and whose taps do not touch it: a black section is
volume_repair's to mend, not the resampler's."""
import functools

import numpy as np

UNIT = 1 << 16


# ---------------------------------------------------------------------------------------------------------- lag sums
def lag_tile_sums(block, c0, c1, y_org, x_org, th, tw, gy, gx, nlag):
    """np.int64[c1 - c0, gy, gx, 3 + nlag] of the block's core planes: (sum v, sum v v, count, sum v v+1, ...)."""
    block = np.asarray(block)
    D, H, W = block.shape
    out = np.zeros((c1 - c0, gy, gx, 3 + nlag), np.int64)
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
                row = [int(v.sum()), int((v * v).sum()), v.size]
                for k in range(1, nlag + 1):
                    row.append(int((v * block[d + k, ya:yb, xa:xb].astype(np.int64)).sum()) if d + k < D else 0)
                out[d - c0, i, j] = row
    return out


def lag_tile_sums_fast(block, c0, c1, y_org, x_org, th, tw, gy, gx, nlag):
    """lag_tile_sums without the loops, for grids of many small tiles: the per-voxel terms, summed between the tile
    boundaries with np.add.reduceat.  test_zspace_plan.py holds it to the loops."""
    v = np.asarray(block).astype(np.int64)
    D, H, W = v.shape
    terms = [v, v * v, np.ones_like(v)]
    for k in range(1, nlag + 1):
        t = np.zeros_like(v)
        if k < D:
            t[:D - k] = v[:D - k] * v[k:]
        terms.append(t)
    q = np.stack(terms, axis=-1)[c0:c1]                                                 # [core, H, W, 3 + nlag]
    out = np.zeros((c1 - c0, gy, gx, 3 + nlag), np.int64)
    if c1 == c0:
        return out
    ti, tj = (y_org + np.arange(H)) // th, (x_org + np.arange(W)) // tw
    ys, xs = np.concatenate([[0], np.flatnonzero(np.diff(ti)) + 1]), np.concatenate([[0], np.flatnonzero(np.diff(tj)) + 1])
    q = np.add.reduceat(np.add.reduceat(q, ys, axis=1), xs, axis=2)
    out[:, ti[0]:ti[-1] + 1, tj[0]:tj[-1] + 1] = q
    return out


def volume_lag_sums(vol, tile, nlag):
    th, tw = tile
    Z, Y, X = vol.shape
    return lag_tile_sums(vol, 0, Z, 0, 0, th, tw, -(-Y // th), -(-X // tw), nlag)


# ------------------------------------------------------------------------------------------------- taps and the blend
def taps(Q, nz=None):
    """int32[NZ, 2] = (z0, w) from quantised positions, in Python integers, one output section at a time."""
    Q = [int(q) for q in Q]
    Z = len(Q)
    NZ = Q[-1] // UNIT + 1 if nz is None else nz
    out = []
    for j in range(NZ):
        t = j * UNIT
        z0 = max(z for z in range(Z) if Q[z] <= t)
        if z0 == Z - 1:
            out.append((z0, 0))
            continue
        den = Q[z0 + 1] - Q[z0]
        w = (512 * (t - Q[z0]) + den) // (2 * den)
        out.append((z0 + 1, 0) if w == 256 else (z0, w))
    return np.array(out, np.int32).reshape(-1, 2)


def resample(vol, table, nearest=False, box=None):
    """The output sections of `table` (all of them, or the (z, y, x) (lo, hi) `box` of the output) from the volume."""
    vol = np.asarray(vol)
    VZ = vol.shape[0]
    (z0, z1), (y0, y1), (x0, x1) = ((0, len(table)), (0, vol.shape[1]), (0, vol.shape[2])) if box is None else box
    out = np.zeros((z1 - z0, y1 - y0, x1 - x0), np.uint8)
    for j in range(z0, z1):
        z, w = int(table[j][0]), int(table[j][1])
        a = vol[z, y0:y1, x0:x1].astype(np.int64)
        b = vol[min(z + 1, VZ - 1), y0:y1, x0:x1].astype(np.int64)
        out[j - z0] = (a if w < 128 else b) if nearest else ((256 - w) * a + w * b + 128) >> 8
    return out


# ------------------------------------------------------------------------------------------------------ the estimator
def scores(s):
    """float64[Z, gy, gx, L] from lag sums, tile by tile."""
    Z, gy, gx, L = s.shape[0], s.shape[1], s.shape[2], s.shape[3] - 3
    c = np.zeros((Z, gy, gx, L))
    for z in range(Z):
        for i in range(gy):
            for j in range(gx):
                n, S1, S2 = (int(v) for v in s[z, i, j, [2, 0, 1]])
                A = n * S2 - S1 * S1
                for k in range(1, L + 1):
                    if z + k >= Z:
                        continue
                    T1, T2 = int(s[z + k, i, j, 0]), int(s[z + k, i, j, 1])
                    B = n * T2 - T1 * T1
                    if A > 0 and B > 0:
                        c[z, i, j, k - 1] = (n * int(s[z, i, j, 2 + k]) - S1 * T1) / (np.sqrt(float(A)) * np.sqrt(float(B)))
    return c


def _lower_median(v):
    v = sorted(v)
    return v[(len(v) - 1) // 2]


def spacing(s, skip=(), min_corr=0.1):
    """(positions, curve, used pairs [(z, k, d)], clipped, unresolved) by the rule of utils.section_spacing, written
    with loops and one dense least-squares solve over the good sections."""
    Z, gy, gx, L = s.shape[0], s.shape[1], s.shape[2], s.shape[3] - 3
    c = scores(s)
    good = [z for z in range(Z) if z not in set(skip)]
    ok = lambda z, k: z in good and z + k in good
    decided = [(i, j) for i in range(gy) for j in range(gx)
               if [z for z in range(Z - 1) if ok(z, 1)] and
               np.median([c[z, i, j, 0] for z in range(Z - 1) if ok(z, 1)]) > min_corr]
    cz = {(z, k): _lower_median([c[z, i, j, k - 1] for i, j in decided])
          for k in range(1, L + 1) for z in range(Z - k) if ok(z, k) and decided}
    curve = [1.0] + [float(np.median([v for (z, kk), v in cz.items() if kk == k])) if any(kk == k for _, kk in cz)
                     else float("nan") for k in range(1, L + 1)]
    if not all(b < a for a, b in zip(curve, curve[1:])):
        raise ValueError("the curve does not decrease")

    def inverse(v):
        v = min(v, 1.0)
        for k in range(L):
            if curve[k + 1] <= v <= curve[k]:
                return k + (curve[k] - v) / (curve[k] - curve[k + 1])
        raise AssertionError

    used = [(z, k, inverse(v)) for (z, k), v in sorted(cz.items()) if v > curve[L]]
    # groups of good sections joined by used pairs
    group = {z: z for z in good}
    for z, k, _ in used:
        a, b = group[z], group[z + k]
        if a != b:
            for g in good:
                if group[g] == max(a, b):
                    group[g] = min(a, b)
    p = {}
    for r in sorted(set(group.values())):
        members = [z for z in good if group[z] == r]
        col = {z: n for n, z in enumerate(members)}
        rows = [(z, k, d) for z, k, d in used if group[z] == r]
        M, y = np.zeros((len(rows) + 1, len(members))), np.zeros(len(rows) + 1)
        for n, (z, k, d) in enumerate(rows):
            w = np.sqrt(1.0 / k)
            M[n, col[z + k]], M[n, col[z]], y[n] = w, -w, w * d
        M[-1, 0] = 1e6                                                                 # p[first] = 0
        sol = np.linalg.lstsq(M, y, rcond=None)[0]
        for z in members:
            p[z] = sol[col[z]] - sol[0]
    unresolved = []
    for n, z in enumerate(good):
        if n and group[z] == z:
            before = good[n - 1]
            shift = p[before] + (z - before)
            for m in good:
                if group[m] == z:
                    p[m] += shift
            unresolved.append((before, z))
    clipped, q = [], {good[0]: 0.0}
    for a, b in zip(good, good[1:]):
        step = min(max(p[b] - p[a], (b - a) / 8), 8.0 * (b - a))
        if step != p[b] - p[a]:
            clipped.append((a, b))
        q[b] = q[a] + step
    P = np.interp(np.arange(Z), good, [q[z] for z in good])
    for z in range(good[0]):
        P[z] = q[good[0]] - (good[0] - z)
    for z in range(good[-1] + 1, Z):
        P[z] = q[good[-1]] + (z - good[-1])
    P = (P - P[0]) * ((Z - 1) / (P[-1] - P[0]))
    return P, np.array(curve), used, clipped, unresolved


def quantize(P):
    return np.rint(np.asarray(P, np.float64) * UNIT).astype(np.int64)


# ------------------------------------------------------------------------------------------------------- the fixture
FIX_SHAPE, FIX_TILE, FIX_LAGS, FIX_SKIP, FIX_GAP = (40, 64, 96), 32, 4, 27, 12
FINE, SIGMA_Z, SIGMA_XY = 8, 2.0, 1.5


def _smooth(a, axis, sigma):
    r = int(np.ceil(4 * sigma))
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    return np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), axis, a)


class Fixture:
    pass


@functools.lru_cache(maxsize=None)
def fixture(seed=5):
    """The fixture of the module's docstring: .volume uint8 [40, 64, 96], .truth uint8 (the even grid), .positions
    float64[40] planted, .skip [FIX_SKIP], .mask uint8 a label volume that moves with the sections.  Read-only."""
    rng = np.random.default_rng(seed)
    Z, Y, X = FIX_SHAPE
    gaps = rng.uniform(0.6, 1.5, Z - 1)
    gaps[FIX_GAP] = 2.6
    pos = np.concatenate([[0.0], np.cumsum(gaps)])
    pos *= (Z - 1) / pos[-1]
    pad = int(np.ceil(4 * SIGMA_Z)) * FINE
    a = rng.standard_normal(((Z - 1) * FINE + 1 + 2 * pad, Y, X))
    a = _smooth(a, 0, SIGMA_Z * FINE)
    a = _smooth(_smooth(a, 1, SIGMA_XY), 2, SIGMA_XY)
    a = a[pad:pad + (Z - 1) * FINE + 1]
    a = 128.0 + 40.0 * a / a.std()

    def sample(p):                                                                      # linear on the fine grid
        f = np.asarray(p) * FINE
        i = np.minimum(f.astype(np.int64), a.shape[0] - 2)
        t = (f - i)[:, None, None]
        return (1 - t) * a[i] + t * a[i + 1]

    fx = Fixture()
    fx.positions, fx.skip = pos, [FIX_SKIP]
    fx.volume = np.clip(np.rint(sample(pos)).astype(np.int64) + rng.integers(-2, 3, FIX_SHAPE), 0, 255).astype(np.uint8)
    fx.volume[FIX_SKIP] = 0
    fx.truth = np.clip(np.rint(sample(np.arange(Z, dtype=np.float64))), 0, 255).astype(np.uint8)
    fx.mask = np.broadcast_to((np.arange(Z) // 4 % 2 * 255).astype(np.uint8)[:, None, None], FIX_SHAPE).copy()
    for v in (fx.positions, fx.volume, fx.truth, fx.mask):
        v.setflags(write=False)
    return fx


@functools.lru_cache(maxsize=None)
def fixture_sums():
    s = volume_lag_sums(fixture().volume, (FIX_TILE, FIX_TILE), FIX_LAGS)
    s.setflags(write=False)
    return s


def rmse_sections(table, skip):
    """The output sections the RMSE is taken over: not skipped, and no tap of weight above 0 on a skipped section."""
    bad = set(skip)
    return [j for j, (z, w) in enumerate(np.asarray(table).tolist())
            if j not in bad and z not in bad and not (w > 0 and z + 1 in bad)]


def rmse(a, b, sections):
    d = a[sections].astype(np.float64) - b[sections].astype(np.float64)
    return float(np.sqrt((d * d).mean()))


def conditions(P, resampled, table):
    """(largest spacing error of good neighbours, that of even spacing, RMSE raw, RMSE resampled) for estimated
    positions `P` and the stack `resampled` through `table`."""
    fx = fixture()
    good = [z for z in range(FIX_SHAPE[0]) if z not in fx.skip]
    true = np.array([fx.positions[b] - fx.positions[a] for a, b in zip(good, good[1:])])
    est = np.array([P[b] - P[a] for a, b in zip(good, good[1:])])
    even = np.array([float(b - a) for a, b in zip(good, good[1:])])
    sec = rmse_sections(table, fx.skip)
    return (float(np.abs(est - true).max()), float(np.abs(even - true).max()), rmse(fx.volume, fx.truth, sec),
            rmse(resampled, fx.truth, sec))


def check_fixture(verbose=False):
    """The module docstring's conditions, from this file alone."""
    fx = fixture()
    s = fixture_sums()
    P, curve, used, clipped, unresolved = spacing(s, fx.skip)
    assert all(b < a for a, b in zip(curve, curve[1:]))
    c = scores(s)
    good1 = [z for z in range(FIX_SHAPE[0] - 1) if z not in fx.skip and z + 1 not in fx.skip]
    assert (np.median(c[good1, :, :, 0], axis=0) > 0.1).all()                           # every tile column is decided
    table = taps(quantize(P))
    got = resample(fx.volume, table)
    e_est, e_even, r_raw, r_res = conditions(P, got, table)
    if verbose:
        r_true = rmse(resample(fx.volume, taps(quantize(fx.positions))), fx.truth, rmse_sections(table, fx.skip))
        print("curve", curve.tolist(), "columns", c.shape[1] * c.shape[2])
        print("spacing error", e_est, "even", e_even)
        print("position error", float(np.abs(P - fx.positions).max()),
              "even", float(np.abs(np.arange(len(P)) - fx.positions).max()))
        print("rmse raw", r_raw, "resampled", r_res, "true positions", r_true, clipped, unresolved)
    assert e_even >= 1.0 and e_est <= 0.25, (e_est, e_even)
    assert r_res <= 0.5 * r_raw, (r_res, r_raw)
    assert clipped == [] and unresolved == []
    return P, curve, e_est, e_even, r_raw, r_res


if __name__ == "__main__":
    check_fixture(verbose=True)
