"""The numpy references of the in-plane measurement, independent of transfer_em_amd.utils: the sums of
include/tem_hip.h's tem_u8_zplane_lags as loops over planes and tiles with slicing (plane_tile_sums) and without the
loops over tiles (plane_tile_sums_fast), the counts by counting, and the scores, the sharpness, find_blurred's verdict,
the in-plane curve, the pitch and its step in Python numbers, one tile at a time.  Also the seeded fixture with planted
blur and a planted pitch that the tests share.

The fixture (fixture()): Gaussian noise on a grid of 47 x 128 x 192 -- twice as fine along z as the stack, padded by
4 sigma at both ends of z -- smoothed separably with sigma 1.5 on all three axes, every second plane kept: FIX_SHAPE =
24 x 128 x 192, and the planted pitch is 2.0 pixels per section.  Scaled to 128 + 40 sigma.  Sections FIX_SECTIONS =
(7, 15) and tile FIX_TILES = ((19, 1, 2),) of section 19 (tiles of FIX_TILE = 64 pixels) are then blurred in plane by a
Gaussian of sigma 2 with reflect padding -- the tile is cut out of its blurred section --, integer noise in [-6, 6] is
added, and the result is clipped to uint8.  The conditions, computed by check_fixture() from this file and zspace_ref
alone on tiles of 64 and 8 in-plane lags (values recorded from it):
  the verdict                                       sections [7, 15], tile (19, 1, 2), nothing else; 6 of 6 columns decided
  g relative to its column's median                 planted at most 0.5799, clean at least 0.8611 (ratio 0.65; margin 0.2812)
  find_defects' relative score of the planted tiles at least 0.8229 (it flags below 0.5: it sees none of them)
  the in-plane curve                                1, 0.8856, 0.629, 0.352, 0.1508, 0.0486, 0.0043, -0.0082 (K = 7)
  the curve along z (3 lags)                        1, 0.6277, 0.1654, 0.0102
  the pitch                                         1.9637 pixels (planted 2.0: 1.8 % off; bar 5 %), per lag 2.0048,
                                                    1.9637, 1.9557; the step 28 / 55"""
import functools
from fractions import Fraction

import numpy as np

import zspace_ref as ZS


# -------------------------------------------------------------------------------------------------------------- sums
def plane_tile_sums(block, c0, c1, r0, r1, y_org, Y, th, tw, gy, gx, nlag):
    """np.int64[c1 - c0, gy, gx, 3 + 2 nlag] of the core planes [c0, c1) and core rows [r0, r1) of a block of whole
    rows whose row 0 is row y_org of a section of Y rows: (sum v, sum v v, count, the y lags, the x lags)."""
    block = np.asarray(block)
    D, H, W = block.shape
    out = np.zeros((c1 - c0, gy, gx, 3 + 2 * nlag), np.int64)
    for d in range(c0, c1):
        for i in range(gy):
            ya, yb = max(i * th - y_org, r0), min((i + 1) * th - y_org, r1)
            if ya >= yb:
                continue
            for j in range(gx):
                xa, xb = j * tw, min((j + 1) * tw, W)
                if xa >= xb:
                    continue
                v = block[d, ya:yb, xa:xb].astype(np.int64)
                row = [int(v.sum()), int((v * v).sum()), v.size] + [0] * (2 * nlag)
                for k in range(1, nlag + 1):
                    ye = min(yb, Y - y_org - k)                        # rows whose partner k down is in the section
                    if ye > ya:
                        e = block[d, ya:ye, xa:xb].astype(np.int64) - block[d, ya + k:ye + k, xa:xb]
                        row[2 + k] = int((e * e).sum())
                    xe = min(xb, W - k)                                 # columns whose partner k right is in the section
                    if xe > xa:
                        e = block[d, ya:yb, xa:xe].astype(np.int64) - block[d, ya:yb, xa + k:xe + k]
                        row[2 + nlag + k] = int((e * e).sum())
                out[d - c0, i, j] = row
    return out


def plane_tile_sums_fast(block, c0, c1, r0, r1, y_org, Y, th, tw, gy, gx, nlag):
    """plane_tile_sums without the loops over tiles, for grids of many small tiles: the per-voxel terms by shifted
    slices, summed between the tile boundaries with np.add.reduceat.  test_zplane_plan.py holds it to the loops."""
    v = np.asarray(block).astype(np.int64)
    D, H, W = v.shape
    out = np.zeros((c1 - c0, gy, gx, 3 + 2 * nlag), np.int64)
    if c1 == c0 or r1 == r0:
        return out
    terms = [v, v * v, np.ones_like(v)]
    for k in range(1, nlag + 1):                                        # y: the partner row must be in the section
        t = np.zeros_like(v)
        n = min(H, Y - y_org) - k
        if n > 0:
            t[:, :n] = (v[:, :n] - v[:, k:k + n]) ** 2
        terms.append(t)
    for k in range(1, nlag + 1):
        t = np.zeros_like(v)
        if W > k:
            t[:, :, :W - k] = (v[:, :, :W - k] - v[:, :, k:]) ** 2
        terms.append(t)
    q = np.stack(terms, axis=-1)[c0:c1, r0:r1]                          # [core planes, core rows, W, 3 + 2 nlag]
    ti, tj = (y_org + np.arange(r0, r1)) // th, np.arange(W) // tw
    ys, xs = np.concatenate([[0], np.flatnonzero(np.diff(ti)) + 1]), np.concatenate([[0], np.flatnonzero(np.diff(tj)) + 1])
    q = np.add.reduceat(np.add.reduceat(q, ys, axis=1), xs, axis=2)
    out[:, ti[0]:ti[-1] + 1, tj[0]:tj[-1] + 1] = q
    return out


def volume_plane_sums(vol, tile, nlag):
    th, tw = tile
    Z, Y, X = vol.shape
    return plane_tile_sums_fast(vol, 0, Z, 0, Y, 0, Y, th, tw, -(-Y // th), -(-X // tw), nlag)


def counts(vol_shape, tile, nlag):
    """int64[gy, gx, 2, nlag] by counting the voxels that have a partner, one tile and lag at a time."""
    Y, X = vol_shape[-2:]
    th, tw = tile
    gy, gx = -(-Y // th), -(-X // tw)
    yy, xx = np.meshgrid(np.arange(Y), np.arange(X), indexing="ij")
    n = np.zeros((gy, gx, 2, nlag), np.int64)
    for i in range(gy):
        for j in range(gx):
            mine = (yy // th == i) & (xx // tw == j)
            for k in range(1, nlag + 1):
                n[i, j, 0, k - 1] = int((mine & (yy + k < Y)).sum())
                n[i, j, 1, k - 1] = int((mine & (xx + k < X)).sum())
    return n


# ------------------------------------------------------------------------------------------------------ the estimators
def scores(s, n):
    """float64[Z, gy, gx, 2, L], tile by tile in Python numbers, in the operation order that utils.plane_scores
    documents."""
    Z, gy, gx = s.shape[:3]
    L = (s.shape[3] - 3) // 2
    r = np.zeros((Z, gy, gx, 2, L))
    for z in range(Z):
        for i in range(gy):
            for j in range(gx):
                S1, S2, N = (int(v) for v in s[z, i, j, :3])
                A = N * S2 - S1 * S1
                for a in range(2):
                    for k in range(L):
                        nk, D = int(n[i, j, a, k]), int(s[z, i, j, 3 + a * L + k])
                        if A > 0 and nk > 0:
                            r[z, i, j, a, k] = 1.0 - (float(D) * float(N * N)) / ((2.0 * float(nk)) * float(A))
    return r


def mean_scores(s, n):
    r = scores(s, n)
    return (r[..., 0, :] + r[..., 1, :]) * 0.5


def sharpness(s, n):
    m = mean_scores(s, n)
    g = np.zeros(m.shape[:3])
    for idx in np.ndindex(*g.shape):
        r1, r2 = float(m[idx][0]), float(m[idx][1])
        g[idx] = 1.0 - r2 / r1 if r1 > 0 else 0.0
    return g


def blurred(s, n, ratio=0.65, min_corr=0.1, section_fraction=0.5):
    """(sections, tiles, undecided, g) by utils.find_blurred's rule, one column of tiles at a time."""
    m, g = mean_scores(s, n), sharpness(s, n)
    Z, gy, gx = g.shape
    undecided, bad = np.ones((gy, gx), bool), np.zeros((Z, gy, gx), bool)
    for i in range(gy):
        for j in range(gx):
            if Z < 2:
                continue
            med = float(np.median(g[:, i, j]))
            undecided[i, j] = float(np.median(m[:, i, j, 0])) <= min_corr or not med > 0
            if not undecided[i, j]:
                bad[:, i, j] = [float(g[z, i, j]) < ratio * med for z in range(Z)]
    decided = int((~undecided).sum())
    sections = [z for z in range(Z) if bad[z].sum() > 0 and bad[z].sum() >= section_fraction * decided]
    tiles = bad.copy()
    for z in sections:
        tiles[z] = False
    return sections, tiles, undecided, g


def curve(s, n, skip=(), min_corr=0.1):
    m = mean_scores(s, n)
    Z, gy, gx, L = m.shape
    good = [z for z in range(Z) if z not in set(skip)]
    decided = [(i, j) for i in range(gy) for j in range(gx)
               if good and float(np.median([m[z, i, j, 0] for z in good])) > min_corr]
    out = [1.0]
    for k in range(L):
        if not decided:
            break
        per_section = [sorted(float(m[z, i, j, k]) for i, j in decided)[(len(decided) - 1) // 2] for z in good]
        v = float(np.median(per_section))
        if not v < out[-1]:
            break
        out.append(v)
    if len(out) < 2:
        raise ValueError("the curve does not decrease")
    return np.array(out)


def pitch(z_curve, p_curve):
    """(pixels, [(k, estimate)]) by utils.z_pitch's rule, with the inverse written out."""
    zc, pc = [float(v) for v in z_curve], [float(v) for v in p_curve]
    K = len(pc) - 1
    per = []
    for k in range(1, len(zc)):
        if pc[K] < zc[k] < 1.0:
            for a in range(K):
                if pc[a + 1] <= zc[k] <= pc[a]:
                    per.append((k, (a + (pc[a] - zc[k]) / (pc[a] - pc[a + 1])) / k))
                    break
    if not per:
        raise ValueError("no lag within reach")
    return float(np.median([v for _, v in per])), per


def step(pixels):
    """The z step p / q, p, q <= 64, nearest to 1 / pixels over ALL pairs; the smallest q on a tie."""
    x = 1 / Fraction(float(pixels))
    if not Fraction(1, 8) <= x <= 8:
        raise ValueError("out of range")
    best = min((abs(Fraction(p, q) - x), q, p) for q in range(1, 65) for p in range(1, 65)
               if Fraction(1, 8) <= Fraction(p, q) <= 8)
    return Fraction(best[2], best[1])


# ------------------------------------------------------------------------------------------------------- the fixture
FIX_SHAPE, FIX_TILE, FIX_LAGS, FIX_ZLAGS = (24, 128, 192), 64, 8, 3
FIX_SECTIONS, FIX_TILES = (7, 15), ((19, 1, 2),)
FIX_PITCH, SIGMA, SIGMA_BLUR, NOISE = 2.0, 1.5, 2.0, 6


def _kernel(sigma):
    r = int(np.ceil(4 * sigma))
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    return k / k.sum(), r


def _smooth(a, axis, sigma, mode):
    """A separable Gaussian along `axis` by shifted adds; the ends are padded by `mode` ("reflect"), or not at all
    ("valid": the result is 2 r shorter)."""
    k, r = _kernel(sigma)
    a = np.moveaxis(a, axis, 0)
    if mode != "valid":
        a = np.pad(a, [(r, r)] + [(0, 0)] * (a.ndim - 1), mode=mode)
    n = a.shape[0] - 2 * r
    out = np.zeros((n,) + a.shape[1:])
    for t in range(2 * r + 1):
        out += k[t] * a[t:t + n]
    return np.moveaxis(out, 0, axis)


def blur_section(img):
    return _smooth(_smooth(np.asarray(img, np.float64), 0, SIGMA_BLUR, "reflect"), 1, SIGMA_BLUR, "reflect")


class Fixture:
    pass


@functools.lru_cache(maxsize=None)
def fixture(seed=11):
    """The fixture of the module's docstring: .volume uint8 FIX_SHAPE, .sections and .tiles what was planted,
    .planted bool[Z, gy, gx].  Read-only."""
    rng = np.random.default_rng(seed)
    Z, Y, X = FIX_SHAPE
    r = _kernel(SIGMA)[1]
    a = rng.standard_normal((2 * Z - 1 + 2 * r, Y, X))
    a = _smooth(a, 0, SIGMA, "valid")
    a = _smooth(_smooth(a, 1, SIGMA, "reflect"), 2, SIGMA, "reflect")[::2]
    a = 128.0 + 40.0 * a / a.std()
    fx = Fixture()
    fx.sections, fx.tiles = list(FIX_SECTIONS), list(FIX_TILES)
    fx.planted = np.zeros((Z, Y // FIX_TILE, X // FIX_TILE), bool)
    for z in FIX_SECTIONS:
        a[z] = blur_section(a[z])
        fx.planted[z] = True
    for z, i, j in FIX_TILES:
        ys, xs = slice(i * FIX_TILE, (i + 1) * FIX_TILE), slice(j * FIX_TILE, (j + 1) * FIX_TILE)
        a[z, ys, xs] = blur_section(a[z])[ys, xs]
        fx.planted[z, i, j] = True
    fx.volume = np.clip(np.rint(a).astype(np.int64) + rng.integers(-NOISE, NOISE + 1, FIX_SHAPE), 0, 255).astype(np.uint8)
    fx.volume.setflags(write=False)
    fx.planted.setflags(write=False)
    return fx


@functools.lru_cache(maxsize=None)
def fixture_sums():
    s = volume_plane_sums(fixture().volume, (FIX_TILE, FIX_TILE), FIX_LAGS)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def fixture_counts():
    n = counts(FIX_SHAPE, (FIX_TILE, FIX_TILE), FIX_LAGS)
    n.setflags(write=False)
    return n


@functools.lru_cache(maxsize=None)
def fixture_zcurve():
    """The correlation at 0...FIX_ZLAGS sections, from zspace_ref's lag sums and estimator with the planted sections
    skipped."""
    s = ZS.volume_lag_sums(fixture().volume, (FIX_TILE, FIX_TILE), FIX_ZLAGS)
    c = ZS.spacing(s, skip=FIX_SECTIONS)[1]
    c.setflags(write=False)
    return c


def relative_g(g, undecided):
    """g over its column's median, NaN in undecided columns."""
    med = np.median(g, axis=0)
    return np.where(undecided[None], np.nan, g / np.where(undecided, 1.0, med)[None])


def zcorr_relative(vol, tile):
    """find_defects' score of every tile relative to its column's median correlation, from zspace_ref's sums: the
    larger of the correlations with the section below and above, over np.median of the column's correlations."""
    c = ZS.scores(ZS.volume_lag_sums(vol, tile, 1))[:-1, :, :, 0]      # [Z - 1, gy, gx]
    t = np.concatenate([c[:1], np.maximum(c[:-1], c[1:]), c[-1:]])
    return t / np.median(c, axis=0)[None]


def check_fixture(verbose=False):
    """The module docstring's conditions, from this file and zspace_ref alone.  Returns (largest planted relative g,
    smallest clean relative g, smallest relative z correlation of a planted tile, pitch, per-lag pitches, curve)."""
    fx, s, n = fixture(), fixture_sums(), fixture_counts()
    sections, tiles, undecided, g = blurred(s, n)
    rel = relative_g(g, undecided)
    planted_max, clean_min = float(rel[fx.planted].max()), float(rel[~fx.planted].min())
    zrel = float(zcorr_relative(fx.volume, (FIX_TILE, FIX_TILE))[fx.planted].min())
    pc = curve(s, n, skip=sections)
    px, per = pitch(fixture_zcurve(), pc)
    if verbose:
        print("sections", sections, "tiles", np.argwhere(tiles).tolist(), "undecided", int(undecided.sum()))
        print("relative g: planted max", planted_max, "clean min", clean_min, "margin", clean_min - planted_max)
        print("z correlation of planted tiles, relative, min", zrel)
        print("plane curve", [round(float(v), 4) for v in pc], "z curve", [round(float(v), 4) for v in fixture_zcurve()])
        print("pitch", px, "per lag", per, "step", step(px))
    assert sections == list(FIX_SECTIONS) and np.argwhere(tiles).tolist() == [list(t) for t in FIX_TILES]
    assert not undecided.any()
    assert planted_max <= 0.65 <= clean_min
    assert zrel >= 0.5                                                  # find_defects flags below 0.5: it sees none
    assert abs(px - FIX_PITCH) <= 0.05 * FIX_PITCH
    return planted_max, clean_min, zrel, px, per, pc


if __name__ == "__main__":
    check_fixture(verbose=True)
