"""The 16-bit ingest restated in numpy and plain Python, independently of transfer_em_amd.utils: the voxel index, the
histogram (np.bincount), the table conversion (fancy indexing), the three host helpers (window16, window_lut16,
match_lut16: Python ints in loops, no searchsorted) and the seeded fixture stack with its four conversion routes."""
import numpy as np

BINS = 65536


def index(a):
    """u = v for uint16, v + 32768 for int16, as int64."""
    a = np.asarray(a)
    assert a.dtype in (np.uint16, np.int16)
    return a.astype(np.int64) + (32768 if a.dtype == np.int16 else 0)


def ref_hist(a):
    return np.bincount(index(a).ravel(), minlength=BINS).astype(np.int64)


def ref_hist_sections(a):
    return np.stack([ref_hist(s) for s in a])


def ref_convert(a, lut, zsec0=0):
    """lut[u], or lut[zsec0 + z][u] for a table per section; a is [z, y, x]."""
    u = index(a)
    if lut.ndim == 1:
        return lut[u]
    return np.stack([lut[zsec0 + z][u[z]] for z in range(a.shape[0])])


def _quantile(c, n, num, den):
    for u in range(BINS):
        if c[u] * den >= num * n:
            return u
    raise AssertionError("the last cumulative count is the total")


def ref_window(h, low, high):
    """(lo, hi) of one histogram row; low and high as (numerator, denominator) pairs."""
    c, a = [], 0
    for v in np.asarray(h).tolist():
        a += v
        c.append(a)
    if a == 0:
        return 0, BINS - 1
    lo, hi = _quantile(c, a, *low), _quantile(c, a, *high)
    if hi == lo:
        if lo == BINS - 1:
            lo -= 1
        else:
            hi += 1
    return lo, hi


def ref_window_lut(lo, hi, invert=False):
    t = []
    for u in range(BINS):
        v = 0 if u <= lo else 255 if u >= hi else (2 * 255 * (u - lo) + (hi - lo)) // (2 * (hi - lo))
        t.append(255 - v if invert else v)
    return np.array(t, np.uint8)


def ref_match(hs, hr):
    """One row: the smallest w with cr[w] ns >= cs[u] nr, in Python ints; an empty source row gives u >> 8."""
    cs, cr, a = [], [], 0
    for v in np.asarray(hs).tolist():
        a += v
        cs.append(a)
    a = 0
    for v in np.asarray(hr).tolist():
        a += v
        cr.append(a)
    ns, nr = cs[-1], cr[-1]
    assert nr > 0
    if ns == 0:
        return np.array([u >> 8 for u in range(BINS)], np.uint8)
    t, w = [], 0
    for u in range(BINS):
        while cr[w] * ns < cs[u] * nr:
            w += 1
        t.append(w)
    return np.array(t, np.uint8)


def ref_match8(hs, hr):
    """match_lut's rule on 256 source bins, restated for the 8-bit legs of the fixture's routes."""
    cs, cr = np.cumsum(hs).tolist(), np.cumsum(hr).tolist()
    t, w = [], 0
    for v in range(256):
        while cr[w] * cs[-1] < cs[v] * cr[-1]:
            w += 1
        t.append(w)
    return np.array(t, np.uint8)


# ---------------------------------------------------------------------------------------------------------- fixture
FIXTURE_SHAPE = (12, 96, 128)
LOW, HIGH = (1, 1000), (999, 1000)


def fixture_stack(seed=2024):
    """(G, raw): a smooth uint8 ground truth G[12][96][128] within [30, 220] and its 16-bit rendering
    raw = gain_z (200 G + 3000) + offset_z + N(0, 60), gains in [0.7, 1.3], offsets in +-1500, with four hot (65535) and
    four dead (0) pixels per section -- section-to-section flicker, detector noise and outliers on a 16-bit range."""
    rng = np.random.default_rng(seed)
    Z, Y, X = FIXTURE_SHAPE
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    g = np.zeros(FIXTURE_SHAPE)
    for _ in range(6):                                                   # a few low-frequency waves: smooth in z, y and x
        fz, fy, fx = rng.uniform(0.0, 0.15), rng.uniform(0.02, 0.09), rng.uniform(0.02, 0.09)
        g += rng.uniform(0.5, 1.0) * np.sin(fz * z + fy * y + fx * x * rng.choice([-1, 1]) + rng.uniform(0, 6.28))
    g = (g - g.min()) / (g.max() - g.min())
    G = np.rint(30 + 190 * g).astype(np.uint8)
    gain, offset = rng.uniform(0.7, 1.3, Z), rng.uniform(-1500, 1500, Z)
    raw = gain[:, None, None] * (200.0 * G + 3000.0) + offset[:, None, None] + rng.normal(0, 60, FIXTURE_SHAPE)
    raw = np.clip(np.rint(raw), 0, 65535).astype(np.uint16)
    for s in range(Z):
        at = rng.choice(Y * X, 8, replace=False)
        raw[s].reshape(-1)[at[:4]] = 65535
        raw[s].reshape(-1)[at[4:]] = 0
    return G, raw


def _hist8(a):
    return np.bincount(a.ravel(), minlength=256).astype(np.int64)


def route_match16_sections(raw, G):
    """Per-section 16-bit match straight to G's sections: the tables [Z, 65536] and the converted stack."""
    luts = np.stack([ref_match(ref_hist(raw[z]), _hist8(G[z])) for z in range(raw.shape[0])])
    return luts, ref_convert(raw, luts)


def fixture_routes(raw, G):
    """The four routes' results, best first: per-section 16-bit match; per-section window then per-section 8-bit
    match; global window then per-section 8-bit match; global window then global 8-bit match."""
    Z = raw.shape[0]
    out = [route_match16_sections(raw, G)[1]]
    per = np.stack([ref_window_lut(*ref_window(ref_hist(raw[z]), LOW, HIGH))[index(raw[z])] for z in range(Z)])
    glob = ref_window_lut(*ref_window(ref_hist(raw), LOW, HIGH))[index(raw)]
    for w in (per, glob):
        out.append(np.stack([ref_match8(_hist8(w[z]), _hist8(G[z]))[w[z]] for z in range(Z)]))
    out.append(ref_match8(_hist8(glob), _hist8(G))[glob])
    return out


def mae(a, G):
    return float(np.abs(a.astype(np.int64) - G.astype(np.int64)).mean())
