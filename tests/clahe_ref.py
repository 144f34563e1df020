"""The numpy reference of CLAHE that the tests compare against: tile histograms, tables and the interpolated remap,
written from the arithmetic alone (integers throughout) and independent of the product's host functions."""
import numpy as np


def ref_grid(Y, X, th, tw):
    return -(-Y // th), -(-X // tw)


def ref_tile_hist(vol, th, tw):
    """h[z, i, j, v]: the count of value v in vol[z, i*th:(i+1)*th, j*tw:(j+1)*tw]."""
    Z, Y, X = vol.shape
    gy, gx = ref_grid(Y, X, th, tw)
    h = np.zeros((Z, gy, gx, 256), np.int64)
    for z in range(Z):
        for i in range(gy):
            for j in range(gx):
                h[z, i, j] = np.bincount(vol[z, i * th:(i + 1) * th, j * tw:(j + 1) * tw].ravel(), minlength=256)
    return h


def ref_clipped(h, clip_limit):
    """One 256-bin histogram (Python ints) clipped at clip_limit and its excess spread; the total is kept."""
    h = [int(c) for c in h]
    n = sum(h)
    if clip_limit is None:
        return h
    clip = max(1, int(np.floor(np.float64(clip_limit) * np.float64(n) / np.float64(256))))
    excess = sum(max(c - clip, 0) for c in h)
    h = [min(c, clip) + excess // 256 for c in h]
    r = excess % 256
    for j in range(r):
        h[(j * 256) // r] += 1
    return h


def ref_tables(h, clip_limit, z_radius=0):
    h = np.asarray(h).astype(np.int64)
    Z = h.shape[0]
    if z_radius > 0:
        h = np.stack([h[max(z - z_radius, 0):min(z + z_radius + 1, Z)].sum(axis=0) for z in range(Z)])
    T = np.zeros(h.shape, np.uint8)
    for idx in np.ndindex(h.shape[:-1]):
        c = ref_clipped(h[idx], clip_limit)
        n = sum(c)
        assert n == int(h[idx].sum()) and n > 0
        cdf = 0
        for v in range(256):
            cdf += c[v]
            T[idx + (v,)] = (cdf * 255 + n // 2) // n
    return T


def ref_remap(block, T, th, tw, zsec0=0, y_org=0, x_org=0):
    """The remap of a block [D, H, W] whose voxel (d, y, x) sits at section zsec0 + d and in-plane volume coordinates
    (y_org + y, x_org + x), by tables T[Z, gy, gx, 256]."""
    D, H, W = block.shape
    gy, gx = T.shape[1:3]

    def axis(n, org, t, g):
        f = 2 * (org + np.arange(n, dtype=np.int64)) + 1 - t
        i0 = f // (2 * t)                                   # floor division: -1 in the first half tile
        w = f - i0 * 2 * t
        assert ((0 <= w) & (w < 2 * t)).all()
        return np.clip(i0, 0, g - 1), np.clip(i0 + 1, 0, g - 1), w
    i0, i1, wy = (a[None, :, None] for a in axis(H, y_org, th, gy))
    j0, j1, wx = (a[None, None, :] for a in axis(W, x_org, tw, gx))
    z = (zsec0 + np.arange(D))[:, None, None]
    v = block.astype(np.int64)
    a, b, c, d = (T[z, i, j, v].astype(np.int64) for i, j in ((i0, j0), (i0, j1), (i1, j0), (i1, j1)))
    Dn = 4 * th * tw
    num = (2 * th - wy) * ((2 * tw - wx) * a + wx * b) + wy * ((2 * tw - wx) * c + wx * d) + Dn // 2
    assert int(num.max(initial=0)) < 2 ** 32
    return (num // Dn).astype(np.uint8)


def ref_nearest(vol, T, th, tw):
    """The remap a kernel without interpolation would do: every voxel by its own tile's table."""
    Z, Y, X = vol.shape
    z, y, x = np.arange(Z)[:, None, None], np.arange(Y)[None, :, None], np.arange(X)[None, None, :]
    return T[z, y // th, x // tw, vol]


def ramp_volume(shape, seed):
    """Normal noise on an intensity ramp along y and x: neighbouring tiles get different tables."""
    Z, Y, X = shape
    rng = np.random.default_rng(seed)
    ramp = 60.0 * np.linspace(-1, 1, Y)[None, :, None] + 50.0 * np.linspace(-1, 1, X)[None, None, :]
    return np.clip(128 + ramp + rng.normal(0, 25, shape), 0, 255).astype(np.uint8)


def assert_input_condition(vol, T, th, tw):
    """The input condition of the end-to-end tests, asserted on the reference alone: all tile tables of a section are
    distinct, and the reference output differs from the nearest-tile lookup in more than half of every section's
    voxels -- a remap that ignores the interpolation cannot pass."""
    ref, near = ref_remap(vol, T, th, tw), ref_nearest(vol, T, th, tw)
    for z in range(vol.shape[0]):
        tabs = {T[z, i, j].tobytes() for i in range(T.shape[1]) for j in range(T.shape[2])}
        assert len(tabs) == T.shape[1] * T.shape[2], (z, len(tabs))
        assert (ref[z] != near[z]).mean() > 0.5, (z, (ref[z] != near[z]).mean())
    return ref
