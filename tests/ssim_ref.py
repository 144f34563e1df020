"""The numpy reference of the windowed SSIM (include/tem_hip.h: tem_u8_ssim), twice:

  * the contract, in integers: the five window sums by cumulative sums in int64, A1...B2, two float64 divisions, one
    multiplication, q = rint(x 2^30); the map byte and the per-section sums of q follow;
  * the textbook form, independent of it: means, sample variances and covariance in float64 over
    sliding_window_view, (2 ma mb + C1)(2 cov + C2) / ((ma^2 + mb^2 + C1)(va + vb + C2)).

Windows are wz x win x win voxels, wz = 1 if flat else win, wholly inside the block, named by their first voxel."""
import numpy as np

Q = 1 << 30
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2                            # 6.5025, 58.5225


def window(win, flat):
    return (1 if flat else win), win, win


def _box_sum(v, w):
    """Sums of `v` (int64 [z, y, x]) over all boxes of extents `w` that lie inside it, by cumulative sums."""
    for ax, n in enumerate(w):
        c = np.cumsum(v, axis=ax, dtype=np.int64)
        c = np.concatenate([np.zeros_like(np.take(c, [0], axis=ax)), c], axis=ax)
        hi = np.take(c, np.arange(n, c.shape[ax]), axis=ax)
        lo = np.take(c, np.arange(0, c.shape[ax] - n), axis=ax)
        v = hi - lo
    return v


def window_sums(a, b, win, flat):
    """Sa, Sb, Saa, Sbb, Sab as int64 arrays over the window box of two uint8 blocks [z, y, x] of one shape."""
    a, b = a.astype(np.int64), b.astype(np.int64)
    w = window(win, flat)
    return tuple(_box_sum(v, w) for v in (a, b, a * a, b * b, a * b))


def terms(a, b, win, flat):
    """A1, B1, A2, B2 (int64) per window."""
    Sa, Sb, Saa, Sbb, Sab = window_sums(a, b, win, flat)
    N = int(np.prod(window(win, flat)))
    A1 = 20000 * Sa * Sb + 65025 * N * N
    B1 = 10000 * (Sa * Sa + Sb * Sb) + 65025 * N * N
    A2 = 20000 * (N * Sab - Sa * Sb) + 585225 * N * (N - 1)
    B2 = 10000 * ((N * Saa - Sa * Sa) + (N * Sbb - Sb * Sb)) + 585225 * N * (N - 1)
    return A1, B1, A2, B2


def quantise(x):
    return np.rint(x * float(Q)).astype(np.int64)                       # np.rint: round half to even


def ssim_q(a, b, win, flat):
    """q_s, q_l, q_cs (int64 [Zw, Yw, Xw]) of two uint8 blocks."""
    A1, B1, A2, B2 = terms(a, b, win, flat)
    l = A1.astype(np.float64) / B1.astype(np.float64)
    cs = A2.astype(np.float64) / B2.astype(np.float64)
    return quantise(l * cs), quantise(l), quantise(cs)


def ssim_map(q_s):
    return ((255 * np.maximum(q_s, 0) + (1 << 29)) >> 30).astype(np.uint8)


def ssim_sums(qs):
    """int64 [Zw, 3]: the sums of q_s, q_l, q_cs per window-section."""
    return np.stack([q.sum(axis=(1, 2), dtype=np.int64) for q in qs], axis=1)


def reference(a, b, win, flat):
    """(sums int64 [Zw, 3], map uint8 [Zw, Yw, Xw]) of two uint8 blocks of one shape."""
    qs = ssim_q(a, b, win, flat)
    return ssim_sums(qs), ssim_map(qs[0])


def textbook(a, b, win, flat):
    """s, l, cs (float64 [Zw, Yw, Xw]) by the textbook formula, straight from the voxels."""
    w = window(win, flat)
    N = int(np.prod(w))
    va = np.lib.stride_tricks.sliding_window_view(a.astype(np.float64), w)
    vb = np.lib.stride_tricks.sliding_window_view(b.astype(np.float64), w)
    ax = (-3, -2, -1)
    ma, mb = va.mean(axis=ax), vb.mean(axis=ax)
    da, db = va - ma[..., None, None, None], vb - mb[..., None, None, None]
    var_a, var_b = (da * da).sum(axis=ax) / (N - 1), (db * db).sum(axis=ax) / (N - 1)
    cov = (da * db).sum(axis=ax) / (N - 1)
    l = (2 * ma * mb + C1) / (ma * ma + mb * mb + C1)
    cs = (2 * cov + C2) / (var_a + var_b + C2)
    return l * cs, l, cs


def checkerboard(shape):
    """A 0 / 255 checkerboard over (z, y, x) and its inverse: the window sums of largest magnitude."""
    z, y, x = np.indices(shape)
    a = (((z + y + x) & 1) * 255).astype(np.uint8)
    return a, (255 - a).astype(np.uint8)


def noisy(a, rng, amp=6):
    return np.clip(a.astype(np.int64) + rng.integers(-amp, amp + 1, a.shape), 0, 255).astype(np.uint8)
