"""The numpy reference of the rescale (include/tem_hip.h: tem_u8_rescale), independent of transfer_em_amd.utils: per axis a
dense integer weight matrix M[j, i] built straight from the definition -- by brute force over every (output, source)
pair where the axis shrinks -- and its row sums W; the voxel is (2 S + Den) // (2 Den) in int64 with
S = M_z M_y M_x applied to the volume and Den = W_z W_y W_x.

A step is a (p, q) pair, the output voxel's edge in source voxels; `steps` are in (z, y, x) order, the volume's."""
import functools

import numpy as np


def grid(n, p, q):
    return -(-n * q // p)


def axis_matrix(n, p, q):
    """(M int64 [n_out, n], W int64 [n_out]) of an axis of n source voxels at step p / q."""
    M = np.zeros((grid(n, p, q), n), np.int64)
    for j in range(M.shape[0]):
        if p >= q:                                       # area: overlap of [j p, (j + 1) p) with [i q, (i + 1) q)
            for i in range(n):
                M[j, i] = max(0, min((i + 1) * q, (j + 1) * p) - max(i * q, j * p))
        else:                                            # linear between voxel centres, clamped
            C = (2 * j + 1) * p - q
            i0 = C // (2 * q)
            f = C - 2 * q * i0
            M[j, min(max(i0, 0), n - 1)] += 2 * q - f
            M[j, min(max(i0 + 1, 0), n - 1)] += f
    return M, M.sum(axis=1)


def sums(v, steps):
    """(S, Den), int64 arrays of the output grid's shape, of a uint8 volume [z, y, x] at `steps` ((pz, qz), (py, qy),
    (px, qx))."""
    (Mz, Wz), (My, Wy), (Mx, Wx) = (axis_matrix(n, p, q) for n, (p, q) in zip(v.shape, steps))
    S = np.einsum("az,zyx->ayx", Mz, v.astype(np.int64))
    S = np.einsum("by,ayx->abx", My, S)
    S = np.einsum("cx,abx->abc", Mx, S)
    return S, Wz[:, None, None] * Wy[None, :, None] * Wx[None, None, :]


def reference(v, steps):
    """The rescaled uint8 volume."""
    S, den = sums(v, steps)
    out = (2 * S + den) // (2 * den)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def reference2d(img, steps):
    """One image [y, x] at ((py, qy), (px, qx))."""
    return reference(img[None], ((1, 1),) + tuple(steps))[0]


@functools.lru_cache(maxsize=64)
def _used(n, p, q):
    M = axis_matrix(n, p, q)[0] > 0
    M.setflags(write=False)
    return M


def hull(lo, hi, n, p, q):
    """The (lo, hi) source voxels with a positive weight in outputs [lo, hi) of an axis."""
    used = np.flatnonzero(_used(n, p, q)[lo:hi].any(axis=0))
    return int(used[0]), int(used[-1]) + 1


def pool2(v):
    """tem_u8_pool2's formula at (2, 2, 2): (sum + (cnt >> 1)) >> log2(cnt) over the children that exist."""
    pad = [(0, n % 2) for n in v.shape]
    s = np.pad(v.astype(np.int64), pad)
    c = np.pad(np.ones(v.shape, np.int64), pad)
    fold = lambda a: a.reshape(a.shape[0] // 2, 2, a.shape[1] // 2, 2, a.shape[2] // 2, 2).sum(axis=(1, 3, 5))
    s, c = fold(s), fold(c)
    return ((s + (c >> 1)) >> np.log2(c).astype(np.int64)).astype(np.uint8)
