"""Element-by-element check of bf16 stores: every stored value must be the round-to-nearest-even bf16 of the float64
reference, except where the reference lies within the fp32 accumulation error of a rounding tie; there one of the two
neighbouring bf16 values is accepted.  A plain helper module (no fixtures); test_bf16_exact.py holds it to simulated
correct and mutated kernels on the CPU, the GPU tests apply it next to their max-norm bars.

The kernels under test compute  acc = sum of K products of bf16 operands (exact in fp32), accumulated in fp32 in some
order;  then an fp32 epilogue (bias, skip-gradient add, LeakyReLU' gate, dropout x2, LeakyReLU);  then ONE store
rounded to nearest even.  With ref the same operation in float64 and S the same operation on magnitudes (|x|, |w|,
|bias|, |add|, the epilogue's positive factors applied as the reference applies them), the fp32 value before the
store is held to

    |v - ref| <= delta = (gamma(K) + roundings * 2^-24) * S,      lo = rne_bf16(ref - delta) <= stored <= hi = rne_bf16(ref + delta)

Derivation of the bar -- from the reference alone, no kernel output enters it:
  * gamma(K) = 4 * rho(K), where rho(K) is the error of the plain sequential float32 sum of K exact products against
    the float64 sum, relative to the sum of magnitudes, worst of 20,000 random rows of bf16-rounded standard normals
    (fixed seed).  Four times the float32 restatement's own error is the convention of test_gpu_glue.py.  An MFMA chain
    adds exact blocks of products with one rounding per block, i.e. fewer roundings than the sequential sum, so the
    sequential sum is the right yardstick and not a loose one.
  * roundings = 4 half-ulps of fp32 (2^-24 each, relative to S) for the epilogue's fp32 operations: the add, the gate
    multiply, the slope multiply, and the bias folded into the accumulator.  A larger number for one kernel must be
    derived from that kernel's code, never fitted to its output.
  * Condition on a case, not a measurement: at most 10 % of its elements may be undecided (lo != hi); an undecided
    element is still pinned to two adjacent bf16 values.  From the reference alone the share is 0.5 % (K = 27) to
    4.4 % (K = 2048).  A case over the cap has badly chosen inputs: change the inputs, never the cap.

Inputs of the tests are O(1); store_interval asserts that no interval reaches the bf16 subnormal range (where the
spacing stops shrinking and rne_bf16's frexp form would not describe the format).

Measured gamma(K) = 4 rho(K) on the CPU (seed 20240, 20,000 rows), for the K = k^dims * C_in the GPU cases use:

       K   gamma          K   gamma          K   gamma          K   gamma
       1   0.0e+00          9   3.4e-07         27   3.1e-07         32   2.9e-07
      72   4.8e-07        128   3.3e-07        144   4.6e-07        216   4.8e-07
     256   3.9e-07        288   3.8e-07        432   3.9e-07        512   5.4e-07
     864   5.5e-07       1024   6.5e-07       1296   5.8e-07       2048   8.5e-07

(rho is the largest of 20,000 samples, so the figures scatter by some 20 % around a slow growth with K; K = 1 has no
sum at all.  test_bf16_exact.py holds this table to the function.)
"""
import functools

import numpy as np

LEAKY = np.float32(0.3)          # oracle.ops.LEAKY_ALPHA: the float32 slope of the kernels' epilogues
ROWS, SEED = 20000, 20240
UNDECIDED_CAP = 0.10
BF16_MIN_NORMAL = 2.0 ** -126


def rne_bf16(v):
    """float64 -> the nearest bf16 value (8 significant bits), as float64, ties to even.  Rounds from float64 directly:
    a detour through float32 would round twice.  Valid for the normal range only (see store_interval)."""
    m, e = np.frexp(np.asarray(v, np.float64))              # |m| in [0.5, 1): 8 bits are m * 256 in [128, 256)
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)


def round_bf16_f32(a):
    """float32 array -> bf16-representable float32 (nearest even), by integer arithmetic on the bits."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32)
    b = (b + np.uint32(0x7fff) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return b.view(np.float32)


@functools.lru_cache(None)
def rho(K):
    """max |seq32 - sum64| / sum|t| over ROWS rows of K products of bf16-rounded standard normals."""
    rng = np.random.default_rng(SEED + K)
    worst, chunk = 0.0, max(1, min(ROWS, (1 << 22) // K))
    for lo in range(0, ROWS, chunk):
        n = min(chunk, ROWS - lo)
        x = round_bf16_f32(rng.standard_normal((n, K), dtype=np.float32))
        w = round_bf16_f32(rng.standard_normal((n, K), dtype=np.float32))
        t = x * w                                           # float32
        assert np.array_equal(t.astype(np.float64), x.astype(np.float64) * w.astype(np.float64)), "products must be exact"
        seq = np.cumsum(t, axis=1, dtype=np.float32)[:, -1]
        t64 = t.astype(np.float64)
        worst = max(worst, float((np.abs(seq.astype(np.float64) - t64.sum(1)) / np.abs(t64).sum(1)).max()))
    return worst


def gamma(K):
    """The fp32 accumulation margin for K products per output, relative to the sum of magnitudes: 4 * rho(K)."""
    return 4.0 * rho(int(K))


def margin(K, roundings=4):
    return gamma(K) + roundings * 2.0 ** -24


def store_interval(ref, S, K, roundings=4):
    """(lo, hi) of the bf16 values a correct kernel may store for the float64 result `ref` (after bias, add, gate,
    dropout and slope, with the float32 values of the slopes) and its magnitude twin `S`."""
    ref, S = np.asarray(ref, np.float64), np.asarray(S, np.float64)
    assert ref.shape == S.shape and (S >= 0).all()
    return interval(ref, margin(K, roundings) * S)


def interval(ref, delta):
    """(lo, hi) = rne_bf16(ref -+ delta), element by element; +-0 where ref is exactly 0."""
    ref, delta = np.asarray(ref, np.float64), np.asarray(delta, np.float64)
    a, b = ref - delta, ref + delta
    ends = np.abs(np.concatenate([a.reshape(-1), b.reshape(-1)]))
    assert not ((ends > 0) & (ends < BF16_MIN_NORMAL)).any(), "a reference interval reaches the bf16 subnormal range"
    lo, hi = rne_bf16(a), rne_bf16(b)
    zero = ref == 0                                          # e.g. a dropped voxel: nothing but +-0 is right
    return np.where(zero, 0.0, lo), np.where(zero, 0.0, hi)


def check_bf16_stores(got, ref, S, K, name, roundings=4, quiet=False):
    """Compare without asserting -> dict(fails, total, undecided, first, gamma, K).  NaN in `got` fails."""
    lo, hi = store_interval(ref, S, K, roundings)
    return check_bounds(got, ref, lo, hi, f"{name}: K {K} gamma {gamma(K):.2e}", quiet, gamma=gamma(K), K=K)


def check_bounds(got, ref, lo, hi, name, quiet=False, **figures):
    """lo <= got <= hi element by element -> dict(fails, total, undecided, first, **figures), printed with `name`."""
    got = np.asarray(got, np.float64)
    assert got.shape == lo.shape, (name, got.shape, lo.shape)
    bad = ~((lo <= got) & (got <= hi))
    fails = int(np.count_nonzero(bad))
    undecided = float(np.count_nonzero(lo != hi)) / max(1, got.size)
    ref = np.asarray(ref, np.float64)
    first = [(tuple(int(i) for i in ix), float(got[tuple(ix)]), float(ref[tuple(ix)]), float(lo[tuple(ix)]), float(hi[tuple(ix)]))
             for ix in np.argwhere(bad)[:5]]
    if not quiet:
        print(f"bf16 stores {name}: {fails} of {got.size} fail, undecided {100 * undecided:.2f} %"
              + ("".join(f"\n    {ix}: got {g!r} ref {r!r} lo {l!r} hi {h!r}" for ix, g, r, l, h in first)))
    return dict(fails=fails, total=int(got.size), undecided=undecided, first=first, **figures)


def assert_bf16_stores(got, ref, S, K, name, roundings=4):
    """`got`: the kernel's bf16 output widened to float32.  Every element within [lo, hi]; no element is exempt and no
    share may fail.  Prints and returns the figures of check_bf16_stores."""
    r = check_bf16_stores(got, ref, S, K, name, roundings)
    assert r["undecided"] <= UNDECIDED_CAP, (name, "badly chosen input: undecided share", r["undecided"])
    assert r["fails"] == 0, (name, f"{r['fails']} of {r['total']} stored bf16 values outside the rounded reference", r["first"])
    return r


def epilogue64(pre, mag, K, saved=None, gate_slope=LEAKY, keep=None, slope=1.0, roundings=4):
    """The kernels' epilogue after bias and add, in float64 on the pair (reference, magnitudes), in their order:
    LeakyReLU' gate on the sign of `saved`, dropout (x2 where kept, 0 where dropped), LeakyReLU.  The positive factors go
    onto the magnitudes as the reference applies them; the LeakyReLU slope only where the reference is negative and
    its interval does not straddle 0 (next to 0 a kernel may be on the other branch, and the unscaled margin covers
    both).  -> (ref, S) for store_interval."""
    ref, S = np.array(pre, np.float64), np.array(mag, np.float64)
    if saved is not None:
        f = np.where(np.asarray(saved) > 0, 1.0, float(np.float32(gate_slope)))
        ref, S = ref * f, S * f
    if keep is not None:
        f = np.where(np.asarray(keep) > 0, 2.0, 0.0)
        ref, S = ref * f, S * f
    if slope != 1.0:
        a = float(np.float32(slope))
        neg = ref + margin(K, roundings) * S < 0
        ref = np.where(ref > 0, ref, a * ref)
        S = np.where(neg, a * S, S)
    return ref, S
