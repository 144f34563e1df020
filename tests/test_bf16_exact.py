"""The bf16 store check (bf16_exact.py) is itself checked, on the CPU: simulated correct kernels pass with zero
failures, every listed mutation of a kernel fails on more than 10 % of the elements, and the undecided share stays
under the cap -- for each K = k^dims * C_in the GPU cases use.  No HIP code is involved: all figures come from the
float64 reference and float32 NumPy restatements of the kernels' arithmetic.

The simulated launch is  v = sum_K x w + add;  v = saved > 0 ? v : 0.3f v  (gate);  out = v > 0 ? v : 0.3f v;  one store
rounded to nearest even -- the operand recipe of test_gpu_bf16.py (bf16-rounded standard normals, kernels x 0.2)."""
import numpy as np
import pytest
import torch

import bf16_exact as B

# (K, C_in): 3-D k3 (27 C), k4 (64 C), the 32 + 16 concat, 1x1x1; 2-D k3 (9 C), k4 (16 C)
KS = [(27, 1), (216, 8), (432, 16), (864, 32), (1296, 48), (512, 8), (1024, 16), (2048, 32), (32, 32),
      (9, 1), (72, 8), (144, 16), (288, 32), (128, 8), (256, 16)]
NOUT = 4000
f32 = np.float32


def rb(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def trunc_bf16(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def seq32(t):
    return np.cumsum(t, axis=1, dtype=np.float32)[:, -1]


def blocked32(t, block, round_blocks=lambda a: a):
    """Exact block sums (float64, one rounding to float32 each: what a matrix-core step does), then an fp32 chain."""
    n, K = t.shape
    pad = (-K) % block
    t64 = np.pad(t.astype(np.float64), ((0, 0), (0, pad)))
    acc = np.zeros(n, np.float32)
    for b in t64.reshape(n, -1, block).sum(2).T:
        acc = round_blocks((acc + b.astype(np.float32)).astype(np.float32))
    return acc


@pytest.fixture(scope="module", params=KS, ids=[f"K{k}" for k, _ in KS])
def sim(request):
    K, ci = request.param
    rng = np.random.default_rng(K)
    x = rb(rng.standard_normal((NOUT, K)))
    w = rb(rng.standard_normal((NOUT, K)) * 0.2)
    t = x * w
    assert np.array_equal(t.astype(np.float64), x.astype(np.float64) * w.astype(np.float64))
    add = rb(rng.standard_normal(NOUT) * 0.2 * np.sqrt(K))
    saved = rng.standard_normal(NOUT).astype(np.float32)
    pre = t.astype(np.float64).sum(1) + add
    mag = np.abs(t.astype(np.float64)).sum(1) + np.abs(add)
    ref, S = B.epilogue64(pre, mag, K, saved=saved, slope=0.3)
    return dict(K=K, ci=ci, t=t, add=add, saved=saved, ref=ref, S=S)


def finish(d, acc, slope=B.LEAKY, add_after_gate=False):
    """The fp32 epilogue of the simulated kernel on the accumulator `acc` -> float32 before the store."""
    acc = np.asarray(acc, np.float32)
    if add_after_gate:
        v = np.where(d["saved"] > 0, acc, slope * acc).astype(np.float32) + d["add"]
    else:
        v = acc + d["add"]
        v = np.where(d["saved"] > 0, v, slope * v).astype(np.float32)
    return np.where(v > 0, v, slope * v).astype(np.float32)


def fails(d, stored, name):
    r = B.check_bf16_stores(stored, d["ref"], d["S"], d["K"], f"{name} K={d['K']}")
    return r["fails"] / r["total"]


def test_correct_kernels_pass_and_share_is_capped(sim):
    d = sim
    r = B.assert_bf16_stores(rb(finish(d, seq32(d["t"]))), d["ref"], d["S"], d["K"], f"sequential K={d['K']}")
    assert r["fails"] == 0 and r["undecided"] <= B.UNDECIDED_CAP
    for block in (32, d["ci"]):
        B.assert_bf16_stores(rb(finish(d, blocked32(d["t"], block))), d["ref"], d["S"], d["K"], f"blocks of {block} K={d['K']}")


def test_mutations_are_rejected(sim):
    d = sim
    t, K = d["t"], d["K"]
    good = seq32(t)
    share = {"truncating store": fails(d, trunc_bf16(finish(d, good)), "truncating store")}
    if K > 64:      # (up to two blocks of 32 the mutation rounds once or twice: K <= 32 is the correct kernel itself)
        share["bf16 accumulation"] = fails(d, rb(finish(d, blocked32(t, 32, rb))), "bf16 accumulation per block")
    half = rb(seq32(t[:, :K // 2])) + seq32(t[:, K // 2:])
    share["bf16 partial sum"] = fails(d, rb(finish(d, half)), "half of K rounded to bf16")
    share["dropped tap"] = fails(d, rb(finish(d, seq32(t[:, 1:]))), "one tap dropped")
    share["bf16 slope"] = fails(d, rb(finish(d, good, slope=f32(rb(np.array([0.3]))[0]))), "slope bf16(0.3)")
    share["add after gate"] = fails(d, rb(finish(d, good, add_after_gate=True)), "add after the gate")
    print(f"K={K}: failing share per mutation", {k: round(v, 3) for k, v in share.items()})
    for what, s in share.items():
        assert s > 0.10, (K, what, s)


def test_gamma_matches_the_documented_table():
    """gamma(K) is 4 x the sequential float32 sum's own error: 3e-7 .. 7e-7 over the K of the GPU cases, growing slowly."""
    assert B.gamma(1) == 0.0 and f"{1:>5d}   {0.0:.1e}" in B.__doc__       # the 1 -> 32 1x1x1 layer: one product, no sum
    for K, _ in KS:
        g = B.gamma(K)
        print(f"gamma({K}) = {g:.2e}")
        assert 2e-7 < g < 1e-6, (K, g)
        assert f"{K:>5d}   {g:.1e}" in B.__doc__, (K, g, "the module's table is out of date")


def test_rne_bf16_equals_the_cast_on_float32_and_rounds_float64_once():
    rng = np.random.default_rng(1)
    a = (rng.standard_normal(200000) * np.exp(rng.uniform(-20, 20, 200000))).astype(np.float32)
    ties = []
    for e in (-3, 0, 1, 7):
        for m in (128, 129, 130, 255):                     # m + 1/2 at 8 bits: odd m rounds up, even m rounds down
            ties += [np.ldexp(m + 0.5, e - 7), -np.ldexp(m + 0.5, e - 7)]
    a = np.concatenate([a, np.array(ties, np.float32), np.array([0.0, -0.0, 1.0, -1.0, 0.3], np.float32)])
    want = torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()
    got = B.rne_bf16(a.astype(np.float64))
    assert np.array_equal(got.astype(np.float32).view(np.uint32), want.view(np.uint32))          # sign of -0 too
    assert np.array_equal(B.round_bf16_f32(a).view(np.uint32), want.view(np.uint32))
    up, down = np.float32(np.ldexp(129.5, -7)), np.float32(np.ldexp(128.5, -7))
    assert B.rne_bf16(float(up)) == np.ldexp(130.0, -7) and B.rne_bf16(float(down)) == np.ldexp(128.0, -7)
    # just above a tie by less than half a float32 ulp: float32 rounds it onto the tie, whose even neighbour is below
    v = np.ldexp(128.5, -7) * (1 + 2.0 ** -30)
    assert np.float32(v) == down
    assert B.rne_bf16(v) == np.ldexp(129.0, -7)
    assert float(torch.tensor([v], dtype=torch.float64).float().to(torch.bfloat16).float()[0]) == np.ldexp(128.0, -7)


def test_zero_reference_and_nan():
    ref = np.array([0.0, 0.0, 0.0, 1.0, 1.0])
    S = np.array([0.0, 0.0, 1.0, 1.0, 1.0])
    got = np.array([0.0, -0.0, 2.0 ** -100, np.nan, 1.0])
    r = B.check_bf16_stores(got, ref, S, 27, "zeros and NaN")
    assert r["fails"] == 2 and [f[0] for f in r["first"]] == [(2,), (3,)]
    with pytest.raises(AssertionError, match="subnormal"):
        B.store_interval(np.array([1e-39]), np.array([1e-39]), 27)


def test_rows_on_the_max_norm_bar_share_their_kernel_with_an_exact_case():
    """fullsize_cases.check_conv leaves the bf16 rows with more than 2^22 output elements on the max-norm bar.  Every
    kernel symbol among them also runs in a table row that gets the element-by-element check or in a case of
    test_gpu_bf16_2d.py (whose launches are built here on uninitialised host tensors, for their symbols)."""
    import fullsize_cases as F
    import test_gpu_bf16_2d as D2
    import test_gpu_bf16_fullsize_oracle as A
    import test_gpu_2d_fullsize_oracle as A2
    import test_gpu_step260 as S260
    from transfer_em_amd import hip_ops as H
    exact, left = set(), []
    for table, rows, n, is3d in (("132^3", A.CONV, A.N, True), ("132^2 x 64", A2.CONV_BF16, A2.N, False),
                                 ("260^3 thin", S260.CONV_BF16, S260.N, True)):
        for c in rows:
            if F.exact_checked(c, n, is3d):
                exact.add(c["kernel"])
            else:
                assert c.get("depth") is None
                left.append((table, c["name"], c["m"], c["kernel"]))
    e = lambda *shape: torch.empty(shape, dtype=torch.bfloat16)
    for CI, CO, k, s, pad, h, w in D2.FWD2:
        oh, ow = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
        exact.add(D2.fwd2_launch(H, e(2, 1, h, w, CI), e(k * k * CI * CO), e(2, 1, oh, ow, CO), k, s, pad,
                                 torch.empty(CO) if CO == 1 else None).meta["kernel"])
    for CI, CO in D2.CONVT2:
        for h, w, pad, lo, osz in D2.CONVT2_WINDOWS:
            exact.add(D2.convT2_launch(H, e(2, 1, h, w, CI), e(16 * CI * CO), e(2, 1, osz, osz, CO), pad + lo,
                                       e(2, 1, osz, osz, CO), e(2, 1, osz - 2, osz - 2, CO)).meta["kernel"])
    print(f"{len(left)} full-size bf16 rows stay on the max-norm bar:")
    for row in left:
        print("   ", *row)
    assert left
    missing = sorted({row[3] for row in left} - exact)
    assert not missing, missing
