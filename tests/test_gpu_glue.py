"""The non-convolution kernels of the step against float64 / integer / bit-exact references, at their edges:
focal losses, Adam, instance normalisation, split-K slab reduction, view copies / adds / gates, casts, the bf16
weight pack, the flip-transpose and the uint8 boundaries.

Operands are crops (strided views) of larger tensors wherever the entry point takes a view; the surrounding frame is
pre-filled with a sentinel and asserted untouched.  Every bar that is not exact is (a) a standing bar of
test_gpu_ops.py / test_gpu_bf16.py, (b) a bound derived in the comment next to it, or (c) 4x the error of a float32
NumPy restatement (util.inorm_f32, util.focal_*_grad_f32) against the float64 oracle, with the measured figure beside
it -- none is taken from a kernel's output.  Each test prints its figures before it asserts.  The bf16 focal gradients
are held element by element, next to TOL_BF16 of the largest gradient: bf16_gradient_stores.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bf16_exact
from util import rel_err, inorm_f32, focal_logits_grad_f32, focal_match_grad_f32

pytestmark = pytest.mark.gpu

TOL_BF16 = 6e-3          # TOL of test_gpu_bf16.py: one bf16 ulp at the top of the range is 2^-8
SENT = -512.0            # frame sentinel: exact in float32 and bf16, outside every value the kernels produce here
CAP = 4096 * 256         # elements one pass of the 4096-workgroup grid (grid_for) covers
GAMMAS = (2.0, 1.5, 3.0, 1.0, 0.5)      # 2: the multiply path; the others: powf, 0.5 with the singular derivative
EINVAL, EUNSUPPORTED, ESHAPE = -1, -2, -3


@pytest.fixture(scope="module")
def H():
    from transfer_em_amd import hip_ops
    hip_ops.require_gpu()
    return hip_ops


@pytest.fixture(scope="module")
def lib(H):
    from transfer_em_amd import _lib
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rb(a):
    """Round a float32 array to bf16-representable values (nearest even, torch on the CPU)."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return np.array_equal(bits(np.asarray(a)), bits(np.asarray(b)))


def host(t):
    """Device tensor -> NumPy with its bits kept (bf16 as float32)."""
    t = t.detach().cpu()
    return (t.float() if t.dtype == torch.bfloat16 else t).numpy()


class Framed:
    """A (N,D,H,W,C) view `v` inside a larger sentinel-filled tensor: unequal margins per axis, so that all four
    strides differ from the dense ones; cpad > 0 also makes it a channel slice (C smaller than sW)."""

    def __init__(self, shape, dtype=torch.float32, lo=(1, 2, 3), hi=(2, 1, 1), cpad=0, fill=None):
        N, D, Hh, W, Cc = shape
        self.sl = (slice(None), slice(lo[0], lo[0] + D), slice(lo[1], lo[1] + Hh), slice(lo[2], lo[2] + W),
                   slice(cpad // 2, cpad // 2 + Cc))
        self.big = torch.full((N, D + lo[0] + hi[0], Hh + lo[1] + hi[1], W + lo[2] + hi[2], Cc + cpad), SENT,
                              dtype=dtype, device="cuda")
        self.v = self.big[self.sl]
        if fill is not None:
            self.set(fill)

    def set(self, a):
        self.v.copy_(torch.from_numpy(np.array(a)).to(self.big.dtype))
        return self

    def get(self):
        return host(self.v.contiguous())

    def frame_ok(self):
        b = self.big.clone()
        b[self.sl] = SENT
        return bool((b == SENT).all())


def call(H, fn, *args):
    """Return code of a C-ABI entry point on the current stream (tem_view arguments by reference)."""
    from transfer_em_amd._lib import tem_view
    return fn(*[C.byref(a) if isinstance(a, tem_view) else a for a in args], H.current_stream())


# ------------------------------------------------------------------------------------------------- 1. focal losses
# one workgroup | just over focal_logits' 256 x 256 grid cap: every thread takes a SECOND pass of the grid-stride loop
# and 256 workgroups' atomics land on the same slots | ragged: 630 = 2 x 256 + 118, the last wave partly idle | C == 3
LOGIT_SHAPES = ((2, 4, 4, 4, 1), (2, 33, 33, 33, 1), (2, 5, 7, 9, 1), (2, 5, 6, 7, 3))
# focal_match caps its grid at sqrt(total / 256 * 1300 / (12 * slots)) workgroups: 2 x 60^3 wants 1688, gets 427 with
# one slot and 246 with three -- second (to seventh) pass of the loop, multi-workgroup atomics.  voff32 (both match
# kernels): C == 1 skips the channel division, C == 3 takes it.
MATCH_SHAPES = ((2, 4, 4, 4, 1), (2, 60, 60, 60, 1), (2, 5, 7, 9, 1), (2, 5, 6, 7, 3))
# saturated logits: float32 `pr` is exactly 0 or 1 there, and for gamma < 1 the derivative of pow is singular (-> 0)
PLANTED = np.array([17, -17, 20, -20, 40, -40, 88.8, -88.8, 100, -100, 0.0, -0.0], np.float32)


@functools.lru_cache(None)
def logits_input(shape, bf16):
    rng = np.random.default_rng(sum(shape))
    z = (rng.standard_normal(shape) * 3).astype(np.float32)
    planted = np.zeros(shape, bool)
    if z.size > 1000:       # (the small shapes stay as they are: one planted |z| = 100 would BE their loss)
        pos = 5 + 101 * np.arange(PLANTED.size)
        z.reshape(-1)[pos] = PLANTED
        planted.reshape(-1)[pos] = True
    if bf16:
        z = rb(z)
    z.setflags(write=False)
    return z, planted


@functools.lru_cache(None)
def match_input(shape, bf16):
    """a, b with |a - b| in [0.05, 1.6] apart from the planted elements.  The loss has a pole at |a - b| = 2
    (-log t, t = 1 - |a-b|/2 -> 0; see util.scaled_params), and for gamma < 1 its float32 form -- the reference's own:
    1 - (1 - |a-b|/2) -- loses the base to rounding as |a - b| -> 0; next to either, the float32 operator itself is
    further from the float64 oracle than the bars, whatever kernel computes it.  The exact ends are planted instead:
    a == b (base 0, t == 1: the clipped branch) and |a - b| > 2 (t < 0: clipped low)."""
    rng = np.random.default_rng(sum(shape) + 1)
    a = rng.standard_normal(shape).astype(np.float32)
    d = rng.uniform(0.05, 1.6, shape) * rng.choice((-1.0, 1.0), shape)
    b = (a + d).astype(np.float32)
    if bf16:
        a, b = rb(a), rb(b)
    fa, fb = a.reshape(-1), b.reshape(-1)
    planted = np.zeros(shape, bool)
    pos = 3 + 17 * np.arange(6)
    fb[pos[:3]] = fa[pos[:3]]
    fb[pos[3]] = fa[pos[3]] + np.float32(5.0)
    fb[pos[4]] = fa[pos[4]] - np.float32(3.0)
    fb[pos[5]] = fa[pos[5]] + np.float32(2.5)
    if bf16:
        b = rb(b)
        b.reshape(-1)[pos[:3]] = fa[pos[:3]]
    planted.reshape(-1)[pos] = True
    a.setflags(write=False); b.setflags(write=False)
    return a, b, planted


def bf16_gradient_stores(name, got, ref, f32, rest, cond=1.0):
    """The bf16 focal gradients element by element: each stored value within rne_bf16 of an interval around its own
    float64 reference `ref`.  The relative half-width is 4 x the per-element relative error of the float32 restatement
    `f32` (util.focal_*_grad_f32: the kernels' formula in NumPy float32, no HIP code) against the float64 oracle, the
    worst over the elements `rest` -- measured, printed, and for these inputs 3.1e-7 .. 7.1e-7 (focal_match) and
    1.2e-7 .. 1.7e-6 (focal_logits, per unit of `cond`).
    cond: the conditioning of the formula itself, where it is not 1.  For target == 1 the base of the modulating factor
    is 1 - p, and float32 has p only to 2^-24: 1 - p is known to 2^-24 p / (1 - p) = 2^-24 e^z relative, whatever computes
    it, and mod, dmod and dbase are powers of it.  Un-normalised, the restatement is 9.6e-3 off at z = 11.6 -- a uniform
    4 x that would be ten bf16 ulps for every element -- so the error is measured per unit of cond = 1 + e^z and the
    half-width of an element is 4 x that figure x its own cond.  The planted elements keep their separate comparison."""
    ref = np.asarray(ref, np.float64)
    cond = np.broadcast_to(np.asarray(cond, np.float64), ref.shape)
    assert (ref[rest] != 0).all()
    e = np.abs(f32.astype(np.float64) - ref)[rest] / np.abs(ref[rest]) / cond[rest]
    rho = float(e.max())
    lo, hi = bf16_exact.interval(ref[rest], 4 * rho * cond[rest] * np.abs(ref[rest]))
    r = bf16_exact.check_bounds(got[rest], ref[rest], lo, hi, f"{name}: float32 restatement {rho:.2e}, half-width 4 x that", rho=rho)
    assert rho < 4e-6, (name, rho)                        # the restatement itself: a few float32 roundings
    assert r["undecided"] <= bf16_exact.UNDECIDED_CAP, (name, r["undecided"])
    assert r["fails"] == 0, (name, r["fails"], r["total"], r["first"])
    return r


def _check_loss_slots(got, mask, want, bar):
    on = [k for k in range(8) if mask >> k & 1]
    off = [k for k in range(8) if not mask >> k & 1]
    e = max(abs(got[k] - want) / abs(want) for k in on)
    assert e < bar, (e, got, want)
    assert not got[off].any()
    return e


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("bf16", [False, True])
def test_focal_logits(H, oracle_lib, bf16, gamma):
    """tem_focal_logits / tem_focal_logits_bf16 vs oracle.ops.focal_logits: z an interior crop (cgan.py's
    cr(real_x, 2*b)), dz written into a crop, N == 2 with a non-dense sN, both targets, every gamma.  Bars of
    test_losses_and_adam / test_pack_weights_and_elementwise_bf16: loss 1e-6, gradient 1e-5 (fp32) / TOL (bf16).
    The planted saturated logits and the rest are compared apart: rel_err is relative to the largest value."""
    dt = torch.bfloat16 if bf16 else torch.float32
    tol = TOL_BF16 if bf16 else 1e-5
    losses = torch.zeros(8, dtype=torch.float64, device="cuda")
    for shape in LOGIT_SHAPES:
        z, planted = logits_input(shape, bf16)
        N, D, Hh, W, Cc = shape
        zbig = torch.full((N, D + 5, Hh + 5, W + 5, Cc), SENT, dtype=dt, device="cuda")
        zv = H.crop(zbig, 2, 3)
        zv.copy_(torch.from_numpy(z.copy()).to(dt))
        for target in (0, 1):
            l_ref, g_ref = oracle_lib.focal_logits(z, target, gamma)
            dzf = Framed(shape, dt, lo=(2, 1, 1), hi=(1, 3, 2))
            losses.zero_()
            H.run([H.focal_logits_launch("t", zv, target, gamma, losses, 0b101, 2.0, dzf.v, 3.0)])
            got, dz = losses.cpu().numpy(), dzf.get()
            e_l = _check_loss_slots(got, 0b101, 2 * l_ref, 1e-6)
            e_g = rel_err(dz[~planted], 3 * g_ref[~planted])
            e_p = rel_err(dz[planted], 3 * g_ref[planted]) if planted.any() else 0.0
            print(f"focal_logits bf16={bf16} gamma={gamma} {shape} t={target}: loss {e_l:.2e} grad {e_g:.2e} planted {e_p:.2e}")
            assert e_g < tol and e_p < tol, (shape, target, e_g, e_p)
            if bf16:
                bf16_gradient_stores(f"focal_logits gamma={gamma} {shape} t={target}", dz, 3 * g_ref,
                                     focal_logits_grad_f32(z, target, gamma, 3.0), ~planted,
                                     cond=1 + target * np.exp(z.astype(np.float64)))
            assert dzf.frame_ok()
        assert same_bits(host(zv.contiguous()), z)                       # the input is only read


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("bf16", [False, True])
def test_focal_match(H, oracle_lib, bf16, gamma):
    """tem_focal_match / tem_focal_match_bf16 vs oracle.ops.focal_prob_match on crops; bars of the existing tests:
    loss 2e-6, gradient 1e-5 (fp32) / TOL (bf16)."""
    dt = torch.bfloat16 if bf16 else torch.float32
    tol = TOL_BF16 if bf16 else 1e-5
    losses = torch.zeros(8, dtype=torch.float64, device="cuda")
    for shape in MATCH_SHAPES:
        a, b, planted = match_input(shape, bf16)
        l_ref, g_ref = oracle_lib.focal_prob_match(a, b, gamma)
        af = Framed(shape, dt, fill=a)
        bf = Framed(shape, dt, lo=(2, 2, 2), hi=(2, 2, 2), fill=b)
        for mask in ((0b10, 0b1101) if shape[1] == 60 else (0b10,)):     # 1-bit and 3-bit slot masks: two grid caps
            dbf = Framed(shape, dt, lo=(3, 1, 2), hi=(0, 2, 1))
            losses.zero_()
            H.run([H.focal_match_launch("t", af.v, bf.v, gamma, losses, mask, 4.0, dbf.v, 4.0)])
            got, db = losses.cpu().numpy(), dbf.get()
            e_l = _check_loss_slots(got, mask, 4 * l_ref, 2e-6)
            e_g = rel_err(db[~planted], 4 * g_ref[~planted])
            e_p = rel_err(db[planted], 4 * g_ref[planted])
            print(f"focal_match bf16={bf16} gamma={gamma} {shape} mask={mask:#b}: loss {e_l:.2e} grad {e_g:.2e} planted {e_p:.2e}")
            assert e_g < tol and e_p < tol, (shape, mask, e_g, e_p)
            if bf16:
                bf16_gradient_stores(f"focal_match gamma={gamma} {shape} mask={mask:#b}", db, 4 * g_ref,
                                     focal_match_grad_f32(a, b, gamma, 4.0), ~planted)
            assert dbf.frame_ok()
        assert af.frame_ok() and bf.frame_ok() and same_bits(af.get(), a) and same_bits(bf.get(), b)


@pytest.mark.parametrize("bf16", [False, True])
def test_focal_accumulation_and_null_arguments(H, lib, oracle_lib, bf16):
    """Two launches onto non-zero `losses` add and leave the slots outside the mask bit-identical; without dz / db
    only the loss is written; with losses == NULL only the gradient (block_accumulate tolerates it)."""
    dt = torch.bfloat16 if bf16 else torch.float32
    shape = (2, 5, 7, 9, 1)
    z, _ = logits_input(shape, bf16)
    a, b, _ = match_input(shape, bf16)
    zf, af, bf = Framed(shape, dt, fill=z), Framed(shape, dt, fill=a), Framed(shape, dt, fill=b)
    init = np.arange(8) * 0.25 + 1.0
    null = H.NULL_VIEW
    fl = lib.tem_focal_logits_bf16 if bf16 else lib.tem_focal_logits
    fm = lib.tem_focal_match_bf16 if bf16 else lib.tem_focal_match
    for gamma in (2.0, 0.5):
        ref_l, _ = oracle_lib.focal_logits(z, 1, gamma)
        ref_m, _ = oracle_lib.focal_prob_match(a, b, gamma)
        for what, ref, bar, mask in (("logits", ref_l, 1e-6, 0b1001), ("match", ref_m, 2e-6, 0b10000010)):
            def launch(losses_ptr, out_view):
                if what == "logits":
                    return call(H, fl, H.view(zf.v), 1, gamma, losses_ptr, mask, 2.0, out_view, 3.0)
                return call(H, fm, H.view(af.v), H.view(bf.v), gamma, losses_ptr, mask, 2.0, out_view, 3.0)
            losses = dev(init.copy())
            gf = Framed(shape, dt)
            assert launch(losses.data_ptr(), H.view(gf.v)) == 0                # loss and gradient
            assert launch(losses.data_ptr(), null) == 0                       # loss only (NULL view)
            got, g_full = losses.cpu().numpy(), gf.get()
            for k in range(8):
                if mask >> k & 1:
                    assert abs(got[k] - init[k] - 4 * ref) < bar * abs(4 * ref), (what, k, got[k], init[k], ref)
                else:
                    assert got[k] == init[k]
            g2 = Framed(shape, dt)
            assert launch(None, H.view(g2.v)) == 0                             # gradient only (losses == NULL)
            assert same_bits(g2.get(), g_full) and g2.frame_ok() and gf.frame_ok()
            assert not (g_full == SENT).any()
    # extents of dz / db (and of a against b) must match
    small = Framed((2, 5, 7, 8, 1), dt)
    losses = dev(init.copy())
    assert call(H, fl, H.view(zf.v), 1, 2.0, losses.data_ptr(), 1, 1.0, H.view(small.v), 1.0) == ESHAPE
    assert call(H, fm, H.view(af.v), H.view(small.v), 2.0, losses.data_ptr(), 1, 1.0, null, 1.0) == ESHAPE
    assert call(H, fm, H.view(af.v), H.view(bf.v), 2.0, losses.data_ptr(), 1, 1.0, H.view(small.v), 1.0) == ESHAPE
    assert np.array_equal(losses.cpu().numpy(), init) and small.frame_ok() and (small.get() == SENT).all()


# ------------------------------------------------------------------------------------------------- 2. Adam
@pytest.mark.parametrize("step0", [0, 9, 999, 20000, 1 << 24])
def test_adam_bias_correction_and_grid_stride(H, lib, oracle_lib, step0):
    """tem_adam_keras + tem_step_tick from a preset step counter, two updates, vs oracle.ops.adam_keras fed the same
    float32 t = (float)step + 1 (at 2^24 the float no longer counts: t stays 2^24 for both updates).
    n = 4096 * 256 + 777: the first 777 threads of the capped grid take a SECOND pass of the grid-stride loop.
    Bars as in test_losses_and_adam: rel_err < 1e-6 on theta, m and v.  theta ~ 0.01 N(0,1), so that the bar sees
    the update (|dtheta| ~ lr = 2e-4 is 4e-3 of the largest theta, 1e-6 of it a 2.5e-4 error of alpha; powf against
    np.power is a few float32 ulp of beta^t, at most 6e-5 of 1 - beta2^t at t = 1).  The planted entries are compared
    apart from the rest -- |g| = 1e18 gives v = 1e33, against which rel_err would see nothing else."""
    f = np.float32
    n = CAP + 777
    rng = np.random.default_rng(21)
    th = (rng.standard_normal(n) * 0.01).astype(f)
    g = rng.standard_normal(n).astype(f)
    m = (rng.standard_normal(n) * 0.1).astype(f)
    v = (rng.random(n) * 0.01).astype(f)
    planted = np.zeros(n, bool)
    pos = np.array([0, 255, 256, CAP - 1, CAP, CAP + 3, n - 1, 4099])
    planted[pos] = True
    zero = pos[:5]                       # g == 0, m == v == 0: theta must stay bit-identical (also past the grid cap)
    g[zero] = 0.0; m[zero] = 0.0; v[zero] = 0.0
    g[pos[1]] = -0.0                     # negative zero gradient
    th[pos[2]] = -0.0                    # negative zero parameter
    g[pos[5]], g[pos[6]], g[pos[7]] = f(1e-20), f(-1e18), f(-1e-20)
    m[pos[5]] = 0.0; v[pos[5]] = 0.0     # g^2 = 1e-40 is denormal in float32
    th0 = th.copy()
    d = [dev(x) for x in (th, g, m, v)]
    step = torch.tensor([step0], dtype=torch.int32, device="cuda")
    for k in range(2):
        t = f(f(np.uint32(step0 + k)) + f(1))
        th, m, v = oracle_lib.adam_keras(th, g, m, v, t)
        H.run([H.adam_launch("adam", d[0], d[1], d[2], d[3], step), H.step_tick_launch(step)])
    assert int(step.item()) == step0 + 2
    got = [host(x) for x in (d[0], d[2], d[3])]
    rest = ~planted
    for name, a, r in zip(("theta", "m", "v"), got, (th, m, v)):
        e = rel_err(a[rest], r[rest])
        # planted entries one by one, to the same 1e-6 of their own value; 1.2e-38 (FLT_MIN) lets a denormal v flush
        ep = np.abs(a[planted].astype(np.float64) - r[planted]) - 1.2e-38
        print(f"adam step0={step0} {name}: rest {e:.2e}, planted {np.max(ep / (np.abs(r[planted]) + 1e-30)):.2e}")
        assert e < 1e-6, (name, e)
        assert (ep <= 1e-6 * np.abs(r[planted])).all(), (name, a[planted], r[planted])
    assert same_bits(got[0][zero], th0[zero])
    assert same_bits(host(d[1]), g)                                     # the gradient is only read
    # n == 0 returns TEM_OK and touches nothing
    before = [x.clone() for x in d]
    assert call(H, lib.tem_adam_keras, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 0, 2e-4, 0.5,
                0.999, 1e-7, 1.0, step.data_ptr()) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(d, before)) and int(step.item()) == step0 + 2


# ------------------------------------------------------------------------------------------------- 3. instance norm
def _inorm_run(H, lib, x, dy, scale, offset, eps=1e-5):
    """tem_instance_norm + tem_instance_norm_bwd through the C ABI with x, y, dy, dx all crops; returns host arrays
    (y, mean, rstd, dx, dscale, doffset) after checking every frame."""
    N, Cc = x.shape[0], x.shape[4]
    xf = Framed(x.shape, fill=x)
    yf = Framed(x.shape, lo=(2, 1, 1), hi=(0, 2, 3))
    gf = Framed(x.shape, lo=(0, 3, 2), hi=(1, 1, 0), cpad=2, fill=dy)
    dxf = Framed(x.shape, lo=(1, 1, 1), hi=(1, 1, 1), cpad=3)
    sc, off = dev(scale), dev(offset)
    mean = torch.full((N * Cc + 1,), SENT, device="cuda")
    rstd = torch.full((N * Cc + 1,), SENT, device="cuda")
    ds = torch.full((Cc + 1,), SENT, device="cuda")
    do = torch.full((Cc + 1,), SENT, device="cuda")
    ws = torch.zeros(2 * N * Cc, dtype=torch.float64, device="cuda")
    assert call(H, lib.tem_instance_norm, H.view(xf.v), sc.data_ptr(), off.data_ptr(), eps, H.view(yf.v),
                mean.data_ptr(), rstd.data_ptr()) == 0
    assert call(H, lib.tem_instance_norm_bwd, H.view(xf.v), H.view(gf.v), sc.data_ptr(), mean.data_ptr(),
                rstd.data_ptr(), H.view(dxf.v), ds.data_ptr(), do.data_ptr(), ws.data_ptr()) == 0
    for fr in (xf, yf, gf, dxf):
        assert fr.frame_ok()
    assert same_bits(xf.get(), x) and same_bits(gf.get(), dy)
    mean, rstd, ds, do = host(mean), host(rstd), host(ds), host(do)
    assert mean[-1] == SENT and rstd[-1] == SENT and ds[-1] == SENT and do[-1] == SENT      # guards past the ends
    return yf.get(), mean[:-1].reshape(N, Cc), rstd[:-1].reshape(N, Cc), dxf.get(), ds[:-1], do[:-1]


def _inorm_params(rng, Cc):
    return ((1.0 + 0.02 * rng.standard_normal(Cc)).astype(np.float32),
            np.linspace(-0.5, 0.5, Cc).astype(np.float32) if Cc > 1 else np.array([0.25], np.float32))


# mean is ONE float32 rounding of a float64 sum: 2^-24 of its value; allowed 2^-23.  rstd = rsqrtf(var + eps): the
# deviations and their squares round once each (3 x 2^-24 on a sum of positive terms), var and var + eps once each,
# the root halves that (2.5 x 2^-24), rsqrtf itself is good to 2 ulp (2^-22): 3.9e-7 in all; allowed 2^-21 = 4.8e-7.
MEAN_BAR, RSTD_BAR = 2.0 ** -23, 2.0 ** -21


def _inorm_stats_ok(mean, rstd, mean_ref, rstd_ref):
    mean_ref, rstd_ref = mean_ref.reshape(mean.shape), rstd_ref.reshape(rstd.shape)
    e_m = np.abs(mean - mean_ref) / (np.abs(mean_ref) + 1e-30)
    e_r = np.abs(rstd - rstd_ref) / rstd_ref
    print(f"   mean {e_m.max():.2e} (bar {MEAN_BAR:.1e}), rstd {e_r.max():.2e} (bar {RSTD_BAR:.1e})")
    assert e_m.max() <= MEAN_BAR and e_r.max() <= RSTD_BAR, (e_m.max(), e_r.max())


INORM_SHAPES = [
    (2, 1, 1, 1, 8),          # 1 voxel per channel: variance 0, dx == 0
    (2, 3, 3, 3, 1),          # 27 voxels: most of the 1024 threads idle; C == 1
    (1, 10, 10, 10, 32),      # 1000: the last wave of the workgroup partly idle
    (2, 8, 8, 16, 8),         # 1024: exactly one element per thread
    (2, 1, 25, 41, 8),        # 1025, 2-D (D == 1): one thread takes a second element
    (3, 9, 10, 11, 8),        # 990, N == 3
    (1, 3, 3, 3, 256),        # the largest supported channel count: all 256 threads of block 0 fold dscale / doffset
]


@pytest.mark.parametrize("shape", INORM_SHAPES)
def test_instance_norm_shapes(H, lib, oracle_lib, shape):
    """tem_instance_norm / tem_instance_norm_bwd on strided views vs oracle.ops.instance_norm[_bwd]; bars of
    test_instance_normalization: y 2e-6, dx / dscale / doffset 1e-5."""
    rng = np.random.default_rng(sum(shape))
    x = (rng.standard_normal(shape) * 2 + 0.7).astype(np.float32)
    dy = rng.standard_normal(shape).astype(np.float32)
    scale, offset = _inorm_params(rng, shape[4])
    y, mean, rstd, dx, ds, do = _inorm_run(H, lib, x, dy, scale, offset)
    y_ref, mean_ref, rstd_ref = oracle_lib.instance_norm(x, scale, offset)
    dx_ref, ds_ref, do_ref = oracle_lib.instance_norm_bwd(x, dy, scale)
    errs = rel_err(y, y_ref), rel_err(ds, ds_ref), rel_err(do, do_ref)
    print(f"inorm {shape}: y {errs[0]:.2e} dscale {errs[1]:.2e} doffset {errs[2]:.2e}")
    _inorm_stats_ok(mean, rstd, np.moveaxis(mean_ref, 4, 1), np.moveaxis(rstd_ref, 4, 1))
    assert errs[0] < 2e-6 and errs[2] < 1e-5
    if shape[1] * shape[2] * shape[3] == 1:
        # one voxel: x - mean == 0 exactly, so y == offset, dx == 0 and dscale == 0 with no rounding at all
        assert np.array_equal(y, np.broadcast_to(offset, shape)) and not dx.any() and not ds.any()
        assert same_bits(mean, x.reshape(mean.shape))
    else:
        e_dx = rel_err(dx, dx_ref)
        print(f"   dx {e_dx:.2e}")
        assert e_dx < 1e-5 and errs[1] < 1e-5


def test_instance_norm_statistics(H, lib, oracle_lib):
    """A constant channel (rstd = 1/sqrt(eps), y == offset), one with spread 1e-3 around 0, beside ordinary ones.  y and
    dx are compared CHANNEL BY CHANNEL (the constant channel's dx is 316x the others' and would hide them)."""
    shape = (2, 9, 10, 11, 8)
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(shape) * 2 + 0.7).astype(np.float32)
    x[..., 0] = np.float32(0.37)
    x[..., 1] = (rng.standard_normal(shape[:4]) * 1e-3).astype(np.float32)
    dy = rng.standard_normal(shape).astype(np.float32)
    scale, offset = _inorm_params(rng, 8)
    y, mean, rstd, dx, ds, do = _inorm_run(H, lib, x, dy, scale, offset)
    y_ref, mean_ref, rstd_ref = oracle_lib.instance_norm(x, scale, offset)
    dx_ref, ds_ref, do_ref = oracle_lib.instance_norm_bwd(x, dy, scale)
    _inorm_stats_ok(mean, rstd, np.moveaxis(mean_ref, 4, 1), np.moveaxis(rstd_ref, 4, 1))
    assert same_bits(mean[:, 0], np.full(2, 0.37, np.float32))
    assert np.array_equal(y[..., 0], np.full(shape[:4], offset[0]))         # x - mean == 0 exactly
    for c in range(8):
        e_y, e_dx = rel_err(y[..., c], y_ref[..., c]), rel_err(dx[..., c], dx_ref[..., c])
        print(f"inorm statistics c={c}: y {e_y:.2e} dx {e_dx:.2e}")
        assert e_y < 2e-6 and e_dx < 1e-5, (c, e_y, e_dx)
    assert rel_err(ds, ds_ref) < 1e-5 and rel_err(do, do_ref) < 1e-5
    assert abs(ds[0]) <= 1e-5 * np.abs(ds_ref).max()                        # xhat == 0 on the constant channel


# util.inorm_f32 (float32 roundings where the kernels round, float64 sums) against the float64 oracle on THIS test's
# inputs (seed 4, mean 10, spread 0.1), measured on the CPU: y 1.22e-6, dscale 3.70e-6 (rounded up), dx 2.0e-7, doffset 1.6e-8.  The
# float32 input itself carries 2^-24 * 10 / 0.1 = 6e-6 of a deviation, so this case sits at the standing bars (2e-6 /
# 1e-5) whatever kernel computes it; y and dscale, which carry that error undamped, get 4x the restatement's figure
# instead, dx and doffset keep the standing 1e-5.
MEAN10_Y_BAR = 4 * 1.22e-6
MEAN10_DSCALE_BAR = 4 * 3.70e-6


def mean10_input():
    shape = (2, 9, 10, 11, 8)
    rng = np.random.default_rng(4)
    x = (10.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
    dy = rng.standard_normal(shape).astype(np.float32)
    scale, offset = _inorm_params(rng, 8)
    return x, dy, scale, offset


def test_instance_norm_large_mean(H, lib, oracle_lib):
    """Mean 10 against a spread of 0.1 in every channel: what the two-pass variance protects (E[x^2] - E[x]^2 in
    float32 would lose the variance 0.01 under 100 * 2^-24 = 6e-6 -- six parts in ten thousand)."""
    x, dy, scale, offset = mean10_input()
    y, mean, rstd, dx, ds, do = _inorm_run(H, lib, x, dy, scale, offset)
    y_ref, mean_ref, rstd_ref = oracle_lib.instance_norm(x, scale, offset)
    dx_ref, ds_ref, do_ref = oracle_lib.instance_norm_bwd(x, dy, scale)
    _inorm_stats_ok(mean, rstd, np.moveaxis(mean_ref, 4, 1), np.moveaxis(rstd_ref, 4, 1))
    errs = rel_err(y, y_ref), rel_err(dx, dx_ref), rel_err(ds, ds_ref), rel_err(do, do_ref)
    print("inorm mean 10: y %.2e dx %.2e dscale %.2e doffset %.2e" % errs)
    r = inorm_f32(x, dy, scale, offset)         # the two bars are what they say: 4x the restatement on these inputs
    assert 4 * rel_err(r[0], y_ref) <= MEAN10_Y_BAR and 4 * rel_err(r[4], ds_ref) <= MEAN10_DSCALE_BAR
    assert errs[0] < MEAN10_Y_BAR and errs[2] < MEAN10_DSCALE_BAR
    assert errs[1] < 1e-5 and errs[3] < 1e-5


def test_instance_norm_rejects(H, lib):
    """C == 257 -> TEM_EUNSUPPORTED, mismatched extents -> TEM_ESHAPE, in both directions, with nothing written."""
    def run(xshape, oshape, want):
        Cc, N = xshape[4], xshape[0]
        xf = Framed(xshape, fill=np.ones(xshape, np.float32))
        of = Framed(oshape)
        par = torch.ones(Cc, device="cuda")
        out = torch.full((4, N * Cc), SENT, device="cuda")
        ws = torch.zeros(2 * N * Cc, dtype=torch.float64, device="cuda")
        assert call(H, lib.tem_instance_norm, H.view(xf.v), par.data_ptr(), par.data_ptr(), 1e-5, H.view(of.v),
                    out[0].data_ptr(), out[1].data_ptr()) == want
        assert call(H, lib.tem_instance_norm_bwd, H.view(xf.v), H.view(xf.v), par.data_ptr(), par.data_ptr(),
                    par.data_ptr(), H.view(of.v), out[2].data_ptr(), out[3].data_ptr(), ws.data_ptr()) == want
        if oshape != xshape:        # dy with other extents than x
            assert call(H, lib.tem_instance_norm_bwd, H.view(xf.v), H.view(of.v), par.data_ptr(), par.data_ptr(),
                        par.data_ptr(), H.view(xf.v), out[2].data_ptr(), out[3].data_ptr(), ws.data_ptr()) == want
        torch.cuda.synchronize()
        assert (of.big == SENT).all() and (out == SENT).all() and not ws.any() and (xf.get() == 1).all()
    run((1, 2, 2, 2, 257), (1, 2, 2, 2, 257), EUNSUPPORTED)
    run((2, 3, 4, 5, 8), (2, 3, 4, 6, 8), ESHAPE)
    run((2, 3, 4, 5, 8), (2, 3, 4, 5, 4), ESHAPE)
    run((2, 3, 4, 5, 8), (1, 3, 4, 5, 8), ESHAPE)


# ------------------------------------------------------------------------------------------------- 4. slab reduction
# Slabs of small integers (|x| <= 64, at most 750 of them: every partial sum is an integer below 2^24) make every
# float32 summation order exact: the reference is an int64 sum and the comparison array_equal.
def _items_table(items):
    from transfer_em_amd import _lib
    arr = (_lib.tem_reduce_item * len(items))(*[_lib.tem_reduce_item(*it) for it in items])
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def _reduce_multi(H, lib, items, scale):
    table = _items_table(items)
    rc = call(H, lib.tem_reduce_slabs_multi, table.data_ptr(), len(items), float(scale))
    torch.cuda.synchronize()
    return rc


NSLABS = (1, 2, 15, 16, 17, 112, 113, 127, 128, 129, 257, 750)
COUNTS = (1, 3, 4, 27, 32, 60, 63, 64)


@pytest.mark.parametrize("scale", [1.0, 0.5, 4.0])
def test_reduce_slabs_multi_geometries(H, lib, scale):
    """tem_reduce_slabs_multi: ONE launch of 288 hand-built items, every (nslab, count) of the lists above in three
    layouts, each with its own geometry (what GradWorkspace.reduce_launches builds per layer):
      - stride a multiple of 4, 16-byte aligned rows: counts 4, 32, 60, 64 take the VECTOR form of reduce_multi_k
        (its 128-slab main loop runs for nslab >= 113 -- at 113 for slab lane 0 alone -- and not below; the 8-deep
        tail handles what is left, down to lanes with no slab at all for nslab < 16), counts 1, 3, 27, 63 the SCALAR
        form (16-slab main loop from nslab 13 up);
      - stride not a multiple of 4: scalar form for every count;
      - stride a multiple of 4 but the slab pointer one float past alignment: scalar form at counts that would
        otherwise vectorise.
    Outputs land 72 floats apart in a sentinel-filled vector: nothing past `count` may be written."""
    rng = np.random.default_rng(int(scale * 8))
    geo, total = [], 0
    for nslab in NSLABS:
        for count in COUNTS:
            for layout in range(3):
                stride = (count + 3) // 4 * 4 + (8 if layout != 1 else 5 + 2 * (count & 1))
                assert (stride % 4 == 0) == (layout != 1)
                off = total + (1 if layout == 2 else 0)
                geo.append((off, stride, nslab, count))
                total += (nslab * stride + 1 + 3) // 4 * 4
    slabs = rng.integers(-64, 65, total).astype(np.float32)
    d_slabs = dev(slabs)
    out = torch.full((72 * len(geo),), SENT, device="cuda")
    assert d_slabs.data_ptr() % 16 == 0
    items = [(d_slabs.data_ptr() + 4 * off, stride, nslab, count, out.data_ptr() + 4 * 72 * i)
             for i, (off, stride, nslab, count) in enumerate(geo)]
    assert _reduce_multi(H, lib, items, scale) == 0
    got = host(out).reshape(len(geo), 72)
    for i, (off, stride, nslab, count) in enumerate(geo):
        rows = slabs[off:off + nslab * stride].reshape(nslab, stride)[:, :count]
        want = (rows.astype(np.int64).sum(axis=0) * scale).astype(np.float32)
        assert np.array_equal(got[i, :count], want), (geo[i], got[i, :count], want)
        assert (got[i, count:] == SENT).all(), geo[i]
    assert same_bits(host(d_slabs), slabs)


@pytest.mark.parametrize("n,n_early,nsl", [(200, 5, 9), (203, 2, 3), (64, 130, 131)])
def test_reduce_slabs_multi_in_place_early_then_final(H, lib, n, n_early, nsl):
    """The IN-PLACE form of reduce_early (GradWorkspace.reduce_launches(split_call=...)): `out` of every item is the
    last of the rows it sums, same columns; the final launch then sums that row and the later ones.  n = 200 / 64:
    vector form (64-column chunks and an 8-column one), 203: scalar form; 130 early rows: the 128-slab main loop."""
    rng = np.random.default_rng(n)
    t0 = rng.integers(-64, 65, (nsl, n)).astype(np.float32)
    t = dev(t0)
    grad = torch.full((n + 1,), SENT, device="cuda")
    first = n_early - 1
    chunks = [(o, min(64, n - o)) for o in range(0, n, 64)]
    early = [(t.data_ptr() + 4 * o, n, n_early, c, t[first].data_ptr() + 4 * o) for o, c in chunks]
    final = [(t[first].data_ptr() + 4 * o, n, nsl - first, c, grad.data_ptr() + 4 * o) for o, c in chunks]
    assert _reduce_multi(H, lib, early, 1.0) == 0
    after = host(t)
    want_row = t0[:n_early].astype(np.int64).sum(axis=0).astype(np.float32)
    assert np.array_equal(after[first], want_row)
    keep = np.arange(nsl) != first
    assert same_bits(after[keep], t0[keep])                               # every other row is only read
    assert _reduce_multi(H, lib, final, 0.5) == 0
    got = host(grad)
    assert np.array_equal(got[:n], (t0.astype(np.int64).sum(axis=0) * 0.5).astype(np.float32)) and got[n] == SENT


def test_reduce_slabs_multi_reversed_rows(H, lib):
    """The item set GradWorkspace.flip_rows produces for a C_out == 1 layer computed in swapped form: slab row r holds
    tap (ntap - 1 - r), one item per tap row writes it to the reversed place -- checked against the reversed tap
    order.  (ntap, row) = (27, 16) vector form, (27, 1) scalar form (the 1x1 head's row is one float)."""
    rng = np.random.default_rng(2)
    for ntap, row, nslab in ((27, 16, 37), (27, 1, 5), (9, 32, 129)):
        n = ntap * row
        t0 = rng.integers(-64, 65, (nslab, n)).astype(np.float32)
        t = dev(t0)
        out = torch.full((n + 1,), SENT, device="cuda")
        items = [(t.data_ptr() + 4 * r * row, n, nslab, row, out.data_ptr() + 4 * (ntap - 1 - r) * row)
                 for r in range(ntap)]
        assert _reduce_multi(H, lib, items, 1.0) == 0
        got = host(out)
        want = t0.astype(np.int64).sum(axis=0).reshape(ntap, row)[::-1].reshape(-1).astype(np.float32)
        assert np.array_equal(got[:n], want) and got[n] == SENT, (ntap, row)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_reduce_slabs_single(H, lib, n):
    """tem_reduce_slabs: one thread per output, n around the 256-thread workgroup and 274 workgroups; slab_stride 0
    (== n) and > n; accumulate on and off; scales 1, 0.5, 4."""
    rng = np.random.default_rng(n)
    nslab = 7
    for stride in (0, n + 5):
        st = stride or n
        slabs = rng.integers(-64, 65, nslab * st).astype(np.float32)
        d_slabs = dev(slabs)
        ssum = slabs.reshape(nslab, st)[:, :n].astype(np.int64).sum(axis=0)
        for accumulate, scale in ((0, 1.0), (1, 0.5), (0, 4.0), (1, 4.0)):
            out0 = rng.integers(-64, 65, n + 1).astype(np.float32)
            out = dev(out0)
            H.run([H.reduce_slabs_launch("t", d_slabs, nslab, n, stride, out, bool(accumulate), scale)])
            got = host(out)
            want = (ssum * scale + (out0[:n] if accumulate else 0)).astype(np.float32)
            assert np.array_equal(got[:n], want), (n, stride, accumulate, scale)
            assert got[n] == out0[n]                                      # the element past the end
    assert call(H, lib.tem_reduce_slabs, d_slabs.data_ptr(), nslab, 0, 0, out.data_ptr(), 0, 1.0) == 0      # n == 0
    assert call(H, lib.tem_reduce_slabs, d_slabs.data_ptr(), 0, n, 0, out.data_ptr(), 0, 1.0) == EINVAL
    torch.cuda.synchronize()
    assert same_bits(host(out), got)


def test_reduce_slabs_deterministic_and_bounded(H, lib):
    """Random floats: two runs are bitwise equal (fixed summation order, no atomics), and every output is within
    nslab * 2^-24 * sum|x| * |scale| of the float64 sum -- the standard bound (n - 1) u sum|x| of recursive
    summation in ANY order, plus one rounding for the scale."""
    rng = np.random.default_rng(9)
    nslab, scale = 750, 0.37
    geo = [(0, 64, 64), (nslab * 64, 67, 63)]                               # (offset, stride, count): vector, scalar
    slabs = rng.standard_normal(nslab * (64 + 67)).astype(np.float32)
    d_slabs = dev(slabs)
    runs = []
    for _ in range(2):
        out = torch.zeros(128, device="cuda")
        items = [(d_slabs.data_ptr() + 4 * off, stride, nslab, count, out.data_ptr() + 4 * 64 * i)
                 for i, (off, stride, count) in enumerate(geo)]
        assert _reduce_multi(H, lib, items, scale) == 0
        runs.append(host(out))
    assert same_bits(runs[0], runs[1])
    single = torch.zeros(64, device="cuda")
    for _ in range(2):
        H.run([H.reduce_slabs_launch("t", d_slabs, nslab, 64, 64, single, False, scale)])
        runs.append(host(single))
    assert same_bits(runs[2], runs[3])
    for i, (off, stride, count) in enumerate(geo):
        rows = slabs[off:off + nslab * stride].reshape(nslab, stride)[:, :count].astype(np.float64)
        bound = nslab * 2.0 ** -24 * np.abs(rows).sum(axis=0) * scale
        for got in ([runs[0][64 * i:64 * i + count]] + ([runs[2]] if i == 0 else [])):
            err = np.abs(got - rows.sum(axis=0) * np.float32(scale))
            print(f"reduce item {i}: worst err / bound {np.max(err / bound):.3f}")
            assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------- 5. views, formats
VIEW_SHAPES = [
    ((2, 7, 9, 11, 1), 0),        # C == 1
    ((2, 6, 7, 8, 5), 3),         # C == 5 as a channel slice of an 8-channel tensor (C < sW)
    ((2, 41, 41, 41, 8), 0),      # 1,102,736 elements > 4096 * 256: 54,160 threads take a SECOND grid-stride pass
    ((1, 1, 1, 1, 1), 0),         # one element
]


@pytest.mark.parametrize("shape,cpad", VIEW_SHAPES)
def test_copy_add_gate_views(H, lib, shape, cpad):
    """tem_copy_view, tem_add_view, tem_leaky_gate_view, tem_copy_view_bf16, tem_add_view_bf16: source and destination
    are crops with DIFFERENT strides; every result is exact (one float32 operation per element)."""
    rng = np.random.default_rng(sum(shape))
    s = rng.standard_normal(shape).astype(np.float32)
    d = rng.standard_normal(shape).astype(np.float32)
    sf = Framed(shape, cpad=cpad, fill=s)
    df = Framed(shape, lo=(2, 1, 2), hi=(1, 3, 0), fill=d)
    H.run([H.copy_view_launch("t", sf.v, df.v, add=True)])
    assert same_bits(df.get(), d + s) and df.frame_ok()
    H.run([H.copy_view_launch("t", sf.v, df.v)])
    assert same_bits(df.get(), s) and df.frame_ok() and sf.frame_ok() and same_bits(sf.get(), s)
    # gate: saved holds both zeros, the smallest positive denormal (> 0: the gradient passes), negatives
    saved = rng.standard_normal(shape).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, -1.0, 1.0], np.float32)
    k = min(saved.size, special.size)
    saved.reshape(-1)[:k] = special[:k]
    if saved.size > CAP:
        saved.reshape(-1)[CAP:CAP + k] = special[:k]
    svf = Framed(shape, lo=(0, 2, 1), hi=(3, 0, 2), fill=saved)
    gf = Framed(shape, cpad=cpad, fill=s)
    slope = np.float32(0.3)
    H.run([H.leaky_gate_launch("t", gf.v, svf.v, float(slope))])
    assert same_bits(gf.get(), np.where(saved > 0, s, slope * s).astype(np.float32))
    assert gf.frame_ok() and svf.frame_ok() and same_bits(svf.get(), saved)
    # bf16: the copy moves bits, the add is bf16(float(d) + float(s)) (torch on the CPU)
    sh, dh = torch.from_numpy(s).to(torch.bfloat16), torch.from_numpy(d).to(torch.bfloat16)
    sfh = Framed(shape, torch.bfloat16, cpad=cpad).set(sh.float().numpy())
    dfh = Framed(shape, torch.bfloat16, lo=(2, 1, 2), hi=(1, 3, 0)).set(dh.float().numpy())
    H.run([H.copy_view_launch("t", sfh.v, dfh.v, add=True)])
    want = (dh.float() + sh.float()).to(torch.bfloat16)
    assert torch.equal(dfh.v.contiguous().cpu().view(torch.int16), want.view(torch.int16)) and dfh.frame_ok()
    H.run([H.copy_view_launch("t", sfh.v, dfh.v)])
    assert torch.equal(dfh.v.contiguous().cpu().view(torch.int16), sh.view(torch.int16)) and dfh.frame_ok() and sfh.frame_ok()


def test_view_kernels_reject_mismatched_extents(H, lib):
    for dt, names in ((torch.float32, ("tem_copy_view", "tem_add_view", "tem_leaky_gate_view")),
                      (torch.bfloat16, ("tem_copy_view_bf16", "tem_add_view_bf16"))):
        a = Framed((2, 3, 4, 5, 8), dt)
        for other in ((2, 3, 4, 5, 5), (2, 3, 4, 6, 8), (2, 3, 5, 5, 8), (2, 4, 4, 5, 8), (1, 3, 4, 5, 8)):
            b = Framed(other, dt)
            for name in names:
                extra = (0.3,) if name == "tem_leaky_gate_view" else ()
                assert call(H, getattr(lib, name), H.view(a.v), H.view(b.v), *extra) == ESHAPE, name
                assert call(H, getattr(lib, name), H.view(b.v), H.view(a.v), *extra) == ESHAPE, name
            torch.cuda.synchronize()
            assert (b.big == SENT).all()
        assert (a.big == SENT).all()


@pytest.mark.parametrize("n", [1, 255, CAP + 1])
def test_fill(H, lib, n):
    """tem_fill_f32: bit patterns of 0, -0.0 and 1e-30; CAP + 1: thread 0 takes a second pass; the element after the
    end stays."""
    for value in (0.0, -0.0, 1e-30):
        t = torch.full((n + 1,), SENT, device="cuda")
        H.run([H.fill_launch("t", t[:n], value)])
        got = host(t)
        assert same_bits(got[:n], np.full(n, value, np.float32)) and got[n] == SENT
    assert call(H, lib.tem_fill_f32, t.data_ptr(), 0, 7.0) == 0                 # n == 0: nothing
    torch.cuda.synchronize()
    assert same_bits(host(t), got)


def test_cast_f32_to_bf16_bit_patterns(H, lib):
    """tem_cast_f32_to_bf16 against torch's CPU cast, bit for bit: ties to even (down and up), just off a tie, +-0,
    denormals, +-inf, the largest finite floats (round to inf); NaN by isnan only.  Length past the grid cap."""
    pat = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F817FFF, 0x3F818001, 0xBF808000, 0xBF818000,
                    0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x00008001, 0x007FFFFF,
                    0x807FFFFF, 0x00800000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,
                    0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7FBFFFFF], np.uint32)
    rng = np.random.default_rng(8)
    n = CAP + 5
    u = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)       # random bit patterns: every exponent
    u[:pat.size] = pat
    u[-pat.size:] = pat                                                     # ... and in the second grid-stride pass
    src = torch.from_numpy(u.view(np.float32).copy())
    want = src.to(torch.bfloat16)
    dst = torch.zeros(n + 1, dtype=torch.bfloat16, device="cuda")
    dst[n] = SENT
    H.run([H.cast_bf16_launch("t", src.cuda(), dst[:n])])
    got = dst.cpu()
    assert float(got[n]) == SENT
    got = got[:n]
    nan = torch.isnan(want)
    assert int(nan.sum()) > 5 and torch.equal(torch.isnan(got), nan)
    assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])
    assert call(H, lib.tem_cast_f32_to_bf16, src.data_ptr(), dst.data_ptr(), -1) == EINVAL


# (ntap, ci, co) of the hand-made kernel table: 3-D and 2-D taps, one-channel sides, a 1x1 layer
WLAYERS = ((27, 8, 16), (64, 16, 8), (9, 1, 8), (16, 32, 1), (1, 32, 32))


def _wtable():
    """tem_wlayer table over a flat vector: a leading run of 5 floats, a bias gap after every layer (of co, at
    least 3, floats), the last of them the trailing run -- all outside the table."""
    rows, off = [], 5
    for ntap, ci, co in WLAYERS:
        rows.append((off, ntap, ci, co))
        off += ntap * ci * co + max(co, 3)
    tab = np.zeros(len(rows), dtype=np.dtype([("offset", "<i8"), ("ntap", "<i4"), ("ci", "<i4"), ("co", "<i4"),
                                              ("pad", "<i4")]))
    for i, (o, nt, ci, co) in enumerate(rows):
        tab[i] = (o, nt, ci, co, 0)
    assert tab.itemsize == 24
    return rows, off, torch.from_numpy(tab.view(np.uint8).copy()).cuda()


def _permuted(theta, rows, flip):
    """NumPy statement of tem_flip_transpose (flip) / theta_ht of tem_pack_weights_bf16 (no flip)."""
    out = theta.copy()
    for off, ntap, ci, co in rows:
        w = theta[off:off + ntap * ci * co].reshape(ntap, ci, co)
        w = w[::-1] if flip else w
        out[off:off + ntap * ci * co] = np.swapaxes(w, 1, 2).reshape(-1)
    return out


def test_flip_transpose_table(H, lib):
    """tem_flip_transpose over a hand-made table: theta = arange (every element identifiable and exact in float32)."""
    rows, total, table = _wtable()
    theta = np.arange(total, dtype=np.float32)
    d_theta = dev(theta)
    out = torch.full((total + 1,), SENT, device="cuda")
    H.run([H.flip_transpose_launch("t", d_theta, out[:total], table, len(rows))])
    got = host(out)
    want = _permuted(theta, rows, flip=True)
    assert want[5 + 26 * 128 + 3 * 8 + 2] == theta[5 + 2 * 16 + 3]             # the header's formula, one element by hand
    assert np.array_equal(got[:total], want) and got[total] == SENT
    out.fill_(SENT)
    H.run([H.flip_transpose_launch("t", d_theta, out[:total], table, 0)])     # nlayers == 0: a plain copy
    got = host(out)
    assert np.array_equal(got[:total], theta) and got[total] == SENT
    assert call(H, lib.tem_flip_transpose, d_theta.data_ptr(), d_theta.data_ptr(), table.data_ptr(), len(rows),
                total) == EINVAL                                              # theta == theta_t
    torch.cuda.synchronize()
    assert np.array_equal(host(d_theta), theta)


def test_pack_weights_bf16_table(H, lib):
    """tem_pack_weights_bf16 over the same table.  theta = arange as far as bf16 tells neighbours apart (multiples of
    1/2 up to 62.5 with the prime period 251, all exact in bf16), then random floats for
    the rounding; theta_h = bf16(theta), theta_ht = the [ci][co] blocks transposed (no tap reversal)."""
    rows, total, table = _wtable()
    rng = np.random.default_rng(6)
    for theta in (((np.arange(total) % 251) - 125).astype(np.float32) * 0.5, rng.standard_normal(total).astype(np.float32)):
        d_theta = dev(theta)
        for nl in (len(rows), 0):                                             # nlayers == 0: a plain cast, twice
            th = torch.full((total + 1,), SENT, dtype=torch.bfloat16, device="cuda")
            tht = torch.full((total + 1,), SENT, dtype=torch.bfloat16, device="cuda")
            H.run([H.pack_weights_launch("t", d_theta, th[:total], tht[:total], table, nl)])
            want_h = torch.from_numpy(theta).to(torch.bfloat16)
            want_ht = torch.from_numpy(_permuted(theta, rows, flip=False) if nl else theta).to(torch.bfloat16)
            assert torch.equal(th.cpu()[:total].view(torch.int16), want_h.view(torch.int16))
            assert torch.equal(tht.cpu()[:total].view(torch.int16), want_ht.view(torch.int16))
            assert float(th[total]) == SENT and float(tht[total]) == SENT
        assert same_bits(host(d_theta), theta)


def test_uint8_round_trip(H, lib):
    """tem_u8_to_f32_std then tem_f32_unstd_to_u8 give back all 256 byte values, for 21 means x 8 stds.  (Checked in
    NumPy for the fused and the two-rounding form of y * std + mean alike: no mismatch, so the 1-LSB allowance the
    kernel's comment grants the oracle comparisons is not needed here.)"""
    u = torch.arange(256, dtype=torch.uint8, device="cuda")
    want = np.arange(256, dtype=np.uint8)
    y = torch.empty((1, 1, 1, 256, 1), dtype=torch.float32, device="cuda")
    back = torch.empty((1, 1, 256), dtype=torch.uint8, device="cuda")
    bad = []
    for mean in np.linspace(-1, 1, 21):
        for std in (0.05, 0.1, 0.3, 0.6, 0.7, 1, 1.7, 2):
            H.u8_to_f32_std(u, y, mean, std)
            back.zero_()
            H.f32_unstd_to_u8(y, back, mean, std)
            got = back.cpu().numpy().reshape(-1)
            if not np.array_equal(got, want):
                bad.append((mean, std, np.flatnonzero(got != want)[:4]))
    assert not bad, bad


def _tie_inputs():
    """float32 v with (v + 1) * 127.5 == k + 0.5 EXACTLY in float32 arithmetic (mean 0, std 1: y * std + mean is v
    in the fused and the two-rounding form alike): the floats next to ((k + 0.5) / 127.5 - 1) for every k."""
    f = np.float32
    k = np.arange(-4, 262)
    v0 = ((k + 0.5) / 127.5 - 1.0).astype(f)
    cand = v0
    for _ in range(3):
        cand = np.concatenate([cand, np.nextafter(cand, f(np.inf)), np.nextafter(cand, f(-np.inf))])
    cand = np.unique(cand)
    q = (cand + f(1.0)) * f(127.5)
    assert q.dtype == f
    tie = (q - np.floor(q)) == f(0.5)
    return cand[tie], q[tie]


def test_uint8_ties_wrap_and_strided_forms(H, lib, oracle_lib):
    """tem_f32_unstd_to_u8 at exact ties (half to even; hundreds of them, even and odd k, ten above 255.5), below -0.5 and above 255.5
    (astype(uint8) wraps, it does not clamp) vs oracle.ops.to_u8; y a crop, out_u8 a transposed and sliced view."""
    v, q = _tie_inputs()
    kk = np.floor(q).astype(int)
    assert v.size >= 21 and (kk % 2 == 0).sum() >= 5 and (kk % 2 == 1).sum() >= 5 and (q > 255.5).sum() >= 5
    rng = np.random.default_rng(12)
    shape = (1, 10, 11, 9, 1)
    y = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    wrap = np.array([-1.0040, -1.0118, -1.2, -3.0, 1.0040, 1.0118, 1.2, 3.1, -1.0, 1.0], np.float32)
    flat = y.reshape(-1)
    flat[:v.size] = v
    flat[v.size:v.size + wrap.size] = wrap
    assert v.size + wrap.size < flat.size
    want = oracle_lib.to_u8(y, (0.0, 1.0))[0, ..., 0]
    lo = (np.float32(wrap[:4]) + 1) * np.float32(127.5)
    assert (lo < -0.5).all() and want.reshape(-1)[v.size] == 0 - 1 + 256       # -0.51 -> -1 -> 255: a wrap, not a clamp
    yf = Framed(shape, fill=y)
    big = torch.full((9 + 3, 11 + 2, 2 * 10 + 1), 77, dtype=torch.uint8, device="cuda")
    out = big[1:10, 2:13, 1::2].permute(2, 1, 0)                               # (10, 11, 9): strides (2, 21, 273)
    assert tuple(out.shape) == (10, 11, 9) and out.stride() == (2, 21, 273)
    H.f32_unstd_to_u8(yf.v, out, 0.0, 1.0)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    rest = big.clone()
    rest[1:10, 2:13, 1::2] = 77
    assert (rest == 77).all() and yf.frame_ok()
