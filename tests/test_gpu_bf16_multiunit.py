"""Small ragged cases that take the branches the full-size bf16 steps take and the batch-2 operator tests do not:

  * bww2d_bf16_k workgroups that own a RUN of (image, band) units (`per` >= 2): accumulators carried across units, the
    next unit prefetched under the current one's matrix work, runs that start and end mid-image;
  * bww_bf16_k z segments of more than one output plane (`zper` >= 2);
  * conv2d_bf16_k / convT2d_bf16_k grids of thousands of workgroups whose count is not a multiple of 8
    (xcd_contiguous_block's remainder branch, the magic-number blockIdx decode);
  * the discriminators' bias gradient, tem_channel_sum / tem_channel_sum_bf16.

Each multi-unit case PROVES its branch from the slab count the library reports (one slab per workgroup): a band has at
most 16 (2-D) / 8 (3-D) output rows, so N * ceil(OH / 16) bounds the units from below, and fewer slabs than that means
some workgroup owns several.  Two routes: shapes whose units exceed the kernel's workgroup budget (256, or 128 for
kernels above 32 KB), and a small shape under a slab budget shrunk through hip_ops.MAX_SLABS.

Oracle and bars as in test_gpu_bf16.py: oracle/torch_ops.py (float64) on bf16-rounded operands, 2e-5 for fp32 slabs, TOL
for bf16 outputs."""
import ctypes as C

import numpy as np
import pytest
import torch

from util import rel_err
from test_gpu_bf16 import TOL, rb, devb, rnd, pack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from transfer_em_amd import hip_ops
    hip_ops.require_gpu()
    return hip_ops


@pytest.fixture(scope="module")
def T():
    from oracle import torch_ops
    return torch_ops


class _P:          # minimal stand-in for a ParamSet
    def __init__(self, shapes):
        self.shapes = shapes
        self.size = {k: int(np.prod(s)) for k, s in shapes.items()}
        self.grad = torch.zeros(sum(self.size.values()), dtype=torch.float32, device="cuda")
        self.theta = self.grad

    def g(self, name):
        off = 0
        for k, n in self.size.items():
            if k == name:
                return self.grad[off:off + n]
            off += n
        raise KeyError(name)


def _bww(H, x, g, shape, k, s, pad, is3d, in1=None):
    ps = _P({"w": shape})
    ws = H.GradWorkspace(ps, 1)
    launch = H.bww_launch("t", x, g, ws, "w", 0, k, s, pad, is3d=is3d, in1=in1)
    H.run([launch] + ws.reduce_launches("t")); torch.cuda.synchronize()
    return ps.grad.cpu().numpy().reshape(shape), launch, launch.args[0]._obj.nslab


def _run2d(H, T, CI, CO, k, s, pad, N, h, w, concat):
    rng = np.random.default_rng(CI * 131 + CO * 7 + k + N + h)
    oh, ow = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    g = rb(rnd(rng, N, 1, oh, ow, CO))
    if concat:                                   # [up | crop(skip)]: two tensors behind one kernel
        c = CI // 2
        up, skip = rb(rnd(rng, N, 1, h, w, c)), rb(rnd(rng, N, 1, h + 3, w + 3, c))
        x = np.concatenate([up, skip[:, :, 1:-2, 1:-2, :]], -1)
        sk = devb(skip)
        x0, in1 = devb(up), H.crop(sk, 1, 2, is3d=False)
    else:
        x = rb(rnd(rng, N, 1, h, w, CI))
        x0, in1 = devb(x), None
    ref = T.conv_bwd_weight(x, g, (1, k, k), (1, s, s), (0, pad, pad))
    got, launch, nslab = _bww(H, x0, devb(g), ref.shape, k, s, pad, False, in1)
    assert launch.meta["kernel"].startswith(f"bww2d_bf16_k<{CI}, {CO}, {k}, {s},"), launch.meta["kernel"]
    e = rel_err(got, ref)
    print(f"bww2d {CI}->{CO} k{k} s{s} p{pad} N={N} O={oh}x{ow}: nslab {nslab}, units >= {N * -(-oh // 16)}, rel_err {e:.2e}")
    return e, nslab, N * -(-oh // 16)


# (CI, CO, k, s, pad, N, H, W, concat): one or more per template family -- C_in == 1, 8/16-channel k3, 32-channel k3
# (budget 128: the 32 -> 32 slab is 36 KB), k4 s2 (budget 128 at 32 channels), the transposed layers' k4 s2 pad 1, concat.
# Bands per image (7, 8 at 16 rows per band) and the unit counts are not multiples of the run length the budget gives,
# so runs start and end inside an image and cross image boundaries.
MULTI2D = [(1, 8, 3, 1, 0, 40, 114, 21, False), (1, 16, 3, 1, 0, 37, 117, 19, False), (8, 8, 3, 1, 0, 40, 114, 23, False),
           (8, 16, 3, 1, 0, 43, 107, 17, False), (16, 16, 3, 1, 0, 41, 103, 17, False), (32, 16, 3, 1, 0, 39, 114, 15, False),
           (32, 32, 3, 1, 0, 20, 114, 13, False), (32, 32, 3, 1, 0, 47, 99, 11, False), (8, 8, 4, 2, 0, 40, 226, 21, False),
           (16, 16, 4, 2, 0, 37, 232, 19, False), (32, 32, 4, 2, 0, 21, 226, 14, False), (8, 16, 4, 2, 1, 40, 224, 22, False),
           (16, 32, 4, 2, 1, 41, 206, 18, False), (16, 16, 3, 1, 0, 40, 114, 19, True), (32, 32, 3, 1, 0, 23, 109, 13, True)]


@pytest.mark.parametrize("CI,CO,k,s,pad,N,h,w,concat", MULTI2D)
def test_kernel_gradient2d_bf16_runs_of_units(H, T, CI, CO, k, s, pad, N, h, w, concat):
    """bww2d_bf16_k with more units than its workgroup budget: every workgroup owns a run (per >= 2)."""
    e, nslab, units_lb = _run2d(H, T, CI, CO, k, s, pad, N, h, w, concat)
    assert nslab < units_lb, (nslab, units_lb)              # fewer workgroups than units: runs of >= 2 units
    assert e < 2e-5


@pytest.mark.parametrize("CI,CO,k,s,pad,N,h,w,concat", [(1, 8, 3, 1, 0, 9, 82, 21, False), (16, 16, 3, 1, 0, 11, 75, 19, False),
                                                        (32, 32, 3, 1, 0, 9, 83, 13, False), (16, 16, 4, 2, 0, 10, 150, 20, False),
                                                        (16, 16, 3, 1, 0, 9, 85, 17, True)])
def test_kernel_gradient2d_bf16_long_runs_under_a_small_slab_budget(H, T, monkeypatch, CI, CO, k, s, pad, N, h, w, concat):
    """The same kernels with the slab budget shrunk to 6: runs of >= 8 units (units > 7 x slabs)."""
    monkeypatch.setattr(H, "MAX_SLABS", 6)
    e, nslab, units_lb = _run2d(H, T, CI, CO, k, s, pad, N, h, w, concat)
    assert nslab <= 6 and units_lb > 7 * nslab, (nslab, units_lb)
    assert e < 2e-5


def _run3d(H, T, CI, CO, k, s, pad, N, dims, concat):
    rng = np.random.default_rng(CI * 31 + CO + k + N + dims[0])
    o = [(d + 2 * pad - k) // s + 1 for d in dims]
    g = rb(rnd(rng, N, *o, CO))
    if concat:
        c = CI // 2
        up, skip = rb(rnd(rng, N, *dims, c)), rb(rnd(rng, N, *[d + 3 for d in dims], c))
        x = np.concatenate([up, skip[:, 1:-2, 1:-2, 1:-2, :]], -1)
        sk = devb(skip)
        x0, in1 = devb(up), H.crop(sk, 1, 2)
    else:
        x = rb(rnd(rng, N, *dims, CI))
        x0, in1 = devb(x), None
    ref = T.conv_bwd_weight(x, g, (k, k, k), s, pad)
    got, launch, nslab = _bww(H, x0, devb(g), ref.shape, k, s, pad, True, in1)
    assert launch.meta["kernel"].startswith(f"bww_bf16_k<{CI}, {CO}, {k}, {s},"), launch.meta["kernel"]
    e = rel_err(got, ref)
    lb = N * -(-o[1] // 8) * o[0]                # (image, band) columns x output planes, bands of at most 8 rows
    print(f"bww {CI}->{CO} k{k} s{s} p{pad} N={N} O={o}: nslab {nslab}, plane units >= {lb}, rel_err {e:.2e}")
    return e, nslab, lb


# (CI, CO, k, s, pad, N, (D, H, W), concat)
MULTI3D = [(8, 8, 3, 1, 0, 2, (39, 35, 21), False), (16, 16, 3, 1, 0, 3, (33, 29, 19), False), (32, 32, 3, 1, 0, 2, (31, 27, 13), False),
           (8, 8, 4, 2, 0, 2, (76, 68, 22), False), (16, 32, 4, 2, 1, 2, (62, 60, 18), False), (16, 16, 3, 1, 0, 2, (37, 34, 17), True)]


@pytest.mark.parametrize("CI,CO,k,s,pad,N,dims,concat", MULTI3D)
def test_kernel_gradient_bf16_z_segments_of_several_planes(H, T, CI, CO, k, s, pad, N, dims, concat):
    """bww_bf16_k with more (column, plane) units than its workgroup budget: z segments of >= 2 planes (zper >= 2)."""
    e, nslab, lb = _run3d(H, T, CI, CO, k, s, pad, N, dims, concat)
    assert nslab < lb, (nslab, lb)
    assert e < 2e-5


@pytest.mark.parametrize("CI,CO,k,s,pad,N,dims,concat", [(8, 8, 3, 1, 0, 2, (27, 14, 19), False), (32, 32, 3, 1, 0, 2, (23, 13, 12), False),
                                                         (16, 16, 4, 2, 0, 2, (50, 26, 20), False), (16, 16, 3, 1, 0, 2, (25, 15, 17), True)])
def test_kernel_gradient_bf16_long_z_segments_under_a_small_slab_budget(H, T, monkeypatch, CI, CO, k, s, pad, N, dims, concat):
    """Slab budget 12: every workgroup marches >= 4 output planes (plane units >= 4 x slabs)."""
    monkeypatch.setattr(H, "MAX_SLABS", 12)
    e, nslab, lb = _run3d(H, T, CI, CO, k, s, pad, N, dims, concat)
    assert nslab <= 12 and lb >= 4 * nslab, (nslab, lb)
    assert e < 2e-5


# ------------------------------------------------------------------------------------------------ rows wider than one band
# A band of one output row must fit the loaders' prefetch registers and the LDS; a pad-0 row that does not is cut into column
# segments of a multiple of 16 output pixels, one launch of the same kernel per segment into its own slab range (run() in
# csrc/bww_bf16.hip and csrc/bww2d_bf16.hip).  Per layer form: the first input width that is segmented (`limit`, from the
# kernels' own arithmetic: K rows x ((OW - 1) S + K) columns x C_in / 8 chunks against 1024 (3-D) / 2048 (2-D) per plane),
# and the width at which the 260 model launches the form (the widest, where it has several).
#         nd ci0 ci1 co  k  s limit model
WIDE = [(3, 8, 8, 16, 3, 1, 171, 228), (3, 16, 0, 32, 3, 1, 171, 108), (3, 32, 0, 16, 3, 1, 86, 116), (3, 16, 16, 32, 3, 1, 86, 118),
        (3, 8, 0, 8, 4, 2, 258, 254), (3, 16, 0, 16, 4, 2, 130, 124), (3, 32, 0, 32, 4, 2, 66, 106),
        (2, 32, 0, 16, 3, 1, 171, 116), (2, 16, 16, 32, 3, 1, 171, 118), (2, 16, 0, 16, 4, 2, 258, 124), (2, 32, 0, 32, 4, 2, 130, 220)]
TOL_SLAB, TOL_SLAB_L2 = 2e-5, 3e-6        # the standing kernel-gradient bars (fullsize_cases.TOL_BF16_SLAB; L2 as for fp32 slabs)


def _wide_operands(rng, nd, ci0, ci1, co, k, s, w):
    """Operands at input width w with the smallest other extents: (x0, skip or None, g) as bf16-rounded numpy arrays.
    A concat form's second half is the crop [1, -2) of `skip`, 3 wider on every cropped axis."""
    N, D, Hh = (2, 6, 10) if nd == 3 else (3, 1, 12)
    od = (D - k) // s + 1 if nd == 3 else 1
    oh, ow = (Hh - k) // s + 1, (w - k) // s + 1
    x0 = rb(rnd(rng, N, D, Hh, w, ci0))
    skip = rb(rnd(rng, N, D + 3 if nd == 3 else 1, Hh + 3, w + 3, ci1)) if ci1 else None
    return x0, skip, rb(rnd(rng, N, od, oh, ow, co))


def _crop_skip(t, nd):
    return t[:, 1:-2, 1:-2, 1:-2, :] if nd == 3 else t[:, :, 1:-2, 1:-2, :]


def _wide_run(H, T, nd, ci0, ci1, co, k, s, x0, skip, g, w, tag):
    """The kernel gradient of the operands cut to input width w -> (float64 slab sum, oracle, slab count, kernel name).
    The slabs land in a NaN-filled allocation one row longer than the query's count: every counted row must come back
    finite and the extra row untouched."""
    from transfer_em_amd import _lib
    lib = _lib.load()
    ow = (w - k) // s + 1
    x0, g = x0[:, :, :, :w, :], g[:, :, :, :ow, :]
    crop1 = None if skip is None else _crop_skip(skip, nd)[:, :, :, :w, :]
    x = x0 if skip is None else np.concatenate([x0, crop1], -1)
    ks, ss = ((k, k, k), (s, s, s)) if nd == 3 else ((1, k, k), (1, s, s))
    ref = T.conv_bwd_weight(x, g, ks, ss, 0)
    t0, tg = devb(x0), devb(g)
    keep = [t0, tg]
    a = _lib.tem_bww_args()
    a.in0, a.dout = H.view(t0), H.view(tg)
    if skip is not None:
        tskip = devb(skip)
        t1 = _crop_skip(tskip, nd)[:, :, :, :w, :]             # a strided view: origin and row pitch are the parent's
        assert not t1.is_contiguous()
        a.in1 = H.view(t1)
        keep.append(tskip)
    a.kd, a.kh, a.kw = ks
    a.sd, a.sh, a.sw = ss
    a.pd = a.ph = a.pw = 0
    a.nslab = H.MAX_SLABS
    name = C.create_string_buffer(96)
    nsl = lib.tem_conv_bwd_weight_bf16_nslab(C.byref(a), name, 96)
    assert nsl >= 1, (tag, w, nsl)
    kern = name.value.decode()
    fam = "bww_bf16_k" if nd == 3 else "bww2d_bf16_k"
    assert kern.startswith(f"{fam}<{ci0 + ci1}, {co}, {k}, {s},"), kern
    slabs = torch.full((nsl + 1, ref.size), float("nan"), device="cuda")
    a.slabs, a.slab_stride, a.nslab, a.accumulate = slabs.data_ptr(), 0, nsl, 0
    rc = lib.tem_conv_bwd_weight_bf16(C.byref(a), H.current_stream())
    assert rc == 0, (tag, w, rc)
    torch.cuda.synchronize()
    host = slabs.cpu().numpy()
    assert np.isfinite(host[:nsl]).all(), (tag, w, "a slab the launch did not write", np.flatnonzero(~np.isfinite(host[:nsl]).all(1)))
    assert np.isnan(host[nsl]).all(), (tag, w, "the launch wrote more slabs than the query counts")
    got = host[:nsl].astype(np.float64).sum(0).reshape(ref.shape)
    e, l2 = rel_err(got, ref), float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print(f"wide {tag} W={w}: {kern} nslab {nsl}, rel_err {e:.2e} l2 {l2:.2e}")
    assert e < TOL_SLAB and l2 < TOL_SLAB_L2, (tag, w, e, l2)
    return got, ref, nsl, kern


@pytest.mark.parametrize("nd,ci0,ci1,co,k,s,limit,model", WIDE,
                         ids=[f"{nd}d-{ci0}{'+' + str(ci1) if ci1 else ''}to{co}-k{k}s{s}" for nd, ci0, ci1, co, k, s, _, _ in WIDE])
def test_kernel_gradient_bf16_rows_wider_than_one_band(H, T, nd, ci0, ci1, co, k, s, limit, model):
    """Each form at limit - 1 (the widest single launch), at limit (the narrowest segmented one) and at the 260 model's
    width, against the float64 oracle on the same bf16-rounded operands; and the single launch against the segmented
    one on operands that make the two sums equal: those of limit - 1, and the same at width limit with the gradient's
    last column -- the only one limit - 1 lacks -- set to zero."""
    tag = f"{nd}d {ci0}+{ci1}->{co} k{k} s{s}"
    rng = np.random.default_rng(1000 * nd + 10 * (ci0 + ci1) + co + k)
    wmax = max(limit, model)
    x0, skip, g = _wide_operands(rng, nd, ci0, ci1, co, k, s, wmax)
    ow = lambda w: (w - k) // s + 1
    assert ow(limit) == ow(limit - 1) + 1
    single, ref1, _, _ = _wide_run(H, T, nd, ci0, ci1, co, k, s, x0, skip, g, limit - 1, tag)
    _wide_run(H, T, nd, ci0, ci1, co, k, s, x0, skip, g, limit, tag)
    if model not in (limit, limit - 1):
        _wide_run(H, T, nd, ci0, ci1, co, k, s, x0, skip, g, model, tag)
    gz = g.copy()
    gz[:, :, :, ow(limit) - 1:, :] = 0
    segmented, _, _, _ = _wide_run(H, T, nd, ci0, ci1, co, k, s, x0, skip, gz, limit, tag + " (last column 0)")
    d = np.abs(single - segmented).max() / np.abs(ref1).max()
    l2 = float(np.linalg.norm(single - segmented) / np.linalg.norm(ref1))
    print(f"wide {tag}: single launch vs segmented on the common width: {d:.2e} l2 {l2:.2e}")
    assert d < TOL_SLAB and l2 < TOL_SLAB_L2, (tag, d, l2)


# ------------------------------------------------------------------------------------------------ large grids
@pytest.mark.parametrize("N", list(range(57, 66)))
@pytest.mark.parametrize("CI,CO,k,s,pad,h,w", [(8, 16, 3, 1, 0, 15, 13), (16, 16, 3, 1, 2, 21, 33), (32, 32, 4, 2, 0, 37, 27),
                                               (1, 8, 3, 1, 0, 35, 29)])
def test_conv2d_bf16_large_grids(H, T, N, CI, CO, k, s, pad, h, w):
    """conv2d_bf16_k decodes blockIdx into (image, band, column block) after xcd_contiguous_block.  Its grid is
    N x patches per image -- a multiple of 8 at N = 64 whatever the plan, so the batch runs through 57 .. 65: nine
    consecutive N give every remainder of the workgroup count modulo 8 its turn (all eight when the patches per image are
    odd), at dividends ~30 x those of the batch-2 tests."""
    rng = np.random.default_rng(N * 17 + CI + h)
    x = rb(rnd(rng, N, 1, h, w, CI))
    wk = rb(rnd(rng, 1, k, k, CI, CO) * float(0.6 / np.sqrt(k * k * CI)))
    ref = T.leaky_relu(T.conv_fwd(x, wk, (1, s, s), (0, pad, pad)))
    out = torch.full(ref.shape, float("nan"), dtype=torch.bfloat16, device="cuda")
    launch = H.conv_launch("t", devb(x), pack(wk), out, k, s, pad, is3d=False, slope=0.3)
    assert launch.meta["kernel"].startswith("conv2d_bf16_k"), launch.meta["kernel"]
    H.run([launch]); torch.cuda.synchronize()
    assert rel_err(out.float().cpu().numpy(), ref) < TOL


@pytest.mark.parametrize("N", list(range(57, 66)))
@pytest.mark.parametrize("CI,CO,h,w,pad", [(16, 8, 9, 11, 1), (32, 16, 17, 13, 1), (8, 8, 23, 10, 0)])
def test_conv_transpose2d_bf16_large_grids(H, T, N, CI, CO, h, w, pad):
    """convT2d_bf16_k: grid N x bands per image, the same decode; odd band counts, batches 57 .. 65."""
    rng = np.random.default_rng(N * 13 + CI + h)
    x = rb(rnd(rng, N, 1, h, w, CI))
    wk = rb(rnd(rng, 1, 4, 4, CO, CI) * float(0.6 / np.sqrt(4 * CI)))
    od = (1, 2 * h + 2 - 2 * pad, 2 * w + 2 - 2 * pad)
    ref = T.leaky_relu(T.convT_fwd(x, wk, (1, 2, 2), (0, pad, pad), out_dims=od))
    out = torch.full(ref.shape, float("nan"), dtype=torch.bfloat16, device="cuda")
    launch = H.conv_launch("t", devb(x), devb(wk.reshape(-1)), out, 4, 2, pad, is3d=False, transposed=True, slope=0.3)
    assert launch.meta["kernel"].startswith("convT2d_bf16_k"), launch.meta["kernel"]
    H.run([launch]); torch.cuda.synchronize()
    assert rel_err(out.float().cpu().numpy(), ref) < TOL


# ------------------------------------------------------------------------------------------------ channel sums
def _bar(rounded, g):
    """One fp32 rounding (2^-23 relative) per rounded quantity, plus the double accumulation of the sum itself."""
    return 2.0 ** -23 * sum(np.abs(r) for r in rounded) + 1e-12 * np.abs(np.asarray(g, np.float64)).reshape(-1, g.shape[-1]).sum(0)


def _views(rng, bf16, C_, is3d):
    """A cropped (strided) view of a larger tensor, batch >= 2: (numpy values, device view)."""
    shape = (2, 11, 13, 15, C_) if is3d else (3, 1, 22, 25, C_)
    a = rnd(rng, *shape) * 3 + 0.25                        # a mean, so the sums do not cancel to ~0
    a = rb(a) if bf16 else a
    t = devb(a) if bf16 else torch.from_numpy(a).cuda()
    sl = (slice(None), slice(2, 9) if is3d else slice(None), slice(1, -3), slice(2, -2), slice(None))
    return a[sl], t[sl]


@pytest.mark.parametrize("is3d", [True, False])
@pytest.mark.parametrize("C_", [1, 8, 32])
@pytest.mark.parametrize("bf16", [False, True])
def test_channel_sum_against_float64(H, T, bf16, C_, is3d):
    """tem_channel_sum / tem_channel_sum_bf16: per-channel sum over batch and voxels of a strided view.  Both kernels
    accumulate in DOUBLE (per thread, across the wave, across the four waves) and round to fp32 once, so the bar is one
    fp32 rounding of the exact sum, |got - ref| <= 2^-23 |ref|, plus 1e-12 sum|g| for the double accumulation (n 2^-53
    sum|g| with n < 10^4).  accumulate = 1 adds the rounded sum to the fp32 value already there: a second rounding, of
    |previous + sum|, joins the bar."""
    from transfer_em_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(C_ + 2 * is3d + bf16)
    a, t = _views(rng, bf16, C_, is3d)
    assert not t.is_contiguous()
    ref = T.channel_sum(a)
    fn = lib.tem_channel_sum_bf16 if bf16 else lib.tem_channel_sum
    v = H.view(t)
    prev = rnd(rng, C_) * 50
    for accumulate in (0, 1):
        out = torch.from_numpy(prev.copy()).cuda()
        H.run([H.Launch(fn, (C.byref(v), out.data_ptr(), accumulate), "channel_sum", [t, out, v])]); torch.cuda.synchronize()
        got = out.cpu().numpy().astype(np.float64)
        want = ref + prev if accumulate else ref
        bar = _bar([ref, want] if accumulate else [ref], a)
        print(f"channel_sum bf16={bf16} C={C_} 3d={is3d} acc={accumulate}: worst error / bar {np.max(np.abs(got - want) / bar):.2f}")
        assert np.all(np.abs(got - want) <= bar), (accumulate, got, want)
    if not bf16:                                           # the fp32 entry point's own launch builder
        out = torch.from_numpy(prev.copy()).cuda()
        H.run([H.channel_sum_launch("t", t, out, accumulate=True)]); torch.cuda.synchronize()
        assert np.all(np.abs(out.cpu().numpy() - (ref + prev)) <= _bar([ref, ref + prev], a))


@pytest.mark.parametrize("is3d", [True, False])
@pytest.mark.parametrize("bf16", [False, True])
def test_bias_gradient_through_grad_workspace(H, T, bf16, is3d):
    """The discriminators' bias gradient as they compute it: bias_grad_launch writes slab 0 of (layer, call) of a
    GradWorkspace -- one call for the real, one for the fake pass -- and the slab reduction sums the two into the
    gradient vector.  Three fp32 roundings: each sum, then their sum."""
    rng = np.random.default_rng(5 + bf16 + 2 * is3d)
    ps = _P({"p2": (1, 1, 1, 32, 1), "p2_bias": (1,)})
    ws = H.GradWorkspace(ps, 2)
    launches, sums, gs = [], [], []
    for call in (0, 1):
        a, t = _views(rng, bf16, 1, is3d)
        launches.append(H.bias_grad_launch("d.bias", t, ws, "p2_bias", call))
        sums.append(T.channel_sum(a)); gs.append(a)
    H.run(launches + ws.reduce_launches("t")); torch.cuda.synchronize()
    got = ps.g("p2_bias").cpu().numpy().astype(np.float64)
    want = sums[0] + sums[1]
    bar = _bar([sums[0], sums[1], want], np.concatenate([g.reshape(-1, 1) for g in gs]))
    print(f"bias gradient bf16={bf16} 3d={is3d}: {got} vs {want}, error / bar {np.max(np.abs(got - want) / bar):.2f}")
    assert np.all(np.abs(got - want) <= bar), (got, want)
