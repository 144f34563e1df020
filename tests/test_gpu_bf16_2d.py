"""bf16 mixed precision for the 2-D networks: conv2d_bf16_k, convT2d_bf16_k and bww2d_bf16_k on (N, 1, H, W, C) views,
and the 2-D train step / inference built on them.

The bars are those of test_gpu_bf16.py (3-D): the oracle evaluated on bf16-rounded operands, TOL for outputs rounded
to bf16 on store, 2e-5 for the fp32 kernel-gradient slabs, and the step thresholds of
test_train_step_bf16_matches_oracle.  Every operator case also checks that the 2-D kernel, not a fallback, ran, and
holds every stored bf16 element to the rounded float64 reference (test_gpu_bf16.stores / bf16_exact.py: 4 x the
sequential float32 sum's error plus four epilogue roundings; at most 10 % of a case's elements next to a tie)."""
import re

import numpy as np
import pytest
import torch

from util import rel_err
from test_gpu_bf16 import TOL, rb, devb, rnd, _inputs, _l2, pm, add_window, stores, T64  # noqa: F401 (T64: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from transfer_em_amd import hip_ops
    hip_ops.require_gpu()
    return hip_ops


def pack2(w):
    """Operator kernel W(1, kh, kw, ci, co) -> packed bf16 [tap][co][ci]."""
    ci, co = w.shape[3:]
    return devb(np.ascontiguousarray(w.reshape(-1, ci, co).transpose(0, 2, 1)).reshape(-1))


def img(rng, n, h, w, c):
    return rb(rnd(rng, n, 1, h, w, c))


def _expect(launch, prefix):
    assert launch.meta["kernel"].startswith(prefix), launch.meta["kernel"]


# forward k3 s1 / k4 s2 (CI, CO, k, s, pad, H, W): the 2-D networks' layers at odd and ragged sizes
FWD2 = [(1, 8, 3, 1, 0, 37, 45), (1, 16, 3, 1, 0, 33, 29), (8, 8, 3, 1, 0, 31, 40), (8, 16, 3, 1, 0, 27, 33),
        (16, 16, 3, 1, 0, 25, 31), (16, 32, 3, 1, 0, 23, 19), (32, 32, 3, 1, 0, 21, 26), (32, 16, 3, 1, 0, 17, 22),
        (16, 1, 3, 1, 0, 29, 35), (8, 8, 4, 2, 0, 35, 41), (16, 16, 4, 2, 0, 27, 30), (32, 32, 4, 2, 0, 19, 23),
        (1, 8, 3, 1, 5, 13, 17), (16, 8, 3, 1, -1, 21, 24)]


def fwd2_launch(H, x, wk, out, k, s, pad, bias=None):
    """The launch of test_conv2d_bf16_forward (test_bf16_exact.py builds it on uninitialised host tensors for its symbol)."""
    return H.conv_launch("t", x, wk, out, k, s, pad, is3d=False, slope=0.3, bias=bias)


@pytest.mark.parametrize("CI,CO,k,s,pad,h,w", FWD2)
def test_conv2d_bf16_forward(H, oracle_lib, T64, CI, CO, k, s, pad, h, w):
    rng = np.random.default_rng(CI * 1000 + CO * 10 + k + h)
    x = img(rng, 2, h, w, CI)
    wk = rb(rnd(rng, 1, k, k, CI, CO) * 0.2)
    bias = rnd(rng, CO) if CO == 1 else None
    xin = x[:, :, -pad:pad, -pad:pad, :] if pad < 0 else x
    ref = oracle_lib.leaky_relu(oracle_lib.conv_fwd(xin, wk, (1, s, s), (0, max(pad, 0), max(pad, 0)), bias))
    out = torch.empty(ref.shape, dtype=torch.bfloat16, device="cuda")
    launch = fwd2_launch(H, devb(x), pack2(wk), out, k, s, pad, torch.from_numpy(bias).cuda() if bias is not None else None)
    H.run([launch])
    _expect(launch, "conv2d_bf16_k")
    assert rel_err(out.float().cpu().numpy(), ref) < TOL
    stores(f"2-D forward {CI}->{CO} k{k} s{s} p{pad} {h}x{w}", out,
           pm(T64.conv_fwd, (xin, wk), (1, s, s), (0, max(pad, 0), max(pad, 0)), bias), k * k * CI, slope=0.3)


# input-gradients of the k3 s1 layers (flipped taps, pad 2), gated unless they produce the one-channel image gradient
# (the networks' dx): (forward CI, forward CO, H, W of the gradient)
BWD2 = [(1, 8, 35, 41), (1, 16, 31, 27), (16, 1, 33, 29), (8, 8, 29, 36), (8, 16, 25, 31), (16, 16, 23, 27),
        (16, 32, 21, 19), (32, 16, 19, 23), (32, 32, 17, 21)]


@pytest.mark.parametrize("FCI,FCO,h,w", BWD2)
def test_conv2d_bf16_input_gradient(H, oracle_lib, T64, FCI, FCO, h, w):
    rng = np.random.default_rng(FCI * 100 + FCO + h)
    g = img(rng, 2, h, w, FCO)
    wf = rb(rnd(rng, 1, 3, 3, FCI, FCO) * 0.2)                # Keras forward kernel (tap, ci, co)
    shape = (2, 1, h + 2, w + 2, FCI)
    full = oracle_lib.conv_bwd_data(g, wf, shape, 1, 0)
    saved = img(rng, 2, h + 2, w + 2, FCI) if FCI > 1 else None
    ref = oracle_lib.leaky_relu_grad_from_out(full, saved) if FCI > 1 else full
    out = torch.empty(shape, dtype=torch.bfloat16, device="cuda")
    launch = H.conv_launch("t", devb(g), devb(wf.reshape(-1)), out, 3, 1, 2, is3d=False, layout=H.TEM_W_FLIP_CO_CI,
                           gate=devb(saved) if FCI > 1 else None, bwd_data=True)
    H.run([launch])
    _expect(launch, "conv2d_bf16_k")
    assert rel_err(out.float().cpu().numpy(), ref) < TOL
    stores(f"2-D input gradient of {FCI}->{FCO} {h}x{w}", out, pm(T64.conv_bwd_data, (g, wf), shape, 1, 0), 9 * FCO, saved=saved)


@pytest.mark.parametrize("CI,CO", [(8, 16), (16, 32)])
def test_conv2d_bf16_k4s2_over_convT_gradient(H, oracle_lib, T64, CI, CO):
    """Input-gradient of the Conv2DTranspose layers u1b (16 -> 8) and u2b (32 -> 16): a k4 s2 pad-1 convolution
    CI -> CO over the output gradient, gated by the saved input of the layer."""
    rng = np.random.default_rng(CI + CO)
    for n_in in (13, 10):
        g = img(rng, 2, 2 * n_in, 2 * n_in + 2, CI)
        wT = rb(rnd(rng, 1, 4, 4, CI, CO) * 0.1)               # Keras Conv2DTranspose kernel (tap, CO_T = CI, CI_T = CO)
        ref_full = oracle_lib.conv_fwd(g, wT, (1, 2, 2), (0, 1, 1))
        saved = rb(rnd(rng, *ref_full.shape))
        ref = oracle_lib.leaky_relu_grad_from_out(ref_full, saved)
        out = torch.empty(ref.shape, dtype=torch.bfloat16, device="cuda")
        launch = H.conv_launch("t", devb(g), pack2(wT), out, 4, 2, 1, is3d=False, gate=devb(saved))
        H.run([launch])
        _expect(launch, "conv2d_bf16_k")
        assert rel_err(out.float().cpu().numpy(), ref) < TOL, n_in
        stores(f"2-D k4 s2 p1 gated {CI}->{CO} n{n_in}", out, pm(T64.conv_fwd, (g, wT), (1, 2, 2), (0, 1, 1)), 16 * CI, saved=saved)


CONVT2 = [(8, 8), (16, 16), (32, 32)]
CONVT2_WINDOWS = ((9, 11, 1, 0, 18), (7, 8, 1, 3, 9), (6, 9, 0, 2, 11))       # (h, w, pad, window origin, window edge)


def convT2_launch(H, x, w, out, pad, gate, add):
    """The launch of test_conv_transpose2d_bf16_add_gate (and of test_bf16_exact.py, on host tensors, for its symbol)."""
    return H.conv_launch("t", x, w, out, 4, 2, pad, is3d=False, transposed=True, gate=gate, add=add, add_off=1)


@pytest.mark.parametrize("CI,CO", CONVT2)
def test_conv_transpose2d_bf16_add_gate(H, oracle_lib, T64, CI, CO):
    """k4 s2 transposed convolution on convT2d_bf16_k: shifted windows, skip-gradient add + gate (the input-gradients of
    the k4 s2 layers), batch 2."""
    rng = np.random.default_rng(CI * 3 + CO)
    w = rb(rnd(rng, 1, 4, 4, CO, CI) * 0.1)
    for h, wd, pad, lo, osz in CONVT2_WINDOWS:
        x = img(rng, 2, h, wd, CI)
        full = oracle_lib.convT_fwd(x, w, (1, 2, 2), (0, pad, pad), out_dims=(1, 2 * h + 2 - 2 * pad, 2 * wd + 2 - 2 * pad))
        win = full[:, :, lo:lo + osz, lo:lo + osz, :]
        saved = rb(rnd(rng, *win.shape))
        addw = rb(rnd(rng, 2, 1, osz - 2, osz - 2, CO))
        ref = win.copy()
        ref[:, :, 1:-1, 1:-1, :] += addw
        ref = oracle_lib.leaky_relu_grad_from_out(ref, saved)
        out = torch.empty(ref.shape, dtype=torch.bfloat16, device="cuda")
        launch = convT2_launch(H, devb(x), devb(w.reshape(-1)), out, pad + lo, devb(saved), devb(addw))
        H.run([launch])
        _expect(launch, "convT2d_bf16_k")
        assert rel_err(out.float().cpu().numpy(), ref) < TOL, (h, wd, pad, lo, osz)
        pre, mag = pm(T64.convT_fwd, (x, w), (1, 2, 2), (0, pad, pad), (1, 2 * h + 2 - 2 * pad, 2 * wd + 2 - 2 * pad))
        cut = np.s_[:, :, lo:lo + osz, lo:lo + osz, :]
        stores(f"2-D convT {CI}->{CO} {h}x{wd} p{pad} window {lo}+{osz}", out,
               add_window((pre[cut].copy(), mag[cut].copy()), addw, np.s_[:, :, 1:-1, 1:-1, :]), 16 * CI, saved=saved)


@pytest.mark.parametrize("CI,CO", [(32, 16), (16, 8)])
def test_conv_transpose2d_bf16_dropout_then_concat_split(H, oracle_lib, T64, CI, CO):
    """u2b / u1b in 2-D: the transposed convolution draws the Dropout keep bits in its epilogue and writes the mask
    (keep_mode 1, the oracle's Philox bits); the input-gradient of the consuming conv over concat([up, crop(skip)])
    splits its output CO | CO, gates and drops the first half reading that mask (keep_mode 2) or drawing it again --
    the same elements either way; and the forward conv over the concat."""
    rng = np.random.default_rng(CI + CO)
    h, wd = 11, 13
    x = img(rng, 2, h, wd, CI)
    w = rb(rnd(rng, 1, 4, 4, CO, CI) * 0.1)
    shape = (2, 1, 2 * h, 2 * wd, CO)
    c = oracle_lib.convT_fwd(x, w, (1, 2, 2), (0, 1, 1), out_dims=shape[1:4])
    keep = oracle_lib.dropout_mask(shape, 42, 5, 2)
    ref_fwd = oracle_lib.leaky_relu(c * keep.astype(np.float32) * 2)
    out = torch.empty(shape, dtype=torch.bfloat16, device="cuda")
    mask = torch.zeros(int(np.prod(shape)) // 8, dtype=torch.uint8, device="cuda")
    step = torch.tensor([2], dtype=torch.int32, device="cuda")
    launch = H.conv_launch("t", devb(x), devb(w.reshape(-1)), out, 4, 2, 1, is3d=False, transposed=True, slope=0.3,
                           dropout=(42, 5, step), keep_mask=(mask, 1))
    H.run([launch])
    _expect(launch, "convT2d_bf16_k")
    assert np.array_equal(np.unpackbits(mask.cpu().numpy(), bitorder="little").astype(bool), keep.reshape(-1))
    assert rel_err(out.float().cpu().numpy(), ref_fwd) < TOL
    stores(f"2-D convT {CI}->{CO} dropout + LeakyReLU", out, pm(T64.convT_fwd, (x, w), (1, 2, 2), (0, 1, 1), shape[1:4]),
           16 * CI, keep=keep, slope=0.3)
    # input-gradient of the 2 CO -> CC k3 conv over concat([up, skip])
    CC = 2 * CO
    g = img(rng, 2, 2 * h - 2, 2 * wd - 2, CC)
    wf = rb(rnd(rng, 1, 3, 3, 2 * CO, CC) * 0.1)
    full = oracle_lib.conv_bwd_data(g, wf, (2, 1, 2 * h, 2 * wd, 2 * CO), 1, 0)
    up = out.float().cpu().numpy()
    ref0 = oracle_lib.leaky_relu_grad_from_out(full[..., :CO], up) * keep.astype(np.float32) * 2
    ref1 = full[..., CO:]
    res = []
    for km in (None, (mask, 2)):
        d0 = torch.empty(shape, dtype=torch.bfloat16, device="cuda")
        d1 = torch.empty(shape, dtype=torch.bfloat16, device="cuda")
        launch = H.conv_launch("t", devb(g), devb(wf.reshape(-1)), d0, 3, 1, 2, is3d=False, layout=H.TEM_W_FLIP_CO_CI,
                               out1=d1, gate=out, dropout=(42, 5, step), keep_mask=km)
        H.run([launch])
        _expect(launch, "conv2d_bf16_k")
        res.append((d0.float().cpu().numpy(), d1.float().cpu().numpy()))
    assert np.array_equal(res[0][0] == 0, res[1][0] == 0)
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert rel_err(res[0][0], ref0) < TOL and rel_err(res[0][1], ref1) < TOL
    pre, mag = pm(T64.conv_bwd_data, (g, wf), (2, 1, 2 * h, 2 * wd, 2 * CO), 1, 0)
    stores(f"2-D split {CC}->{CO}|{CO} gate + dropout", res[0][0], (pre[..., :CO], mag[..., :CO]), 9 * CC, saved=up, keep=keep)
    stores(f"2-D split {CC}->{CO}|{CO} plain half", res[0][1], (pre[..., CO:], mag[..., CO:]), 9 * CC)
    # forward conv over [up | crop(skip)]
    skip = img(rng, 2, 2 * h + 3, 2 * wd + 3, CO)
    cat = np.concatenate([up, skip[:, :, 1:-2, 1:-2, :]], -1)
    ref = oracle_lib.leaky_relu(oracle_lib.conv_fwd(cat, wf))
    o2 = torch.empty(ref.shape, dtype=torch.bfloat16, device="cuda")
    sk = devb(skip)
    launch = H.conv_launch("t", out, pack2(wf), o2, 3, in1=H.crop(sk, 1, 2, is3d=False), is3d=False, slope=0.3)
    H.run([launch])
    _expect(launch, "conv2d_bf16_k")
    assert rel_err(o2.float().cpu().numpy(), ref) < TOL
    stores(f"2-D concat [up | crop(skip)] {CC}->{CC}", o2, pm(T64.conv_fwd, (cat, wf), 1, 0), 9 * CC, slope=0.3)


# kernel gradients (CI, CO, k, s, pad, H, W of the input)
BWW2 = [(1, 8, 3, 1, 0, 40, 37), (1, 16, 3, 1, 0, 35, 30), (8, 8, 3, 1, 0, 33, 45), (8, 16, 3, 1, 0, 31, 26),
        (16, 8, 3, 1, 2, 27, 22), (16, 16, 3, 1, 0, 29, 37), (16, 32, 3, 1, 0, 25, 23), (32, 16, 3, 1, 0, 21, 26),
        (32, 32, 3, 1, 0, 19, 22), (8, 8, 4, 2, 0, 37, 30), (16, 16, 4, 2, 0, 27, 33), (32, 32, 4, 2, 0, 21, 19),
        (8, 16, 4, 2, 1, 26, 28), (16, 32, 4, 2, 1, 20, 22), (1, 8, 3, 1, 4, 15, 19), (16, 16, 3, 1, 0, 131, 129)]


@pytest.mark.parametrize("CI,CO,k,s,pad,h,w", BWW2)
def test_kernel_gradient2d_bf16(H, oracle_lib, CI, CO, k, s, pad, h, w):
    rng = np.random.default_rng(CI * 7 + CO + k + h)
    x = img(rng, 2, h, w, CI)
    oh, ow = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    g = img(rng, 2, oh, ow, CO)
    ref = oracle_lib.conv_bwd_weight(x, g, (1, k, k), (1, s, s), (0, pad, pad))
    got, _, launch = _bww2d(H, devb(x), devb(g), ref.shape, k, s, pad)
    assert launch.meta["kernel"].startswith("bww2d_bf16_k"), launch.meta["kernel"]
    assert rel_err(got, ref) < 2e-5, launch.meta["kernel"]


class _P:          # minimal stand-in for a ParamSet: one layer "w"
    def __init__(self, shape):
        self.shapes = {"w": shape}
        self.grad = torch.zeros(int(np.prod(shape)), dtype=torch.float32, device="cuda")
        self.theta = self.grad

    def g(self, name):
        return self.grad


def _bww2d(H, x, g, shape, k, s=1, pad=0, in1=None):
    ps = _P(shape)
    ws = H.GradWorkspace(ps, 1)
    launch = H.bww_launch("t0", x, g, ws, "w", 0, k, s, pad, is3d=False, in1=in1)
    H.run([launch] + ws.reduce_launches("t"))
    return ps.grad.cpu().numpy().reshape(shape), ws, launch


def test_kernel_gradient2d_bf16_concat_swapped_and_transposed(H, oracle_lib):
    rng = np.random.default_rng(11)
    # 8 + 8 and 16 + 16 concats (f1, mid)
    for c in (8, 16):
        up, skip = img(rng, 2, 19, 23, c), img(rng, 2, 22, 26, c)
        g = img(rng, 2, 17, 21, 2 * c)
        ref = oracle_lib.conv_bwd_weight(np.concatenate([up, skip[:, :, 1:20, 1:24]], -1), g, (1, 3, 3))
        sk = devb(skip)
        got, _, launch = _bww2d(H, devb(up), devb(g), ref.shape, 3, in1=H.crop(sk, 1, 2, is3d=False))
        assert launch.meta["kernel"].startswith("bww2d_bf16_k"), launch.meta["kernel"]
        assert rel_err(got, ref) < 2e-5, c
    # C_out == 1 (f2): bww_launch swaps the roles (pd = 0, ph = pw = 2 in 2-D)
    x = img(rng, 2, 27, 31, 16)
    g = img(rng, 2, 25, 29, 1)
    ref = oracle_lib.conv_bwd_weight(x, g, (1, 3, 3))
    got, ws, launch = _bww2d(H, devb(x), devb(g), ref.shape, 3)
    assert ws.flip_rows.get("w") == 16 and launch.args[0]._obj.ph == 2 and launch.args[0]._obj.pd == 0
    assert launch.meta["kernel"].startswith("bww2d_bf16_k<1, 16"), launch.meta["kernel"]
    assert rel_err(got, ref) < 2e-5
    # Conv2DTranspose layers (u2b, u1b): roles swapped, k4 s2 pad 1
    for ci_t, co_t in ((32, 16), (16, 8)):
        xt = img(rng, 2, 9, 11, ci_t)
        gy = img(rng, 2, 18, 22, co_t)
        refT = oracle_lib.convT_bwd_weight(xt, gy, (1, 4, 4), (1, 2, 2), (0, 1, 1))
        got, _, launch = _bww2d(H, devb(gy), devb(xt), refT.shape, 4, 2, 1)
        assert launch.meta["kernel"].startswith("bww2d_bf16_k"), launch.meta["kernel"]
        assert rel_err(got, refT) < 2e-5, (ci_t, co_t)


def test_dropout_keep_masks_fp32_equal_bf16_2d():
    """The fp32 and bf16 2-D generator forwards with one seed, call site and step drop the same activations of u2b / u1b:
    byte-identical keep masks."""
    from transfer_em_amd.models.generator import UNetGenerator, GenForward
    net = UNetGenerator(74, is3d=False, seed=5)
    x = torch.from_numpy(_inputs((2, 1, 74, 74, 1), 7)).cuda()
    step = torch.tensor([3], dtype=torch.int32, device="cuda")
    masks = []
    for dtype in (torch.float32, torch.bfloat16):
        f = GenForward(net, x.to(dtype).contiguous(), training=True, drop=(42, 1, step), pack=True)
        f.run()
        torch.cuda.synchronize()
        masks.append([f.keep[b].cpu().numpy() for b in (0, 1)])
        if dtype == torch.bfloat16:
            kern = [l.meta.get("kernel", "") for l in f.launches]
            assert sum(k.startswith("convT2d_bf16_k") for k in kern) == 2, kern
    for a, b in zip(*masks):
        assert a.any() and np.array_equal(a, b)


def test_generator_inference_bf16_2d(oracle_lib):
    """The 2-D twin of test_generator_inference_bf16: generator_g at 74^2 in bf16 (dropout off) against the oracle
    rounding at the same storage points."""
    from oracle import graph
    from transfer_em_amd.models.generator import unet_generator
    from util import scaled_params
    model, out = unet_generator(74, is3d=False)
    P = scaled_params(graph.generator_param_shapes(False), 3)
    model.params.load_dict(P)
    x = _inputs((2, 1, 74, 74, 1), 99)
    y = model(torch.from_numpy(x).to(torch.bfloat16)).float().cpu().numpy()
    plan = model.plan((2, 1, 74, 74, 1), torch.bfloat16)
    kern = [l.meta.get("kernel", "") for l in plan.launches if "kernel" in l.meta]
    assert all(k.startswith(("conv2d_bf16_k", "convT2d_bf16_k")) for k in kern), kern
    with graph.precision("bf16"):
        ref, _ = graph.generator_forward(P, graph.round_bf16(x), False, training=False)
    assert y.shape == (2, 1, 40, 40, 1)
    print("bf16 2-D generator: max-rel", rel_err(y, ref), "l2", _l2(y, ref))
    assert rel_err(y, ref) < 2e-2 and _l2(y, ref) < 5e-3
    y32 = model(torch.from_numpy(x)).cpu().numpy()
    assert 1e-4 < _l2(y, y32) < 3e-2


def _step_bf16_2d_matches_oracle(tmp_path, n, batch, amplitude=1.0):
    """EM2EM(n, is3d=False, precision='bf16').train_step at `batch` against the oracle's bf16 storage mode with the HIP
    forward's LeakyReLU branches (util.hip_gates): the thresholds of test_train_step_bf16_matches_oracle.  amplitude
    scales the two input images; an instance that scales them claims to stay clear of the pole of the cycle / identity
    terms and is held to that, as in test_gpu_step._step_matches_oracle."""
    from oracle import graph
    from transfer_em_amd.cgan import EM2EM
    from test_gpu_step import _load, _pole_margin, _state
    from util import activation_stats, hip_gates
    shape = (batch, 1, n, n, 1)
    rx, ry = np.float32(amplitude) * _inputs(shape, 1234), np.float32(amplitude) * _inputs(shape, 5678)
    st = _state(graph, False, True)
    model = EM2EM(n, "bf16_2d", is3d=False, seed=42, checkpoint_root=str(tmp_path), precision="bf16")
    _load(model, st)
    got = model.train_step(torch.from_numpy(rx), torch.from_numpy(ry)).cpu().numpy()
    cs = model._steps[batch]
    grads_hip = {k: net.params.to_dict("grad") for k, net in zip(("g", "f", "dx", "dy"), model._nets)}
    with graph.precision("bf16"):
        losses, grads, aux = graph.train_step(st, rx, ry, False, 2.0, 42, gates=hip_gates(cs, False))
    flips, total, worst_act, where = activation_stats(cs, aux["saved"], False)
    print("bf16 2-D step losses", got, losses, f"flips {flips} of {total}, worst activation error {worst_act:.1e} at {where}")
    assert worst_act < 2e-2 and flips < 5e-3 * total, (worst_act, where, flips, total)
    assert rel_err(got, losses) < 5e-3, (got, losses)
    b = model.buffer
    crop = lambda t: t[:, :, b:-b, b:-b, :]
    if amplitude != 1.0:
        margin = _pole_margin(aux, rx, ry, b, lambda t, c: t[:, :, c:-c, c:-c, :])
        print(f"smallest 1 - |a - b| / 2 of the cycle / identity terms (oracle, bf16 storage mode): {margin:.3g}")
        assert margin >= 0.05, margin
    for key, plan in (("fake_y", "g1"), ("cyc_x", "f2"), ("fake_x", "f1"), ("cyc_y", "g2"), ("same_x", "f3"), ("same_y", "g3")):
        ref = crop(aux[key]) if key.startswith("cyc") else aux[key]
        e = _l2(cs.fwd[plan].y.float().cpu().numpy(), ref)
        assert e < 1e-2, (key, e)
    worst = 0.0
    for net in ("g", "f", "dx", "dy"):
        for name, ref in grads[net].items():
            if name.endswith("_bias"):
                continue
            e = _l2(grads_hip[net][name], ref)
            worst = max(worst, e)
            assert e < 4e-2, (net, name, e)
    print("bf16 2-D step: worst kernel-gradient L2 error", worst)
    for net, obj in zip(("g", "f", "dx", "dy"), model._nets):
        m = obj.params.to_dict("m")
        for name, ref in st["m"][net].items():
            if not name.endswith("_bias"):
                assert _l2(m[name], ref) < 4e-2, (net, name)
    assert model.generator_g.params.theta.dtype == torch.float32
    # every spatial convolution of the step ran on the 2-D bf16 kernels (the 1x1 head stays on the 1x1x1 ones)
    kern = {l.meta["kernel"] for p in list(cs.fwd.values()) + list(cs.bwd.values()) for l in p.launches
            if l.meta.get("kernel", "").startswith(("conv", "bww"))}
    assert all(k.startswith(("conv2d_bf16_k", "convT2d_bf16_k", "bww2d_bf16_k")) or
               re.match(r"(conv|bww)_bf16_k<\d+, \d+, 1, 1,", k) for k in kern), kern


def test_train_step_bf16_2d_matches_oracle(tmp_path, oracle_lib):
    _step_bf16_2d_matches_oracle(tmp_path, 74, 2)


def test_train_step_bf16_2d_notebook_config_matches_oracle(tmp_path, oracle_lib):
    """The reference's training example at its own size, 132^2 batch 64, with every assertion and bar of the 74^2
    instance: the only check of the bf16 step's gradients, moments and activations at the configuration users run."""
    _step_bf16_2d_matches_oracle(tmp_path, 132, 64)


def test_train_step_bf16_2d_260_matches_oracle(tmp_path, oracle_lib):
    """The largest compatible size, 260^2 at batch 1, with every assertion and bar of the 74^2 instance: the discriminators'
    32 -> 32 k4 s2 kernel gradient at 220^2 is the one 2-D launch whose row is wider than one band (cut into column
    segments, csrc/bww2d_bf16.hip).  Half amplitude keeps the oracle's 1 - |a - b| / 2 at 0.37 (asserted >= 0.05); at
    amplitude 1 it crosses the pole with these weights."""
    _step_bf16_2d_matches_oracle(tmp_path, 260, 1, amplitude=0.5)


def test_train_step_bf16_2d_notebook_config(tmp_path):
    """The reference's training example at its own size: 2-D 132^2, batch 64.  The multi-stream and single-stream bf16
    steps are bit-identical, everything is finite, the 7 losses agree with the fp32 2-D step of the same weights, inputs
    and dropout stream to 5e-3, and graph replay equals eager."""
    from oracle import graph
    from transfer_em_amd.cgan import EM2EM
    from test_gpu_step import _load, _state
    shape = (64, 1, 132, 132, 1)
    rx, ry = torch.from_numpy(_inputs(shape, 1234)), torch.from_numpy(_inputs(shape, 5678))
    st = _state(graph, False, True)
    runs = {}
    for tag, prec, streams, use_graph in (("bf16", "bf16", True, False), ("bf16_1s", "bf16", False, False),
                                          ("bf16_graph", "bf16", True, True), ("fp32", "fp32", True, False)):
        model = EM2EM(132, tag, is3d=False, seed=42, checkpoint_root=str(tmp_path), precision=prec, two_streams=streams,
                      use_graph=use_graph)
        _load(model, st)
        steps = 3 if use_graph else 1                 # graph: capture + replay, replay
        losses = np.stack([model.train_step(rx, ry).cpu().numpy() for _ in range(steps)])
        assert np.isfinite(losses).all(), (tag, losses)
        theta = torch.cat([net.params.theta for net in model._nets]).cpu().numpy()
        assert np.isfinite(theta).all(), tag
        if use_graph:
            assert model._steps[64].graphs is not None
            # eager reference for the same three steps
            ref = EM2EM(132, tag + "_eager", is3d=False, seed=42, checkpoint_root=str(tmp_path), precision=prec,
                        two_streams=streams, use_graph=False)
            _load(ref, st)
            ref_losses = np.stack([ref.train_step(rx, ry).cpu().numpy() for _ in range(steps)])
            ref_theta = torch.cat([net.params.theta for net in ref._nets]).cpu().numpy()
            assert np.array_equal(losses, ref_losses) and np.array_equal(theta, ref_theta)
            del ref
        runs[tag] = (losses[0], theta)
        del model
        torch.cuda.empty_cache()
    assert np.array_equal(runs["bf16"][0], runs["bf16_1s"][0]) and np.array_equal(runs["bf16"][1], runs["bf16_1s"][1])
    print("132^2 x 64 losses bf16", runs["bf16"][0], "fp32", runs["fp32"][0])
    assert rel_err(runs["bf16"][0], runs["fp32"][0]) < 5e-3


@pytest.mark.parametrize("is3d", [False, True])
def test_bf16_with_disc_prior_raises(tmp_path, is3d):
    from transfer_em_amd.cgan import EM2EM
    with pytest.raises(RuntimeError, match="disc_prior"):
        EM2EM(74, "prior", is3d=is3d, checkpoint_root=str(tmp_path), precision="bf16", disc_prior=object())
