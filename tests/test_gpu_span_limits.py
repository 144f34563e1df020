"""The convolution kernels at their span limits, executed: every row of tests/span_cases.LIMITS, fp32 and bf16, operands
and keep-bit frames, is launched just below its limit and just at or above it, and the 64-bit kernels behind the limits past 2^31 (2^32) elements.

Per launch:
* the kernel symbol is the family's below the limit and the fallback's at it (the dry query the launch is built from;
  for convT_direct_k and bww_mfma_k, which no query names, the check is only that no tiled kernel took the launch:
  span_cases.route);
* the result is held to the float64 oracle on the compact operands, with the bar the same family has in test_gpu_ops
  (2e-5 of scale), test_gpu_wino (2e-6 x 3 of scale forward, 6e-6 gated, 3e-6 for the kernel gradient);
* where the dense placement of the same operands runs the same kernel symbol, the two results are equal bit for bit (no
  kernel here orders its sums by stride: a stride enters addresses only);
* the stretched operand lies behind head room in one allocation that starts as a NaN sentinel: after the launch every
  element of a stretched output's allocation outside the view still holds the sentinel and every element inside is
  finite; a stretched input's surroundings are the same NaN, so a read beside the view poisons the result.

The head room is min(span, 2^31) elements: a true in-view offset truncated to 32 bits (element or byte, signed or
unsigned) still lands inside the allocation, so a kernel with wrong address arithmetic fails here, it does not fault.
A case needs at most 16 GiB (24 GiB at 2^32); one that does not fit the free memory skips with the two numbers.
No case is meant to see a kernel leave its view: the limits were audited first."""
import ctypes as C

import numpy as np
import pytest
import torch

from span_cases import GEOM, LIMITS, Case, Row, dense, extents, frame_intact, framed, head_room, out_dims, route, span
from util import rel_err

pytestmark = pytest.mark.gpu
TOL = 2e-5                                      # test_gpu_ops.TOL; kernel gradients of bf16 inputs as well (test_gpu_bf16)
TOL_H = 6e-3                                    # test_gpu_bf16.TOL: bf16 outputs
FP32_ROWS = [r for r in LIMITS if GEOM[r.geom]["esz"] == 4]
BF16_ROWS = [r for r in LIMITS if GEOM[r.geom]["esz"] == 2]

# the kernels without a span limit (64-bit strides), one stretched operand each at 2^31 + d elements; conv_direct_k and
# conv_rows_k once with out0 at 2^32 + d.  (kernel, geometry, operand, elements)
GEOM.update({
    "d_direct": dict(GEOM["lds"], gate=True, slope=1.0),                                     # conv_direct_k<16, 0, 32, 0>
    "d_rows": dict(GEOM["lds"], ci=8, co=8, dims=(6, 18, 12)),                                # conv_rows_k: output height 16
    "d_convT": dict(GEOM["convT_bd"], add=False),                                            # convT_direct_k<8, 8, 0>
    "d_bwwlds": dict(GEOM["bs2"], k=3, s=1, dims=(10, 12, 14)),                               # bww_lds_k 16 -> 16
    "d_bwwmfma": dict(GEOM["bs2"], ci=32, co=32, k=1, s=1, dims=(5, 6, 7)),                   # bww_mfma_k: the 1x1x1 layers
})
B31, B32 = (1 << 31) + 4096, (1 << 32) + 4096      # span = this or a grid step more: the last image's offsets cross the power of two
DIRECT64 = [Row("64-bit", k, g, o, "view", n, "image", k, "no limit: 64-bit strides")
            for k, g, o, n in [("conv_direct_k", "d_direct", "in0", B31), ("conv_direct_k", "d_direct", "out0", B31),
                               ("conv_direct_k", "d_direct", "gate", B31), ("conv_direct_k", "d_direct", "out0", B32),
                               ("conv_rows_k", "d_rows", "in0", B31), ("conv_rows_k", "d_rows", "out0", B31),
                               ("conv_rows_k", "d_rows", "out0", B32),
                               ("convT_direct_k", "d_convT", "in0", B31), ("convT_direct_k", "d_convT", "out0", B31),
                               ("convT_direct_k", "d_convT", "gate", B31),
                               ("bww_lds_k", "d_bwwlds", "in0", B31), ("bww_lds_k", "d_bwwlds", "dout", B31),
                               ("bww_mfma_k", "d_bwwmfma", "in0", B31), ("bww_mfma_k", "d_bwwmfma", "dout", B31)]]


@pytest.fixture(scope="module")
def lib():
    from transfer_em_amd import hip_ops
    return hip_ops.require_gpu()


# ------------------------------------------------------------------------------------------------ operands and oracle
_DATA = {}


def _data(gname, N):
    """compact operands of geometry `gname` at batch N and their float64-oracle result, computed once"""
    key = (gname, N)
    if key in _DATA:
        return _DATA[key]
    from oracle import ops as O
    O.build()
    g = GEOM[gname]
    rng = np.random.default_rng(sum(map(ord, gname)) + N)
    ext = extents(g)
    bf = g["esz"] == 2                  # bf16: the oracle gets the values the bf16 tensors hold
    rb = (lambda a: torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()) if bf else (lambda a: a)
    d = {o: rb(rng.standard_normal((N,) + e).astype(np.float32)) for o, e in ext.items() if not o.startswith("out")}
    k, ci, co = g["k"], g["ci"] + g["ci1"], g["co"] + g["co1"]
    k3, s, p = ((k,) * 3, (g["s"],) * 3, (g["p"],) * 3) if g["is3d"] else ((1, k, k), (1, g["s"], g["s"]), (0, g["p"], g["p"]))
    x = np.concatenate([d["in0"], d["in1"]], -1) if g["ci1"] else d["in0"]
    if g["entry"].startswith("bww"):
        ref = O.conv_bwd_weight(x, d["dout"], k3, s, p)
        _DATA[key] = (d, None, ref, None)
        return _DATA[key]
    if g["entry"].startswith("convT"):
        w = rb((rng.standard_normal(k3 + (co, ci)) * 0.1).astype(np.float32))                  # Keras (tap, CO, CI)
        raw = O.convT_fwd(x, w, s, p)
    elif g["flip"]:        # the input-gradient of a co -> ci layer, whose kernel (tap, co, ci) is read flipped / transposed
        w = (rng.standard_normal(k3 + (co, ci)) * 0.1).astype(np.float32)
        raw = O.conv_fwd(x, np.ascontiguousarray(np.flip(w, (0, 1, 2)).transpose(0, 1, 2, 4, 3)), s, p)
    else:
        w = rb((rng.standard_normal(k3 + (ci, co)) * 0.1).astype(np.float32))
        raw = O.conv_fwd(x, w, s, p)
    assert raw.shape == (N,) + out_dims(g) + (co,), (raw.shape, out_dims(g))
    keep = None
    if g["keep"]:          # the bits of the Philox stream the argument struct names: a kernel that draws them agrees with one that reads them
        keep = O.dropout_mask((N,) + out_dims(g) + (g["co"],), 42, 3, 7)
        d["keep"] = np.packbits(keep.reshape(-1), bitorder="little")
    _DATA[key] = (d, w, _epilogue(g, d, raw, keep), raw)
    return _DATA[key]


def _epilogue(g, d, raw, keep):
    """tem_epilogue's order on out0: add, gate, keep bits, slope; out1 stays raw"""
    ref = np.array(raw, np.float64)
    c0 = g["co"]
    if g["add"]:
        ref[..., :c0] += d["add"]
    if g["gate"]:
        ref[..., :c0] = np.where(d["gate"] > 0, ref[..., :c0], 0.3 * ref[..., :c0])
    if keep is not None:
        ref[..., :c0] = np.where(keep > 0, 2.0 * ref[..., :c0], 0.0)
    if g["slope"] != 1.0:
        ref[..., :c0] = np.where(ref[..., :c0] > 0, ref[..., :c0], g["slope"] * ref[..., :c0])
    return ref


def _bar(kernel, got, ref, bf16_out=False):
    """the family's own oracle bar -> (error, bound), in the measure the family's test uses"""
    err = float(np.abs(got - ref).max())
    if kernel.startswith("wino_conv_k"):                    # test_gpu_wino: forward 2e-6 x 3, gated input-gradient 6e-6
        return err, 6e-6 * max(1.0, float(np.abs(ref).max()))
    if kernel.startswith("wino_bww_k"):                     # test_gpu_wino: 3e-6 of the largest entry + 1e-4, and 3e-6 in L2
        assert np.linalg.norm(got - ref) <= 3e-6 * np.linalg.norm(ref), kernel
        return err, 3e-6 * float(np.abs(ref).max()) + 1e-4
    return rel_err(got, ref), TOL_H if bf16_out else TOL


# ------------------------------------------------------------------------------------------------ one launch
def _launch(lib, row, case, stretched=True):
    """run `case` (stretched: as built; else every operand dense) -> (kernel symbol, result fp64/fp32 ndarray, sentinel
    damage, all finite)"""
    from transfer_em_amd import hip_ops as H
    g = case.geom
    views = case.views if stretched else {o: dense(e, case.views["in0"].N) for o, e in extents(g).items()}
    N = views["in0"].N
    d, w, case.ref, raw = _data(row.geom, N)
    esz = g["esz"]
    dtype = torch.bfloat16 if esz == 2 else torch.float32
    need = sum(esz * (span(v) + (head_room(span(v)) if (stretched and o == row.operand) else 0)) for o, v in views.items())
    free, _ = torch.cuda.mem_get_info()
    if need + (2 << 30) > free:
        pytest.skip(f"needs {need + (2 << 30)} bytes, {free} free")
    bufs, t = {}, {}
    for o, v in views.items():
        head = head_room(span(v)) if (stretched and o == row.operand) else 0
        bufs[o], t[o] = framed(v, dtype, "cuda", head)
        if o in d:
            t[o].copy_(torch.from_numpy(d[o]).cuda())             # (bf16: exact, the values are bf16 numbers)
    c2 = Case(row, case.side)
    c2.views = views
    mask = torch.from_numpy(d["keep"]).cuda() if g["keep"] else None
    if case.frame:
        # the keep bits of a whole dropout frame just below / at the limit (512 MiB of mask; 1 GiB for bf16): random bytes
        # on the device, and the oracle takes the bits of the output's window, the frame's far corner
        c8, (oz, oy, ox), (OD, OH, OW) = g["co"] // 8, case.org, out_dims(g)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(5)
        mask = torch.randint(0, 256, case.frame + (c8,), dtype=torch.uint8, device="cuda", generator=gen)
        win = mask[oz:oz + OD, oy:oy + OH, ox:ox + OW].cpu().numpy()
        case.ref = _epilogue(g, d, raw, np.unpackbits(win, axis=-1, bitorder="little").reshape((1, OD, OH, OW, g["co"])))
    ptr = {o: t[o].data_ptr() for o in t}
    bww = g["entry"].startswith("bww")
    wd = u = None
    if not bww:
        wd = torch.from_numpy(w.reshape(-1)).cuda()
        if esz == 2 and g["entry"] == "conv_h":                 # the packed bf16 kernel [tap][co][ci] (test_gpu_bf16.pack)
            wd = torch.from_numpy(np.ascontiguousarray(w.reshape(-1, w.shape[3], w.shape[4]).transpose(0, 2, 1)).reshape(-1)).cuda()
        wd = wd.to(dtype)
        if g["wino"]:
            ci, co = g["ci"] + g["ci1"], g["co"] + g["co1"]
            u = torch.zeros(H.wino_u_floats(ci, co), device="cuda")
            H.run([H.wino_weights_launch("u", wd, u, H.wino_table([(0, 0, ci, co, 1 if g["flip"] else 0)], "cuda"), 1)])
    a = c2.args(ptr, wd.data_ptr() if wd is not None else 0, keep_mask=mask.data_ptr() if mask is not None else 0)
    rc, kernel = route(lib, c2, a, u.data_ptr() if u is not None else None)
    assert rc >= 0 and kernel, (row.id, rc, kernel)
    stream = H.current_stream()
    direct = row.family == "64-bit" and not stretched
    if bww:
        ci, co = g["ci"] + g["ci1"], g["co"]
        slabs = torch.full((a.nslab, g["k"] ** (3 if g["is3d"] else 2) * ci * co), float("nan"), device="cuda")
        a.slabs, a.accumulate = slabs.data_ptr(), 0
        fn = lib.tem_conv_bwd_weight_winograd if kernel.startswith("wino_bww_k") else lib.tem_conv_bwd_weight
        if esz == 2:
            fn = lib.tem_conv_bwd_weight_bf16
        assert fn(C.byref(a), stream) == 0, (row.id, kernel)
        torch.cuda.synchronize()
        got = slabs.double().sum(0).cpu().numpy().reshape(case.ref.shape)
        return kernel, got, 0, bool(np.isfinite(got).all())
    if direct:
        # the dense twin of a 64-bit case would run a tiled kernel: it goes to the direct entry point, whose choice among
        # its kernels (conv_direct.hip: channels, layout, kernel size, output height) does not look at a stride
        fn = lib.tem_conv_transpose_direct if g["entry"] == "convT" else lib.tem_conv_direct
    elif esz == 2:
        fn = lib.tem_conv_transpose_bf16 if g["entry"] == "convT_h" else lib.tem_conv_bf16
    else:
        fn = lib.tem_conv_transpose if g["entry"] == "convT" else lib.tem_conv
    assert fn(C.byref(a), stream) == 0, (row.id, kernel)
    torch.cuda.synchronize()
    outs, bad = [], 0
    for o in ("out0", "out1")[:2 if g["co1"] else 1]:
        inside, b = frame_intact(bufs[o], t[o])
        outs.append(inside)
        bad += b
    got = torch.cat(outs, -1)
    finite = bool(torch.isfinite(got).all())
    return kernel, got.float().cpu().numpy(), bad, finite


_DENSE = {}


def _check(lib, row, side, expect):
    case = Case(row, side)
    try:
        kernel, got, bad, finite = _launch(lib, row, case)
        key = (row.geom, case.views["in0"].N)
        if key not in _DENSE and not case.frame:          # (a frame row stretches no operand: it has no dense twin)
            dk, dgot = _launch(lib, row, case, stretched=False)[:2]
            _DENSE[key] = (kernel if row.family == "64-bit" and not case.geom["entry"].startswith("bww") else dk, dgot)
    except RuntimeError as e:                  # a device error: nothing more is launched on a card that may have faulted
        if "out of memory" in str(e):
            raise
        pytest.exit(f"{row.id} {side}: {e}", returncode=3)
    finally:
        torch.cuda.empty_cache()
    ref = case.ref
    err, bound = _bar(kernel, got, ref, case.geom["esz"] == 2 and not case.geom["entry"].startswith("bww"))
    print(f"{row.id} {side}: {row.quantity} = {case.value} ({case.value - row.limit:+d}) -> {kernel}: "
          f"error {err:.3g} (bar {bound:.3g}), outside the view {bad} damaged")
    assert kernel.startswith(expect + "<"), (row.id, side, kernel)
    assert bad == 0 and finite, (row.id, side, kernel, bad, finite)
    assert err <= bound, (row.id, side, kernel, err, bound)
    dk, dgot = (None, None) if case.frame else _DENSE[key]      # (a frame row's keep bits are its own: nothing to compare with)
    if dk == kernel:
        assert np.array_equal(got, dgot), (row.id, side, kernel, float(np.abs(got - dgot).max()))
    return kernel, err


@pytest.mark.parametrize("side", ["below", "at"])
@pytest.mark.parametrize("row", FP32_ROWS, ids=lambda r: r.id)
def test_limit_row_executes_on_both_sides(lib, row, side):
    # (argument structs and routes as conv_launch / bww_launch build them, without hip_ops.WINO_MIN_VOXELS: span_cases.route)
    _check(lib, row, side, row.kernel if side == "below" else row.fallback)


@pytest.mark.parametrize("side", ["below", "at"])
@pytest.mark.parametrize("row", BF16_ROWS, ids=lambda r: r.id)
def test_bf16_limit_row_executes_on_both_sides(lib, row, side):
    """bf16 has no direct form: at a limit with no other bf16 kernel behind it the entry point refuses, and there is nothing to
    run -- the refusal itself is the answer (as in tests/test_span_routing.py)."""
    if side == "at" and row.fallback is None:
        case = Case(row, side)
        ptr = {o: 0x7f0000000000 + (i << 40) for i, o in enumerate(case.views)}
        rc, kernel = route(lib, case, case.args(ptr, 0x7e0000000000, slabs=0x40000000))
        assert (rc, kernel) == (-2, ""), (row.id, rc, kernel)
        return
    _check(lib, row, side, row.kernel if side == "below" else row.fallback)


@pytest.mark.parametrize("row", DIRECT64, ids=lambda r: f"{r.id}-2^{r.limit.bit_length() - 1}")
def test_64bit_kernels_past_the_limits(lib, row):
    kernel, _ = _check(lib, row, "at", row.kernel)
    # the dense twin was compared bit for bit.  For the forward kernels its symbol is taken to be the stretched launch's
    # (tem_conv_direct reports none; its choice among its kernels does not look at a stride), so this line holds by
    # construction there and only the bit-for-bit comparison would notice another choice; for the gradients it is the query's
    assert _DENSE[(row.geom, 3)][0] == kernel
