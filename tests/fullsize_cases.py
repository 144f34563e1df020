"""Table-driven operator cases at a train step's own shapes, and the key that ties a table to the step.

A case row (`_c` convolution / transposed convolution, `_b` kernel gradient) describes ONE launch of a compiled train
step the way the model code calls hip_ops.conv_launch / bww_launch: extents, channel split, k / s / p, the cropped
views behind an input, and the epilogue.  `build_conv` / `build_bww` turn a row into the launch (with random operands
when a generator is given), `check_conv` / `check_bww` run it and compare it with oracle/torch_ops.py (float64) on the
same -- for bf16 tensors bf16-rounded -- operands, and `launch_key` reduces any Launch, a table's or the step's, to the
fields the coverage guards compare (test_gpu_bf16_fullsize_oracle.py, test_gpu_2d_fullsize_oracle.py).

Extents are cubes (3-D) or squares (2-D, depth 1), so a row carries edges.  A 3-D row may also carry `depth`, the
depth of its input, where it is smaller than the edge (test_gpu_step260.py: the 260^3 step on thin slabs): every other
tensor of the row then loses as many planes as the cube's counterpart has more than its own input or output needs --
inputs, skip crops and cone windows n - depth planes, outputs, gates, skip-gradient windows and dropout frames the
planes the shorter input no longer produces -- while k / s / p, offsets and origins stay the step's."""
import numpy as np
import torch

import bf16_exact
from util import rel_err

# bf16 outputs: the max-norm bar below and, for the rows exact_checked names, every stored element against the rounded
# float64 reference (bf16_exact.py: 4 x the sequential float32 sum's error plus four epilogue roundings, <= 10 % undecided)
TOL_BF16 = 6e-3           # test_gpu_bf16.TOL: one bf16 ulp at the top of the range is 2^-8 = 3.9e-3
TOL_BF16_SLAB = 2e-5      # fp32 slabs from bf16 operands: exact products, fp32 summation order (test_gpu_bf16.py)
TOL_FP32 = 3e-5           # test_gpu_fullsize_oracle.py: the direct fp32 forms
TOL_FP32_WINO = 1e-5      # test_gpu_fullsize_oracle.py: the Winograd forms' reordered arithmetic
TOL_FP32_SLAB = 1e-5      # test_gpu_fullsize_oracle.py: fp32 kernel gradients (and 3e-6 in the L2 norm)
SEED, SITE, STEP = 42, 5, 3


def _c(name, kernel, n, ci0, m, co0, k, s=1, p=0, *, ci1=0, in1=None, in0=None, co1=0, T=False, layout=0, slope=1.0,
       bias=False, gate=None, add=None, drop=None, depth=None):
    """Convolution row: in0 (edge n, ci0 channels) [| in1 (ci1 channels)] -> out0 (edge m, co0) [| out1 (co1)].
    in0 / in1 = (parent edge, lo): the tensor is the crop [lo, lo + n) of a larger one.  T: transposed convolution.
    gate = gate_slope of the LeakyReLU' gate on out0; add = (edge, offset) of the skip-gradient window added first;
    drop = (origin, full edge, keep_mode) of the Dropout frame out0 is a window of."""
    return dict(kind="conv", name=name, kernel=kernel, n=n, ci0=ci0, m=m, co0=co0, k=k, s=s, p=p, ci1=ci1, in1=in1, in0=in0,
                co1=co1, T=T, layout=layout, slope=slope, bias=bias, gate=gate, add=add, drop=drop, depth=depth)


def _b(name, kernel, n, ci0, m, co, k, s=1, p=0, *, ci1=0, in1=None, in0=None, depth=None):
    """Kernel-gradient row as bww_launch is called (before it swaps the roles of a C_out == 1 layer)."""
    return dict(kind="bww", name=name, kernel=kernel, n=n, ci0=ci0, m=m, co=co, k=k, s=s, p=p, ci1=ci1, in1=in1, in0=in0,
                depth=depth)


def select(rows, which):
    """Rows of a two-precision table (kernel = (bf16 symbol, fp32 symbol), layout likewise) for one precision."""
    out = []
    for r in rows:
        if r["kernel"][which] is None:
            continue
        r = dict(r, kernel=r["kernel"][which])
        if isinstance(r.get("layout"), tuple):
            r["layout"] = r["layout"][which]
        out.append(r)
    return out


# ------------------------------------------------------------------------------------------------ launch keys
def _view_key(v):
    if not v.ptr:
        return None
    dense = (v.sW, v.sH, v.sD, v.sN) == (v.C, v.W * v.C, v.H * v.W * v.C, v.D * v.H * v.W * v.C)
    return (v.N, v.D, v.H, v.W, v.C, "dense" if dense else "view")


def launch_struct(launch):
    """The tem_conv_args / tem_bww_args behind a Launch, or None for every other entry point."""
    from transfer_em_amd import _lib
    a = getattr(launch.args[0], "_obj", None) if launch.args else None
    return a if isinstance(a, (_lib.tem_conv_args, _lib.tem_bww_args)) else None


def launch_key(launch):
    """Entry point, kernel symbol, every extent / channel count / k / s / p of the argument struct, whether each view is
    dense, and the epilogue: slope, bias, gate (+ slope), add (+ offset), dropout frame, keep_mode."""
    from transfer_em_amd import _lib
    a = launch_struct(launch)
    geo = ((a.kd, a.kh, a.kw), (a.sd, a.sh, a.sw), (a.pd, a.ph, a.pw))
    if isinstance(a, _lib.tem_bww_args):
        return ("bww", launch.fn.__name__, launch.meta["kernel"], _view_key(a.in0), _view_key(a.in1), _view_key(a.dout),
                geo, a.nslab)
    ep = a.ep
    return ("conv", launch.fn.__name__, launch.meta["kernel"], _view_key(a.in0), _view_key(a.in1), _view_key(a.out0),
            _view_key(a.out1), geo, a.w_layout, round(ep.slope, 4), bool(ep.bias),
            (_view_key(ep.gate), round(ep.gate_slope, 4)) if ep.gate.ptr else None,
            (_view_key(ep.add), tuple(ep.add_off)) if ep.add.ptr else None,
            (tuple(ep.drop_org), tuple(ep.drop_dims), ep.keep_mode, bool(ep.keep_mask)) if ep.dropout else None)


def thin_key(launch):
    """launch_key without what the depth of a thin slab changes: the D extent of every view, the batch stride in the
    test of whether a view is dense, the depth of the dropout frame, and the slab count."""
    from transfer_em_amd import _lib
    a = launch_struct(launch)

    def vk(v):
        if not v.ptr:
            return None
        return (v.N, v.H, v.W, v.C, "dense" if (v.sW, v.sH, v.sD) == (v.C, v.W * v.C, v.H * v.W * v.C) else "view")
    geo = ((a.kd, a.kh, a.kw), (a.sd, a.sh, a.sw), (a.pd, a.ph, a.pw))
    if isinstance(a, _lib.tem_bww_args):
        return ("bww", launch.fn.__name__, launch.meta["kernel"], vk(a.in0), vk(a.in1), vk(a.dout), geo)
    ep = a.ep
    return ("conv", launch.fn.__name__, launch.meta["kernel"], vk(a.in0), vk(a.in1), vk(a.out0), vk(a.out1), geo, a.w_layout,
            round(ep.slope, 4), bool(ep.bias), (vk(ep.gate), round(ep.gate_slope, 4)) if ep.gate.ptr else None,
            (vk(ep.add), tuple(ep.add_off)) if ep.add.ptr else None,
            (tuple(ep.drop_org), tuple(ep.drop_dims)[1:], ep.keep_mode, bool(ep.keep_mask)) if ep.dropout else None)


# Every entry point of a step that is not a convolution, transposed convolution or kernel gradient (by kernel symbol
# where the launch carries one, by C entry point otherwise): casts and per-step kernel copies, dropout bits, losses,
# view adds, the bias gradient, the slab reduction, Adam, the step counter and the fp32 discriminator head.
OTHER_FAMILIES = ("tem_cast_f32_to_bf16", "tem_pack_weights_bf16", "tem_flip_transpose", "dropout_masks_k", "tem_focal_logits",
                  "tem_focal_match", "tem_add_view", "tem_channel_sum", "reduce_multi_k", "tem_adam_keras", "tem_step_tick",
                  "head_fwd_k", "head_bwd_k",
                  "both")        # fp32 3-D: ParamSet's tem_flip_transpose + tem_winograd_weights behind one Launch


def step_keys(step, key=launch_key):
    """Keys of every convolution / kernel-gradient launch of a compiled step; any other launch must belong to
    OTHER_FAMILIES."""
    keys = set()
    for l in step.compute + step.update:
        if launch_struct(l) is not None:
            keys.add(key(l))
            continue
        sym = l.meta.get("kernel") or l.fn.__name__
        assert sym.startswith(OTHER_FAMILIES), f"launch {l.name}: unknown kernel family {sym}"
    return keys


def assert_tables_cover(step, table_keys, key=launch_key):
    got = step_keys(step, key)
    missing, stale = got - table_keys, table_keys - got
    assert not missing and not stale, ("step launches without a table case:", sorted(map(str, missing)),
                                       "table cases the step does not launch:", sorted(map(str, stale)))


# ------------------------------------------------------------------------------------------------ operands
def _rb(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


class _Ctx:
    """Geometry and tensor factory of one table: batch N, 3-D or 2-D, bf16 or fp32 tensors, data or shapes only."""

    def __init__(self, N, is3d, bf16, rng, cut_in=0, cut_out=0, device="cuda"):
        self.N, self.is3d, self.bf16, self.rng = N, is3d, bf16, rng
        self.dtype = torch.bfloat16 if bf16 else torch.float32
        # thin slabs: planes an input-side (out=False) / output-side (out=True) tensor has less than its edge
        self.cut = {False: cut_in, True: cut_out}
        self.device = device

    def shape(self, e, c, out=False):
        return (self.N, e - self.cut[out] if self.is3d else 1, e, e, c)

    def k3(self, k):
        return (k, k, k) if self.is3d else (1, k, k)

    def s3(self, s):
        return (s, s, s) if self.is3d else (1, s, s)

    def p3(self, p):
        return (p, p, p) if self.is3d else (0, p, p)

    def win(self, a, lo, n, out=False):
        if self.is3d:
            return a[:, lo:lo + n - self.cut[out], lo:lo + n, lo:lo + n, :]
        return a[:, :, lo:lo + n, lo:lo + n, :]

    def values(self, shape, scale=1.0):
        a = self.rng.standard_normal(shape, dtype=np.float32) * np.float32(scale)
        return _rb(a) if self.bf16 else a

    def tensor(self, shape, scale=1.0):
        """(numpy values or None, device tensor)."""
        if self.rng is None:
            return None, torch.empty(shape, dtype=self.dtype, device=self.device)
        a = self.values(shape, scale)
        return a, torch.from_numpy(a).to(self.dtype).to(self.device)

    def cropped(self, e, c, crop):
        """A tensor of edge e, dense or the crop (parent edge, lo) of a larger one."""
        if crop is None:
            return self.tensor(self.shape(e, c))
        par, lo = crop
        a, t = self.tensor(self.shape(par, c))
        return (None if a is None else self.win(a, lo, e)), self.win(t, lo, e)


class _P:          # minimal stand-in for a ParamSet: one layer "w"
    def __init__(self, shape, device="cuda"):
        self.shapes = {"w": shape}
        self.grad = torch.zeros(int(np.prod(shape)), dtype=torch.float32, device=device)
        self.theta = self.grad

    def g(self, name):
        return self.grad


# ------------------------------------------------------------------------------------------------ convolutions
GUARD = 1     # thin rows: NaN planes in front of and behind every output, which the launch must leave alone


def _natural(n, k, s, p, T):
    return (n - 1) * s + k - 2 * p if T else (n + 2 * p - k) // s + 1


def _ctx(c, N, is3d, bf16, rng, device):
    """The row's tensor factory; with a depth, the planes its input-side and output-side tensors lose."""
    dn = c.get("depth")
    if dn is None:
        return _Ctx(N, is3d, bf16, rng, device=device)
    assert is3d and dn <= c["n"]
    T = c.get("T", False)
    return _Ctx(N, is3d, bf16, rng, c["n"] - dn, _natural(c["n"], c["k"], c["s"], c["p"], T) - _natural(dn, c["k"], c["s"], c["p"], T), device)


def _output(X, c, co, thin):
    """A NaN-filled output (uninitialised for the coverage guards); a thin row's is the middle of a tensor with GUARD more
    planes at either end -> (the tensor the launch writes, the whole allocation)."""
    shp = X.shape(c["m"], co, out=True)
    if thin:
        shp = (shp[0], shp[1] + 2 * GUARD) + shp[2:]
    big = torch.empty(shp, dtype=X.dtype, device=X.device) if X.rng is None else \
        torch.full(shp, float("nan"), dtype=X.dtype, device=X.device)
    return (big[:, GUARD:-GUARD] if thin else big), big


def build_conv(H, c, N, is3d, bf16, rng=None, device="cuda", plant=False):
    """The launch of row c.  With rng, random operands (O(1) outputs: kernels scaled 0.6 / sqrt(taps C_in)) and
    everything check_conv needs; without, uninitialised tensors of the right shapes (the coverage guards, which run
    on host tensors too: device="cpu").  plant: the kernel the launch gets has its centre tap scaled by 1.05, the
    reference keeps the true one."""
    X = _ctx(c, N, is3d, bf16, rng, device)
    thin = c.get("depth") is not None
    k, s, p = c["k"], c["s"], c["p"]
    ci, co = c["ci0"] + c["ci1"], c["co0"] + c["co1"]
    dims = 3 if is3d else 2
    d = dict(c=c, X=X)
    x0, t0 = X.cropped(c["n"], c["ci0"], c["in0"])
    x1, t1 = X.cropped(c["n"], c["ci1"], c["in1"]) if c["ci1"] else (None, None)
    taps = k ** dims / (s ** dims if c["T"] else 1)           # taps that meet one output voxel
    scale = 0.6 / np.sqrt(taps * ci)
    if c["T"]:
        wshape = X.k3(k) + (co, ci)                            # Keras Conv3DTranspose kernel (tap, CO, CI)
    elif c["layout"] == H.TEM_W_FLIP_CO_CI:
        wshape = X.k3(k) + (co, ci)                            # the forward layer's kernel (tap, ci_f = co, co_f = ci)
    else:
        wshape = X.k3(k) + (ci, co)                            # operator kernel (tap, ci, co)
    if rng is None:
        w, tw = None, torch.empty(int(np.prod(wshape)), dtype=X.dtype, device=device)
    else:
        w = X.values(wshape, scale)
        wl = w
        if plant:
            wl = w.copy()
            wl[(0 if wl.shape[0] == 1 else k // 2), k // 2, k // 2] *= np.float32(1.05)
            wl = _rb(wl) if bf16 else wl
            assert not np.array_equal(wl, w)
        if bf16 and not c["T"] and c["layout"] == H.TEM_W_TAP_CI_CO:      # packed bf16 copy [tap][co][ci]
            flat = np.ascontiguousarray(wl.reshape(-1, ci, co).transpose(0, 2, 1)).reshape(-1)
        else:
            flat = wl.reshape(-1)
        tw = torch.from_numpy(np.ascontiguousarray(flat)).to(X.dtype).to(device)
    out0, big0 = _output(X, c, c["co0"], thin)
    out1, big1 = _output(X, c, c["co1"], thin) if c["co1"] else (None, None)
    kw = {}
    if not bf16 and is3d and k == 3 and s == 1 and not c["T"] and H.wino_channels(ci, co):
        # the layer's Winograd-domain kernel copy, as ParamSet keeps it (conv_launch takes it where the library runs the
        # geometry and epilogue in that form)
        u = torch.zeros(H.wino_u_floats(ci, co), device=device)
        if rng is not None:
            H.run([H.wino_weights_launch("u", tw, u, H.wino_table([(0, 0, ci, co, int(c["layout"] == H.TEM_W_FLIP_CO_CI))], device), 1)])
        kw["wino"] = u
    if c["bias"]:
        d["bias"] = None if rng is None else rng.standard_normal(co, dtype=np.float32)
        kw["bias"] = torch.empty(co, device=device) if rng is None else torch.from_numpy(d["bias"]).to(device)
    if c["gate"] is not None:
        d["saved"], tg = X.tensor(X.shape(c["m"], c["co0"], out=True))
        kw.update(gate=tg, gate_slope=c["gate"])
    if c["add"] is not None:
        d["add"], ta = X.tensor(X.shape(c["add"][0], co, out=True))
        kw.update(add=ta, add_off=c["add"][1])
    if c["drop"] is not None:
        org, full, mode = c["drop"]
        frame = X.shape(full, c["co0"], out=True)
        count = int(np.prod(frame))
        d["step"] = torch.tensor([STEP], dtype=torch.int32, device=device)
        kw.update(dropout=(SEED, SITE, d["step"]), drop_frame=(org, full))
        if mode:
            nbytes = ((count + 7) // 8 + 15) // 16 * 16
            if mode == 2 and rng is not None:                  # the launch reads the keep bits an earlier launch wrote
                bits = rng.integers(0, 2, size=frame).astype(np.uint8)
                host = np.zeros(nbytes, np.uint8)
                packed = np.packbits(bits.reshape(-1), bitorder="little")
                host[:packed.size] = packed
                d["bits"], d["mask"] = bits, torch.from_numpy(host).to(device)
            else:
                d["mask"] = torch.zeros(nbytes, dtype=torch.uint8, device=device)
            kw["keep_mask"] = (d["mask"], mode)
    launch = H.conv_launch(c["name"], t0, tw, out0, k, s, p, is3d=is3d, in1=t1, out1=out1, layout=c["layout"],
                           transposed=c["T"], slope=c["slope"], **kw)
    if thin and c["drop"] is not None:
        launch_struct(launch).ep.drop_dims[0] = frame[1]      # conv_launch takes the frame's edge: a thin frame is no cube
    d.update(x0=x0, x1=x1, w=w, out0=out0, out1=out1, big=[b for b in (big0, big1) if b is not None])
    return launch, d


def conv_reference(T, oracle_lib, d, mag=False, act=True):
    """float64 result of the row on the operands build_conv drew: (N, ..., co0 + co1).  mag: the same operation on the
    magnitudes of inputs, kernel, bias and add, with the gate's and the dropout's factors as the row applies them (the S
    of bf16_exact.store_interval).  act=False leaves out the final LeakyReLU."""
    c, X = d["c"], d["X"]
    k, s, p, m = c["k"], c["s"], c["p"], c["m"]
    if mag:
        d = dict(d, **{key: np.abs(d[key]) for key in ("x0", "x1", "w", "bias", "add") if d.get(key) is not None})
    x = d["x0"] if d["x1"] is None else np.concatenate([d["x0"], d["x1"]], -1)
    w = d["w"]
    if c["T"]:
        y = T.convT_fwd(x, w, X.s3(s), X.p3(p), out_dims=X.shape(m, 1, out=True)[1:4])
    else:
        if c["layout"] == 1:                                   # tap-reversed, (ci, co)-transposed forward kernel
            w = w[::-1, ::-1, ::-1].transpose(0, 1, 2, 4, 3).copy()
        xin, pe = (X.win(x, -p, c["n"] + p), 0) if p < 0 else (x, p)      # negative pad: the window starts inside the input
        y = T.conv_fwd(xin, w, X.s3(s), X.p3(pe), d.get("bias"))
        assert y.shape[2] >= m and y.shape[1] >= X.shape(m, 1, out=True)[1]
        y = X.win(y, 0, m, out=True)                           # the output window starts at -p and may end early
    y = np.array(y, np.float64)
    co0 = c["co0"]
    if c["add"] is not None:
        e, off = c["add"]
        X.win(y, off, e, out=True)[...] += d["add"]
    y0 = y[..., :co0]
    if c["gate"] is not None:
        y0 = np.where(d["saved"] > 0, y0, np.float32(c["gate"]) * y0)
    if c["drop"] is not None:
        org, full, mode = c["drop"]
        if "keep" not in d:
            if mode == 2:
                keep = d["bits"]
            else:
                keep = oracle_lib.dropout_mask(X.shape(full, co0, out=True), SEED, SITE, STEP)
            d["keep"] = X.win(keep, org, m, out=True)
        y0 = np.where(d["keep"] > 0, 2.0 * y0, 0.0)
    y = np.concatenate([y0, y[..., co0:]], -1) if c["co1"] else y0
    if act and c["slope"] != 1.0:
        y = np.where(y > 0, y, np.float32(c["slope"]) * y)
    return y


EXACT_MAX = 1 << 22       # full-depth bf16 rows with more output elements keep the max-norm bar only (see exact_checked)


def exact_checked(c, N, is3d):
    """Whether check_conv holds the bf16 row's stores element by element to the rounded float64 reference
    (bf16_exact.py), which takes a second float64 pass of the oracle on magnitudes: every thin row, and every full-depth
    row of at most EXACT_MAX output elements -- at 132^3 a second pass takes longer than a test here should."""
    elems = N * c["m"] ** (3 if is3d else 2) * (c["co0"] + c["co1"])
    return c.get("depth") is not None or elems <= EXACT_MAX


def check_conv(H, T, oracle_lib, c, N, is3d, bf16, seed, plant=False, report=None):
    """Build, check the kernel symbol, run, compare; returns the measured errors of out0 (and out1).  report: a dict
    that receives the figures (errs, tol, and the exact check's counts) before anything is asserted."""
    launch, d = build_conv(H, c, N, is3d, bf16, np.random.default_rng(seed), plant=plant)
    assert launch.meta["kernel"] == c["kernel"], (c["name"], launch.meta["kernel"])
    H.run([launch]); torch.cuda.synchronize()
    if c.get("depth") is not None:
        for big in d["big"]:                                   # nothing written outside the window
            assert torch.isnan(big[:, :GUARD]).all() and torch.isnan(big[:, -GUARD:]).all(), (c["name"], "guard planes written")
    pre = conv_reference(T, oracle_lib, d, act=False)
    ref = np.where(pre > 0, pre, np.float32(c["slope"]) * pre) if c["slope"] != 1.0 else pre
    tol = TOL_BF16 if bf16 else (TOL_FP32_WINO if launch.meta["kernel"].startswith("wino_conv_k") else TOL_FP32)
    co0 = c["co0"]
    got = [d["out0"].float().cpu().numpy()] + ([d["out1"].float().cpu().numpy()] if c["co1"] else [])
    errs = [rel_err(got[0], ref[..., :co0])]
    if c["co1"]:
        errs.append(rel_err(got[1], ref[..., co0:]))
    print(f"{c['name']} {launch.meta['kernel']}: rel_err", *(f"{e:.2e}" for e in errs))
    exact = None
    if bf16 and exact_checked(c, N, is3d):
        # the stores element by element: S from a second pass on magnitudes, the LeakyReLU slope where the reference is
        # clear of 0 (bf16_exact.epilogue64); K = k^dims (ci0 + ci1), an upper bound for the transposed forms
        K = c["k"] ** (3 if is3d else 2) * (c["ci0"] + c["ci1"])
        r64, S = bf16_exact.epilogue64(pre, conv_reference(T, oracle_lib, d, mag=True, act=False), K, slope=c["slope"])
        exact = bf16_exact.check_bf16_stores(np.concatenate(got, -1), r64, S, K, f"{c['name']} {launch.meta['kernel']}")
    if report is not None:
        report.update(errs=errs, tol=tol, exact=exact)
    assert all(e < tol for e in errs), (c["name"], launch.meta["kernel"], errs)     # (NaN: an output voxel not written)
    if exact is not None:
        assert exact["undecided"] <= bf16_exact.UNDECIDED_CAP, (c["name"], "undecided share", exact["undecided"])
        assert exact["fails"] == 0, (c["name"], launch.meta["kernel"], f"{exact['fails']} of {exact['total']} stored bf16 "
                                     "values outside the rounded reference", exact["first"])
    if c["drop"] is not None and c["drop"][2] == 1:
        # the launch drew the keep bits itself and wrote them into the frame's mask: inside its window the oracle's bits
        org, full, _ = c["drop"]
        X = d["X"]
        count = int(np.prod(X.shape(full, co0, out=True)))
        bits = np.unpackbits(d["mask"].cpu().numpy(), bitorder="little")[:count].reshape(X.shape(full, co0, out=True))
        assert np.array_equal(X.win(bits, org, c["m"], out=True), d["keep"]), c["name"]
    return max(errs)


# ------------------------------------------------------------------------------------------------ kernel gradients
def build_bww(H, c, N, is3d, bf16, rng=None, device="cuda"):
    X = _ctx(c, N, is3d, bf16, rng, device)
    k, s, p = c["k"], c["s"], c["p"]
    ci = c["ci0"] + c["ci1"]
    x0, t0 = X.cropped(c["n"], c["ci0"], c["in0"])
    x1, t1 = X.cropped(c["n"], c["ci1"], c["in1"]) if c["ci1"] else (None, None)
    g, tg = X.tensor(X.shape(c["m"], c["co"], out=True))
    P = _P(X.k3(k) + (ci, c["co"]), device)
    ws = H.GradWorkspace(P, 1)
    launch = H.bww_launch(c["name"], t0, tg, ws, "w", 0, k, s, p, is3d=is3d, in1=t1)
    return launch, dict(c=c, X=X, x0=x0, x1=x1, g=g, P=P, ws=ws)


def check_bww(H, T, c, N, is3d, bf16, seed):
    launch, d = build_bww(H, c, N, is3d, bf16, np.random.default_rng(seed))
    assert launch.meta["kernel"] == c["kernel"], (c["name"], launch.meta["kernel"])
    X, k, s, p = d["X"], c["k"], c["s"], c["p"]
    H.run([launch] + d["ws"].reduce_launches("r")); torch.cuda.synchronize()
    x = d["x0"] if d["x1"] is None else np.concatenate([d["x0"], d["x1"]], -1)
    g = d["g"]
    full = (c["n"] + 2 * p - k) // s + 1                     # a gradient window that ends early: zero rows change nothing
    if full > c["m"]:
        z = np.zeros(X.shape(full, c["co"], out=True), np.float32)
        X.win(z, 0, c["m"], out=True)[...] = g
        g = z
    ref = T.conv_bwd_weight(x, g, X.k3(k), X.s3(s), X.p3(p))
    got = d["P"].grad.cpu().numpy().reshape(ref.shape)
    e = rel_err(got, ref)
    l2 = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print(f"{c['name']} {launch.meta['kernel']} nslab {launch_struct(launch).nslab}: rel_err {e:.2e} l2 {l2:.2e}")
    assert e < (TOL_BF16_SLAB if bf16 else TOL_FP32_SLAB), (c["name"], launch.meta["kernel"], e)
    if not bf16:
        assert l2 <= 3e-6, (c["name"], l2)
    return e
