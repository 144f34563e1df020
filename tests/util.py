"""Shared helpers for the parity tests (HIP path vs oracle/)."""
import numpy as np


def rel_err(a, b):
    """max|a-b| / max|b| -- the 'relative to the tensor's scale' error used for every float compare."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def inorm_f32(x, dy, scale, offset, eps=1e-5):
    """InstanceNormalization and its gradient restated in float32, op for op as csrc/elementwise.hip computes them:
    mean, deviation, variance, rstd and every product are rounded to float32 where the kernels round them, the
    sums run in float64.  Pure NumPy -- the yardstick for what float32 itself costs against the float64 oracle
    (the bars of tests/test_gpu_glue.py that are not the project's standing ones are 4x this function's error).
    Returns (y, mean, rstd, dx, dscale, doffset)."""
    f = np.float32
    x, dy = np.asarray(x, f), np.asarray(dy, f)
    scale, offset = np.asarray(scale, f), np.asarray(offset, f)
    ax, vox = (1, 2, 3), x.shape[1] * x.shape[2] * x.shape[3]
    mean = (x.sum(axis=ax, keepdims=True, dtype=np.float64) / vox).astype(f)
    d = x - mean
    var = ((d * d).sum(axis=ax, keepdims=True, dtype=np.float64) / vox).astype(f)
    rstd = (1.0 / np.sqrt((var + f(eps)).astype(np.float64))).astype(f)
    xh = d * rstd
    y = scale * xh + offset
    s1 = dy.sum(axis=ax, keepdims=True, dtype=np.float64)
    s2 = (dy * xh).sum(axis=ax, keepdims=True, dtype=np.float64)
    m1, m2 = (s1 / vox).astype(f), (s2 / vox).astype(f)
    dx = scale * rstd * (dy - m1 - xh * m2)
    return (y, mean.reshape(x.shape[0], -1), rstd.reshape(x.shape[0], -1), dx,
            s2.sum(axis=0).reshape(-1).astype(f), s1.sum(axis=0).reshape(-1).astype(f))


def _pow_f32(base, gamma):
    """(base ** gamma, d / d base) in float32, as the focal kernels' pow_gamma: the multiply path for gamma == 2, a
    non-finite derivative (0 ** negative) -> 0."""
    f = np.float32
    if gamma == 2:
        return base * base, f(2) * base
    with np.errstate(all="ignore"):
        val = np.power(base, f(gamma))
        grd = f(gamma) * np.power(base, f(gamma) - f(1))
    return val, np.where(np.isfinite(grd), grd, f(0)).astype(f)


def focal_logits_grad_f32(z, target, gamma, grad_scale):
    """d/dz of oracle.ops.focal_logits times grad_scale, restated in float32 op for op as csrc/elementwise*.hip computes
    it (every intermediate rounded to float32).  Pure NumPy: the yardstick of what float32 costs against float64."""
    f = np.float32
    z = np.asarray(z, f)
    with np.errstate(over="ignore"):
        ce = np.maximum(z, f(0)) - z * f(target) + np.log1p(np.exp(-np.abs(z)))
        pr = f(1) / (f(1) + np.exp(-z))
    dce = pr - f(target)
    base = f(1) - pr if target else pr
    dbase = -pr * (f(1) - pr) if target else pr * (f(1) - pr)
    mod, dmod = _pow_f32(base, gamma)
    out = (f(grad_scale) / f(z.size)) * f(0.5) * (dmod * dbase * ce + mod * dce)
    assert out.dtype == f
    return out


def focal_match_grad_f32(a, b, gamma, grad_scale):
    """d/db of oracle.ops.focal_prob_match times grad_scale in float32, op for op as the kernels compute it."""
    f = np.float32
    a, b = np.asarray(a, f), np.asarray(b, f)
    eps, hi = f(1e-7), f(1) - f(1e-7)
    diff = a - b
    t = f(1) - np.abs(diff) * f(0.5)
    tc = np.minimum(np.maximum(t, eps), hi)
    ce = -np.log(tc + eps)
    dce = np.where((t >= eps) & (t <= hi), f(-1) / (tc + eps), f(0)).astype(f)
    mod, dmod = _pow_f32(f(1) - t, gamma)
    dper = f(0.5) * (-dmod * ce + mod * dce)
    out = (f(grad_scale) / f(a.size)) * dper * f(0.5) * np.sign(diff).astype(f)
    assert out.dtype == f
    return out


def scaled_params(shapes, seed, gain=1.0):
    """Kernels with variance-preserving scale (so that every layer carries signal and gradient:
    the reference's N(0, 0.02) init makes the inner layers' gradients ~1e-10 of the outer ones,
    which would hide errors there).  He-style: std = gain * sqrt(2 / fan_in) / sqrt(1 + 0.3^2)."""
    from collections import OrderedDict
    rng = np.random.default_rng(seed)
    p = OrderedDict()
    for name, shp in shapes.items():
        if name.endswith("_bias"):
            p[name] = (rng.standard_normal(shp) * 0.1).astype(np.float32)
            continue
        taps = int(np.prod(shp[:3]))
        cin = shp[4] if name in ("u2b", "u1b") else shp[3]
        fan_in = taps * cin / (8 if name in ("u2b", "u1b") else 1)     # stride-2 transposed: 1/8 of taps hit
        std = gain * np.sqrt(2.0 / fan_in) / np.sqrt(1 + 0.09)
        if name == "f2":
            # keep generator outputs small: the reference's cycle/identity loss is -log(1-|a-b|/2),
            # whose gradient -1/t blows up as |a-b| -> 2; outputs of O(1) put many voxels next to that
            # pole and make ANY two float implementations disagree at the 1e-3 level
            std *= 0.05
        p[name] = (rng.standard_normal(shp) * std).astype(np.float32)
    return p


_GEN_SAVED = dict(f1="f1", u1b="u1", u1a="b1", mid="m", u2b="u2", u2a="b2", d2b="d2", d2a="s1", d1b="d1", d1a="s0",
                  c0="a0")
_DISC_SAVED = dict(d1a="e1", d1b="e2", hack="h", d2a="e3", d2b="e4", d3a="e5", d3b="e6", p1="p1")


def gate_flips(cs, saved, is3d=True):
    """Number of LeakyReLU outputs whose SIGN differs between the HIP forward and the oracle forward.

    LeakyReLU' is discontinuous at 0: an activation that is 1e-7 on one side and -1e-7 on the other (fp32
    MFMA chain vs the oracle's double accumulation) scales that element's gradient by 0.3 instead of 1,
    and the difference spreads to every kernel gradient below it.  One flip among ~10^6 elements already
    shows as ~1e-4..1e-3 relative error, so the step-level gradient tolerance is tight only when this
    returns 0.  `cs` is the compiled step (cgan._CompiledStep), `saved` is aux["saved"] of the oracle."""
    return activation_stats(cs, saved, is3d)[0]


FLIP_BOUND = 1e-5       # gate flips allowed per compared activation (measured: ~1e-6, pre-activations within rounding of 0)


def _saved_pairs(fwd, sv, generator, is3d):
    """(layer, HIP activation, oracle activation) of one call site: every saved LeakyReLU output that both sides hold,
    the oracle's cut to the region the forward evaluated (a generator's fwd.regions; the full tensor for an inference
    plan, whose in_pad and out_crop are 0)."""
    for layer, key in (_GEN_SAVED if generator else _DISC_SAVED).items():
        if key not in sv or layer not in fwd.act:
            continue
        ref = np.asarray(sv[key])
        if generator:
            lo, hi = fwd.regions[layer]
            ref = ref[:, lo:hi, lo:hi, lo:hi, :] if is3d else ref[:, :, lo:hi, lo:hi, :]
        got = fwd.act[layer].float().cpu().numpy()
        assert got.shape == ref.shape, (layer, got.shape, ref.shape)
        yield layer, got, ref


def compare_stats(got, ref):
    """(rel_err, l2_err, sign flips) of two equally shaped float32 arrays in one pass over slabs of the second axis:
    the float64 temporaries of a 226^3 x 16 activation stay at one plane's size.  rel_err is exactly util.rel_err's;
    the sums of l2_err run in float64."""
    dmax = rmax = d2 = r2 = 0.0
    flips = 0
    for g, r in zip(np.moveaxis(got, 1, 0), np.moveaxis(ref, 1, 0)):
        flips += int(np.count_nonzero((g > 0) != (r > 0)))
        g, r = g.astype(np.float64), r.astype(np.float64)
        d = g - r
        dmax, rmax = max(dmax, float(np.abs(d).max())), max(rmax, float(np.abs(r).max()))
        d2, r2 = d2 + float(np.vdot(d, d)), r2 + float(np.vdot(r, r))
    return dmax / (rmax + 1e-30), float(np.sqrt(d2) / (np.sqrt(r2) + 1e-30)), flips


def l2_err(a, b):
    """|a-b|_2 / |b|_2 -- the norm the bf16 comparisons use (one bf16 ulp moves single entries past any max-norm bar)."""
    return compare_stats(np.asarray(a, np.float32), np.asarray(b, np.float32))[1]


def forward_stats(fwd, sv, y_ref, is3d=True):
    """activation_stats for one bare GenForward (an inference plan of UNetGenerator.plan, or one call site of a step):
    OrderedDict layer -> (rel_err, l2_err, sign flips, elements) of the eleven saved activations of the oracle's
    generator_forward `sv` and, under "y", of the output against `y_ref`."""
    from collections import OrderedDict
    out = OrderedDict()
    for layer, got, ref in _saved_pairs(fwd, sv, True, is3d):
        out[layer] = compare_stats(got, ref) + (got.size,)
    lo, hi = fwd.regions["f2"]
    ref = np.asarray(y_ref)
    ref = ref[:, lo:hi, lo:hi, lo:hi, :] if is3d else ref[:, :, lo:hi, lo:hi, :]
    got = fwd.y.float().cpu().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    out["y"] = compare_stats(got, ref) + (got.size,)
    return out


def failed_bars(stats, rel_tol=None, l2_bars=None, flip_bound=None):
    """The layers of a forward_stats result that miss a bar, as {layer: (figure, bar)}: rel_err < rel_tol (a number for
    every layer, or a dict for some), l2_err < l2_bars[layer], and under "flips" the sign flips of the activations (the
    output has no gate) against max(2, flip_bound * elements), the bound of activation_stats.  Empty: all bars hold."""
    bad = {}
    for layer, (rel, l2, _, _) in stats.items():
        tol = rel_tol.get(layer) if isinstance(rel_tol, dict) else rel_tol
        if tol is not None and not rel < tol:
            bad[layer] = (rel, tol)
        if l2_bars is not None and layer in l2_bars and not l2 < l2_bars[layer]:
            bad[layer] = (l2, l2_bars[layer])
    if flip_bound is not None:
        n = sum(s[2] for k, s in stats.items() if k != "y")
        total = sum(s[3] for k, s in stats.items() if k != "y")
        if n > max(2, flip_bound * total):
            bad["flips"] = (n, max(2, flip_bound * total))
    return bad


def activation_stats(cs, saved, is3d=True, tol=None):
    """(gate flips, compared elements, worst relative activation error, its (call, layer)) over every saved LeakyReLU
    output of the step: the HIP forward's activation buffers against the oracle's (on the evaluated region for the
    cycle-path call sites).  With `tol` every activation is asserted to it (relative to the tensor's largest value)
    and the flip count to FLIP_BOUND of the compared elements -- so a forward kernel that is wrong on small activations
    cannot hide behind the gate alignment of the backward comparison."""
    n = total = 0
    worst, where = 0.0, None
    for call, sv in saved.items():
        for layer, got, ref in _saved_pairs(cs.fwd[call], sv, call[0] in "gf", is3d):
            n += int(np.count_nonzero((got > 0) != (ref > 0)))
            total += got.size
            e = rel_err(got, ref)
            if e > worst:
                worst, where = e, (call, layer)
            if tol is not None:
                assert e < tol, (call, layer, e)
    if tol is not None:
        assert n <= max(2, FLIP_BOUND * total), (n, total)
    return n, total, worst, where


def gate_masks(cs):
    """The LeakyReLU branches of the HIP forward, off the device: {call: {saved key: (act > 0, region or None)}} for every
    saved layer of the ten call sites of the compiled step `cs` (cgan._CompiledStep).  region = (lo, hi) of fwd.regions for
    a generator's layer -- the cycle-path call sites hold only that window of each tensor -- and None for a discriminator's."""
    out = {}
    for call, fwd in cs.fwd.items():
        gen = call[0] in "gf"
        out[call] = {key: (fwd.act[layer].float().cpu().numpy() > 0, tuple(fwd.regions[layer]) if gen else None)
                     for layer, key in (_GEN_SAVED if gen else _DISC_SAVED).items() if layer in fwd.act}
    return out


def pack_masks(masks, prefix="gate"):
    """gate_masks() as flat arrays for np.savez: per mask its packed bits, its shape and its region (-1, -1: none)."""
    out = {}
    for call, g in masks.items():
        for key, (pos, region) in g.items():
            out[f"{prefix}.{call}.{key}.bits"] = np.packbits(pos)
            out[f"{prefix}.{call}.{key}.shape"] = np.asarray(pos.shape, np.int64)
            out[f"{prefix}.{call}.{key}.region"] = np.asarray(region if region is not None else (-1, -1), np.int64)
    return out


def unpack_masks(rec, prefix="gate"):
    """Inverse of pack_masks over a loaded .npz (or any mapping with its keys)."""
    out = {}
    for name in rec.keys() if hasattr(rec, "keys") else rec.files:
        if not (name.startswith(prefix + ".") and name.endswith(".bits")):
            continue
        call, key = name[len(prefix) + 1:-len(".bits")].split(".")
        shape = tuple(int(v) for v in rec[f"{prefix}.{call}.{key}.shape"])
        lo, hi = (int(v) for v in rec[f"{prefix}.{call}.{key}.region"])
        pos = np.unpackbits(rec[name], count=int(np.prod(shape))).reshape(shape).astype(bool)
        out.setdefault(call, {})[key] = (pos, None if lo < 0 else (lo, hi))
    return out


def gates_from_masks(masks, is3d=True):
    """`gates` argument of oracle.graph.train_step(_grads) from gate_masks(): a callable that takes the oracle's `saved`.

    Inside a generator layer's region the mask replaces the oracle's own sign pattern; outside it the oracle's signs stay
    (every gradient is exactly zero there).  The callable's `.flips` is filled per call site with (positions where the mask
    differs from the oracle's own sign inside the region, positions compared): pre-activations within rounding of 0."""
    def build(saved):
        out = {}
        for call, sv in saved.items():
            g, n, total = {}, 0, 0
            for key, (got, region) in masks[call].items():
                if key not in sv:
                    continue
                pos = np.asarray(sv[key]) > 0
                if region is not None:
                    lo, hi = region
                    win = pos[:, lo:hi, lo:hi, lo:hi, :] if is3d else pos[:, :, lo:hi, lo:hi, :]
                    assert win.shape == got.shape, (call, key, win.shape, got.shape)
                    n, total = n + int(np.count_nonzero(win != got)), total + got.size
                    win[...] = got
                else:
                    assert pos.shape == got.shape, (call, key, pos.shape, got.shape)
                    n, total = n + int(np.count_nonzero(pos != got)), total + got.size
                    pos = got
                g[key] = pos
            out[call] = g
            build.flips[call] = (n, total)
        return out
    build.flips = {}
    return build


def hip_gates(cs, is3d=True):
    """`gates` argument of oracle.graph.train_step(_grads): the LeakyReLU branches of the HIP forward.

    For every saved activation of the oracle the sign pattern is taken from the HIP path's own activation
    buffer (cs.fwd[call].act[layer]); the cycle-path call sites hold only the region R[layer] of each tensor
    (models/generator.needed_regions) -- outside it the oracle's own signs stay (every gradient is exactly
    zero there).  With this the oracle differentiates the very branch the HIP backward gates on, and the
    step-level gradient comparison needs no widened tolerance; gate_flips() stays a printed diagnostic."""
    return gates_from_masks(gate_masks(cs), is3d)


def _inputs(shape, seed):
    """A standardized uint8 volume (B, D, H, W, 1) as the data pipeline delivers it: zero mean, unit deviation."""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 256, shape[:-1], dtype=np.uint8)
    x = (u.astype(np.float32) / np.float32(127.5) - np.float32(1.0))[..., None]
    return ((x - x.mean()) / x.std()).astype(np.float32)


DP_AMPLITUDE = 0.5      # of the two-replica tests' inputs; see dp_inputs
DP_OUTPUTS = (("fake_y", "g1"), ("cyc_x", "f2"), ("fake_x", "f1"), ("cyc_y", "g2"), ("same_x", "f3"), ("same_y", "g3"))


def dp_inputs(rank, is3d, n=74):
    """(real_x, real_y) of one replica of the two-replica tests (tests/tools/dp_rank.py and the oracle side of
    test_gpu_dp.py): standardized uint8 volumes, seeds 1000 + rank / 2000 + rank, at half amplitude.  At amplitude 1 the
    inputs reach +-1.73 and the test weights' outputs +-0.3 .. 0.8, so the oracle's own 1 - |a - b| / 2 of the cycle /
    identity terms runs through the pole for EVERY seed (60 seed pairs scanned in 2-D: -0.25 .. -0.02; 6 in 3-D: -0.07 ..
    -0.02); at 0.5 it is 0.37 .. 0.49 (2-D) and 0.48 (3-D), as for the 132^2 / 260^2 instances of test_gpu_step.py."""
    shape = (1, n if is3d else 1, n, n, 1)
    return np.float32(DP_AMPLITUDE) * _inputs(shape, 1000 + rank), np.float32(DP_AMPLITUDE) * _inputs(shape, 2000 + rank)


def _pole_margin(aux, rx, ry, b, crop_by):
    """Smallest 1 - |a - b| / 2 over the pixels of the four cycle / identity terms, from the oracle's own outputs: the
    loss -log(1 - |a - b| / 2) has a pole there, and its gradient moves by delta / (2 margin) of itself when an output
    moves by delta (conditioning note)."""
    worst = np.inf
    for key, real in (("same_x", rx), ("same_y", ry), ("cyc_x", rx), ("cyc_y", ry)):
        a, o = (crop_by(real, 2 * b), crop_by(aux[key], b)) if key.startswith("cyc") else (crop_by(real, b), aux[key])
        worst = min(worst, float((1.0 - np.abs(a.astype(np.float64) - o) / 2).min()))
    return worst


def linearise(lists, priority):
    """One serial order of a stream-list set (cgan._CompiledStep.lists / lists_fused) under a priority order over the
    lists: the launches and ("allreduce", key) items, in the order a host loop like EM2EM._run_streams's would issue them
    if list priority[0] always went first.  Each turn advances, by ONE item, the highest-priority list that is not
    blocked on an event no list has recorded yet (a `record` marks its event; "inputs" is recorded up front), then starts
    again from the top -- so a list overtakes every lower one the moment the event it waits for exists.

    Every order the declared events allow is a legal execution of the schedule.  A dependency with no event between
    list i and list j is broken by the order that ranks the consumer's list above the producer's: the consumer then runs
    first.  The permutations of the lists give the extremal orders of that kind, not all orders."""
    lists = [list(l) for l in lists]
    assert sorted(priority) == list(range(len(lists))), priority
    pos, recorded, out = [0] * len(lists), {"inputs"}, []
    while any(p < len(l) for p, l in zip(pos, lists)):
        for i in priority:
            if pos[i] == len(lists[i]):
                continue
            item = lists[i][pos[i]]
            if isinstance(item, tuple) and item[0] == "wait" and item[1] not in recorded:
                continue
            if isinstance(item, tuple) and item[0] == "record":
                recorded.add(item[1])
            elif not (isinstance(item, tuple) and item[0] == "wait"):
                out.append(item)
            pos[i] += 1
            break
        else:
            raise AssertionError("stream schedule deadlocked")
    return out


def reference_tile(volume, roi, edge, meanstd_x):
    """The generator input (1, edge, edge, edge, 1) of the 3-D tile whose haloed box starts at roi = (x, y, z) of the
    uint8 `volume` [z, y, x]: zeros outside the volume, scaled and standardised on the host by the oracle's ops."""
    from oracle import ops
    rx, ry, rz = roi
    Z, Y, X = volume.shape
    tile = np.zeros((edge, edge, edge), np.uint8)
    z0, y0, x0, z1, y1, x1 = max(rz, 0), max(ry, 0), max(rx, 0), min(rz + edge, Z), min(ry + edge, Y), min(rx + edge, X)
    tile[z0 - rz:z1 - rz, y0 - ry:y1 - ry, x0 - rx:x1 - rx] = volume[z0:z1, y0:y1, x0:x1]
    return ops.standardize(ops.scale_u8(tile), meanstd_x)[None]


def reference_predict(volume, start, size, P, meanstd_x, meanstd_y, outdim, buffer, tiles=None):
    """utils.py:62-130 with the cloud fetch replaced by array slicing (zeros outside).  `tiles`: the indices into
    tile_plan's rois of the tiles to predict (None: all of them); the others' voxels stay 0."""
    from oracle import graph, ops
    from transfer_em_amd.utils import tile_plan
    outdim, buffer, tpad, rois, index = tile_plan(start, size, outdim, buffer)
    edge = outdim + 2 * buffer
    rnd = lambda v: v + ((outdim - v % outdim) if v % outdim else 0)
    out = np.zeros((rnd(size[2]), rnd(size[1]), rnd(size[0])), np.uint8)
    for i, (roi, (ix, iy, iz)) in enumerate(zip(rois, index)):
        if tiles is not None and i not in tiles:
            continue
        x = reference_tile(volume, roi, edge, meanstd_x)
        y, _ = graph.generator_forward(P, x, True, training=False)
        if tpad:
            y = y[:, tpad:-tpad, tpad:-tpad, tpad:-tpad, :]
        out[iz:iz + outdim, iy:iy + outdim, ix:ix + outdim] = ops.to_u8(y, meanstd_y)[0, ..., 0]
    return out[:size[2], :size[1], :size[0]]


def prior_layers(is3d, seed=5, extra_tail=True):
    """A frozen prior in the layer-list form of transfer_em_amd.models.prior (shaped like the
    discriminator trunk up to Downsample_2 so that its output matches, discriminator.py:62-66).
    With extra_tail the list continues past the cut point, as a full classifier would."""
    rng = np.random.default_rng(seed)
    kd = lambda k: (k if is3d else 1, k, k)
    conv = lambda k, ci, co, s=1, bias=False, gain=1.0: {
        "type": "conv", "kernel": (rng.standard_normal(kd(k) + (ci, co)) * gain / np.sqrt(k ** (3 if is3d else 2) * ci)
                                   ).astype(np.float32),
        "bias": (rng.standard_normal(co) * 0.1).astype(np.float32) if bias else None, "stride": s}
    act = lambda a=0.3: {"type": "leaky_relu", "alpha": a}
    L = [{"type": "input"}]
    if is3d:
        L += [conv(3, 1, 8, gain=2.0), act(), conv(4, 8, 8, 2, bias=True, gain=2.0), act(), conv(3, 8, 16, gain=2.0), act(0.2)]
    else:
        L += [conv(3, 1, 16, gain=2.0), act()]
    L += [conv(3, 16, 24, bias=True, gain=2.0), act(), conv(4, 24, 32, 2, gain=2.0), act(0.1)]     # 24: off the channel table
    cut = len(L) - 1
    if extra_tail:
        L += [conv(3, 32, 8), act()]
    return L, cut
