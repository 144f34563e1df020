"""wino_conv_k, wino_bww_k, conv_lds_k and conv3_bf16_k held to the oracle across their plan space: every case of
tests/plan_cases.py is launched once per plan of its sweep list -- the whole feasible list of a small shape, one plan per
class signature of a large one (tests/test_plan_space.py holds those lists to the workload on the CPU) -- with the plan
pinned through tem_plan_pin and read back through tem_plan_last.

Forward / input-gradient kernels: the default plan's output is held to the float64 oracle at the family's own bar
(test_gpu_wino 6e-6 of scale, test_gpu_ops 2e-5, test_gpu_bf16 6e-3) and every pinned plan's output must equal it bit for
bit: a plan deals output voxels to workgroups, waves and z steps and leaves each voxel's own chain of multiply-adds alone
(no field was found to enter it; DESIGN.md, "Plan space").  wino_bww_k sums a workgroup's voxels into its slab, so the
split reorders the sums: every plan goes against the oracle's kernel gradient at test_gpu_wino's bar, twice, and must
reproduce itself bit for bit.

conv_s2_k and convT_mfma_k (one pinned number: workgroups, Q_y rows per band) ride the same forward test at test_gpu_ops.TOL,
every pinned plan bit-equal to the default one; bww_s2_k / bww_s2tb_k (row ranges R, which regroup the sum) go against the
oracle's kernel gradient per R after tem_reduce_slabs, twice, with the slabs behind the R-th left untouched.  Three planted
errors at the end lie on paths only a pin opens at these shapes.

Operands are strided windows of larger allocations that start as a NaN sentinel (span_cases), a plane, a row and a voxel
of head room on every side; after each launch the output is finite, the allocation outside the window untouched, and the
window is back to the sentinel for the next plan.  Comparisons run on the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import plan_cases as P
from plan_cases import BWW_S2, CASES, CONV3_BF16, CONVT_MFMA, CONV_LDS, CONV_S2, WINO, WINO_BWW
from span_cases import SENTINEL, View, _bits, extents, frame_intact, out_dims, span

pytestmark = pytest.mark.gpu
TOL = {CONV_LDS: 2e-5, CONV3_BF16: 6e-3, CONV_S2: 2e-5, CONVT_MFMA: 2e-5, BWW_S2: 2e-5}   # test_gpu_ops.TOL, test_gpu_bf16.TOL (max error over the largest |ref|)


@pytest.fixture(scope="module")
def lib():
    from transfer_em_amd import hip_ops
    return hip_ops.require_gpu()


@pytest.fixture(autouse=True)
def _clear_pins():
    yield
    from transfer_em_amd import _lib
    P.clear_pins(_lib.load())


# ------------------------------------------------------------------------------------------------ operands
def window(ext, N):
    """(View, head): the operand as a window of an enclosing tensor one voxel larger on every side"""
    D, H, W, Cc = ext
    sW, sH = Cc, (W + 2) * Cc
    sD = (H + 2) * sH
    return View(N, D, H, W, Cc, (D + 2) * sD, sD, sH, sW), sD + sH + sW


def framed(v, head, dtype):
    """an allocation filled with the sentinel, the view inside it with `head` elements in front and behind"""
    buf = torch.empty(head + span(v) + head, dtype=dtype, device="cuda")
    _bits(buf).fill_(SENTINEL[buf.element_size()])
    return buf, buf.as_strided((v.N, v.D, v.H, v.W, v.C), (v.sN, v.sD, v.sH, v.sW, 1), head)


def operands(case):
    """-> (d, w, ref): compact inputs, the kernel as the entry point takes it, the float64 oracle result with tem_epilogue's
    order on out0 (add, gate, keep bits, slope; out1 stays raw); a kernel gradient has w = None"""
    from oracle import ops as O
    O.build()
    g, N = case.geom, case.N
    rng = np.random.default_rng(sum(map(ord, case.id)))
    bf = g["esz"] == 2                  # bf16: the oracle gets the values the bf16 tensors hold
    rb = (lambda a: torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()) if bf else (lambda a: a)
    d = {o: rb(rng.standard_normal((N,) + e).astype(np.float32)) for o, e in case.extents().items() if not o.startswith("out")}
    k, s, p = g["k"], g["s"], g["p"]
    ci, co = case.channels
    x = np.concatenate([d["in0"], d["in1"]], -1) if g["ci1"] else d["in0"]
    if case.family in (WINO_BWW, BWW_S2):
        return d, None, O.conv_bwd_weight(x, d["dout"], (k, k, k), s, p)
    if g["entry"] == "convT":             # the kernel in Keras' layout (tap, co, ci)
        w = (rng.standard_normal((k, k, k, co, ci)) * 0.1).astype(np.float32)
        raw = O.convT_fwd(x, w, s, p, out_dims=out_dims(g))
    elif g["flip"]:          # the input-gradient of a co -> ci layer, whose kernel (tap, co, ci) is read flipped / transposed
        w = (rng.standard_normal((k, k, k, co, ci)) * 0.1).astype(np.float32)
        raw = O.conv_fwd(x, np.ascontiguousarray(np.flip(w, (0, 1, 2)).transpose(0, 1, 2, 4, 3)), s, p)
    else:
        w = rb((rng.standard_normal((k, k, k, ci, co)) * 0.1).astype(np.float32))
        raw = O.conv_fwd(x, w, s, p)
    assert raw.shape == (N,) + out_dims(g) + (co,)
    ref, c0 = np.array(raw, np.float64), g["co"]
    if g["add"]:                          # tem_epilogue's order: skip-gradient (inside its window), gate, keep bits, slope
        oz, oy, ox = case.add_off or (0, 0, 0)
        _, aD, aH, aW, _ = d["add"].shape
        ref[:, oz:oz + aD, oy:oy + aH, ox:ox + aW, :c0] += d["add"]
    if g["gate"]:
        ref[..., :c0] = np.where(d["gate"] > 0, ref[..., :c0], 0.3 * ref[..., :c0])
    if g["keep"]:
        keep = O.dropout_mask((N,) + out_dims(g) + (c0,), 42, 3, 7)          # the stream span_cases.Case.args names
        d["keep"] = np.packbits(keep.reshape(-1), bitorder="little")
        ref[..., :c0] = np.where(keep > 0, 2.0 * ref[..., :c0], 0.0)
    if g["slope"] != 1.0:
        ref[..., :c0] = np.where(ref[..., :c0] > 0, ref[..., :c0], g["slope"] * ref[..., :c0])
    return d, w, ref


class Launcher:
    """one case on the device: operands placed once, then one launch per plan"""

    def __init__(self, lib, case):
        from transfer_em_amd import _lib, hip_ops as H
        self.lib, self.case, self.H = lib, case, H
        g, f = case.geom, case.family
        d, w, ref = operands(case)
        self.ref = torch.from_numpy(ref).cuda()
        dtype = torch.bfloat16 if g["esz"] == 2 else torch.float32
        self.bufs, self.t, views = {}, {}, {}
        for o, e in case.extents().items():
            views[o], head = window(e, case.N)
            self.bufs[o], self.t[o] = framed(views[o], head, dtype)
            if o in d:
                self.t[o].copy_(torch.from_numpy(d[o]).cuda())
        placed = P.PlanCase(case.name, f, g, case.N, case.add_off)
        placed.views = views
        self.keep = torch.from_numpy(d["keep"]).cuda() if g["keep"] else None
        self.mask = None
        if g["keep"] == 1:                 # the launch draws the bits itself and writes them: a mask of its own inside a frame of bytes
            self.mask_ref, self.keep = self.keep, torch.full((self.keep.numel() + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            self.mask = self.keep
        ptr = {o: t.data_ptr() for o, t in self.t.items()}
        self.outs = [o for o in ("out0", "out1") if o in views]
        if f in (WINO_BWW, BWW_S2):
            self.a = placed.args(ptr, 0)
            self.fn = lib.tem_conv_bwd_weight_winograd if f == WINO_BWW else lib.tem_conv_bwd_weight
            return
        if f == CONV3_BF16:                               # the packed bf16 kernel [tap][co][ci] (test_gpu_bf16.pack)
            w = np.ascontiguousarray(w.reshape(-1, w.shape[3], w.shape[4]).transpose(0, 2, 1))
        self.w = torch.from_numpy(w.reshape(-1)).cuda().to(dtype)
        self.a = placed.args(ptr, self.w.data_ptr(), keep_mask=self.keep.data_ptr() if self.keep is not None else 0)
        self.fn = lib.tem_conv_bf16 if f == CONV3_BF16 else lib.tem_conv_transpose if f == CONVT_MFMA else lib.tem_conv
        if f == WINO:
            ci, co = case.channels
            self.u = torch.zeros(H.wino_u_floats(ci, co), device="cuda")
            H.run([H.wino_weights_launch("u", self.w, self.u, H.wino_table([(0, 0, ci, co, 1 if g["flip"] else 0)], "cuda"), 1)])
            self.plain = (self.a.w, self.a.w_layout)
            self.a.w, self.a.w_layout = self.u.data_ptr(), _lib.TEM_W_WINOGRAD

    def _guard(self, what, fn):
        try:
            return fn()
        except RuntimeError as e:                  # a device error: nothing more is launched on a card that may have faulted
            pytest.exit(f"{self.case.id} {what}: {e}", returncode=3)

    def forward(self, v4=None):
        """launch under pin v4 (None: the planner's own choice) -> (output window(s) compact, elements damaged outside them,
        the plan read back)"""
        def go():
            P.pin(self.lib, self.case.family, v4)
            rc = self.fn(C.byref(self.a), self.H.current_stream())
            P.pin(self.lib, self.case.family, None)
            assert rc == 0, (self.case.id, v4, rc)
            plan = P.last(self.lib, self.case.family)
            torch.cuda.synchronize()
            got, bad = [], 0
            for o in self.outs:
                inside, b = frame_intact(self.bufs[o], self.t[o])           # (leaves the window NaN-filled for the next launch)
                got.append(inside)
                bad += b
            if self.mask is not None:      # the keep bits are the oracle's Philox mask, the bytes behind them untouched; reset for the next plan
                n = self.mask_ref.numel()
                bad += int((self.mask[:n] != self.mask_ref).sum()) + int((self.mask[n:] != 0xA5).sum())
                self.mask.fill_(0xA5)
            return torch.cat(got, -1), bad, plan
        return self._guard(v4, go)

    def gradient(self, v4=None):
        """slab-count query and launch under the same pin, twice -> (slab sum fp64, the two runs equal bit for bit, plan)"""
        ci, co = self.case.channels

        def go():
            P.pin(self.lib, self.case.family, v4)
            taken, sym = P.describe(self.lib, self.case, self.a)              # sets a.nslab to the plan's slab count
            assert taken, (self.case.id, v4, sym)
            plan, runs = P.last(self.lib, self.case.family), []
            for _ in range(2):
                slabs = torch.full((self.a.nslab, 27 * ci * co), float("nan"), device="cuda")
                self.a.slabs, self.a.accumulate = slabs.data_ptr(), 0
                rc = self.fn(C.byref(self.a), self.H.current_stream())
                assert rc == 0 and P.last(self.lib, self.case.family) == plan, (self.case.id, v4, rc)
                torch.cuda.synchronize()
                runs.append(slabs)
            P.pin(self.lib, self.case.family, None)
            return runs[0].double().sum(0).reshape(self.ref.shape), torch.equal(runs[0], runs[1]), plan
        return self._guard(v4, go)

    def ranges(self, v4=None):
        """bww_s2_k / bww_s2tb_k under pin v4: slab-count query, launch and tem_reduce_slabs, twice, each into a fresh workspace
        of R + 2 sentinel slabs -> (reduced gradient fp32, the two runs equal bit for bit in slabs and sum, sentinel elements
        lost in the slabs behind the R-th, plan)"""
        ci, co = self.case.channels
        n = self.case.geom["k"] ** 3 * ci * co

        def go():
            P.pin(self.lib, BWW_S2, v4)
            taken, sym = P.describe(self.lib, self.case, self.a)              # sets a.nslab to the plan's R
            assert taken, (self.case.id, v4, sym)
            plan, R, runs, lost = P.last(self.lib, BWW_S2), self.a.nslab, [], 0
            for _ in range(2):
                slabs, out = torch.empty((R + 2, n), device="cuda"), torch.empty(n, device="cuda")
                _bits(slabs).fill_(SENTINEL[4])
                self.a.slabs, self.a.accumulate = slabs.data_ptr(), 0
                rc = self.fn(C.byref(self.a), self.H.current_stream())
                assert rc == 0 and P.last(self.lib, BWW_S2) == plan, (self.case.id, v4, rc)
                rc = self.lib.tem_reduce_slabs(slabs.data_ptr(), R, n, 0, out.data_ptr(), 0, 1.0, self.H.current_stream())
                assert rc == 0, (self.case.id, v4, rc)
                torch.cuda.synchronize()
                lost += int((_bits(slabs[R:]) != SENTINEL[4]).sum())
                runs.append((slabs[:R], out))
            P.pin(self.lib, BWW_S2, None)
            same = torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1])
            return runs[0][1].reshape(self.ref.shape), same, lost, plan
        return self._guard(v4, go)

    def error(self, got):
        """(error, bound) in the family's own measure, computed on the device"""
        f, ref = self.case.family, self.ref
        err = float((got.double() - ref).abs().max())
        scale = float(ref.abs().max())
        if f == WINO:
            return err, 6e-6 * max(1.0, scale)
        if f == WINO_BWW:
            return err, 3e-6 * scale + 1e-4
        return err / (scale + 1e-30), TOL[f]


def _npin(case):
    return P.NPIN[case.family]


# ------------------------------------------------------------------------------------------------ the sweep
FORWARD = [c for f in (WINO, CONV_LDS, CONV3_BF16, CONV_S2, CONVT_MFMA) for c in CASES[f]]


@pytest.mark.parametrize("case", FORWARD, ids=lambda c: c.id)
def test_every_plan_equals_the_default_plan_which_matches_the_oracle(lib, case):
    run = P.sweep_list(lib, case)
    L = Launcher(lib, case)
    base, bad, plan = L.forward()
    assert plan == P.default_plan(lib, case) and plan in run
    err, bound = L.error(base)
    print(f"{case.id}: default {dict(zip(P.FIELDS[case.family], plan))} error {err:.3g} (bar {bound:.3g}); {len(run)} plans")
    assert bad == 0 and bool(torch.isfinite(base).all()), (case.id, plan, bad)
    assert err <= bound, (case.id, plan, err, bound)
    wrong = []
    for v in run:
        got, bad, plan = L.forward(v[:_npin(case)])
        if plan != v:
            wrong.append((v, "read back", plan))
        elif bad or not bool(torch.isfinite(got).all()):
            wrong.append((v, "outside the window" if bad else "not finite", bad))
        elif not torch.equal(got, base):
            wrong.append((v, "differs from the default plan", float((got.double() - base.double()).abs().max())))
    assert not wrong, (case.id, len(wrong), len(run), wrong[:8])


@pytest.mark.parametrize("case", CASES[WINO_BWW], ids=lambda c: c.id)
def test_every_kernel_gradient_plan_matches_the_oracle(lib, case):
    run = P.sweep_list(lib, case)
    L = Launcher(lib, case)
    nref = float(torch.linalg.vector_norm(L.ref))
    wrong, worst = [], 0.0
    for v in [None] + run:
        got, same, plan = L.gradient(None if v is None else v[:4])
        err, bound = L.error(got)
        l2 = float(torch.linalg.vector_norm(got - L.ref))
        worst = max(worst, err / bound)
        if v is None:
            assert plan == P.default_plan(lib, case) and plan in run
            v = plan
        if plan != v:
            wrong.append((v, "read back", plan))
        elif not same:
            wrong.append((v, "two runs differ"))
        elif not (err <= bound and l2 <= 3e-6 * nref):            # (a NaN fails both)
            wrong.append((v, "oracle", err, bound, l2 / nref))
    print(f"{case.id}: {len(run)} plans, worst error / bar {worst:.3g}")
    assert not wrong, (case.id, len(wrong), len(run), wrong[:8])


@pytest.mark.parametrize("case", CASES[BWW_S2], ids=lambda c: c.id)
def test_every_row_range_count_matches_the_oracle_and_reproduces_itself(lib, case):
    """R regroups the sum over the output rows, so the plans differ in their bits: each goes against the float64 oracle at
    test_gpu_ops.TOL after tem_reduce_slabs, twice, and must reproduce itself; the slabs behind the R-th stay untouched.  A
    pad-1 8 -> 16 case is a transposed layer's kernel gradient with input and gradient swapped: oracle.ops.convT_bwd_weight of
    the swapped operands is held to the same numbers."""
    from oracle import ops as O
    run = P.sweep_list(lib, case)
    L = Launcher(lib, case)
    if case.geom["p"] == 1 and case.channels == (8, 16):
        refT = O.convT_bwd_weight(L.t["dout"].cpu().numpy(), L.t["in0"].cpu().numpy(), (4, 4, 4), 2, 1)
        assert refT.shape == tuple(L.ref.shape)
        assert float(np.abs(refT - L.ref.cpu().numpy()).max()) <= 1e-9 * float(L.ref.abs().max())
    wrong, worst = [], 0.0
    for v in [None] + run:
        got, same, lost, plan = L.ranges(None if v is None else v[:1])
        err, bound = L.error(got)
        worst = max(worst, err / bound)
        if v is None:
            assert plan == P.default_plan(lib, case) and plan in run
            v = plan
        if plan != v:
            wrong.append((v, "read back", plan))
        elif not same:
            wrong.append((v, "two runs differ"))
        elif lost:
            wrong.append((v, "slabs behind the last range written", lost))
        elif not err <= bound:                                     # (a NaN fails)
            wrong.append((v, "oracle", err, bound))
    print(f"{case.id}: {len(run)} plans, worst error / bar {worst:.3g}")
    assert not wrong, (case.id, len(wrong), len(run), wrong[:8])


# ------------------------------------------------------------------------------------------------ sensitivity
# What the changed plane gains.  A voxel below it moves by BUMP times the sum of the kernel's entries over the 9 taps of the
# bottom plane and the input channels: for entries of 0.1 N(0, 1) that sum has a standard deviation of 0.1 sqrt(9 C_in) >= 0.85,
# so the largest of the plane's outputs moves by several units -- hundreds of times the widest bar here (bf16: 6e-3 of a
# scale of ~6).  The tests ask for ten times the bar.
BUMP = 8.0
def _whole_axis_plan(lib, case):
    """a plan that marches the whole z axis in one run of at least 3 steps, with a ragged tile block"""
    plans = P.enumerate_plans(lib, case)
    v = next(v for v in plans if P.signature(case, v, plans)[:3] == ("all", False, "rag"))
    assert v[P.FIELDS[case.family].index("zper")] >= 3
    return v


def _case(family, tag, variant, channels):
    return next(c for c in CASES[family] if c.name.endswith(tag) and c.variant == variant and c.channels == channels)


@pytest.mark.parametrize("case", [_case(WINO, "17x25x31", "ep0", (16, 16)), _case(CONV_LDS, "9x16x21", "plain", (16, 16)),
                                  _case(CONV3_BF16, "9x24x33", "plain", (8, 8))], ids=lambda c: c.id)
def test_the_comparison_sees_an_error_only_the_march_makes(lib, case):
    """With the whole z axis in one run, the last input plane is read by the run's last step alone (pad 0: output plane
    OD - 1 reads input planes OD - 1 .. OD + 1).  With that plane changed on the device and the reference left alone, the
    result must leave the reference in the last output plane and nowhere above it: the oracle comparison reaches into the
    steady state of the march, which no default plan of a small shape enters."""
    assert case.geom["p"] == 0 and case.geom["k"] == 3
    v = _whole_axis_plan(lib, case)
    L = Launcher(lib, case)
    clean, _, plan = L.forward(v[:_npin(case)])
    assert plan == v
    err, bound = L.error(clean)
    assert err <= bound
    L.t["in0"][:, -1] += BUMP
    got, bad, plan = L.forward(v[:_npin(case)])
    assert plan == v and bad == 0
    bar = bound if case.family == WINO else bound * float(L.ref.abs().max())           # the family's bar as an absolute error
    per_plane = (got.double() - L.ref).abs().amax(dim=(0, 2, 3, 4))
    assert float(per_plane[:-1].max()) <= bar and float(per_plane[-1]) > 10 * bar, (bar, per_plane.tolist())
    assert torch.equal(got[:, :-1], clean[:, :-1]) and not torch.equal(got[:, -1], clean[:, -1])


def test_the_gradient_comparison_sees_an_error_only_the_march_makes(lib):
    """the same for wino_bww_k: the last input plane meets the gradient's last plane in tap kz = 2 alone"""
    case = _case(WINO_BWW, "17x25x31", "p0", (16, 16))
    v = _whole_axis_plan(lib, case)
    L = Launcher(lib, case)
    L.t["in0"][:, -1] += BUMP
    got, same, plan = L.gradient(v[:4])
    assert plan == v and same
    bound = 3e-6 * float(L.ref.abs().max()) + 1e-4
    per_tap = (got - L.ref).abs().amax(dim=(1, 2, 3, 4))
    assert float(per_tap[:2].max()) <= bound and float(per_tap[2]) > 10 * bound, per_tap.tolist()


def test_bit_equality_tells_two_kernels_apart(lib):
    """the sweep's equality check is not vacuous: the same operands through the Winograd form and through the direct form
    both meet the oracle, and differ in their bits"""
    from transfer_em_amd import _lib
    case = _case(WINO, "small", "ep0", (16, 16))
    L = Launcher(lib, case)
    wino, _, _ = L.forward()
    L.a.w, L.a.w_layout = L.plain
    name = C.create_string_buffer(96)
    lib.tem_conv_is_tiled(C.byref(L.a), 0, name, 96)
    assert name.value and not name.value.startswith(b"wino_conv_k"), name.value
    direct, bad, _ = L.forward()
    assert bad == 0
    err, bound = L.error(wino)
    assert err <= bound, (err, bound)
    rel = float((direct.double() - L.ref).abs().max() / L.ref.abs().max())
    assert rel <= TOL[CONV_LDS], rel                                   # the direct forms' bar (test_gpu_ops.TOL)
    assert not torch.equal(wino, direct)
    assert _lib.TEM_PLAN_WINO == WINO and _lib.TEM_PLAN_CONV3_BF16 == CONV3_BF16


# ---- the k4 s2 kernels: an error on a path only the pin opens
def _s2_case(family, tag, variant, channels):
    return next(c for c in CASES[family] if c.name.split("-", 3)[3] == tag and c.variant == variant and c.channels == channels)


def test_the_comparison_sees_an_error_only_a_second_iteration_makes(lib):
    """conv_s2_k 16 -> 16 at (3, 5, 7) x 2: 9 iterations of two tiles.  The default plan gives every iteration a workgroup of
    its own.  With 5 workgroups pinned (one walk: workgroup b owns b and b + 5) iterations 5 .. 8 -- tiles 10 .. 17, which hold the
    last output plane of the last sample, tiles 15 .. 17 -- run as second iterations, on the second fragment set and LDS buffer.
    The last two input planes of that sample are read by that output plane alone (pad 0: plane 2 reads planes 4 .. 7)."""
    case = _s2_case(CONV_S2, "small", "fwd", (16, 16))
    assert case.geom["p"] == 0 and P.default_plan(lib, case)[:4] == (9, 1, 2, 9)
    assert P.s2_owned(5, 9) == [2, 2, 2, 2, 1] and P.s2_owned(9, 9).count(0) == 1
    L = Launcher(lib, case)
    clean, _, plan = L.forward((5,))
    assert plan[0] == 5
    err, bound = L.error(clean)
    assert err <= bound
    L.t["in0"][-1, -2:] += BUMP
    got, bad, plan = L.forward((5,))
    assert plan[0] == 5 and bad == 0
    bar = bound * float(L.ref.abs().max())
    per_plane = (got.double() - L.ref).abs().amax(dim=(2, 3, 4)).reshape(-1)            # (sample, output plane)
    assert float(per_plane[:-1].max()) <= bar and float(per_plane[-1]) > 10 * bar, (bar, per_plane.tolist())
    assert torch.equal(got.reshape(-1, *got.shape[2:])[:-1], clean.reshape(-1, *clean.shape[2:])[:-1])


def test_the_comparison_sees_an_error_only_a_second_band_makes(lib):
    """convT_mfma_k 16 -> 8, input (3, 5, 6), pad 1: nQy = 6, one band by default.  TY = 3 pinned makes two; the second holds
    Q_y = 3 .. 5, output rows 5 .. 9.  The last input row j_y = 4 reaches the output rows 2 j_y + t - 1 = 7 .. 9 alone, through
    Q_y = 4 and 5: the second band's patch."""
    case = _s2_case(CONVT_MFMA, "small", "plain", (16, 8))
    assert P.default_plan(lib, case)[:2] == (6, 1)
    L = Launcher(lib, case)
    clean, _, plan = L.forward((3,))
    assert plan[:2] == (3, 2)
    err, bound = L.error(clean)
    assert err <= bound
    L.t["in0"][:, :, -1] += BUMP
    got, bad, plan = L.forward((3,))
    assert plan[:2] == (3, 2) and bad == 0
    bar = bound * float(L.ref.abs().max())
    per_row = (got.double() - L.ref).abs().amax(dim=(0, 1, 3, 4))
    assert per_row.numel() == 10 and float(per_row[:7].max()) <= bar and float(per_row[7:].min()) > 10 * bar, (bar, per_row.tolist())
    assert torch.equal(got[:, :, :7], clean[:, :, :7])


def test_the_gradient_comparison_sees_an_error_only_a_ranges_last_wave_makes(lib):
    """bww_s2_k 16 -> 16 at (3, 5, 7) x 2: 30 output rows, two ranges by default.  In the second range [15, 30) the fourth wave
    takes rows 18, 22 and 26.  With the gradient's row 18 = (sample 1, plane 0, row 3) changed on the device, the result must
    leave the reference and meet the oracle's kernel gradient of the changed operand."""
    from oracle import ops as O
    case = _s2_case(BWW_S2, "small", "p0", (16, 16))
    assert P.default_plan(lib, case)[:2] == (2, 30) and P.bww_ranges(2, 30)[1] == (15, 30)
    L = Launcher(lib, case)
    clean, same, lost, plan = L.ranges((2,))
    err, bound = L.error(clean)
    assert plan[0] == 2 and same and not lost and err <= bound
    L.t["dout"][1, 0, 3] += BUMP
    got, same, lost, plan = L.ranges((2,))
    assert plan[0] == 2 and same and not lost
    err, bound = L.error(got)
    assert err > 10 * bound, (err, bound)
    ref2 = torch.from_numpy(O.conv_bwd_weight(L.t["in0"].cpu().numpy(), L.t["dout"].cpu().numpy(), (4, 4, 4), 2, 0)).cuda()
    assert float((got.double() - ref2).abs().max() / ref2.abs().max()) <= bound
