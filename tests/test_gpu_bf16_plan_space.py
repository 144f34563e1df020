"""conv_bf16_k, convT_bf16_k and bww_bf16_k held to the oracle across their launch geometry: every case of
tests/bf16_plan_cases.py is launched once per plan of its sweep list -- the whole feasible list of a small shape, one plan per
class signature of a larger one (tests/test_bf16_plan_space.py holds those lists to the workload on the CPU) -- with the plan
pinned through tem_plan_pin (families 8, 9, 10) and read back through tem_plan_last.

Forward / transposed: the default plan's output is held to oracle/torch_ops.py (float64) at the standing bf16 bars --
tests/bf16_exact.py element by element, and 6e-3 of the largest |ref| -- and every pinned plan's output must equal it bit for
bit: a patch or band geometry deals voxels to workgroups, waves and tiles and leaves each voxel's k-ordered MFMA chain alone.
Written keep bits equal the Philox mask under every plan.

Kernel gradients: the sums follow the plan.  Every plan goes against the float64 kernel gradient after tem_reduce_slabs at the
standing bars (2e-5 of the largest entry, 3e-6 in L2), twice, must reproduce itself bit for bit and write exactly the slabs the
query announced; a segmented launch is held to the single launch of the same band and z split at the same bars, wherever a
single launch of that band height fits the row (the test counts these comparisons; tests/test_bf16_plan_space.py holds the count
above zero for every instance that has one).

Operands are strided windows of larger allocations that start as a NaN sentinel (test_gpu_plan_space.window / framed); after
each launch the allocation outside the window is untouched.  Four planted errors at the end lie on paths only a pin opens at
these shapes: the equality and oracle checks are not vacuous there."""
import ctypes as C

import numpy as np
import pytest
import torch

import bf16_exact
import bf16_plan_cases as B
import plan_cases as P
from bf16_plan_cases import CASES
from plan_cases import BWW_BF16, CONV_BF16, CONVT_BF16
from span_cases import SENTINEL, _bits, frame_intact, out_dims
from test_gpu_plan_space import framed, window

pytestmark = pytest.mark.gpu
TOL = 6e-3                                   # test_gpu_bf16.TOL: max error over the largest |ref|
TOL_SLAB, TOL_SLAB_L2 = 2e-5, 3e-6           # the standing kernel-gradient bars (test_gpu_bf16_multiunit)


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
def rb(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def operands(case):
    """-> (d, packed kernel or None, ref, S): bf16-rounded compact inputs, the bf16 kernel [tap][co][ci] as the entry point takes
    it, the float64 oracle result with tem_epilogue's order on out0 (bias, add, gate, keep bits, slope; out1 stays raw) and its
    magnitude twin for bf16_exact.store_interval; a kernel gradient has no kernel and no S"""
    from oracle import ops as O
    from oracle import torch_ops as T
    g, N = case.geom, case.N
    rng = np.random.default_rng(sum(map(ord, case.id)))
    d = {o: rb(rng.standard_normal((N,) + e)) for o, e in case.extents().items() if not o.startswith("out")}
    k, s, p = g["k"], g["s"], g["p"]
    ci, co = case.channels
    x = np.concatenate([d["in0"], d["in1"]], -1) if g["ci1"] else d["in0"]
    if case.family == BWW_BF16:
        return d, None, T.conv_bwd_weight(x, d["dout"], (k, k, k), s, p), None
    if g["entry"] == "convT_h":              # Keras' layout (tap, co, ci) is the packed one
        w = rb(rng.standard_normal((k, k, k, co, ci)) * 0.1)
        op = lambda xx, ww: T.convT_fwd(xx, ww, s, p, out_dims=out_dims(g))
        packed = w
    elif g["flip"]:                          # the input-gradient of a co -> ci layer, whose kernel (tap, co, ci) is read flipped
        w = rb(rng.standard_normal((k, k, k, co, ci)) * 0.1)
        op = lambda xx, ww: T.conv_fwd(xx, np.flip(ww, (0, 1, 2)).transpose(0, 1, 2, 4, 3).copy(), s, p)      # (a copy: no negative strides)
        packed = w
    else:
        w = rb(rng.standard_normal((k, k, k, ci, co)) * 0.1)
        op = lambda xx, ww: T.conv_fwd(xx, ww, s, p)
        packed = np.ascontiguousarray(w.reshape(-1, ci, co).transpose(0, 2, 1))
    ref, S = np.array(op(x, w), np.float64), np.array(op(np.abs(x), np.abs(w)), np.float64)
    assert ref.shape == (N,) + out_dims(g) + (co,)
    c0, K = g["co"], k ** 3 * ci
    if case.bias:
        d["bias"] = rng.standard_normal(c0).astype(np.float32)
        ref[..., :c0] += d["bias"].astype(np.float64)
        S[..., :c0] += np.abs(d["bias"]).astype(np.float64)
    if g["add"]:
        oz, oy, ox = case.add_off or (0, 0, 0)
        _, aD, aH, aW, _ = d["add"].shape
        ref[:, oz:oz + aD, oy:oy + aH, ox:ox + aW, :c0] += d["add"]
        S[:, oz:oz + aD, oy:oy + aH, ox:ox + aW, :c0] += np.abs(d["add"])
    keep = None
    if g["keep"]:
        keep = O.dropout_mask((N,) + out_dims(g) + (c0,), 42, 3, 7)           # the stream span_cases.Case.args names
        d["keep"] = np.packbits(keep.reshape(-1), bitorder="little")
    ref[..., :c0], S[..., :c0] = bf16_exact.epilogue64(ref[..., :c0], S[..., :c0], K, saved=d["gate"] if g["gate"] else None,
                                                        keep=keep, slope=g["slope"])
    return d, packed, ref, S


class Launcher:
    """one case on the device: operands placed once, then one launch per plan"""

    def __init__(self, lib, case):
        from transfer_em_amd import hip_ops as H
        self.lib, self.case, self.H = lib, case, H
        g, f = case.geom, case.family
        self.d, w, ref, S = operands(case)
        d = self.d
        self.ref_np, self.S_np, self.K = ref, S, g["k"] ** 3 * case.channels[0]
        self.ref = torch.from_numpy(ref).cuda()
        self.bufs, self.t, views = {}, {}, {}
        for o, e in case.extents().items():
            views[o], head = window(e, case.N)
            self.bufs[o], self.t[o] = framed(views[o], head, torch.bfloat16)
            if o in d:
                self.t[o].copy_(torch.from_numpy(d[o]).cuda())
        placed = B.Bf16Case(case.name, f, g, case.N, case.add_off, case.bias, case.decline)
        placed.views = views
        ptr = {o: t.data_ptr() for o, t in self.t.items()}
        self.outs = [o for o in ("out0", "out1") if o in views]
        if f == BWW_BF16:
            self.a = placed.args(ptr, 0)
            return
        if case.bias:
            self.bias = torch.from_numpy(d["bias"]).cuda()
            ptr["bias"] = self.bias.data_ptr()
        self.keep = torch.from_numpy(d["keep"]).cuda() if g["keep"] else None
        self.mask = None
        if g["keep"] == 1:                 # the launch draws the bits itself and writes them: a mask of its own inside a frame of bytes
            self.mask_ref, self.keep = self.keep, torch.full((self.keep.numel() + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            self.mask = self.keep
        self.w = torch.from_numpy(w.reshape(-1)).cuda().to(torch.bfloat16)
        self.a = placed.args(ptr, self.w.data_ptr(), keep_mask=self.keep.data_ptr() if self.keep is not None else 0)
        self.fn = lib.tem_conv_transpose_bf16 if f == CONVT_BF16 else lib.tem_conv_bf16

    def _guard(self, what, fn):
        try:
            return fn()
        except RuntimeError as e:                  # a device error: nothing more is launched on a card that may have faulted
            pytest.exit(f"{self.case.id} {what}: {e}", returncode=3)

    def forward(self, v4=None):
        """launch under pin v4 (None: the rule's own choice) -> (output window(s) compact, elements damaged outside them or in the
        keep mask, the plan read back)"""
        def go():
            with B.declined(self.lib, self.case):
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
        """slab-count query, launch and tem_reduce_slabs under pin v4, twice, each into a fresh workspace of the announced slabs
        + 2 sentinel ones -> (reduced gradient fp32, the two runs equal bit for bit in slabs and sum, sentinel elements lost behind
        the last slab or slabs left unwritten, plan)"""
        ci, co = self.case.channels
        n = self.case.geom["k"] ** 3 * ci * co

        def go():
            P.pin(self.lib, BWW_BF16, v4)
            taken, sym = P.describe(self.lib, self.case, self.a)              # sets a.nslab to the plan's slab count
            assert taken, (self.case.id, v4, sym)
            plan, R, runs, lost = P.last(self.lib, BWW_BF16), self.a.nslab, [], 0
            assert plan[7] == R
            for _ in range(2):
                slabs, out = torch.empty((R + 2, n), device="cuda"), torch.empty(n, device="cuda")
                _bits(slabs).fill_(SENTINEL[4])
                self.a.slabs, self.a.accumulate = slabs.data_ptr(), 0
                rc = self.lib.tem_conv_bwd_weight_bf16(C.byref(self.a), self.H.current_stream())
                assert rc == 0 and P.last(self.lib, BWW_BF16) == plan, (self.case.id, v4, rc)
                rc = self.lib.tem_reduce_slabs(slabs.data_ptr(), R, n, 0, out.data_ptr(), 0, 1.0, self.H.current_stream())
                assert rc == 0, (self.case.id, v4, rc)
                torch.cuda.synchronize()
                lost += int((_bits(slabs[R:]) != SENTINEL[4]).sum()) + int((_bits(slabs[:R]) == SENTINEL[4]).sum())
                runs.append((slabs[:R], out))
            P.pin(self.lib, BWW_BF16, None)
            same = torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1])
            return runs[0][1].reshape(self.ref.shape), same, lost, plan
        return self._guard(v4, go)

    def error(self, got):
        """(max error over the largest |ref|, L2 error over |ref|'s), computed on the device"""
        diff = got.double() - self.ref
        return (float(diff.abs().max() / (self.ref.abs().max() + 1e-30)),
                float(torch.linalg.vector_norm(diff) / (torch.linalg.vector_norm(self.ref) + 1e-30)))


# ------------------------------------------------------------------------------------------------ the sweep
FORWARD = CASES[CONV_BF16] + CASES[CONVT_BF16]


@pytest.mark.parametrize("case", FORWARD, ids=lambda c: c.id)
def test_every_plan_equals_the_default_plan_which_matches_the_oracle(lib, case):
    run = B.sweep_list(lib, case)
    L = Launcher(lib, case)
    base, bad, plan = L.forward()
    assert plan == B.default_plan(lib, case) and plan in run
    err, _ = L.error(base)
    print(f"{case.id}: default {dict(zip(P.FIELDS[case.family], plan))} error {err:.3g} (bar {TOL:.3g}); {len(run)} plans")
    assert bad == 0 and bool(torch.isfinite(base).all()), (case.id, plan, bad)
    assert err <= TOL, (case.id, plan, err)
    bf16_exact.assert_bf16_stores(base.float().cpu().numpy(), L.ref_np, L.S_np, L.K, case.id)
    wrong = []
    for v in run:
        got, bad, plan = L.forward(B.pin_of(case.family, v))
        if plan != v:
            wrong.append((v, "read back", plan))
        elif bad or not bool(torch.isfinite(got).all()):
            wrong.append((v, "outside the window or keep bits" if bad else "not finite", bad))
        elif not torch.equal(got, base):
            wrong.append((v, "differs from the default plan", float((got.double() - base.double()).abs().max())))
    assert not wrong, (case.id, len(wrong), len(run), wrong[:8])


@pytest.mark.parametrize("case", CASES[BWW_BF16], ids=lambda c: c.id)
def test_every_kernel_gradient_plan_matches_the_oracle_and_reproduces_itself(lib, case):
    """A pad-1 / pad-3 case is a transposed layer's kernel gradient with input and gradient swapped: oracle.torch_ops.convT_bwd_weight
    of the swapped operands is held to the same numbers."""
    from oracle import torch_ops as T
    run = B.sweep_list(lib, case)
    L = Launcher(lib, case)
    if case.variant.endswith("T"):
        refT = T.convT_bwd_weight(L.d["dout"], L.d["in0"], (4, 4, 4), 2, case.geom["p"])
        assert refT.shape == L.ref_np.shape and float(np.abs(refT - L.ref_np).max()) <= 1e-9 * float(np.abs(L.ref_np).max())
    feasible = B.enumerate_plans(lib, case)
    twin = {(v[0], v[2]): v for v in feasible if v[4] == 1}       # the single launch of a band height and z split, where one fits
    expect = sum(1 for v in run if v[4] > 1 and (v[0], v[2]) in twin)
    wrong, worst, single, compared = [], (0.0, 0.0), {}, 0

    def one(v):
        got, same, lost, plan = L.gradient(None if v is None else B.pin_of(BWW_BF16, v))
        err, l2 = L.error(got)
        if v is None:
            assert plan == B.default_plan(lib, case) and plan in run
            v = plan
        if plan != v:
            wrong.append((v, "read back", plan))
        elif not same:
            wrong.append((v, "two runs differ"))
        elif lost:
            wrong.append((v, "slabs behind the last written, or announced slabs left unwritten", lost))
        elif not (err <= TOL_SLAB and l2 <= TOL_SLAB_L2):          # (a NaN fails both)
            wrong.append((v, "oracle", err, l2))
        else:
            return got, (err, l2)
        return None, (err, l2)
    for v in [None] + run:
        got, e = one(v)
        worst = max(worst, e)
        if got is None or v is None:
            continue
        if v[4] == 1:
            single[v[0], v[2]] = got
        elif (v[0], v[2]) in twin:                                 # (a twin the thinning left out of the list is launched for this)
            if (v[0], v[2]) not in single:
                single[v[0], v[2]], e = one(twin[v[0], v[2]])
                worst = max(worst, e)
            if single[v[0], v[2]] is None:
                continue
            compared += 1
            diff = got.double() - single[v[0], v[2]].double()
            dm, dl = float(diff.abs().max() / L.ref.abs().max()), float(torch.linalg.vector_norm(diff) / torch.linalg.vector_norm(L.ref))
            if not (dm <= TOL_SLAB and dl <= TOL_SLAB_L2):
                wrong.append((v, "segmented against the single launch", dm, dl))
    nseg = sum(1 for v in run if v[4] > 1)
    print(f"{case.id}: {nseg} segmented plans, {compared} held to their single launch ({nseg - expect}: no single launch of that band fits)")
    assert compared == expect or wrong, (case.id, compared, expect)
    print(f"{case.id}: {len(run)} plans, worst error {worst[0]:.3g} (bar {TOL_SLAB:.3g}), L2 {worst[1]:.3g} (bar {TOL_SLAB_L2:.3g})")
    assert not wrong, (case.id, len(wrong), len(run), wrong[:8])


# ------------------------------------------------------------------------------------------------ sensitivity
# What a changed input voxel does: an output below it moves by BUMP times kernel entries of 0.1 N(0, 1) summed over the taps and
# channels that reach it -- a standard deviation of 0.1 BUMP sqrt(taps C_in) >= 0.8 BUMP / 3 -- hundreds of times the bar of 6e-3
# of a scale of ~6 over a row or column of outputs.  The tests ask for ten times the bar.
BUMP = 8.0


def _case(family, variant, channels, k, tag):
    return next(c for c in CASES[family] if c.variant == variant and c.channels == channels and c.geom["k"] == k and
                c.name.split("-", 3)[3] == tag)


def _bar(L):
    return TOL * float(L.ref.abs().max())


def test_the_comparison_sees_an_error_only_a_ragged_last_patch_column_makes(lib):
    """conv_bf16_k 8 -> 8 k3 s1 at (4, 6, 9) x 2, pad 0: one patch per plane by default.  With TY 4, nbx 2 pinned there are two
    columns of TX 5 | 4 and two bands of 4 | 2 rows; the last input column ix = 10 reaches the output column ox = 8 alone -- the
    ragged column's last voxel, whose tiles run over a full-width patch."""
    case = _case(CONV_BF16, "plain", (8, 8), 3, "small")
    assert case.geom["p"] == 0 and B.default_plan(lib, case)[:4] == (6, 1, 9, 1)
    L = Launcher(lib, case)
    clean, _, plan = L.forward((4, 2))
    assert plan[:4] == (4, 2, 5, 2) and L.error(clean)[0] <= TOL
    L.t["in0"][:, :, :, -1] += BUMP
    got, bad, plan = L.forward((4, 2))
    assert plan[:4] == (4, 2, 5, 2) and bad == 0
    per_col = (got.double() - L.ref).abs().amax(dim=(0, 1, 2, 4))
    assert per_col.numel() == 9 and float(per_col[:8].max()) <= _bar(L) and float(per_col[8]) > 10 * _bar(L), (_bar(L), per_col.tolist())
    assert torch.equal(got[:, :, :, :8], clean[:, :, :, :8])


def test_the_comparison_sees_an_error_only_a_second_bands_halo_makes(lib):
    """convT_bf16_k 16 -> 8, input (3, 5, 6), pad 1: nQy = 6, one band by default.  TY = 3 pinned makes two; the second holds
    Q_y = 3 .. 5, output rows 5 .. 9.  The last input row j_y = 4 reaches the output rows 2 j_y + t - 1 = 7 .. 9 alone, through
    Q_y = 4 and 5: the second band's patch."""
    case = _case(CONVT_BF16, "plain", (16, 8), 4, "small")
    assert B.default_plan(lib, case)[:2] == (6, 1)
    L = Launcher(lib, case)
    clean, _, plan = L.forward((3,))
    assert plan[:2] == (3, 2) and L.error(clean)[0] <= TOL
    L.t["in0"][:, :, -1] += BUMP
    got, bad, plan = L.forward((3,))
    assert plan[:2] == (3, 2) and bad == 0
    per_row = (got.double() - L.ref).abs().amax(dim=(0, 1, 3, 4))
    assert per_row.numel() == 10 and float(per_row[:7].max()) <= _bar(L) and float(per_row[7:].min()) > 10 * _bar(L), (_bar(L), per_row.tolist())
    assert torch.equal(got[:, :, :7], clean[:, :, :7])


def test_the_gradient_comparison_sees_an_error_only_the_march_makes(lib):
    """bww_bf16_k 16 -> 16 k3 s1 at (8, 7, 40) x 2, pad 0: one plane per workgroup by default.  With the whole z axis in one run
    (TY 3, zsegs 1) the last input plane is read by the run's last step alone, through the tap plane kz = 2: with that plane
    changed on the device the result must leave the reference in those taps and in no other."""
    case = _case(BWW_BF16, "p0", (16, 16), 3, "small")
    assert B.default_plan(lib, case)[:4] == (7, 1, 8, 1)
    L = Launcher(lib, case)
    clean, same, lost, plan = L.gradient((3, 1, 48))
    assert plan[:6] == (3, 3, 1, 8, 1, 40) and same and not lost and L.error(clean)[0] <= TOL_SLAB
    L.t["in0"][:, -1] += BUMP
    got, same, lost, plan = L.gradient((3, 1, 48))
    assert plan[:6] == (3, 3, 1, 8, 1, 40) and same and not lost
    bound = TOL_SLAB * float(L.ref.abs().max())
    per_tap = (got.double() - L.ref).abs().amax(dim=(1, 2, 3, 4))
    assert float(per_tap[:2].max()) <= bound and float(per_tap[2]) > 10 * bound, per_tap.tolist()


def test_the_gradient_comparison_sees_an_error_in_the_padded_last_k_block(lib):
    """the same case, rows of 40 = two k-blocks of 16 and a third of 8 voxels and 8 zeros, in bands of 3 | 3 | 1 rows: with the
    gradient's last column -- in the padded k-block -- of the last row -- the ragged band -- changed on the device, the result
    must leave the reference and meet the oracle's kernel gradient of the changed operand."""
    from oracle import torch_ops as T
    case = _case(BWW_BF16, "p0", (16, 16), 3, "small")
    L = Launcher(lib, case)
    L.t["dout"][:, :, -1, -1] += BUMP
    got, same, lost, plan = L.gradient((3, 2, 48))
    assert plan[:6] == (3, 3, 2, 4, 1, 40) and same and not lost
    assert L.error(got)[0] > 10 * TOL_SLAB
    ref2 = torch.from_numpy(T.conv_bwd_weight(L.t["in0"].float().cpu().numpy(), L.t["dout"].float().cpu().numpy(), (3, 3, 3), 1, 0)).cuda()
    assert float((got.double() - ref2).abs().max() / ref2.abs().max()) <= TOL_SLAB
