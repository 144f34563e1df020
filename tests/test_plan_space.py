"""The launch plans of wino_conv_k, wino_bww_k, conv_lds_k and conv3_bf16_k through the pin / readback seam of the C ABI
(tem_plan_pin, tem_plan_last), without a GPU: the dry queries take made-up pointers, as in tests/test_span_routing.py.

* a pin comes back as pinned, with derived fields that follow from it; a pin no candidate matches is refused and changes
  nothing; a pinned query neither reads nor writes the planner's memo;
* the feasible plans of every case of tests/plan_cases.py, enumerated through the library, take every value of every
  class coordinate somewhere in the family's sweep, and hold the default plan;
* every launch of the workload that one of the four kernels takes -- the step-shape tables of
  test_gpu_fullsize_oracle.py and test_gpu_bf16_fullsize_oracle.py, utils.plan_routes of the 132 and 260 models -- has a
  default plan whose class signature the GPU sweep (tests/test_gpu_plan_space.py) executes for the same kernel instance.
  A cost-model change that moves a layer onto a plan class no oracle-checked test has run fails here;
* the same for the one pinned number of conv_s2_k, convT_mfma_k and bww_s2_k / bww_s2tb_k (section "the k4 s2 kernels"): the seam,
  the unpinned geometry held to a restatement of the three rules, every class value in every kernel
  instance's sweep, and the class signature of every k4 s2 launch of the 74, 132 and 260 train steps inside it."""
import ctypes as C

import pytest
import torch

import plan_cases as P
from plan_cases import BWW_S2, CASES, CONV3_BF16, CONVT_MFMA, CONV_LDS, CONV_S2, FAMILIES, KERNEL, PLANNED, S2, WINO, WINO_BWW
from span_cases import _g, out_dims


@pytest.fixture(scope="module")
def lib():
    from transfer_em_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def _no_pin_left(lib):
    yield
    P.clear_pins(lib)


def _case(family, tag, variant=None, channels=None):
    return next(c for c in CASES[family] if c.name.endswith(tag) and (variant is None or c.variant == variant) and
                (channels is None or c.channels == channels))


def ceil(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the seam
def test_readback_before_any_decision_and_unknown_family():
    """(in a fresh thread: the pin and the last plan are per thread)"""
    import threading
    from transfer_em_amd import _lib
    lib, seen = _lib.load(), {}

    def ask():
        v = (C.c_int32 * 8)()
        seen["last"] = [lib.tem_plan_last(f, v) for f in FAMILIES]
        past = max(FAMILIES) + 1                                        # the first number past the last family
        seen["unknown"] = [lib.tem_plan_last(0, v), lib.tem_plan_last(past, v), lib.tem_plan_pin(0, None), lib.tem_plan_pin(past, None)]
        seen["null"] = lib.tem_plan_last(WINO, None)
        c = _case(WINO, "small", "ep0", (16, 16))
        seen["plan"] = P.decide(lib, c, (17, 2, 3, 1))
    P.decide(lib, _case(WINO, "small", "ep0", (16, 16)))                # this thread has decided; the other has not
    t = threading.Thread(target=ask)
    t.start(); t.join()
    assert seen["last"] == [P.EINVAL] * len(FAMILIES) and seen["unknown"] == [P.EINVAL] * 4 and seen["null"] == P.EINVAL
    assert seen["plan"][:4] == (17, 2, 3, 1)
    c = _case(WINO, "small", "ep0", (16, 16))
    assert P.decide(lib, c) == P.default_plan(lib, c) and P.decide(lib, c)[:4] != (17, 2, 3, 1)      # the other thread's pin is not ours


@pytest.mark.parametrize("family", PLANNED, ids=lambda f: KERNEL[f])
def test_pin_in_pin_out(lib, family):
    """every feasible plan of the family's first large case: the pinned fields come back, the derived ones follow from them,
    and a partial pin leaves the planner its choice among the rest"""
    case = _case(family, P.LARGE[family])
    plans = P.enumerate_plans(lib, case)                   # (asserts readback == pin and the family's kernel per plan)
    assert len(plans) > 40 and len(set(plans)) == len(plans)
    _, OH, OW = out_dims(case.geom)
    n = P.zaxis(case)
    for v in plans:
        if family in (WINO, WINO_BWW):
            E, BY, BX, zsegs, zper, nby, nbx, ndma = v
            assert (nby, nbx) == (ceil(ceil(OH, 2), BY), ceil(ceil(OW, 2), BX)) and BX + 1 <= E and BY * BX <= P.tile_cap(case)
            assert 1 <= ndma <= P.dma_cap(case)
        elif family == CONV_LDS:
            MTW, R, patch, zsegs, zper, nych, ntiles, zero = v
            assert nych == ceil(OH, R) and zero == 0 and ntiles * ceil(case.channels[1], 16) <= MTW * 8
        else:
            nbx, TY, zsegs, zper, nby, RD, ndma, zero = v
            assert nby == ceil(OH, TY) and RD == case.geom["k"] + case.geom["s"] and zero == 0 and ndma >= 1
        assert zper == ceil(n, zsegs) and zsegs == ceil(n, zper)
    free = P.decide(lib, case, (-1, -1, -1, -1))
    assert free == P.default_plan(lib, case)               # nothing pinned: the planner's own choice
    v = plans[len(plans) // 2]
    part = P.decide(lib, case, (v[0], -1, -1, -1))
    assert part is not None and part[0] == v[0] and part in plans


def test_infeasible_pins_are_refused_and_change_nothing(lib):
    w = _case(WINO, "15x31x31", "ep0", (16, 16))               # 16 x 16 tiles, 8 z steps, at most 64 tiles per workgroup
    b = _case(WINO_BWW, "15x31x31", "p0", (16, 16))
    l = _case(CONV_LDS, "8x16x21", "plain", (16, 16))
    h = _case(CONV3_BF16, "9x24x33", "plain", (8, 8))
    bad = [(w, (9, 9, 8, 1), "BY x BX = 72 tiles, above the cap of 64"), (w, (17, 5, 13, 1), "65 tiles"),
           (w, (9, 2, 9, 1), "BX + 1 > E"), (w, (9, 2, 16, 1), "BX + 1 > E"), (w, (11, 2, 4, 1), "no such pitch"),
           (w, (9, 2, 4, 5), "5 z-runs: runs of 2 steps make 4"), (w, (9, 2, 4, 7), "7 z-runs: likewise"),
           (w, (9, 17, 1, 1), "more tile rows than the output has"),
           (b, (9, 4, 3, 1), "odd BX: wino_bww_k pairs tiles along x"), (b, (9, 4, 1, 1), "odd BX"), (b, (9, 9, 8, 1), "72 tiles"),
           (b, (9, 2, 10, 1), "BX + 1 > E"), (b, (9, 2, 4, 6), "6 z-runs"),
           (l, (3, 1, 20, 1), "no MTW 3"), (l, (4, 17, 20, 1), "R above 16"), (l, (4, 1, 8, 1), "no patch 8"), (l, (4, 1, 20, 5), "5 z-runs of 8 planes"),
           (h, (1, 25, 1), "TY above 24"), (h, (1, 1, 1), "TY below 2"), (h, (3, 2, 1), "three columns of 33 voxels are narrower than 16"),
           (h, (1, 2, 7), "7 z-runs of 9 planes")]
    for case, v4, why in bad:
        want = P.default_plan(lib, case)
        assert want is not None and P.last(lib, case.family) == want
        a = P.dry_args(case)
        with P.pinned(lib, case.family, v4):
            taken, sym = P.describe(lib, case, a)
            assert not taken and not sym.startswith(KERNEL[case.family]), (case.id, v4, why, sym)
            if case.family == WINO_BWW:
                a.nslab = P.MAX_SLABS
                assert lib.tem_conv_bwd_weight_winograd_nslab(C.byref(a), None, 0) == P.EUNSUPPORTED, (v4, why)
            elif case.family == WINO:
                assert sym == "", (v4, why, sym)                   # the Winograd layout has no other reader: refused outright
            assert P.last(lib, case.family) == want, (case.id, v4, why)         # the refusal left the last decision alone
        assert P.default_plan(lib, case) == want, (case.id, v4, why)
    # the refusals are the planner's, not the seam's: each pin's neighbour is feasible
    for case, v4 in [(w, (9, 8, 8, 1)), (w, (17, 4, 16, 1)), (w, (9, 2, 8, 4)), (w, (9, 8, 1, 1)), (b, (9, 4, 4, 1)), (b, (9, 8, 8, 1)),
                     (l, (4, 16, 20, 1)), (l, (4, 1, 16, 4)), (h, (1, 24, 1)), (h, (2, 2, 5))]:
        assert P.decide(lib, case, v4)[:len(v4)] == v4, (case.id, v4)


def _fresh(family, od, N=3):
    """a case at output extents no other test asks about (the memo is the process's)"""
    ci, co = {WINO: (16, 16), WINO_BWW: (16, 16), CONV_LDS: (16, 16), CONV3_BF16: (8, 8)}[family]
    g = _g(P.ENTRY[family], ci, co, 3, 1, 0, tuple(d + 2 for d in od), wino=family == WINO)
    return P.PlanCase(f"fresh-{od}", family, g, N)


@pytest.mark.parametrize("family", PLANNED, ids=lambda f: KERNEL[f])
def test_a_pinned_query_neither_reads_nor_writes_the_memo(lib, family):
    """the other plan: one run over the whole z axis with the smallest tile block -- never the cost model's choice for a
    batch of three at these sizes, so a memo that had kept it would answer the unpinned query with it"""
    other = {WINO: (9, 1, 2, 1), WINO_BWW: (9, 1, 2, 1), CONV_LDS: (1, 1, 0, 1), CONV3_BF16: (1, 2, 1)}[family]
    # unpinned first: the memo holds the default, the pinned query must not read it, the third must still find it
    c = _fresh(family, (11, 14, 35))
    first = P.decide(lib, c)
    assert first is not None and first[:len(other)] != other
    assert P.decide(lib, c, other)[:len(other)] == other
    assert P.decide(lib, c) == first
    # pinned first, on a geometry not asked before: the memo must not have kept the pinned plan
    c = _fresh(family, (12, 15, 34))
    assert P.decide(lib, c, other)[:len(other)] == other
    second = P.decide(lib, c)
    assert second is not None and second[:len(other)] != other
    assert P.decide(lib, c, other)[:len(other)] == other and P.decide(lib, c) == second


# ------------------------------------------------------------------------------------------------ enumeration
@pytest.mark.parametrize("case", P.ALL_CASES, ids=lambda c: c.id)
def test_case_is_the_familys_and_its_default_plan_is_in_the_list(lib, case):
    taken, sym = P.describe(lib, case, P.dry_args(case))
    assert taken, (case.id, sym)
    plans = P.enumerate_plans(lib, case)
    d = P.default_plan(lib, case)
    assert d in plans, (case.id, d)
    run = P.sweep_list(lib, case)
    assert d in run and set(run) <= set(plans)
    assert {P.signature(case, v, plans) for v in run} == {P.signature(case, v, plans) for v in plans}      # thinning loses no class
    assert (len(run) == len(plans)) if case.small else (len(run) <= 170), (case.id, len(run), len(plans))


@pytest.mark.parametrize("family", PLANNED, ids=lambda f: KERNEL[f])
def test_every_value_of_every_class_coordinate_is_swept(lib, family):
    """the condition the sweep shapes were chosen by (plan_cases.SHAPES): over the family's cases, every coordinate takes
    every one of its values; and every kernel instance sees every z-run class and both pitches / all MTW"""
    have, per = {c: set() for c in P.COORDS}, {}
    for case in CASES[family]:
        plans = P.enumerate_plans(lib, case)
        for v in P.sweep_list(lib, case):
            s = P.signature(case, v, plans)
            for c, x in zip(P.COORDS, s):
                have[c].add(x)
            per.setdefault(P.instance(case), set()).add(s)
    assert have == P.VALUES[family], {c: P.VALUES[family][c] ^ have[c] for c in P.COORDS}
    for inst, sigs in per.items():
        assert {(s[0], s[1]) for s in sigs} == {("all", False), ("1", False), ("2", False), ("2", True), ("3+", False), ("3+", True)}, inst
        assert {s[2] for s in sigs} == {"min", "div", "rag"}, inst
        if family != CONV3_BF16:
            assert {s[4] for s in sigs} == P.VALUES[family]["third"], inst


def test_feasible_plan_counts(lib):
    """the numbers of DESIGN.md's "Plan space" table"""
    count = lambda f, tag, var, ch: len(P.enumerate_plans(lib, _case(f, tag, var, ch)))
    assert [count(WINO, "small", "ep0", p) for p in P.WINO_PAIRS] == [120, 120, 120, 120, 90, 90, 75]
    assert [count(WINO, "15x31x31", "ep0", p) for p in P.WINO_PAIRS] == [1410, 885, 790, 790, 375, 400, 240]
    assert [count(WINO_BWW, "15x31x31", "p0", p) for p in [(8, 8), (16, 16), (32, 16), (32, 32)]] == [435, 435, 220, 220]
    assert [count(CONV_LDS, "8x16x21", "plain", p) for p in [(16, 16), (16, 32), (32, 16), (32, 32)]] == [480, 270, 450, 270]
    assert [count(CONV3_BF16, "9x24x33", "plain", p) for p in [(8, 8)]] == [230]


# ------------------------------------------------------------------------------------------------ the workload
def _swept(lib):
    out = {}
    for case in P.ALL_CASES:
        plans = P.enumerate_plans(lib, case)
        out.setdefault(P.instance(case), set()).update(P.signature(case, v, plans) for v in P.sweep_list(lib, case))
    return out


def _family_of(sym):
    return next((f for f in PLANNED if sym.startswith(KERNEL[f] + "<")), None)


def _case_of_args(family, a, name):
    """the PlanCase of an argument struct a workload launch was asked with"""
    ci1 = a.in1.C if a.in1.ptr else 0
    if family == WINO_BWW:
        g = _g("bww_wino", a.in0.C, a.dout.C, a.kd, a.sd, a.pd, (a.in0.D, a.in0.H, a.in0.W), ci1=ci1)
    else:
        co1 = a.out1.C if a.out1.ptr else 0
        g = _g(P.ENTRY[family], a.in0.C, a.out0.C, a.kd, a.sd, a.pd, (a.in0.D, a.in0.H, a.in0.W), ci1=ci1, co1=co1)
        assert out_dims(g) == (a.out0.D, a.out0.H, a.out0.W), name
    return P.PlanCase(name, family, g, a.in0.N)


def _table_launches(lib):
    """(name, case) of the step-shape tables' rows that one of the four kernels takes"""
    import test_gpu_bf16_fullsize_oracle as BO
    import test_gpu_fullsize_oracle as FO
    rows = []

    def add(name, family, entry, ci0, ci1, co0, co1, k, s, p, n, want, **kw):
        if co1 and family == WINO:
            kw.update(keep=2)                               # the split output comes with the keep bits (EP 2)
        g = _g(entry, ci0, co0, k, s, p, (n, n, n), ci1=ci1, co1=co1, wino=family == WINO, **kw)
        case = P.PlanCase(name, family, g, 1)
        taken, sym = P.describe(lib, case, P.dry_args(case))
        assert taken and sym.startswith(want), (name, sym, want)
        rows.append((name, case))
    for layer, ci0, ci1, co, n, *_ in FO.WINO_FWD:
        add(layer, WINO, "conv", ci0, ci1, co, 0, 3, 1, 0, n, "wino_conv_k")
    for layer, ci, co0, co1, n, _mask in FO.WINO_BWD:
        add(layer, WINO, "conv", ci, 0, co0, co1, 3, 1, 2, n, "wino_conv_k", flip=True, slope=1.0, gate=True)
    for layer, ci, co, k, s, pad, n, kern in FO.BWW:
        if kern.startswith("wino_bww_k"):
            add(layer, WINO_BWW, "bww_wino", ci, 0, co, 0, k, s, pad, n, "wino_bww_k")
    for c in BO.CONV:
        if c["kernel"].startswith("conv3_bf16_k"):
            add("bf16 " + c["name"], CONV3_BF16, "conv_h", c["ci0"], c["ci1"], c["co0"], c["co1"], c["k"], c["s"], c["p"], c["n"],
                c["kernel"], slope=c["slope"], gate=c["gate"] is not None, add=c["add"] is not None, keep=2 if c["drop"] else 0)
    return rows


class _Recorder:
    """stands in for the loaded library inside utils.plan_routes: every dry query is passed on and, where one of the four
    kernels answered, the argument struct and the plan of that decision are kept"""

    def __init__(self, lib, tag):
        self.lib, self.tag, self.seen = lib, tag, []

    def __getattr__(self, fn):
        real = getattr(self.lib, fn)

        def call(ref, *rest):
            rc = real(ref, *rest)
            buf = next((r for r in rest if isinstance(r, C.Array)), None)
            f = _family_of(buf.value.decode()) if buf is not None else None
            if f and (rc == 1 if fn == "tem_conv_is_tiled" else rc == 0):
                case = _case_of_args(f, ref._obj, f"{self.tag} {buf.value.decode()}")
                self.seen.append((case.name, case, P.last(self.lib, f)))
            return rc
        return call


def _model_launches(lib, monkeypatch):
    from transfer_em_amd import _lib, utils
    out = []
    for edge in (132, 260):
        for dtype in (torch.float32, torch.bfloat16):
            for N in sorted({1, utils.default_tile_batch(edge, True)}):
                rec = _Recorder(lib, f"{edge} {'bf16' if dtype == torch.bfloat16 else 'fp32'} N={N}")
                monkeypatch.setattr(_lib, "load", lambda rec=rec: rec)
                routes = utils.plan_routes(edge, N, True, dtype)
                monkeypatch.undo()
                assert len(rec.seen) == sum(_family_of(k) is not None for k in routes.values()), (rec.tag, routes)
                out += rec.seen
    return out


def test_the_workloads_default_plans_stay_inside_the_sweep(lib, monkeypatch):
    swept = _swept(lib)
    launches = [(name, case, P.default_plan(lib, case)) for name, case in _table_launches(lib)] + _model_launches(lib, monkeypatch)
    assert len(launches) > 80 and {c.family for _, c, _ in launches} >= {WINO, WINO_BWW, CONV3_BF16}
    outside = []
    for name, case, plan in launches:
        assert plan is not None and plan == P.default_plan(lib, case), name
        feasible = P.enumerate_plans(lib, case) if case.family == CONV3_BF16 else None      # (its dcap is read off the list)
        sig = P.signature(case, plan, feasible)
        print(f"{name}: {dict(zip(P.FIELDS[case.family], plan))} {sig}")
        if sig not in swept.get(P.instance(case), ()):
            outside.append((name, plan, sig))
    assert not outside, "\n".join(map(str, outside))


# ------------------------------------------------------------------------------------------------ the k4 s2 kernels
# conv_s2_k, convT_mfma_k, bww_s2_k / bww_s2tb_k: one pinned number each, in place of the closed-form rule's
@pytest.fixture(scope="module")
def s2_plans(lib):
    """{case id: (default plan, feasible list)} of every k4 s2 case"""
    return {c.id: (P.default_plan(lib, c), P.enumerate_plans(lib, c)) for f in S2 for c in CASES[f]}


def _refused(lib, case, x):
    """a pin outside the family's range: the family declines (the C ABI shows it by what answers instead) -> the symbol the
    dry query names"""
    a = P.dry_args(case)
    with P.pinned(lib, case.family, (x,)):
        taken, sym = P.describe(lib, case, a)
        assert not taken and not sym.startswith(P.SYMBOLS[case.family]), (case.id, x, sym)
    return sym


@pytest.mark.parametrize("family", S2, ids=lambda f: KERNEL[f])
def test_s2_pin_in_pin_out(lib, s2_plans, family):
    """every case: the accepted pins are 1 .. K without a gap, K the valid range of include/tem_hip.h's table; the pinned number
    comes back and nothing else moves but what follows from it; 0 and K + 1 are refused by the family (TEM_EUNSUPPORTED inside
    the library: tem_conv_is_tiled / tem_bww_is_tiled go on and name the next kernel, or none for a transposed layer, whose direct
    form has no dry query), and the refusal leaves the last decision alone"""
    nxt = {CONV_S2: lambda sym: sym.startswith(("conv_lds_k<", "conv_direct_k<")), CONVT_MFMA: lambda sym: sym == "",
           BWW_S2: lambda sym: sym == "" or sym.startswith("bww_lds_k<")}[family]
    for case in CASES[family]:
        d, plans = s2_plans[case.id]
        K = len(plans)
        assert [v[0] for v in plans] == list(range(1, K + 1)) and d in plans, (case.id, d, plans)
        if family == CONV_S2:
            assert K == min(d[3], d[7]) and all(v[1:] == d[1:] for v in plans), case.id            # min(iters, resident)
        elif family == CONVT_MFMA:
            assert d[0] <= K <= min(d[3], 32), case.id                                            # the hard bounds may stop short of nQy
            assert all(v[1] == ceil(v[3], v[0]) and v[2:] == d[2:] for v in plans), case.id
        else:
            assert K == min(d[1], P.MAX_SLABS) and all(v[1:] == d[1:] for v in plans), case.id     # min(rows, max slabs)
        assert P.decide(lib, case, (-1, -1, -1, -1)) == d
        for x in (0, K + 1, 1 << 20):
            want = P.default_plan(lib, case)
            sym = _refused(lib, case, x)
            assert nxt(sym), (case.id, x, sym)
            assert P.last(lib, family) == want, (case.id, x)
        assert P.default_plan(lib, case) == d                                                      # set and clear: nothing moved


def test_s2_slab_count_is_the_pinned_R_and_the_budget_still_binds(lib):
    case = _case(BWW_S2, "small", "p0", (16, 16))
    a = P.dry_args(case)
    for R in (1, 7, 30):
        with P.pinned(lib, BWW_S2, (R,)):
            a.nslab = P.MAX_SLABS
            assert lib.tem_conv_bwd_weight_nslab(C.byref(a)) == R
            a.nslab = R
            name = C.create_string_buffer(96)
            assert lib.tem_bww_is_tiled(C.byref(a), name, 96) == 1 and name.value.startswith(b"bww_s2_k<"), name.value
            assert P.last(lib, BWW_S2)[0] == R
    with P.pinned(lib, BWW_S2, (7,)):                    # a pin above the caller's slab budget: max_slabs applies unchanged
        a.nslab = 6
        assert lib.tem_conv_bwd_weight_nslab(C.byref(a)) != 7


@pytest.mark.parametrize("family", S2, ids=lambda f: KERNEL[f])
def test_s2_pins_are_per_thread(lib, family):
    import threading
    case = CASES[family][0]
    d, seen = P.default_plan(lib, case), {}
    P.pin(lib, family, (1,))                             # stays set in this thread while the other one asks

    def ask():
        seen["before"] = P.last(lib, family)
        seen["plan"] = P.decide(lib, case)
    t = threading.Thread(target=ask)
    t.start(); t.join()
    assert seen["before"] is None and seen["plan"] == d and d[0] != 1
    assert P.last(lib, family) == d and P.decide(lib, case, None, P.dry_args(case))[0] == 1      # ours is still pinned
    P.pin(lib, family, None)
    assert P.decide(lib, case) == d


# The three closed-form rules, restated: unpinned, the seam must not move any launch's geometry.
S2_INSTANCE = {(8, 8): (4, 1, 1), (8, 16): (2, 1, 0), (16, 16): (2, 1, 0), (16, 32): (2, 2, 0), (32, 32): (1, 1, 0)}     # conv_s2_k: T, NT, TB


def _rule(case, v, max_slabs=P.MAX_SLABS):
    (ci, co), g, N = case.channels, case.geom, case.N
    OD, OH, OW = out_dims(g)
    if case.family == CONV_S2:
        T, NT, TB = S2_INSTANCE[(ci, co)]
        tiles_pp = ceil(OH * (OW + TB), 16 - TB)
        total = N * OD * tiles_pp
        iters, ny = ceil(total, T), ceil(co, 16 * NT)
        resident = 256 * (2 if ci == 8 else 1) // ny
        return (min(iters, resident), ny, T, iters, total, tiles_pp, TB, resident)
    if case.family == CONVT_MFMA:
        p = g["p"]
        nQz, nQy, nQx = ((o - 1 + p) // 2 - p // 2 + 1 for o in (OD, OH, OW))
        TY = 0
        for ty in range(1, min(nQy, 32) + 1):
            if 2 * (ty + 1) * (nQx + 1) * (ci // 4) > 12 * 256 or (2 * (ty + 1) * (nQx + 1) * (ci + 2) + 4 * 16 * 20 + 4) * 4 > 56 * 1024:
                break
            TY = ty
            if ceil(ty * nQx, 16) >= 16:
                break
        return (TY, ceil(nQy, TY), nQz, nQy, nQx, 1, v[6], 0)
    k, rows = g["k"], N * OD * OH
    tb = int(k == 4 and (ci, co) == (8, 8))
    if tb:
        R, least = 512, 8
    else:
        lds = 0 if ci == 32 else 4 * k * (ci // 4) * ceil(co, 16) * 64 * 16
        R, least = (128 if lds <= 80 * 1024 and ci != 32 else 64), (2 if ci == 32 else 8)
    while R > 1 and rows // R < least:
        R >>= 1
    return (min(R, max_slabs), rows, tb, k, OW, 0, 0, 0)


def _s2_family_of(sym):
    return next((f for f in S2 if sym.startswith(P.SYMBOLS[f])), None)


_STEP_LAUNCHES = []


def _step_launches(lib, monkeypatch):
    """(name, case, default plan, slab budget) of every launch of the 3-D fp32 train steps at 74, 132 and 260 that one of the k4 s2
    kernels takes: the launch lists tests/test_step_admission.py builds, each asked again from its finished struct"""
    if _STEP_LAUNCHES:
        return _STEP_LAUNCHES
    import test_step_admission as SA
    from fullsize_cases import launch_struct
    from transfer_em_amd import _lib
    for n, is3d, prec, b in SA.CONFIGS:
        if not is3d or prec != "fp32":
            continue
        with SA.dry_step(monkeypatch, n, is3d, prec, b) as st:
            for l in st.compute + st.update:
                a, f = launch_struct(l), _s2_family_of(l.meta.get("kernel") or "")
                if a is None or f is None:
                    continue
                name, buf = f"{n} b{b} {l.name}", C.create_string_buffer(96)
                if f == BWW_S2:
                    assert lib.tem_conv_bwd_weight_nslab(C.byref(a)) == a.nslab, name
                    g = _g("bww", a.in0.C, a.dout.C, a.kd, a.sd, a.pd, (a.in0.D, a.in0.H, a.in0.W))
                    g["out"], budget = (a.dout.D, a.dout.H, a.dout.W), a.nslab
                else:
                    assert lib.tem_conv_is_tiled(C.byref(a), int(f == CONVT_MFMA), buf, 96) == 1 and buf.value.decode() == l.meta["kernel"], name
                    g = _g(P.ENTRY[f], a.in0.C, a.out0.C, a.kd, a.sd, a.pd, (a.in0.D, a.in0.H, a.in0.W))
                    g["out"], budget = (a.out0.D, a.out0.H, a.out0.W), 0
                _STEP_LAUNCHES.append((name, P.PlanCase(name, f, g, a.in0.N), P.last(lib, f), budget))
    return _STEP_LAUNCHES


def test_s2_unpinned_geometry_is_the_closed_form_rule(lib, s2_plans, monkeypatch):
    for f in S2:
        for case in CASES[f]:
            d = s2_plans[case.id][0]
            assert d == _rule(case, d), (case.id, d)
    launches = _step_launches(lib, monkeypatch)
    assert len(launches) > 100 and {c.family for _, c, _, _ in launches} == set(S2)
    for name, case, plan, budget in launches:
        assert plan == _rule(case, plan, budget or P.MAX_SLABS), (name, plan)


@pytest.mark.parametrize("family", S2, ids=lambda f: KERNEL[f])
def test_every_value_of_every_s2_coordinate_is_swept_in_every_instance(lib, family):
    """no class is waived: what an instance lacks is what it cannot have (plan_cases.s2_values)"""
    per, want = {}, {}
    for case in CASES[family]:
        have = per.setdefault(P.instance(case), {c: set() for c in P.S2_COORDS[family]})
        want[P.instance(case)] = P.s2_values(case)
        for v in P.sweep_list(lib, case):
            for c, x in zip(P.S2_COORDS[family], P.signature(case, v)):
                have[c].add(x)
    assert len(per) == {CONV_S2: 5, CONVT_MFMA: 5, BWW_S2: 7}[family]
    for inst, have in per.items():
        assert all(have[c] >= want[inst][c] for c in have), (inst, {c: want[inst][c] - have[c] for c in have})
        assert all(have[c] == want[inst][c] for c in have if c != "zpar"), (inst, have)      # (the generator's pairs also run pad 2 and 3)
    if family == CONVT_MFMA:                               # the three compiled epilogues of every pair, the Philox form as well
        assert {(P.instance(c), P.default_plan(lib, c)[6], c.geom["keep"]) for c in CASES[family]} == \
            {(i, e, k) for i in per for e, k in ((0, 0), (0, 1), (1, 2), (2, 0))}
        assert all(P.default_plan(lib, c)[5] == 1 for c in CASES[family])                   # NCLS: every CT_CASE compiles 1 today


def test_the_steps_stride2_default_plans_stay_inside_the_sweep(lib, monkeypatch):
    swept = _swept(lib)
    outside, seen = [], set()
    for name, case, plan, _ in _step_launches(lib, monkeypatch):
        sig = P.signature(case, plan)
        if (P.instance(case), plan, case.N) + out_dims(case.geom) not in seen:
            seen.add((P.instance(case), plan, case.N) + out_dims(case.geom))
            print(f"{name}: {case.channels} {case.N} x {out_dims(case.geom)} {dict(zip(P.FIELDS[case.family], plan))} {sig}")
        if sig not in swept.get(P.instance(case), ()):
            outside.append((name, plan, sig))
    assert not outside, "\n".join(map(str, sorted(set(map(str, outside)))))


# (feasible, run) per shape of plan_cases.S2_SHAPES, by (kernel, C_in, C_out, k[, pad of a transposed layer])
S2_COUNTS = {
    ('conv_s2_k', 8, 8, 4): [(5, 5), (1, 1), (4, 4), (18, 6), (24, 5), (32, 5), (30, 6), (27, 6)],
    ('conv_s2_k', 8, 16, 4): [(9, 9), (1, 1), (8, 8), (32, 5), (48, 6), (59, 7), (48, 6), (45, 7)],
    ('conv_s2_k', 16, 16, 4): [(9, 9), (1, 1), (8, 8), (32, 5), (48, 6), (59, 7), (48, 6), (45, 7)],
    ('conv_s2_k', 16, 32, 4): [(9, 9), (1, 1), (8, 8), (32, 5), (48, 6), (59, 7), (48, 6), (45, 7)],
    ('conv_s2_k', 32, 32, 4): [(18, 18), (2, 2), (15, 15), (63, 7), (96, 5), (117, 7), (96, 5), (90, 7)],
    ('convT_mfma_k', 16, 8, 4, 1): [(6, 6), (6, 6), (12, 12)],
    ('convT_mfma_k', 16, 8, 4, 0): [(6, 6), (6, 6), (12, 12)],
    ('convT_mfma_k', 32, 16, 4, 1): [(6, 6), (6, 6), (10, 10)],          # TY = 11 would pass 56 KB of LDS: the hard bound, not nQy, ends the list
    ('convT_mfma_k', 32, 16, 4, 0): [(6, 6), (6, 6), (10, 10)],
    ('convT_mfma_k', 8, 8, 4, 1): [(6, 6), (6, 6), (12, 12)],
    ('convT_mfma_k', 8, 8, 4, 0): [(6, 6), (6, 6), (12, 12)],
    ('convT_mfma_k', 16, 16, 4, 1): [(6, 6), (6, 6), (12, 12)],
    ('convT_mfma_k', 16, 16, 4, 0): [(6, 6), (6, 6), (12, 12)],
    ('convT_mfma_k', 32, 32, 4, 1): [(6, 6), (6, 6), (10, 10)],
    ('convT_mfma_k', 32, 32, 4, 0): [(6, 6), (6, 6), (10, 10)],
    ('convT_mfma_k', 16, 8, 4, 2): [(4, 4), (4, 4), (10, 10)],
    ('convT_mfma_k', 16, 8, 4, 3): [(4, 4), (4, 4), (10, 10)],
    ('convT_mfma_k', 32, 16, 4, 2): [(4, 4), (4, 4), (10, 10)],
    ('convT_mfma_k', 32, 16, 4, 3): [(4, 4), (4, 4), (10, 10)],
    ('bww_s2_k', 8, 16, 4): [(30, 30), (8, 8), (28, 28)],
    ('bww_s2_k', 16, 16, 4): [(30, 30), (8, 8), (28, 28)],
    ('bww_s2_k', 16, 32, 4): [(30, 30), (8, 8), (28, 28)],
    ('bww_s2_k', 32, 32, 4): [(30, 30), (8, 8), (28, 28)],
    ('bww_s2_k', 8, 8, 4): [(30, 30), (8, 8), (28, 28)],
    ('bww_s2_k', 16, 32, 3): [(30, 30), (8, 8), (28, 28)],
    ('bww_s2_k', 32, 32, 3): [(30, 30), (8, 8), (28, 28)],
}


def test_s2_feasible_plan_counts(lib, s2_plans):
    """the numbers of DESIGN.md's table for the k4 s2 kernels: feasible plans / plans run, per instance and shape (the variants of
    an instance at one padding agree; convT_mfma_k's Q ranges follow the padding)"""
    table = {}
    for f in S2:
        for case in CASES[f]:
            tag = case.name.split("-", 3)[3]
            key = (KERNEL[f],) + case.channels + (case.geom["k"],) + ((case.geom["p"],) if f == CONVT_MFMA else ())
            table.setdefault(key, {}).setdefault(tag, set()).add((len(s2_plans[case.id][1]), len(P.sweep_list(lib, case))))
    assert all(len(v) == 1 for row in table.values() for v in row.values()), table
    family = {KERNEL[f]: f for f in S2}
    got = {k: [next(iter(row[tag])) for tag, _, _ in P.S2_SHAPES[family[k[0]]]] for k, row in table.items()}
    assert got == S2_COUNTS, got
