"""The launch plans of wino_conv_k, wino_bww_k, conv_lds_k and conv3_bf16_k through the pin / readback seam of the C ABI
(tem_plan_pin, tem_plan_last), without a GPU: the dry queries take made-up pointers, as in tests/test_span_routing.py.

* a pin comes back as pinned, with derived fields that follow from it; a pin no candidate matches is refused and changes
  nothing; a pinned query neither reads nor writes the planner's memo;
* the feasible plans of every case of tests/plan_cases.py, enumerated through the library, take every value of every
  class coordinate somewhere in the family's sweep, and hold the default plan;
* every launch of the workload that one of the four kernels takes -- the step-shape tables of
  test_gpu_fullsize_oracle.py and test_gpu_bf16_fullsize_oracle.py, utils.plan_routes of the 132 and 260 models -- has a
  default plan whose class signature the GPU sweep (tests/test_gpu_plan_space.py) executes for the same kernel instance.
  A cost-model change that moves a layer onto a plan class no oracle-checked test has run fails here."""
import ctypes as C

import pytest
import torch

import plan_cases as P
from plan_cases import CASES, CONV3_BF16, CONV_LDS, FAMILIES, KERNEL, WINO, WINO_BWW
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
        seen["unknown"] = [lib.tem_plan_last(0, v), lib.tem_plan_last(5, v), lib.tem_plan_pin(0, None), lib.tem_plan_pin(5, None)]
        seen["null"] = lib.tem_plan_last(WINO, None)
        c = _case(WINO, "small", "ep0", (16, 16))
        seen["plan"] = P.decide(lib, c, (17, 2, 3, 1))
    P.decide(lib, _case(WINO, "small", "ep0", (16, 16)))                # this thread has decided; the other has not
    t = threading.Thread(target=ask)
    t.start(); t.join()
    assert seen["last"] == [P.EINVAL] * 4 and seen["unknown"] == [P.EINVAL] * 4 and seen["null"] == P.EINVAL
    assert seen["plan"][:4] == (17, 2, 3, 1)
    c = _case(WINO, "small", "ep0", (16, 16))
    assert P.decide(lib, c) == P.default_plan(lib, c) and P.decide(lib, c)[:4] != (17, 2, 3, 1)      # the other thread's pin is not ours


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: KERNEL[f])
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


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: KERNEL[f])
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


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: KERNEL[f])
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
    return next((f for f in FAMILIES if sym.startswith(KERNEL[f] + "<")), None)


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
