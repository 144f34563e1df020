"""The launch geometry of conv_bf16_k, convT_bf16_k and bww_bf16_k through the pin / readback seam of the C ABI (tem_plan_pin
families 8, 9, 10), without a GPU: the dry queries take made-up pointers, as in tests/test_plan_space.py.

* a pin comes back as pinned, with derived fields that follow from it; a pin outside the valid range is refused and changes
  nothing; pins are per thread; the slab-count query answers the pinned geometry and the caller's budget still binds;
* unpinned, the geometry equals the Python restatement of the three host rules (bf16_plan_cases: conv_rule -- the arg-max of the
  restated score, the first of equal scores in loop order --, convT_rule, bww_rule) for every sweep case and for every launch
  of the workload: the bf16 3-D train steps at 74, 132 and 260 and utils.plan_routes of the 132 and 260 models;
* the two conditions the sweep shapes were chosen by: every value of every class coordinate occurs in the sweep of every kernel
  instance that can reach it (what it cannot is listed with its reason, and held to the arithmetic), and the class signature
  of every default plan of the workload occurs in the sweep of the same instance;
* the feasible / swept counts of DESIGN.md's table."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import bf16_plan_cases as B
import plan_cases as P
from bf16_plan_cases import CASES, FAMILIES, ceil
from plan_cases import BWW_BF16, CONV_BF16, CONVT_BF16, KERNEL
from span_cases import _g, out_dims


@pytest.fixture(scope="module")
def lib():
    from transfer_em_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def _no_pin_left(lib):
    yield
    P.clear_pins(lib)


@pytest.fixture(scope="module")
def plans(lib):
    """{case id: (default plan, feasible list)}"""
    return {c.id: (B.default_plan(lib, c), B.enumerate_plans(lib, c)) for c in B.ALL_CASES}


def _case(family, variant, channels, k, tag):
    return next(c for c in CASES[family] if c.variant == variant and c.channels == channels and c.geom["k"] == k and
                c.name.split("-", 3)[3] == tag)


def _refused(lib, case, v4):
    """a pin outside the family's range: the family declines -- these kernels are the last of their routes, so the entry point
    itself answers TEM_EUNSUPPORTED -- and the last decision stays"""
    want = B.default_plan(lib, case)
    a = P.dry_args(case)
    name = C.create_string_buffer(96)
    with B.declined(lib, case), P.pinned(lib, case.family, v4):
        if case.family == BWW_BF16:
            a.nslab = case.budget or P.MAX_SLABS
            rc = lib.tem_conv_bwd_weight_bf16_nslab(C.byref(a), name, 96)
        else:
            fn = lib.tem_conv_bf16_describe if case.family == CONV_BF16 else lib.tem_conv_transpose_bf16_describe
            rc = fn(C.byref(a), name, 96)
        assert rc == P.EUNSUPPORTED, (case.id, v4, rc, name.value)
        assert P.last(lib, case.family) == want, (case.id, v4)
    assert B.default_plan(lib, case) == want, (case.id, v4)


# ------------------------------------------------------------------------------------------------ the seam
@pytest.mark.parametrize("case", B.ALL_CASES, ids=lambda c: c.id)
def test_case_is_the_familys_and_its_default_plan_is_in_the_list(lib, plans, case):
    with B.declined(lib, case):
        taken, sym = P.describe(lib, case, P.dry_args(case))
    assert taken and sym.startswith(KERNEL[case.family] + "<"), (case.id, sym)
    d, feasible = plans[case.id]
    assert d in feasible and len(set(feasible)) == len(feasible), (case.id, d)       # (enumerate_plans: each readback repeats its pin)
    assert B.decide(lib, case, (-1, -1, -1, -1)) == d                                # nothing pinned: the rule's own choice
    run = B.sweep_list(lib, case)
    assert d in run and set(run) <= set(feasible)
    assert {B.signature(case, v) for v in run} == {B.signature(case, v) for v in feasible}       # thinning loses no class
    assert (len(run) == len(feasible)) if case.small else len(run) <= 60, (case.id, len(run), len(feasible))


def test_conv_pin_in_pin_out_and_refusals(lib, plans):
    """conv_bf16_k: the feasible list is the restated search's candidate list -- the same patches in the same order, with the same
    derived fields; everything else is refused, the nbx with an empty last column among it"""
    for case in CASES[CONV_BF16]:
        _, OH, OW = out_dims(case.geom)
        d, feasible = plans[case.id]
        assert feasible == [v for _, v in B.conv_search(B.instance(case)[1:], OH, OW)], case.id
        part = B.decide(lib, case, (-1, feasible[-1][1]))                             # a partial pin leaves the search its choice among the rest
        assert part in feasible and part[1] == feasible[-1][1]
    case = _case(CONV_BF16, "plain", (8, 8), 3, "small")                               # output rows of 9 voxels, 6 of them
    for v4, why in [((1, 4), "nbx 4 gives TX 3, the TX of nbx 3: a fourth column at ox0 = OW"), ((1, 6), "TX 2 is nbx 5's"),
                    ((1, 7), "likewise"), ((1, 8), "likewise"), ((1, 0), "no column"), ((1, 9), "nbx above 8"), ((0, 1), "no row"),
                    ((7, 1), "TY above OH"), ((17, 1), "TY above 16")]:
        _refused(lib, case, v4)
    for v4 in [(1, 3), (1, 5), (6, 1)]:                                                # ... and each refusal's neighbour is feasible
        assert B.decide(lib, case, v4)[:2] == v4
    wide = _case(CONV_BF16, "plain", (32, 32), 4, "4x17x33")
    _refused(lib, wide, (6, 5))                                                        # rows 14 x cols 16 x 4 planes x 4 chunks = 3584 > 3072
    assert B.decide(lib, wide, (5, 5))[:3] == (5, 5, 7)
    lds = _case(CONV_BF16, "cat", (16, 16), 3, "4x16x32")
    _refused(lib, lds, (13, 1))                                                        # 15 x 34 x 3 voxels of 32 bytes + 16.4 KB > 64 KB
    assert B.decide(lib, lds, (12, 1))[7] == 65376


def test_convT_pin_in_pin_out_and_refusals(lib, plans):
    """convT_bf16_k: the accepted TY are 1 .. K without a gap, K = min(nQy, 32) or where the loader's registers or the 56 KB end
    the list; nothing but nband moves; 0 and K + 1 are refused"""
    for case in CASES[CONVT_BF16]:
        d, feasible = plans[case.id]
        K = len(feasible)
        assert [v[0] for v in feasible] == list(range(1, K + 1)) and d[0] <= K <= min(d[3], 32), (case.id, d)
        assert all(v[1] == ceil(v[3], v[0]) and v[2:] == d[2:] for v in feasible), case.id
        for x in (0, K + 1, 1 << 20):
            _refused(lib, case, (x,))
    case = _case(CONVT_BF16, "plain", (32, 32), 4, "small-3x17x15")                    # 2 (ty + 1) 17 voxels of 64 bytes: 25 rows pass 56 KB
    assert len(plans[case.id][1]) == 18


def test_bww_pin_in_pin_out_and_refusals(lib, plans):
    for case in CASES[BWW_BF16]:
        OD, OH, OW = out_dims(case.geom)
        inst, (d, feasible) = B.instance(case)[1:], plans[case.id]
        for v in feasible:
            TY, nband, zsegs, zper, nseg, seg, G, slabs = v
            assert 1 <= TY <= B.band_rows(inst, min(seg, OW), OH) and zper == ceil(OD, zsegs) and zsegs == ceil(OD, zper), (case.id, v)
            assert nseg == ceil(OW, seg) and (seg == OW or (seg % 16 == 0 and case.geom["p"] == 0)), (case.id, v)
            if nseg == 1 or B.band_rows(inst, OW - (nseg - 1) * seg, OH) >= TY:       # (every segment has the pinned band)
                assert slabs == nseg * case.N * ceil(OH, TY) * zsegs and nband == ceil(OH, TY), (case.id, v)
        zs = {z for z in range(1, OD + 1) if ceil(OD, ceil(OD, z)) == z}
        assert {v[2] for v in feasible} == zs, case.id                                # every canonical z split, and no other
    case = _case(BWW_BF16, "p0", (16, 16), 3, "small")                                 # (8, 7, 40) x 2
    for v4, why in [((0, 1, -1), "no row"), ((8, 1, -1), "TY above OH = 7"), ((9, 1, -1), "TY above 8"), ((1, 0, -1), "no z-run"),
                    ((1, 9, -1), "more z-runs than planes"), ((1, 5, -1), "5 runs of 2 planes are 4"), ((1, 6, -1), "likewise"),
                    ((1, 7, -1), "likewise"), ((1, 1, 8), "seg below 16"), ((1, 1, 24), "seg no multiple of 16"), ((1, 1, 0), "no segment"),
                    ((1, 1, 20), "seg no multiple of 16")]:
        _refused(lib, case, v4)
    for v4 in [(7, 1, -1), (1, 8, -1), (1, 4, 16), (1, 1, 32), (2, 3, 48), (2, 3, 1 << 20)]:
        got = B.decide(lib, case, v4)
        assert got is not None and B.pin_of(BWW_BF16, got)[:2] == v4[:2] and got[5] == (v4[2] if 0 < v4[2] < 40 else 40), (v4, got)
    padded = _case(BWW_BF16, "p1T", (8, 16), 4, "small")
    _refused(lib, padded, (1, 1, 16))                                                  # pad 1: the zero frame belongs to the row's ends
    assert B.decide(lib, padded, (1, 1, 48))[4:6] == (1, 40)
    wide = _case(BWW_BF16, "p0", (32, 32), 4, "small")                                 # rows of 40: 31 at most fit one band
    _refused(lib, wide, (1, 1, 32))
    _refused(lib, wide, (1, 1, 48))                                                    # the single launch does not fit either
    _refused(lib, wide, (3, 1, 16))                                                    # 8 rows x 34 columns x 4 chunks > 1024
    assert B.decide(lib, wide, (2, 1, 16))[:6] == (2, 4, 1, 8, 3, 16)


def test_slab_count_is_the_pinned_geometrys_and_the_budget_still_binds(lib):
    case = _case(BWW_BF16, "p0", (16, 16), 3, "small")                                 # N 2, 7 rows, 8 planes
    a = P.dry_args(case)
    for v4, n in [((7, 1, -1), 2), ((1, 8, -1), 112), ((2, 3, 16), 3 * 2 * 4 * 3), ((3, 2, 32), 2 * 2 * 3 * 2)]:
        with P.pinned(lib, BWW_BF16, v4):
            a.nslab = P.MAX_SLABS
            assert lib.tem_conv_bwd_weight_bf16_nslab(C.byref(a), None, 0) == n, v4
            a.nslab = n                                    # the launch asks again with the count it was given: the pin answers the same
            assert lib.tem_conv_bwd_weight_bf16_nslab(C.byref(a), None, 0) == n and P.last(lib, BWW_BF16)[7] == n
            want = P.last(lib, BWW_BF16)
            for short in sorted({n - 1, n // 2, 1}):       # a pin above the caller's budget: nblocks <= max_slabs applies unchanged, in
                a.nslab = short                            # the first segment or in a later one, and the refusal changes nothing
                assert lib.tem_conv_bwd_weight_bf16_nslab(C.byref(a), None, 0) == P.EUNSUPPORTED, (v4, short)
                assert P.last(lib, BWW_BF16) == want, (v4, short, P.last(lib, BWW_BF16))
    a.nslab = 50                                           # unpinned, the budget enters the rule: 50 // (2 bands) z-runs at most
    assert lib.tem_conv_bwd_weight_bf16_nslab(C.byref(a), None, 0) == 16 and P.last(lib, BWW_BF16)[:4] == (7, 1, 8, 1)
    a.nslab = 9
    assert lib.tem_conv_bwd_weight_bf16_nslab(C.byref(a), None, 0) == 8 and P.last(lib, BWW_BF16)[:4] == (7, 1, 4, 2)
    assert P.last(lib, BWW_BF16) == B.bww_rule((16, 16, 3, 1), 2, 8, 7, 40, 0, 9)
    # an unpinned row that the rule cuts into segments (32 -> 32 k4 s2, rows of 40: 16 | 16 | 8, two bands of two rows for each of 2
    # samples): a budget that admits the first segments and not the last refuses the launch and leaves the last decision alone
    wide = _case(BWW_BF16, "p0", (32, 32), 4, "small")
    b = P.dry_args(wide)
    b.nslab = P.MAX_SLABS
    n = lib.tem_conv_bwd_weight_bf16_nslab(C.byref(b), None, 0)
    want = P.last(lib, BWW_BF16)
    assert n == 24 and want[4:8] == (3, 16, 4, 24) and B.bww_rule((32, 32, 4, 2), 2, 8, 7, 40, 0, 20) is None
    for short in (20, 11, 8, 7, 1):
        b.nslab = short
        assert lib.tem_conv_bwd_weight_bf16_nslab(C.byref(b), None, 0) == P.EUNSUPPORTED, short
        assert P.last(lib, BWW_BF16) == want, (short, P.last(lib, BWW_BF16))


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: KERNEL[f])
def test_pins_are_per_thread(lib, family):
    case = CASES[family][0]
    d, seen = B.default_plan(lib, case), {}
    other = B.enumerate_plans(lib, case)[0]
    assert other != d
    P.pin(lib, family, B.pin_of(family, other))            # stays set in this thread while the other one asks

    def ask():
        seen["before"] = P.last(lib, family)
        seen["plan"] = B.decide(lib, case)
    t = threading.Thread(target=ask)
    t.start(); t.join()
    assert seen["before"] is None and seen["plan"] == d
    with B.declined(lib, case):
        taken, _ = P.describe(lib, case, P.dry_args(case))
    assert taken and P.last(lib, family) == other          # ours is still pinned
    P.pin(lib, family, None)
    assert B.decide(lib, case) == d


# ------------------------------------------------------------------------------------------------ the rules, restated
def _rule(case, v=None, budget=0):
    inst, N = B.instance(case)[1:], case.N
    OD, OH, OW = out_dims(case.geom)
    if case.family == CONV_BF16:
        return B.conv_rule(inst, OH, OW)
    if case.family == CONVT_BF16:
        return B.convT_rule(inst[0], OD, OH, OW, case.geom["p"], v[6])
    return B.bww_rule(inst, N, OD, OH, OW, case.geom["p"], budget or P.MAX_SLABS)


_WORKLOAD = []


def _family_of(sym):
    return next((f for f in FAMILIES if sym.startswith(KERNEL[f] + "<")), None)


def _case_of_args(f, a, name):
    ci1 = a.in1.C if a.in1.ptr else 0
    dims = (a.in0.D, a.in0.H, a.in0.W)
    if f == BWW_BF16:
        g = _g("bww_h", a.in0.C, a.dout.C, a.kd, a.sd, a.pd, dims, ci1=ci1)
        g["out"] = (a.dout.D, a.dout.H, a.dout.W)
        return B.Bf16Case(name, f, g, a.in0.N, budget=a.nslab)
    g = _g(B.ENTRY[f], a.in0.C, a.out0.C, a.kd, a.sd, a.pd, dims, ci1=ci1, co1=a.out1.C if a.out1.ptr else 0)
    g["out"] = (a.out0.D, a.out0.H, a.out0.W)
    return B.Bf16Case(name, f, g, a.in0.N)


class _Recorder:
    """stands in for the loaded library inside utils.plan_routes: every dry query is passed on and, where one of the three kernels
    answered, the case of its argument struct and the plan of that decision are kept"""

    def __init__(self, lib, tag):
        self.lib, self.tag, self.seen = lib, tag, []

    def __getattr__(self, fn):
        real = getattr(self.lib, fn)

        def call(ref, *rest):
            rc = real(ref, *rest)
            buf = next((r for r in rest if isinstance(r, C.Array)), None)
            f = _family_of(buf.value.decode()) if buf is not None and rc == 0 else None
            if f:
                self.seen.append((f"{self.tag} {buf.value.decode()}", _case_of_args(f, ref._obj, self.tag), P.last(self.lib, f)))
            return rc
        return call


def _workload(lib, monkeypatch):
    """(name, case, default plan) of every launch of the workload that one of the three kernels takes: the launch lists of the
    bf16 3-D train steps (tests/test_step_admission.py), each asked again from its finished struct -- a kernel gradient with the
    slab count its launch passes --, and the dry queries of utils.plan_routes at N = 1 and at the default tile batch"""
    if _WORKLOAD:
        return _WORKLOAD
    import test_step_admission as SA
    from fullsize_cases import launch_struct
    from transfer_em_amd import _lib, utils
    for n, is3d, prec, b in SA.CONFIGS:
        if not is3d or prec != "bf16":
            continue
        with SA.dry_step(monkeypatch, n, is3d, prec, b) as st:
            for l in st.compute + st.update:
                a, f = launch_struct(l), _family_of(l.meta.get("kernel") or "")
                if a is None or f is None:
                    continue
                name = f"{n} b{b} {l.name}"
                assert SA._requery(lib, l) == 0, name
                _WORKLOAD.append((name, _case_of_args(f, a, name), P.last(lib, f)))
    for edge in (132, 260):
        for N in sorted({1, utils.default_tile_batch(edge, True)}):
            rec = _Recorder(lib, f"{edge} routes N={N}")
            monkeypatch.setattr(_lib, "load", lambda rec=rec: rec)
            routes = utils.plan_routes(edge, N, True, torch.bfloat16)
            monkeypatch.undo()
            assert len(rec.seen) == sum(_family_of(k) is not None for k in routes.values()), (rec.tag, routes)
            _WORKLOAD.extend(rec.seen)
    return _WORKLOAD


def test_unpinned_geometry_is_the_restated_rule(lib, plans, monkeypatch):
    for case in B.ALL_CASES:
        d = plans[case.id][0]
        assert d == _rule(case, d), (case.id, d, _rule(case, d))
    launches = _workload(lib, monkeypatch)
    assert len(launches) > 300 and {c.family for _, c, _ in launches} == set(FAMILIES)
    for name, case, plan in launches:
        assert plan == _rule(case, plan, case.budget), (name, plan, _rule(case, plan, case.budget))


def test_the_search_keeps_the_first_of_equal_scores(lib):
    """conv_bf16_k's choice is the arg-max of the restated score with `>`: of equal scores the first in loop order (TY outer,
    nbx inner) stays.  A case where the best score is tied -- 32 -> 32 1x1x1 at 16 x 32: no halo, so every patch of whole tiles
    scores 1.0 -- shows the order"""
    case = _case(CONV_BF16, "plain", (32, 32), 1, "4x16x32")
    cand = B.conv_search((32, 32, 1, 1), 16, 32)
    best = max(s for s, _ in cand)
    tied = [v for s, v in cand if s == best]
    assert len(tied) > 1 and B.default_plan(lib, case) == tied[0] == B.conv_rule((32, 32, 1, 1), 16, 32)


# ------------------------------------------------------------------------------------------------ the two cover conditions
def _swept(lib):
    out = {}
    for case in B.ALL_CASES:
        out.setdefault(B.instance(case), set()).update(B.signature(case, v) for v in B.sweep_list(lib, case))
    return out


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: KERNEL[f])
def test_every_reachable_value_of_every_coordinate_is_swept_in_every_instance(lib, family):
    per, want = {}, {}
    for case in CASES[family]:
        have = per.setdefault(B.instance(case), {c: set() for c in B.COORDS[family]})
        want[B.instance(case)] = B.values(case)
        mine = {c: set() for c in B.COORDS[family]}
        for v in B.sweep_list(lib, case):
            for c, x in zip(B.COORDS[family], B.signature(case, v)):
                have[c].add(x), mine[c].add(x)
        assert all(mine[c] <= B.case_values(case)[c] for c in mine if c != "zpar"), (case.id, mine)   # (a padded case: no segments)
    assert len(per) == {CONV_BF16: 11, CONVT_BF16: 5, BWW_BF16: 16}[family]
    for inst, have in per.items():
        assert all(have[c] >= want[inst][c] for c in have), (inst, {c: want[inst][c] - have[c] for c in have})
        assert all(have[c] == want[inst][c] for c in have if c != "zpar"), (inst, have)   # what is listed as unreachable never occurs
    if family == CONVT_BF16:                               # the three compiled epilogues of every pair, the Philox form as well
        assert {(B.instance(c), B.default_plan(lib, c)[6], c.geom["keep"]) for c in CASES[family]} == \
            {(i, e, k) for i in per for e, k in ((0, 0), (0, 1), (1, 2), (2, 0))}
        assert all(B.default_plan(lib, c)[5] == 1 for c in CASES[family])                 # NCLS: every CT_CASE compiles 1 today


def test_segmented_plans_have_a_single_launch_to_be_held_to(lib, plans):
    """the GPU sweep holds a segmented plan to the single launch of its band height and z split where one is feasible.  Every
    unpadded instance but 32 -> 32 k4 s2 -- whose rows of 32 and more fit no single band: its segmented plans go against the oracle
    alone -- has such pairs on every shape with segments, and over the sweep most segmented plans have one"""
    paired = lone = 0
    for case in CASES[BWW_BF16]:
        _, feasible = plans[case.id]
        twin = {(v[0], v[2]) for v in feasible if v[4] == 1}
        seg = [v for v in B.sweep_list(lib, case) if v[4] > 1]
        n = sum((v[0], v[2]) in twin for v in seg)
        paired, lone = paired + n, lone + len(seg) - n
        if seg and B.instance(case)[1:] != (32, 32, 4, 2):
            assert n > 0, case.id
        if seg and B.instance(case)[1:] == (32, 32, 4, 2) and out_dims(case.geom)[2] >= 32:
            assert n == 0 and not twin, case.id
    print(f"segmented plans of the sweep: {paired} with a single launch to be held to, {lone} without")
    assert paired > 4 * lone > 0


def test_what_is_listed_as_unreachable_is_so_by_the_arithmetic():
    """conv_bf16_k: the restated feasibility over every patch up to the sweep's widest and highest; bww_bf16_k: the band rule"""
    full = dict(trips={"single", "pair", "loop"}, tail={False, True}, cap={"none", "regs", "lds"})
    for inst in {B.instance(c)[1:] for c in CASES[CONV_BF16]}:
        reach = B.conv_reach(inst)
        listed = {(c, x) for (i, c, x) in B.UNREACHABLE if i == inst}
        assert listed == {(c, x) for c in full for x in full[c] - reach[c]}, (inst, listed, reach)
    assert B.band_rows((32, 32, 4, 2), 31, 1) == 1 and B.band_rows((32, 32, 4, 2), 32, 1) == 0
    assert {i for (i, _, _) in B.UNREACHABLE_BWW if i[0] == 1} == {(1, 8, 3, 1), (1, 16, 3, 1)}
    # convT_bf16_k: the listed instances are those with one wave per n-tile, where no tile count leaves a wave idle
    for _, ci, co, _, _ in {B.instance(c) for c in CASES[CONVT_BF16]}:
        wpn = 4 // (2 * co // 16)
        idle = any(B._trips(t, wpn)[0] for t in range(1, 65))
        assert idle == (((ci, co, 4, 2), "wtiles", "idle") not in B.UNREACHABLE_CONVT) and (wpn == 1) == (not idle), (ci, co)


def test_a_padded_kernel_gradient_has_no_column_segments(lib, plans):
    """UNREACHABLE_PADDED: every padded case has single launches alone, and a pinned segment width below the row is refused"""
    padded = [c for c in CASES[BWW_BF16] if c.geom["p"] != 0]
    assert len(padded) >= 9 and set(B.UNREACHABLE_PADDED) == {("segs", "2+eq"), ("segs", "2+short")}
    for case in padded:
        assert all(v[4] == 1 for v in plans[case.id][1]), case.id
        if out_dims(case.geom)[2] > 16:
            _refused(lib, case, (1, 1, 16))


def test_the_workloads_default_plans_stay_inside_the_sweep(lib, monkeypatch):
    swept = _swept(lib)
    outside, seen = [], set()
    for name, case, plan in _workload(lib, monkeypatch):
        sig = B.signature(case, plan)
        key = (B.instance(case), plan, case.N) + out_dims(case.geom)
        if key not in seen:
            seen.add(key)
            print(f"{name}: {case.channels} {case.N} x {out_dims(case.geom)} {dict(zip(P.FIELDS[case.family], plan))} {sig}")
        if sig not in swept.get(B.instance(case), ()):
            outside.append((B.instance(case), sig))
    assert not outside, "\n".join(sorted(set(map(str, outside))))


def test_the_references_alone_stay_inside_the_undecided_cap():
    """bf16_exact's condition on a case's inputs, from the reference alone: at most 10 % of the elements of every forward and
    transposed sweep case may lie within the accumulation margin of a rounding tie (tests/test_gpu_bf16_plan_space.py applies the
    element-by-element check to the default plan's output; every other plan must equal that output bit for bit)"""
    import bf16_exact
    from test_gpu_bf16_plan_space import operands
    worst = 0.0
    for case in CASES[CONV_BF16] + CASES[CONVT_BF16]:
        _, _, ref, S = operands(case)
        lo, hi = bf16_exact.store_interval(ref, S, case.geom["k"] ** 3 * case.channels[0])
        share = float(np.count_nonzero(lo != hi)) / ref.size
        worst = max(worst, share)
        assert share <= bf16_exact.UNDECIDED_CAP, (case.id, share)
    print(f"largest undecided share {100 * worst:.2f} %")


# ------------------------------------------------------------------------------------------------ counts
# (feasible, run) per shape of the instance's cases, in table order, by (kernel, C_in, C_out, k, variant)
COUNTS = {
    ('conv_bf16_k', 1, 8, 3, 'plain'): [(24, 24), (112, 13), (128, 25)],
    ('conv_bf16_k', 1, 16, 3, 'bd'): [(24, 24), (112, 13), (128, 25)],
    ('conv_bf16_k', 8, 8, 3, 'plain'): [(24, 24), (112, 13), (128, 25)],
    ('conv_bf16_k', 16, 16, 3, 'cat'): [(24, 24), (107, 14), (124, 24)],
    ('conv_bf16_k', 16, 16, 3, 'add'): [(24, 24), (107, 14), (124, 24)],
    ('conv_bf16_k', 16, 16, 3, 'keepw'): [(24, 24), (107, 14), (124, 24)],
    ('conv_bf16_k', 16, 16, 3, 'keepr'): [(24, 24), (107, 14), (124, 24)],
    ('conv_bf16_k', 32, 32, 3, 'plain'): [(24, 24), (96, 15), (113, 27)],
    ('conv_bf16_k', 32, 32, 4, 'plain'): [(21, 21), (24, 8), (33, 9), (1, 1), (23, 23), (34, 10)],
    ('conv_bf16_k', 16, 32, 4, 'plain'): [(24, 24), (58, 11), (75, 16)],
    ('conv_bf16_k', 8, 16, 4, 'bd'): [(24, 24), (89, 13), (106, 20)],
    ('conv_bf16_k', 32, 32, 1, 'plain'): [(24, 24), (112, 13), (128, 29), (1, 1), (60, 15), (84, 20)],
    ('conv_bf16_k', 32, 32, 1, 'bd'): [(24, 24), (112, 13), (128, 29), (1, 1), (60, 15), (84, 20)],
    ('conv_bf16_k', 1, 32, 1, 'bd'): [(24, 24), (112, 13), (128, 29), (1, 1), (60, 15), (84, 20)],
    ('conv_bf16_k', 32, 1, 1, 'bias'): [(24, 24), (112, 13), (128, 25), (1, 1), (60, 11), (84, 17)],
    ('convT_bf16_k', 16, 8, 4, 'keepw'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 16, 8, 4, 'keepr'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 16, 8, 4, 'plain'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 16, 8, 4, 'bd'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 32, 16, 4, 'keepw'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 32, 16, 4, 'keepr'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 32, 16, 4, 'plain'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 32, 16, 4, 'bd'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 8, 8, 4, 'keepw'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 8, 8, 4, 'keepr'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 8, 8, 4, 'plain'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 8, 8, 4, 'bd'): [(6, 6), (6, 6), (18, 18), (16, 16)],
    ('convT_bf16_k', 16, 16, 4, 'keepw'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 16, 16, 4, 'keepr'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 16, 16, 4, 'plain'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 16, 16, 4, 'bd'): [(6, 6), (6, 6), (18, 18), (8, 8)],
    ('convT_bf16_k', 32, 32, 4, 'keepw'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 32, 32, 4, 'keepr'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 32, 32, 4, 'plain'): [(6, 6), (6, 6), (18, 18)],
    ('convT_bf16_k', 32, 32, 4, 'bd'): [(6, 6), (6, 6), (18, 18), (2, 2)],
    ('convT_bf16_k', 16, 8, 4, 'keepr2'): [(4, 4), (4, 4), (16, 16)],
    ('convT_bf16_k', 16, 8, 4, 'keepr3'): [(4, 4), (4, 4), (16, 16)],
    ('convT_bf16_k', 32, 16, 4, 'keepr2'): [(4, 4), (4, 4), (16, 16)],
    ('convT_bf16_k', 32, 16, 4, 'keepr3'): [(4, 4), (4, 4), (16, 16), (6, 6)],
    ('bww_bf16_k', 1, 8, 3, 'p0'): [(105, 105)],
    ('bww_bf16_k', 1, 16, 3, 'p0'): [(105, 105)],
    ('bww_bf16_k', 8, 8, 3, 'p0'): [(105, 105), (60, 31), (9, 9), (80, 46), (30, 30), (10, 10), (20, 20), (10, 10)],
    ('bww_bf16_k', 8, 16, 3, 'p0'): [(105, 105), (60, 31), (9, 9), (80, 46), (30, 30), (10, 10), (20, 20), (10, 10)],
    ('bww_bf16_k', 16, 8, 3, 'p0'): [(105, 105), (60, 31), (9, 9), (80, 46), (30, 30), (10, 10), (20, 20), (10, 10)],
    ('bww_bf16_k', 16, 16, 3, 'p0'): [(105, 105), (60, 31), (9, 9), (80, 46), (30, 30), (10, 10), (20, 20), (10, 10)],
    ('bww_bf16_k', 16, 32, 3, 'p0'): [(100, 100), (60, 31), (9, 9), (80, 46), (30, 30), (10, 10), (20, 20), (10, 10)],
    ('bww_bf16_k', 32, 16, 3, 'p0'): [(75, 75), (55, 31), (9, 9), (65, 40), (30, 30), (10, 10), (20, 20), (10, 10)],
    ('bww_bf16_k', 32, 32, 3, 'p0'): [(75, 75), (55, 31), (9, 9), (65, 40), (30, 30), (10, 10), (20, 20), (10, 10)],
    ('bww_bf16_k', 8, 8, 4, 'p0'): [(85, 85), (60, 31), (9, 9), (75, 45), (30, 30), (10, 10), (20, 20), (10, 10)],
    ('bww_bf16_k', 16, 16, 4, 'p0'): [(45, 45), (40, 25), (9, 9), (40, 30), (25, 25), (10, 10), (20, 20), (10, 10)],
    ('bww_bf16_k', 8, 16, 4, 'p0'): [(85, 85), (60, 31), (9, 9), (70, 40), (30, 30), (10, 10), (20, 20), (10, 10)],
    ('bww_bf16_k', 16, 32, 4, 'p0'): [(40, 40), (35, 25), (9, 9), (40, 30), (25, 25), (10, 10), (20, 20), (10, 10)],
    ('bww_bf16_k', 32, 32, 4, 'p0'): [(10, 10), (10, 10), (6, 6), (10, 10), (15, 15), (10, 10), (10, 10), (10, 10), (6, 6)],
    ('bww_bf16_k', 32, 32, 1, 'p0'): [(100, 100), (60, 31), (9, 9), (80, 46), (30, 30), (10, 10), (20, 20), (10, 10)],
    ('bww_bf16_k', 1, 32, 1, 'p0'): [(100, 100), (60, 31), (9, 9), (80, 46), (30, 30), (10, 10), (20, 20), (10, 10)],
    ('bww_bf16_k', 16, 16, 3, 'cat'): [(105, 105), (60, 31), (9, 9), (80, 46), (30, 30), (10, 10), (20, 20), (10, 10)],
    ('bww_bf16_k', 8, 16, 4, 'p1T'): [(20, 20), (30, 16), (9, 9), (10, 10), (15, 15), (10, 10), (10, 10), (10, 10)],
    ('bww_bf16_k', 16, 32, 4, 'p3T'): [(5, 5)],
}


def test_feasible_plan_counts(lib, plans):
    """the numbers of DESIGN.md's table for families 8 .. 10: feasible plans / plans run per case"""
    got = {}
    for case in B.ALL_CASES:
        key = (KERNEL[case.family],) + case.channels + (case.geom["k"], case.variant)
        got.setdefault(key, []).append((len(plans[case.id][1]), len(B.sweep_list(lib, case))))
    for k, v in got.items():
        print(f"    {k}: {v},")
    assert got == COUNTS
    total = {f: [0, 0] for f in FAMILIES}
    for case in B.ALL_CASES:
        total[case.family][0] += len(plans[case.id][1])
        total[case.family][1] += len(B.sweep_list(lib, case))
    print({KERNEL[f]: tuple(t) for f, t in total.items()})
