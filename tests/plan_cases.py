"""The plan space of the four z-marching kernels whose tile plan comes from a host-side cost model, as case tables and
the helpers that walk it through the C ABI (tem_plan_pin / tem_plan_last, include/tem_hip.h).

A case is a geometry (span_cases._g) at a batch N for one planner family.  `enumerate_plans` pins every point of the
family's pin grid in turn and asks the library's dry query: the answers are the feasible plans, as the v8 readback of
tem_plan_last.  Nothing here restates a planner: feasibility is the library's word.  What is restated are the caps that
define two class coordinates (tile count and LDS-DMA count "at the cap"), each next to the line of the planner it quotes.

Class signature of a plan ("Plan space") -- the coordinates along which the kernels take different paths:
  zrun   workgroup's z-run: "1" step (prologue only) / "2" (one ring rotation) / "3+" with more than one run / "all" =
         the whole axis in one run
  zrag   the last z-run is shorter than the others
  t1     first tile field (BY / R / TY): "min" (1; TY: 2) / "div" (divides its extent) / "rag" (leaves a ragged block)
  t2     Winograd: BX "1" / "div16" (a 16-tile MFMA row block holds whole tile rows) / "nodiv16" (a row block wraps
         tile rows) / ">8" (needs pitch 17; 16 also divides 16 and counts here).  wino_bww_k pairs tiles along x: no "1".
         conv3_bf16_k: nbx "1" / ">1".  conv_lds_k: the transpose patch 20 / 16 / 0
  third  Winograd: the LDS row pitch E, 9 / 17.  conv_lds_k: MTW 4 / 2 / 1.  conv3_bf16_k: none (0)
  tcap   the tile count of a workgroup is at its cap
  dcap   Winograd: the LDS-DMA count of a plane is at its cap.  conv3_bf16_k: one more tile row is refused (LDS-DMA budget or LDS
         bytes) although the row count is in range.  conv_lds_k stages through registers: False
The k4 s2 kernels (conv_s2_k, convT_mfma_k, bww_s2_k / bww_s2tb_k) have no cost model: one number each comes from a closed-form
rule, and the same seam pins it.  Their cases, shapes and class coordinates stand in the section "the k4 s2 kernels" below.
tests/test_plan_space.py holds the tables to these definitions on the CPU, tests/test_gpu_plan_space.py runs them.
Families 8 .. 10 (conv_bf16_k, convT_bf16_k, bww_bf16_k) have their constants and dry queries here, so that one `clear_pins`
serves every test; their cases, coordinates and restated rules stand in tests/bf16_plan_cases.py."""
import contextlib
import ctypes as C

from span_cases import MAX_SLABS, Case, _g, dense, extents, out_dims

WINO, WINO_BWW, CONV_LDS, CONV3_BF16, CONV_S2, CONVT_MFMA, BWW_S2 = 1, 2, 3, 4, 5, 6, 7
PLANNED = (WINO, WINO_BWW, CONV_LDS, CONV3_BF16)        # the plan comes from a cost model's search
S2 = (CONV_S2, CONVT_MFMA, BWW_S2)                      # the k4 s2 kernels: one number from a closed-form rule (further down)
CONV_BF16, CONVT_BF16, BWW_BF16 = 8, 9, 10                 # the other 3-D kernels of bf16 mode: tests/bf16_plan_cases.py
BF16 = (CONV_BF16, CONVT_BF16, BWW_BF16)
FAMILIES = PLANNED + S2 + BF16
KERNEL = {WINO: "wino_conv_k", WINO_BWW: "wino_bww_k", CONV_LDS: "conv_lds_k", CONV3_BF16: "conv3_bf16_k",
          CONV_S2: "conv_s2_k", CONVT_MFMA: "convT_mfma_k", BWW_S2: "bww_s2_k",
          CONV_BF16: "conv_bf16_k", CONVT_BF16: "convT_bf16_k", BWW_BF16: "bww_bf16_k"}
SYMBOLS = {f: (k + "<",) for f, k in KERNEL.items()}
SYMBOLS[BWW_S2] += ("bww_s2tb_k<",)                     # 8 -> 8: the two-block form, same rule and the same family
FIELDS = {WINO: "E BY BX zsegs zper nby nbx ndma".split(), WINO_BWW: "E BY BX zsegs zper nby nbx ndma".split(),
          CONV_LDS: "MTW R patch zsegs zper nych ntiles -".split(), CONV3_BF16: "nbx TY zsegs zper nby RD ndma -".split(),
          CONV_S2: "nblocks ny T iters total tiles_pp TB resident".split(), CONVT_MFMA: "TY nband nQz nQy nQx NCLS EPM -".split(),
          BWW_S2: "R rows tb KS OW - - -".split(), CONV_BF16: "TY nbx TX nby rows cols tiles lds".split(),
          CONVT_BF16: "TY nband nQz nQy nQx NCLS EPM -".split(), BWW_BF16: "TY nband zsegs zper nseg seg NGRP slabs".split()}
NPIN = {WINO: 4, WINO_BWW: 4, CONV_LDS: 4, CONV3_BF16: 3, CONV_S2: 1, CONVT_MFMA: 1, BWW_S2: 1, CONV_BF16: 2, CONVT_BF16: 1,
        BWW_BF16: 3}
EUNSUPPORTED, EINVAL = -2, -1


class PlanCase(Case):
    """span_cases.Case without a limit row: geometry `g` at batch N, every operand dense (the dry queries and the plan
    depend on extents alone; the GPU test places the operands itself)"""

    def __init__(self, name, family, g, N, add_off=None):
        self.name, self.family, self.geom, self.N, self.add_off = name, family, g, N, add_off
        self.row = self.side = self.frame = None
        self.views = {o: dense(e, N) for o, e in self.extents().items()}

    def extents(self):
        """span_cases.extents; with `add_off` the skip-gradient is a window of the output that starts there and stops one voxel
        short of the far faces (tem_epilogue.add_off: voxels outside the window get no skip-gradient)"""
        e = extents(self.geom)
        if self.add_off:
            self.add_off = tuple(min(o, d - 1) for d, o in zip(e["add"][:3], self.add_off))        # (an axis of one voxel: the whole of it)
            e["add"] = tuple(max(1, d - o - 1) for d, o in zip(e["add"][:3], self.add_off)) + e["add"][3:]
        return e

    def args(self, ptr, w, **kw):
        a = super().args(ptr, w, **kw)
        if self.add_off:
            a.ep.add_off[0], a.ep.add_off[1], a.ep.add_off[2] = self.add_off
        return a

    @property
    def id(self):
        return f"{KERNEL[self.family]}-{self.name}"

    @property
    def channels(self):
        g = self.geom
        return g["ci"] + g["ci1"], g["co"] + g["co1"]

    @property
    def key(self):
        """what a plan depends on: the kernel instance's channels and geometry, the batch, the output extents and (conv3_bf16_k)
        whether there are two inputs"""
        g = self.geom
        key = (self.family,) + self.channels + (g["k"], g["s"], self.N) + out_dims(g) + (bool(g["ci1"]),)
        if self.family in S2:               # convT_mfma_k: the Q ranges follow the padding, the readback names the compiled epilogue
            key += (g["p"], g["gate"], g["keep"])
        return key


# ------------------------------------------------------------------------------------------------ the seam
def pin(lib, family, v4):
    v = None if v4 is None else (C.c_int32 * 4)(*(list(v4) + [-1] * 4)[:4])
    assert lib.tem_plan_pin(family, v) == 0


def clear_pins(lib):
    for f in FAMILIES:
        pin(lib, f, None)


@contextlib.contextmanager
def pinned(lib, family, v4):
    pin(lib, family, v4)
    try:
        yield
    finally:
        pin(lib, family, None)


def last(lib, family):
    """the v8 of tem_plan_last as a tuple, or None before any decision"""
    v = (C.c_int32 * 8)()
    rc = lib.tem_plan_last(family, v)
    assert rc in (0, EINVAL), rc
    return tuple(v) if rc == 0 else None


FAKE = {o: 0x7f0000000000 + (i << 40) for i, o in enumerate(("in0", "in1", "out0", "out1", "gate", "add", "dout"))}


def dry_args(case):
    return case.args(FAKE, 0x7e0000000000, slabs=0x40000000)


def describe(lib, case, a):
    """-> (taken, kernel symbol): the family's dry query on argument struct `a` (its slab count set for a kernel gradient);
    taken = the family's own kernel answered"""
    from transfer_em_amd import _lib
    name, f = C.create_string_buffer(96), case.family
    if f == WINO:
        a.w_layout = _lib.TEM_W_WINOGRAD
        ok = lib.tem_conv_is_tiled(C.byref(a), 0, name, 96) == 1
    elif f == CONV_LDS:
        ok = lib.tem_conv_is_tiled(C.byref(a), 0, name, 96) == 1
    elif f == CONV3_BF16:
        ok = lib.tem_conv_bf16_describe(C.byref(a), name, 96) == 0
    elif f == CONV_S2:
        ok = lib.tem_conv_is_tiled(C.byref(a), 0, name, 96) == 1
    elif f == CONVT_MFMA:
        ok = lib.tem_conv_is_tiled(C.byref(a), 1, name, 96) == 1
    elif f == CONV_BF16:
        ok = lib.tem_conv_bf16_describe(C.byref(a), name, 96) == 0
    elif f == CONVT_BF16:
        ok = lib.tem_conv_transpose_bf16_describe(C.byref(a), name, 96) == 0
    elif f == BWW_BF16:                    # the slab count follows the plan; asked again with it, the query repeats it (the launch's check)
        a.nslab = MAX_SLABS if not getattr(case, "budget", 0) else case.budget
        n = lib.tem_conv_bwd_weight_bf16_nslab(C.byref(a), name, 96)
        ok = n > 0
        if ok:
            a.nslab = n
            ok = lib.tem_conv_bwd_weight_bf16_nslab(C.byref(a), name, 96) == n
    elif f == BWW_S2:                      # the slab count is the plan's R; asked with it, tem_bww_is_tiled names the launch's kernel
        a.nslab = MAX_SLABS
        n = lib.tem_conv_bwd_weight_nslab(C.byref(a))
        ok = n > 0
        if ok:
            a.nslab = n
            ok = lib.tem_bww_is_tiled(C.byref(a), name, 96) == 1
    else:
        a.nslab = MAX_SLABS
        n = lib.tem_conv_bwd_weight_winograd_nslab(C.byref(a), name, 96)
        ok = n > 0
        if ok:
            a.nslab = n
    sym = name.value.decode()
    return ok and sym.startswith(SYMBOLS[f]), sym


def decide(lib, case, v4=None, a=None):
    """the plan the family's planner answers under pin v4 (None: unpinned) -> v8 tuple, or None if the family's kernel
    does not take the launch"""
    a = a or dry_args(case)
    if v4 is None:
        taken, _ = describe(lib, case, a)
    else:
        with pinned(lib, case.family, v4):
            taken, _ = describe(lib, case, a)
    return last(lib, case.family) if taken else None


# ------------------------------------------------------------------------------------------------ enumeration
def zaxis(case):
    """steps along z: 2-plane tiles for the Winograd kernels, output planes for the others"""
    od = out_dims(case.geom)[0]
    return (od + 1) // 2 if case.family in (WINO, WINO_BWW) else od


def extent1(case):
    """what the first tile field divides: tile rows (Winograd), output rows (the others)"""
    oh = out_dims(case.geom)[1]
    return (oh + 1) // 2 if case.family in (WINO, WINO_BWW) else oh


def tile_grid(case):
    """the (field 0, field 1, field 2) triples of the family's pin grid without the z split"""
    _, OH, OW = out_dims(case.geom)
    f = case.family
    if f in (WINO, WINO_BWW):
        TY, TX = (OH + 1) // 2, (OW + 1) // 2
        return [(E, by, bx) for E in (9, 17) for by in range(1, min(TY, 64) + 1) for bx in range(1, min(TX, 64) + 1)]
    if f == CONV_LDS:
        return [(m, r, p) for m in (4, 2, 1) for r in range(1, min(OH, 16) + 1) for p in (20, 16, 0)]
    return [(nbx, ty) for nbx in (1, 2, 3, 4) for ty in range(2, min(24, OH + 1) + 1)]


_PLANS = {}


def pin_range(lib, case):
    """the values a k4 s2 family's one pinned number is asked at: 0 .. one past the extent it counts (iterations, Q_y rows,
    output rows), which the unpinned readback names.  The library's answers, not this range, are the feasible list."""
    d = default_plan(lib, case)
    return range(0, d[{CONV_S2: 3, CONVT_MFMA: 3, BWW_S2: 1}[case.family]] + 2)


def enumerate_plans(lib, case):
    """every feasible plan of the case, as v8 tuples in grid order.  A tile triple is asked once with the z split free;
    only where that is feasible, once per z split."""
    if case.key in _PLANS:
        return _PLANS[case.key]
    if case.family in S2:
        _PLANS[case.key] = plans = [v for v in (decide(lib, case, (x,)) for x in pin_range(lib, case)) if v is not None]
        return plans
    a, n, plans = dry_args(case), zaxis(case), []
    for t in tile_grid(case):
        if decide(lib, case, t + (-1,) * (NPIN[case.family] - len(t)), a) is None:
            continue
        for zs in range(1, n + 1):
            v4 = t + (zs,)
            got = decide(lib, case, v4, a)
            if got is not None:
                assert got[:len(v4)] == v4, (case.id, v4, got)
                plans.append(got)
    _PLANS[case.key] = plans
    return plans


def default_plan(lib, case):
    return decide(lib, case)


# ------------------------------------------------------------------------------------------------ class signatures
def tile_cap(case):
    """Winograd: tiles of a workgroup (wino.hip plan(): PAIR ? 128 : 64 / NB; wino_bww.hip plan_bww(): TB)"""
    ci, co = case.channels
    if case.family == WINO:
        return 128 if (ci, co) == (8, 8) else 64 // ((co + 15) // 16)
    return 32 if ci == 32 else 64


def dma_cap(case):
    """Winograd: LDS-DMA wave-instructions per sub-image, 8 NI (NI = 3 for wino_conv_k 8 -> 8, else 2: the WINO_CASE table)"""
    return 24 if case.family == WINO and case.channels == (8, 8) else 16


def signature(case, v, feasible=None):
    """class signature of plan v (a v8 tuple) of `case`; `feasible`: the case's feasible list (conv3_bf16_k's dcap is
    read off it: the plan with one more row is refused although the row count is inside the planner's range)"""
    if case.family in S2:
        return s2_signature(case, v)
    f, n, e1 = case.family, zaxis(case), extent1(case)
    _, OH, OW = out_dims(case.geom)
    if f in (WINO, WINO_BWW):
        E, t1, bx, zsegs, zper, _, _, ndma = v
        t2 = "1" if bx == 1 else ">8" if bx > 8 else "div16" if 16 % bx == 0 else "nodiv16"
        third, tcap, dcap, t1min = E, t1 * bx == tile_cap(case), ndma == dma_cap(case), 1
    elif f == CONV_LDS:
        mtw, t1, patch, zsegs, zper, _, ntiles, _ = v
        nt = (case.channels[1] + 15) // 16
        t2, third, tcap, dcap, t1min = patch, mtw, ntiles * nt == mtw * 8, False, 1       # conv_lds.hip run(): ntiles NT <= MTW NW, NW = 8
    else:
        nbx, t1, zsegs, zper, _, _, ndma, _ = v
        t2, third, tcap, t1min = ("1" if nbx == 1 else ">1"), 0, t1 == 24, 2               # conv3_bf16.hip run(): TY <= 24
        dcap = False
        if feasible is not None and t1 < min(24, OH + 1):
            dcap = not any(w[0] == nbx and w[1] == t1 + 1 for w in feasible)
    assert zper == -(-n // zsegs) and zsegs == -(-n // zper), (case.id, v)
    zrun = "all" if zsegs == 1 else "1" if zper == 1 else "2" if zper == 2 else "3+"
    t1c = "min" if t1 == t1min else "div" if e1 % t1 == 0 else "rag"
    return (zrun, n % zper != 0, t1c, t2, third, tcap, dcap)


COORDS = ("zrun", "zrag", "t1", "t2", "third", "tcap", "dcap")
# the values each coordinate must take somewhere in a family's sweep
VALUES = {
    WINO: dict(zrun={"1", "2", "3+", "all"}, zrag={False, True}, t1={"min", "div", "rag"}, t2={"1", "div16", "nodiv16", ">8"},
               third={9, 17}, tcap={False, True}, dcap={False, True}),
    WINO_BWW: dict(zrun={"1", "2", "3+", "all"}, zrag={False, True}, t1={"min", "div", "rag"}, t2={"div16", "nodiv16", ">8"},
                   third={9, 17}, tcap={False, True}, dcap={False, True}),
    CONV_LDS: dict(zrun={"1", "2", "3+", "all"}, zrag={False, True}, t1={"min", "div", "rag"}, t2={20, 16, 0},
                   third={4, 2, 1}, tcap={False, True}, dcap={False}),
    CONV3_BF16: dict(zrun={"1", "2", "3+", "all"}, zrag={False, True}, t1={"min", "div", "rag"}, t2={"1", ">1"},
                     third={0}, tcap={False, True}, dcap={False, True}),
}


def one_per_signature(case, plans):
    """the first plan of every class signature, in grid order"""
    seen, out = set(), []
    for v in plans:
        s = signature(case, v, plans)
        if s not in seen:
            seen.add(s)
            out.append(v)
    return out


def sweep_list(lib, case):
    """the plans the GPU sweep executes for a case: the whole feasible list of a small shape, one plan per class signature
    of a large one -- and the default plan in either"""
    plans = enumerate_plans(lib, case)
    run = plans if case.small else one_per_signature(case, plans)
    d = default_plan(lib, case)
    return run if d in run else run + [d]


# ------------------------------------------------------------------------------------------------ case tables
# Sweep shapes are OUTPUT extents, tagged "small" or "DxHxW".  The small shape's whole feasible list is run, of a large shape's
# one plan per class signature.  The large shapes were chosen by two conditions that tests/test_plan_space.py asserts:
# every value of every class coordinate occurs in the family, and the class signature of every workload launch's default plan
# (a combination of values) occurs for the same kernel instance.  What each extent is there for:
#   z          8 steps give z-runs of {8, 4, 3r, 2, 1}, 9 steps {9, 5r, 3, 2r, 1} (r: ragged last run): a run of 2 is even only on an
#              even axis and ragged only on an odd one, so every family has both.  Winograd steps are 2 planes: OD = 15 | 17,
#              the last step half a tile deep
#   Winograd   (6, 7, 9) x 2: 4 x 5 tiles, 3 z steps.  OW = 31: 16 tile columns, BX = 16 needs pitch 17.  OH = 31: 16 tile rows,
#              which BY = 2, 4, 8, 16 divide (BY x BX reaches the tile cap with whole blocks: 16 x 8 for 8 -> 8); OH = 25: 13 rows,
#              which no BY but 13 divides (the tile cap with ragged blocks) and where BY = 13 is the LDS-DMA cap at pitch 9;
#              OH = 27: 14 rows (BY = 2, 7 divide, 4, 8 do not)
#   conv_lds   (4, 6, 9) x 2 (32 -> 32 k4 s2 fits one row at the large shapes; its R = 2, 3 divide 6 here); (8 | 9, 16, 21): R runs
#              to its cap of 16 rows, which 1, 2, 4, 8, 16 divide
#   conv3_bf16 (5, 6, 17) x 2; OH = 24 | 25: TY runs to its cap of 24, as a whole and as a ragged block; OW = 33 admits nbx = 2,
#              OW = 127 nbx = 4 and rows so wide that a few of them fill the LDS-DMA budget; OW = 62: 16 -> 16 k4 s2 fits
#              two tile rows and no third (the 260 model's g.d2b)
SHAPES = {
    WINO: [("small", (6, 7, 9), 2), ("15x31x31", (15, 31, 31), 1), ("15x27x31", (15, 27, 31), 1), ("17x25x31", (17, 25, 31), 1)],
    WINO_BWW: [("small", (6, 7, 9), 2), ("15x31x31", (15, 31, 31), 1), ("17x25x31", (17, 25, 31), 1)],
    CONV_LDS: [("small", (4, 6, 9), 2), ("8x16x21", (8, 16, 21), 1), ("9x16x21", (9, 16, 21), 1)],
    CONV3_BF16: [("small", (5, 6, 17), 2), ("8x25x33", (8, 25, 33), 1), ("9x24x33", (9, 24, 33), 1), ("8x24x127", (8, 24, 127), 1),
                 ("9x6x62", (9, 6, 62), 1)],
}
LARGE = {f: SHAPES[f][1][0] for f in PLANNED}          # tag of the family's first large shape
ENTRY = {WINO: "conv", WINO_BWW: "bww_wino", CONV_LDS: "conv", CONV3_BF16: "conv_h"}


def _cases(family, variant, ci, co, k, s, p, **kw):
    """one PlanCase per sweep shape of the family: `variant` names the operand form, the geometry's input extents follow
    from the shape's output extents"""
    out = []
    for tag, od, N in SHAPES[family]:
        dims = tuple((d - 1) * s + k - 2 * p for d in od)
        g = _g(ENTRY[family], ci, co, k, s, p, dims, wino=family == WINO, **kw)
        assert out_dims(g) == od, (variant, od, out_dims(g))
        c = PlanCase(f"{ci + kw.get('ci1', 0)}to{co + kw.get('co1', 0)}-k{k}s{s}-{variant}-{tag}", family, g, N)
        c.small, c.variant = tag == "small", variant
        out.append(c)
    return out


GATED = dict(flip=True, slope=1.0, gate=True)          # the input-gradient form: pad 2, flipped layout, LeakyReLU' gate
WINO_PAIRS = [(8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32)]
CASES = {f: [] for f in FAMILIES}
for _ci, _co in WINO_PAIRS:
    CASES[WINO] += _cases(WINO, "ep0", _ci, _co, 3, 1, 0)                                   # EP 0: pad 0, LeakyReLU 0.3
    CASES[WINO] += _cases(WINO, "ep1", _ci, _co, 3, 1, 2, **GATED)                          # EP 1
CASES[WINO] += _cases(WINO, "ep2", 16, 8, 3, 1, 2, co1=8, keep=2, **GATED)                   # EP 2: keep bits, split output
CASES[WINO] += _cases(WINO, "ep2", 32, 16, 3, 1, 2, co1=16, keep=2, **GATED)
CASES[WINO] += _cases(WINO, "cat", 8, 16, 3, 1, 0, ci1=8)                                    # concat through in1
CASES[WINO] += _cases(WINO, "cat", 16, 32, 3, 1, 0, ci1=16)
for _ci, _co in [(8, 8), (8, 16), (16, 16), (16, 32), (32, 16), (32, 32)]:
    CASES[WINO_BWW] += _cases(WINO_BWW, "p0", _ci, _co, 3, 1, 0)
    CASES[WINO_BWW] += _cases(WINO_BWW, "p2", _ci, _co, 3, 1, 2)
CASES[WINO_BWW] += _cases(WINO_BWW, "cat", 8, 16, 3, 1, 0, ci1=8)
# conv_lds_k: each compiled (CI, CO, K, S) of CONV_CASE.  tem_conv offers a k4 s2 layer to conv_s2_k first, which takes
# neither two inputs nor the flipped layout: those are the k4 s2 forms that reach conv_lds_k
for _ci, _co in [(16, 16), (16, 32), (32, 16), (32, 32)]:
    CASES[CONV_LDS] += _cases(CONV_LDS, "plain", _ci, _co, 3, 1, 0)
    CASES[CONV_LDS] += _cases(CONV_LDS, "flip", _ci, _co, 3, 1, 2, **GATED)
CASES[CONV_LDS] += _cases(CONV_LDS, "drop", 16, 8, 3, 1, 2, co1=8, keep=2, **GATED)          # CONV_CASE_DROP: split 8 | 8
CASES[CONV_LDS] += _cases(CONV_LDS, "cat", 8, 16, 3, 1, 0, ci1=8)
CASES[CONV_LDS] += _cases(CONV_LDS, "cat", 8, 16, 4, 2, 0, ci1=8)
CASES[CONV_LDS] += _cases(CONV_LDS, "flip", 32, 32, 4, 2, 1, **GATED)
CASES[CONV_LDS] += _cases(CONV_LDS, "flip", 16, 32, 4, 2, 1, **GATED)
# conv3_bf16_k: every compiled (CI, CO, K, S), with one and two inputs, gated, and the SPLIT instances (32 -> 32 k3, 16 -> 32 k4:
# column blocks on wave groups)
H_GATED = dict(slope=1.0, gate=True)
CASES[CONV3_BF16] += _cases(CONV3_BF16, "plain", 8, 8, 3, 1, 0)
CASES[CONV3_BF16] += _cases(CONV3_BF16, "plain", 8, 16, 3, 1, 0)
CASES[CONV3_BF16] += _cases(CONV3_BF16, "gated", 16, 8, 3, 1, 2, **H_GATED)
CASES[CONV3_BF16] += _cases(CONV3_BF16, "cat", 8, 16, 3, 1, 0, ci1=8)
CASES[CONV3_BF16] += _cases(CONV3_BF16, "plain", 16, 32, 3, 1, 0)
CASES[CONV3_BF16] += _cases(CONV3_BF16, "gated", 32, 16, 3, 1, 2, **H_GATED)
CASES[CONV3_BF16] += _cases(CONV3_BF16, "cat", 16, 32, 3, 1, 0, ci1=16)
CASES[CONV3_BF16] += _cases(CONV3_BF16, "plain", 8, 8, 4, 2, 0)
CASES[CONV3_BF16] += _cases(CONV3_BF16, "gated", 8, 16, 4, 2, 1, **H_GATED)
CASES[CONV3_BF16] += _cases(CONV3_BF16, "plain", 16, 16, 4, 2, 0)
CASES[CONV3_BF16] += _cases(CONV3_BF16, "plain", 16, 32, 4, 2, 1)


# ------------------------------------------------------------------------------------------------ the k4 s2 kernels
# conv_s2_k, convT_mfma_k and bww_s2_k / bww_s2tb_k take one number each from a closed-form rule (workgroups; Q_y rows per band;
# row ranges).  Their class coordinates name what that number changes in the kernel, computed from the readback and the case's
# extents -- the kernels' own index arithmetic is restated where a coordinate is that arithmetic (conv_s2_k's two walks, the row
# ranges of bww_s2_k), next to the line it quotes:
#   conv_s2_k     walk   "one" interleaved walk (fewer workgroups than XCDs) / "xcd": per XCD over contiguous eighths
#                 ipw    the most iterations a workgroup owns: "1" / "2" / "3+odd" (the ping-pong ends on the first fragment
#                        set) / "4+even"
#                 dead   some workgroup owns no iteration
#                 tail   total % T != 0: the last iteration carries dead tiles (T = 1: never)
#                 prag   plane_vox % VPT != 0: a plane's last tile is partial
#   convT_mfma_k  bands  "1" / "div" (TY divides nQy) / "rag" (a shorter last band)
#                 ty     "1" / ">1"
#                 wtiles a full band's 16-voxel tiles ceil(TY nQx / 16) against the WPN = 4 / NT waves of an n-tile:
#                        "<WPN" (idle waves) / "div" / "rag" (C_out = 32: one wave per n-tile, "div" alone)
#                 zpar   OD "even" / "odd", with the padding: "/p0", "/p1" (odd OD: a class group has no plane at one end)
#   bww_s2_k      rows   rows per wave in the shortest range: "0" (a wave without a row; not with 32 input channels, where a
#                        wave takes one ky of every row) / "1" / "2+"
#                 even   rows % R == 0: all ranges have one length
#                 cross  a range spans two planes (or samples)
#                 ring   k-steps of the longest wave share against the ring of 8 fragment sets: "<8" (the steady-state loop is
#                        never entered) / ">=8"
#                 xtail  OW % 4 != 0: a row's last k-step is partial
S2_COORDS = {CONV_S2: ("walk", "ipw", "dead", "tail", "prag"), CONVT_MFMA: ("bands", "ty", "wtiles", "zpar"),
             BWW_S2: ("rows", "even", "cross", "ring", "xtail")}


def s2_owned(nblocks, iters):
    """iterations each workgroup of conv_s2_k owns (conv_s2.hip, conv_s2_k: `one`, `step`, `x0`, `it1`, `it0`)"""
    if nblocks < 8:
        return [len(range(b, iters, nblocks)) for b in range(nblocks)]
    own = []
    for b in range(nblocks):
        xcd = b & 7
        step, x0, it1 = (nblocks - xcd + 7) >> 3, (xcd * iters) >> 3, ((xcd + 1) * iters) >> 3
        own.append(len(range(x0 + (b >> 3), it1, step)))
    return own


def bww_ranges(R, rows):
    """[ra, rb) of every row range (bww_s2.hip, bww_s2_k: `ra`, `rb`)"""
    return [(i * rows // R, (i + 1) * rows // R) for i in range(R)]


def s2_signature(case, v):
    f = case.family
    OD, OH, OW = out_dims(case.geom)
    ci, co = case.channels
    if f == CONV_S2:
        nblocks, _, T, iters, total, tiles_pp, tb, _ = v
        own = s2_owned(nblocks, iters)
        assert sum(own) == iters, (case.id, v)                    # every iteration has exactly one owner
        m = max(own)
        plane_vox, vpt = OH * (OW + tb), 16 - tb                  # conv_s2.hip run(): RL = TB ? OW + 1 : OW; VPT = TB ? 15 : 16
        assert tiles_pp == -(-plane_vox // vpt) and iters == -(-total // T), (case.id, v)
        return ("one" if nblocks < 8 else "xcd", "1" if m == 1 else "2" if m == 2 else "3+odd" if m % 2 else "4+even",
                min(own) == 0, total % T != 0, plane_vox % vpt != 0)
    if f == CONVT_MFMA:
        TY, nband, _, nQy, nQx, _, _, _ = v
        assert nband == -(-nQy // TY), (case.id, v)
        wpn, ntiles = 4 // (2 * co // 16), -(-TY * nQx // 16)     # convT_mfma.hip: NT = 2 CO / 16, WPN = 4 / NT
        return ("1" if nband == 1 else "div" if nQy % TY == 0 else "rag", "1" if TY == 1 else ">1",
                "<WPN" if ntiles < wpn else "div" if ntiles % wpn == 0 else "rag", f"{'odd' if OD % 2 else 'even'}/p{case.geom['p']}")
    R, rows, tb, _, ow, _, _, _ = v
    assert rows == case.N * OD * OH and ow == OW, (case.id, v)
    ranges = bww_ranges(R, rows)
    lens = [b - a for a, b in ranges]
    wky = ci == 32                                                # bww_s2.hip: WKY, a wave takes one ky of every row of the range
    per_wave = (lambda n: n) if wky else (lambda n: n // 4)       # the fourth wave's rows: (n - 3 + 3) >> 2
    ksteps = (OW + 4) // 4 if tb else -(-OW // 4)                 # (bww_s2tb_k: slots 0 .. OW)
    longest = max(lens) if wky else -(-max(lens) // 4)            # the first wave's rows
    lo = per_wave(min(lens))
    return ("0" if lo == 0 else "1" if lo == 1 else "2+", rows % R == 0, any(a // OH != (b - 1) // OH for a, b in ranges),
            "<8" if longest * ksteps < 8 else ">=8", OW % 4 != 0)


def s2_values(case):
    """the values each coordinate must take in the sweep of the case's kernel instance: every one, but for the three an
    instance cannot have (named above)"""
    f, (ci, co) = case.family, case.channels
    if f == CONV_S2:
        return dict(walk={"one", "xcd"}, ipw={"1", "2", "3+odd", "4+even"}, dead={False, True},
                    tail={False} if ci == 32 else {False, True}, prag={False, True})
    if f == CONVT_MFMA:
        return dict(bands={"1", "div", "rag"}, ty={"1", ">1"}, wtiles={"div"} if co == 32 else {"<WPN", "div", "rag"},
                    zpar={"even/p0", "even/p1", "odd/p0", "odd/p1"})
    return dict(rows={"1", "2+"} if ci == 32 else {"0", "1", "2+"}, even={False, True}, cross={False, True},
                ring={"<8", ">=8"}, xtail={False, True})


# Shapes (OUTPUT extents of conv_s2_k and bww_s2_k, INPUT extents of convT_mfma_k; batch).  A tag that starts with "small": the whole
# feasible list runs; of the others one plan per class signature.  The lists are a greedy cover, over a few thousand candidate
# extents, of the two conditions tests/test_plan_space.py asserts per kernel instance: every value of every coordinate, and the
# class signature of every k4 s2 launch of the 74, 132 and 260 train steps.
#   conv_s2_k     (3, 5, 7) x 2: iters 5 / 9 / 18 for T = 4 (two-block form) / 2 / 1 -- the one walk through ipw 1 .. 4+, the XCD
#                 walk with and without dead workgroups; a plane's last tile is partial; the two-block form has a tail.
#                 (1, 3, 4) x 2 and (5, 3, 4) x 3: a tile per plane, fewer iterations than XCDs (the step's 32 -> 32 layer at 74
#                 is one iteration).  The batches of three make odd tile counts, which T = 2 needs for a tail (a batch of two
#                 makes every count even); 8 must divide the iterations for the XCD walk to give every workgroup exactly one, and
#                 ipw 3+odd / 4+even without a dead workgroup, as the full-size launches have it, needs 17 .. 32 iterations or
#                 more: (3, 7, 16), (4, 6, 19), (3, 9, 22), (4, 8, 16), (6, 10, 8) x 3 bring these together with each
#                 (tail, prag) pair the step has (planes of 128 = 8 x 16 voxels: whole tiles)
#   convT_mfma_k  input (3, 5, 6): nQy = 6, nQx = 7 (8 with pad 0), TY = 1 .. 6 gives bands 6, 3, 2, 2 ragged, 2 ragged, 1; its twin
#                 with the output one plane short (odd OD); input (3, 11, 14): nQy = 12, rows of 15 (16 with pad 0; 13 with
#                 pad 3) voxels, so a band's tile count runs through every remainder of the waves of an n-tile, with whole and
#                 ragged bands
#   bww_s2_k      rows = N OD OH of 30, 8 and 28 with OW = 7 (partial last k-step, 2 k-steps a row), 12 (whole k-steps) and 33
#                 (9 k-steps: one row fills the ring; rows = 28 has R = 3 with ranges of 9, 9, 10 rows -- unequal, two rows a
#                 wave and more -- which is what every full-size launch looks like): every R = 1 .. rows runs
S2_SHAPES = {
    CONV_S2: [("small", (3, 5, 7), 2), ("small-1x3x4", (1, 3, 4), 2), ("small-5x3x4", (5, 3, 4), 3), ("3x7x16", (3, 7, 16), 3),
              ("4x6x19", (4, 6, 19), 3), ("3x9x22", (3, 9, 22), 3), ("4x8x16", (4, 8, 16), 3), ("6x10x8", (6, 10, 8), 3)],
    CONVT_MFMA: [("small", (3, 5, 6), 2), ("small-odd", (3, 5, 6), 2), ("small-3x11x14", (3, 11, 14), 2)],
    BWW_S2: [("small", (3, 5, 7), 2), ("small-1x4x12", (1, 4, 12), 2), ("small-2x7x33", (2, 7, 33), 2)],
}
ENTRY.update({CONV_S2: "conv", CONVT_MFMA: "convT", BWW_S2: "bww"})
ADD_OFF = (1, 1, 2)


def _s2_cases(family, variant, ci, co, k, s, p, add_off=None, **kw):
    out = []
    for tag, dims, N in S2_SHAPES[family]:
        if family == CONVT_MFMA:
            g = _g("convT", ci, co, k, s, p, dims, **kw)
            if tag.endswith("odd"):
                od = out_dims(g)
                g["out"] = (od[0] - 1,) + od[1:]
        else:
            g = _g(ENTRY[family], ci, co, k, s, p, tuple((d - 1) * s + k - 2 * p for d in dims), **kw)
            assert out_dims(g) == dims, (variant, dims, out_dims(g))
        c = PlanCase(f"{ci}to{co}-k{k}s{s}-{variant}-{tag}", family, g, N, add_off)
        c.small, c.variant = tag.startswith("small"), variant
        out.append(c)
    return out


S2_PAIRS = [(8, 8), (8, 16), (16, 16), (16, 32), (32, 32)]          # conv_s2.hip dispatch(): <8,1,4,true> <8,1,2> <16,1,2> <16,2,2> <32,1,1>
CONVT_PAIRS = [(16, 8), (32, 16), (8, 8), (16, 16), (32, 32)]       # convT_mfma.hip CT_CASE
BWW_S2_PAIRS = [(8, 16), (16, 16), (16, 32), (32, 32), (8, 8)]       # bww_s2.hip dispatch(); 8 -> 8: bww_s2tb_k
CASES.update({f: [] for f in S2})
for _ci, _co in S2_PAIRS:
    CASES[CONV_S2] += _s2_cases(CONV_S2, "fwd", _ci, _co, 4, 2, 0)                                        # LeakyReLU 0.3
    CASES[CONV_S2] += _s2_cases(CONV_S2, "bd", _ci, _co, 4, 2, 1, ADD_OFF, slope=1.0, gate=True, add=True)   # input-gradient of a transposed layer
for _ci, _co in CONVT_PAIRS:
    CASES[CONVT_MFMA] += _s2_cases(CONVT_MFMA, "keepw", _ci, _co, 4, 2, 1, keep=1)                         # EPM 0: Philox, keep bits written
    CASES[CONVT_MFMA] += _s2_cases(CONVT_MFMA, "keepr", _ci, _co, 4, 2, 1, keep=2)                         # EPM 1: keep bits read
    CASES[CONVT_MFMA] += _s2_cases(CONVT_MFMA, "plain", _ci, _co, 4, 2, 1)                                 # EPM 0, no Dropout
    CASES[CONVT_MFMA] += _s2_cases(CONVT_MFMA, "bd", _ci, _co, 4, 2, 0, ADD_OFF, slope=1.0, gate=True, add=True)   # EPM 2
for _ci, _co in CONVT_PAIRS[:2]:                                     # the generator's two: pad 1 and a crop of one (two) voxels a side
    CASES[CONVT_MFMA] += _s2_cases(CONVT_MFMA, "keepr2", _ci, _co, 4, 2, 2, keep=2)
    CASES[CONVT_MFMA] += _s2_cases(CONVT_MFMA, "keepr3", _ci, _co, 4, 2, 3, keep=2)
for _ci, _co in BWW_S2_PAIRS:
    CASES[BWW_S2] += _s2_cases(BWW_S2, "p0", _ci, _co, 4, 2, 0)
    CASES[BWW_S2] += _s2_cases(BWW_S2, "p1", _ci, _co, 4, 2, 1)                                           # 8 -> 16: a transposed layer's, operands swapped
CASES[BWW_S2] += _s2_cases(BWW_S2, "p0", 16, 32, 3, 1, 0)                                                 # the small k3 s1 layers routed here
CASES[BWW_S2] += _s2_cases(BWW_S2, "p0", 32, 32, 3, 1, 0)
ALL_CASES = [c for f in PLANNED + S2 for c in CASES[f]]


def instance(case):
    """the compiled kernel instance a case vouches for: family, channels, kernel size and stride"""
    return (case.family,) + case.channels + (case.geom["k"], case.geom["s"])
