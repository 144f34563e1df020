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
tests/test_plan_space.py holds the tables to these definitions on the CPU, tests/test_gpu_plan_space.py runs them."""
import contextlib
import ctypes as C

from span_cases import MAX_SLABS, Case, _g, dense, extents, out_dims

WINO, WINO_BWW, CONV_LDS, CONV3_BF16 = 1, 2, 3, 4
FAMILIES = (WINO, WINO_BWW, CONV_LDS, CONV3_BF16)
KERNEL = {WINO: "wino_conv_k", WINO_BWW: "wino_bww_k", CONV_LDS: "conv_lds_k", CONV3_BF16: "conv3_bf16_k"}
FIELDS = {WINO: "E BY BX zsegs zper nby nbx ndma".split(), WINO_BWW: "E BY BX zsegs zper nby nbx ndma".split(),
          CONV_LDS: "MTW R patch zsegs zper nych ntiles -".split(), CONV3_BF16: "nbx TY zsegs zper nby RD ndma -".split()}
NPIN = {WINO: 4, WINO_BWW: 4, CONV_LDS: 4, CONV3_BF16: 3}
EUNSUPPORTED, EINVAL = -2, -1


class PlanCase(Case):
    """span_cases.Case without a limit row: geometry `g` at batch N, every operand dense (the dry queries and the plan
    depend on extents alone; the GPU test places the operands itself)"""

    def __init__(self, name, family, g, N):
        self.name, self.family, self.geom, self.N = name, family, g, N
        self.row = self.side = self.frame = None
        self.views = {o: dense(e, N) for o, e in extents(g).items()}

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
        return (self.family,) + self.channels + (g["k"], g["s"], self.N) + out_dims(g) + (bool(g["ci1"]),)


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
    else:
        a.nslab = MAX_SLABS
        n = lib.tem_conv_bwd_weight_winograd_nslab(C.byref(a), name, 96)
        ok = n > 0
        if ok:
            a.nslab = n
    sym = name.value.decode()
    return ok and sym.startswith(KERNEL[f] + "<"), sym


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


def enumerate_plans(lib, case):
    """every feasible plan of the case, as v8 tuples in grid order.  A tile triple is asked once with the z split free;
    only where that is feasible, once per z split."""
    if case.key in _PLANS:
        return _PLANS[case.key]
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
LARGE = {f: SHAPES[f][1][0] for f in FAMILIES}          # tag of the family's first large shape
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
ALL_CASES = [c for f in FAMILIES for c in CASES[f]]


def instance(case):
    """the compiled kernel instance a case vouches for: family, channels, kernel size and stride"""
    return (case.family,) + case.channels + (case.geom["k"], case.geom["s"])
