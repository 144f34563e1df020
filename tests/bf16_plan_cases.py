"""The launch geometry of the other three 3-D kernels of bf16 mode -- conv_bf16_k, convT_bf16_k, bww_bf16_k -- as case tables,
class coordinates and restated host rules, beside tests/plan_cases.py (whose seam helpers and PlanCase this module uses).

conv_bf16_k takes its output patch TY x TX = ceil(OW / nbx) from a score search (conv_bf16.hip run()), convT_bf16_k the Q_y rows
of a band and bww_bf16_k band rows, z-runs and column segments from closed forms.  tem_plan_pin families 8, 9, 10 pin them.
Feasibility is the library's word (`enumerate_plans` asks the dry queries); the rules restated here are what
tests/test_bf16_plan_space.py holds the UNPINNED geometry to, and what the coordinate `cap` quotes.

Class coordinates ("Plan space"):
  conv_bf16_k   ycut   "one" band of rows (nby 1) / "div" (TY divides OH) / "rag": the last band's TYo < TY
                xcut   "one" column of patches / "div" / "rag": the last column's TXo < TX (tiles run over the full-width patch,
                       lanes past TXo compute a clamped voxel and store nothing)
                wrap   "rows": TX a multiple of 16, a tile never spans a row end / "wraps"
                trips  tiles of a full patch against the WPN = 4 / NT waves of an n-tile: "single" (<= WPN: no wave holds a second
                       tile in flight) / "pair" (<= 2 WPN) / "loop" (a second trip of `for (t ...; t += 2 WPN)`)
                tail   some wave's last trip has one tile after a trip with two (its tile count is odd and >= 3)
                cap    one more patch row or column is refused: "regs" (the loader's chunk count) / "lds" (the bytes) / "none"
  convT_bf16_k  bands, ty, zpar as convT_mfma_k's (plan_cases.S2_COORDS); wtiles read against this kernel's loop, two tiles per
                wave and trip: "idle" (a wave without a tile) / "single" / "pair" / "loop", "+tail" as above
  bww_bf16_k    zrun, zrag as the z-marching kernels' (plan_cases.signature)
                t1     TY "1" / "div" / "rag": TYr < TY in the last band
                kblk   k-blocks of 16 voxels in the (last segment's) row: "1" / ">1", and "/whole" or "/pad": the last k-block is
                       zero-padded
                segs   "1" launch / "2+eq" (equal column segments) / "2+short" (a shorter last segment)
"""
import contextlib

import plan_cases as P
from plan_cases import BWW_BF16, CONV3_BF16, CONV_BF16, CONVT_BF16
from span_cases import MAX_SLABS, _g, out_dims

FAMILIES = (CONV_BF16, CONVT_BF16, BWW_BF16)
COORDS = {CONV_BF16: ("ycut", "xcut", "wrap", "trips", "tail", "cap"), CONVT_BF16: ("bands", "ty", "wtiles", "zpar"),
          BWW_BF16: ("zrun", "zrag", "t1", "kblk", "segs")}
NO_CONV3 = ((CONV3_BF16, (1, 1, 1)),)      # conv3_bf16_k's TY starts at 2: no candidate matches, it declines and conv_bf16_k answers


def ceil(a, b):
    return -(-a // b)


class Bf16Case(P.PlanCase):
    """PlanCase with a bias (the 32 -> 1 head), the pins under which the kernels in front of the family's decline, and (kernel
    gradient) the caller's slab budget"""

    def __init__(self, name, family, g, N, add_off=None, bias=False, decline=(), budget=0):
        super().__init__(name, family, g, N, add_off)
        self.bias, self.decline, self.budget = bias, decline, budget

    def args(self, ptr, w, **kw):
        a = super().args(ptr, w, **kw)
        if self.bias:
            a.ep.bias = ptr.get("bias", 0x7c0000000000)
        return a

    @property
    def key(self):
        g = self.geom
        return super().key + (g["p"], g["gate"], g["add"], g["keep"], g["flip"], self.bias, self.budget)


# ------------------------------------------------------------------------------------------------ the seam
def pin_of(family, v):
    """the v4 that pins the plan of readback v"""
    if family == BWW_BF16:                  # (the single launch reads back seg = OW: the next multiple of 16 pins it)
        return (v[0], v[2], v[5] if v[4] > 1 else ceil(v[5], 16) * 16)
    return (v[0], v[1]) if family == CONV_BF16 else (v[0],)


@contextlib.contextmanager
def declined(lib, case):
    for f, v4 in case.decline:
        P.pin(lib, f, v4)
    try:
        yield
    finally:
        for f, _ in case.decline:
            P.pin(lib, f, None)


def decide(lib, case, v4=None, a=None):
    """plan_cases.decide with the case's `decline` pins set around the query"""
    with declined(lib, case):
        return P.decide(lib, case, v4, a)


def pin_grid(case):
    """the pins the dry query is asked at: every number from 0 to one past the extent it counts (the library's answers, not this
    grid, are the feasible list).  A segment width that covers the row is the single launch: one such width is asked."""
    OD, OH, OW = out_dims(case.geom)
    if case.family == CONV_BF16:
        return [(ty, nbx) for ty in range(0, 18) for nbx in range(0, 10)]
    if case.family == CONVT_BF16:
        return [(ty,) for ty in range(0, 34)]
    segs = list(range(16, OW, 16)) + [ceil(OW, 16) * 16]
    return [(ty, zs, seg) for seg in segs[::-1] for ty in range(0, 10) for zs in range(0, OD + 2)]


_PLANS = {}


def enumerate_plans(lib, case):
    """every feasible plan of the case as v8 tuples, in grid order; each readback repeats its pin"""
    if case.key not in _PLANS:
        a, plans = P.dry_args(case), []
        for v4 in pin_grid(case):
            got = decide(lib, case, v4, a)
            if got is not None:
                assert pin_of(case.family, got) == v4, (case.id, v4, got)
                plans.append(got)
        _PLANS[case.key] = plans
    return _PLANS[case.key]


def default_plan(lib, case):
    return decide(lib, case)


def one_per_signature(case, plans):
    seen, out = set(), []
    for v in plans:
        s = signature(case, v)
        if s not in seen:
            seen.add(s)
            out.append(v)
    return out


def sweep_list(lib, case):
    """the plans the GPU sweep executes: the whole feasible list of a small shape, one plan per class signature of a large one,
    and the default plan in either"""
    plans = enumerate_plans(lib, case)
    run = plans if case.small else one_per_signature(case, plans)
    d = default_plan(lib, case)
    return run if d in run else run + [d]


# ------------------------------------------------------------------------------------------------ the host rules, restated
PF = 12                                                   # loader chunks per thread, every instance (the dispatch tables)
NOT_BLDS = {(32, 32, 3, 1), (32, 32, 4, 2), (16, 32, 4, 2)}     # conv_bf16.hip dispatch(): CBG, kernel taps read from L2


def conv_patch(inst, TY, TX):
    """conv_bf16.hip run(): (rows, cols, loader chunks, LDS bytes) of an output patch TY x TX"""
    ci, co, k, s = inst
    blds = inst not in NOT_BLDS
    nstep, nt = ceil(k ** 3 * ci, 32), ceil(co, 16)
    pitch, cpv = (ci, ci // 8) if ci >= 8 else (1, 1)
    fixed = (nstep * nt * 64 * 16 if blds else 0) + (32 if ci == 1 else (1 if blds else 2) * ((nstep * 4 + 3) & ~3)) * 4 + 4 * 16 * 20 * 4
    rows, cols = (TY - 1) * s + k, (TX - 1) * s + k
    return rows, cols, k * rows * cols * cpv, ((k * rows * cols * pitch * 2 + 15) & ~15) + fixed


def conv_fits(inst, TY, TX):
    _, _, chunks, nbytes = conv_patch(inst, TY, TX)
    return "regs" if chunks > PF * 256 else "lds" if nbytes > 64 * 1024 else None


def conv_search(inst, OH, OW):
    """-> [(score, v8)] of every candidate of the search in loop order (TY outer, nbx inner), without the nbx that repeat the TX
    of a smaller one (their last column would be empty; conv_bf16.hip run())"""
    s, out = inst[3], []
    for TY in range(1, min(16, OH) + 1):
        for nbx in range(1, 9):
            TX = ceil(OW, nbx)
            if ceil(OW, TX) != nbx or conv_fits(inst, TY, TX):
                continue
            rows, cols, _, nbytes = conv_patch(inst, TY, TX)
            tiles = ceil(TX * TY, 16)
            halo = float(TX * TY * s * s) / (float(rows) * cols)
            lanes = float(TX * TY) / (tiles * 16.0)
            work = 1.0 if tiles >= 8 else tiles / 8.0
            out.append((halo * lanes * work, (TY, nbx, TX, ceil(OH, TY), rows, cols, tiles, nbytes)))
    return out


def conv_rule(inst, OH, OW):
    """the search's choice: the first of the best scores"""
    best = None
    for score, v in conv_search(inst, OH, OW):
        if best is None or score > best[0]:
            best = (score, v)
    return best and best[1]


def convT_rule(ci, OD, OH, OW, p, epm):
    """convT_bf16.hip run(): rows per band"""
    nQz, nQy, nQx = ((o - 1 + p) // 2 - p // 2 + 1 for o in (OD, OH, OW))
    cols, TY = nQx + 1, 0
    for ty in range(1, min(nQy, 32) + 1):
        if 2 * (ty + 1) * cols * (ci // 8) > PF * 256 or 2 * (ty + 1) * cols * ci * 2 + 16 + 4 * 16 * 20 * 4 > 56 * 1024:
            break
        TY = ty
        if ceil(ty * nQx, 16) >= 16:
            break
    return (TY, ceil(nQy, TY), nQz, nQy, nQx, 1, epm, 0)


#               (CI, CO, K, S): MTG, m-tiles per row group (bww_bf16.hip dispatch(): BW)
BWW_MTG = {(1, 8, 3, 1): 2, (1, 16, 3, 1): 2, (8, 8, 3, 1): 14, (8, 16, 3, 1): 14, (16, 8, 3, 1): 27, (16, 16, 3, 1): 27,
           (16, 32, 3, 1): 27, (32, 16, 3, 1): 54, (32, 32, 3, 1): 27, (8, 8, 4, 2): 32, (16, 16, 4, 2): 64, (8, 16, 4, 2): 32,
           (16, 32, 4, 2): 32, (32, 32, 4, 2): 32, (32, 32, 1, 1): 2, (1, 32, 1, 1): 1}


def ngrp(inst):
    ci, _, k, _ = inst
    return ceil(ceil(k ** 3 * ci, 16), BWW_MTG[inst])


def band_rows(inst, OW, OH):
    """bww_bf16.hip band_rows(): the largest band (<= 8 rows) whose patch fits the loaders' registers and the LDS; 0: none"""
    ci, co, k, s = inst
    pitch = (ci if ci <= 16 else ci + 4) if ci >= 8 else 1
    gp, cpx, cpg = (co if co <= 16 else co + 4), (ci // 8 if ci >= 8 else 1), co // 8
    OWp = (OW + 15) & ~15
    colsR, colsA, TY = (OW - 1) * s + k, (OWp - 1) * s + k + 4, 0
    for ty in range(1, min(8, OH) + 1):
        rows = (ty - 1) * s + k
        nbytes = ((((k * rows * colsA * pitch + 7) & ~7) + ty * OWp * gp + 16) * 2 + 15) & ~15
        if rows * colsR * cpx > ((PF + 2) // 3) * 256 or ty * OW * cpg > 4 * 256 or nbytes > (120 if ty == 1 else 72) * 1024:
            break
        TY = ty
    return TY


def bww_rule(inst, N, OD, OH, OW, p, max_slabs=MAX_SLABS):
    """bww_bf16.hip run() / run_seg(): -> the readback v8, or None where the kernel does not take the launch"""
    ci, co, k, _ = inst
    G = ngrp(inst)
    knob = 256 if k ** 3 * ci * co * 4 <= 32 * 1024 else 128

    def one(ow, budget, nseg):
        TY = band_rows(inst, ow, OH)
        if TY < 1:
            return None
        nband = ceil(OH, TY)
        zsegs = min(max(min(budget, knob // G // nseg) // (N * nband), 1), OD)
        zper = ceil(OD, zsegs)
        zsegs = ceil(OD, zper)
        return None if N * nband * zsegs > budget else (TY, nband, zsegs, zper, N * nband * zsegs)
    if band_rows(inst, OW, 1) >= 1:
        r = one(OW, max_slabs, 1)
        return r and r[:4] + (1, OW, G, r[4])
    if p != 0:
        return None
    seg = OW & ~15
    while seg >= 16 and band_rows(inst, seg, 1) < 1:
        seg -= 16
    if seg < 16:
        return None
    nseg = ceil(OW, seg)
    seg = (ceil(OW, nseg) + 15) & ~15
    total, first = 0, None
    for x0 in range(0, OW, seg):
        r = one(min(seg, OW - x0), max_slabs - total, nseg) if max_slabs - total >= 1 else None
        if r is None:
            return None
        first, total = first or r, total + r[4]
    return first[:4] + (nseg, seg, G, total)


# ------------------------------------------------------------------------------------------------ class signatures
def instance(case):
    return (case.family,) + case.channels + (case.geom["k"], case.geom["s"])


def _trips(tiles, wpn):
    """(idle, trips, tail) of `tiles` 16-voxel tiles dealt to the wpn waves of an n-tile, two per wave and trip
    (`for (t = wave / NT; t < ntiles; t += 2 * WPN)` with t2 = t + WPN)"""
    per = [len(range(j, tiles, wpn)) for j in range(wpn)]
    trips = "single" if tiles <= wpn else "pair" if tiles <= 2 * wpn else "loop"
    return min(per) == 0, trips, any(n % 2 == 1 and n >= 3 for n in per)


def signature(case, v):
    f, (ci, co) = case.family, case.channels
    OD, OH, OW = out_dims(case.geom)
    if f == CONV_BF16:
        TY, nbx, TX, nby, rows, cols, tiles, _ = v
        inst = instance(case)[1:]
        assert TX == ceil(OW, nbx) and nby == ceil(OH, TY) and tiles == ceil(TX * TY, 16) and (rows, cols) == conv_patch(inst, TY, TX)[:2], (case.id, v)
        nt = ceil(co, 16)
        _, trips, tail = _trips(tiles, 1 if nt >= 4 else 4 // nt)
        cap = conv_fits(inst, TY + 1, TX) or conv_fits(inst, TY, TX + 1) or "none"
        return ("one" if nby == 1 else "div" if OH % TY == 0 else "rag", "one" if nbx == 1 else "div" if OW % TX == 0 else "rag",
                "rows" if TX % 16 == 0 else "wraps", trips, tail, cap)
    if f == CONVT_BF16:
        TY, nband, _, nQy, nQx, _, _, _ = v
        assert nband == ceil(nQy, TY), (case.id, v)
        idle, trips, tail = _trips(ceil(TY * nQx, 16), 4 // (2 * co // 16))                # convT_bf16.hip: NT = 2 CO / 16, WPN = 4 / NT
        return ("1" if nband == 1 else "div" if nQy % TY == 0 else "rag", "1" if TY == 1 else ">1",
                ("idle" if idle else trips) + ("+tail" if tail else ""), f"{'odd' if OD % 2 else 'even'}/p{case.geom['p']}")
    TY, nband, zsegs, zper, nseg, seg, G, _ = v
    assert nseg == ceil(OW, seg) and G == ngrp(instance(case)[1:]) and (nseg > 1 or (nband == ceil(OH, TY) and
           zper == ceil(OD, zsegs) and zsegs == ceil(OD, zper))), (case.id, v)
    last = OW - (nseg - 1) * seg                          # the row's last (or only) segment
    return ("all" if zsegs == 1 else "1" if zper == 1 else "2" if zper == 2 else "3+", OD % zper != 0,
            "1" if TY == 1 else "div" if OH % TY == 0 else "rag",
            f"{'1' if last <= 16 else '>1'}/{'whole' if last % 16 == 0 else 'pad'}",
            "1" if nseg == 1 else "2+eq" if OW % seg == 0 else "2+short")


# What an instance cannot have -- (instance, coordinate, value): reason.  Everything else must occur in the instance's sweep, and
# tests/test_bf16_plan_space.py holds each entry to the arithmetic it quotes (conv_reach, band_rows).
TX_MAX, TY_MAX = 33, 16                                     # the widest and highest patch of the sweep shapes
_HEAD = "no halo: the patch is TX x TY voxels, 16 x 33 of them at 64 bytes are 34 KB in 2112 chunks -- inside both caps at every sweep extent, and at the workload's (24^3 at most)"
_C1 = "one bf16 per voxel: the 3 x 18 x 35 patch of a 16 x 33 output is 1890 chunks and 4 KB"
_S2 = "(TY + 1)(TX + 1) <= 48 (3072 chunks of 4 planes x 4 chunks a voxel): at most 36 output voxels, 3 tiles for the 2 waves of an n-tile"
UNREACHABLE = {
    ((1, 8, 3, 1), "cap", "regs"): _C1, ((1, 8, 3, 1), "cap", "lds"): _C1, ((1, 16, 3, 1), "cap", "regs"): _C1, ((1, 16, 3, 1), "cap", "lds"): _C1,
    ((8, 8, 3, 1), "cap", "regs"): "3 x 18 x 35 voxels of one chunk: 1890 of 3072", ((8, 8, 3, 1), "cap", "lds"): "30 KB of patch beside 7 KB of fragments",
    ((16, 16, 3, 1), "cap", "regs"): "the bytes bind first: 14 KB of fragments leave 45 KB = 1400 voxels of 2 chunks, 2800 < 3072",
    ((32, 32, 3, 1), "cap", "lds"): "fragments in L2: 3072 chunks are 48 KB",
    ((32, 32, 4, 2), "cap", "lds"): "fragments in L2: 3072 chunks are 48 KB", ((16, 32, 4, 2), "cap", "lds"): "fragments in L2: 3072 chunks are 48 KB",
    ((32, 32, 4, 2), "trips", "loop"): _S2, ((32, 32, 4, 2), "tail", True): _S2,
    ((32, 32, 1, 1), "cap", "regs"): _HEAD, ((32, 32, 1, 1), "cap", "lds"): _HEAD, ((32, 1, 1, 1), "cap", "regs"): _HEAD,
    ((32, 1, 1, 1), "cap", "lds"): _HEAD, ((1, 32, 1, 1), "cap", "regs"): _HEAD, ((1, 32, 1, 1), "cap", "lds"): _HEAD,
}
_ODD = "a 1 -> C 3x3x3 layer with rows of an even length is bww_c1m_h_k's: this kernel sees odd rows alone"
_W32 = "a row of 32 voxels is 66 input columns x 4 rows x 4 chunks = 1056 of the loader's 1024: rows of 31 at most fit one band"
UNREACHABLE_BWW = {
    ((1, 8, 3, 1), "kblk", "1/whole"): _ODD, ((1, 8, 3, 1), "kblk", ">1/whole"): _ODD, ((1, 8, 3, 1), "segs", "2+eq"): _ODD,
    ((1, 16, 3, 1), "kblk", "1/whole"): _ODD, ((1, 16, 3, 1), "kblk", ">1/whole"): _ODD, ((1, 16, 3, 1), "segs", "2+eq"): _ODD,
    ((32, 32, 4, 2), "kblk", ">1/whole"): _W32,
}
UNREACHABLE_CONVT = {       # convT_bf16_k
    ((32, 32, 4, 2), "wtiles", "idle"): "C_out = 32: NT = 2 x 32 / 16 = 4 n-tiles, WPN = 4 / NT = 1 wave each, and a band has a tile",
}
_PAD = "bww_bf16.hip run() cuts unpadded rows only: the zero frame of a padded row belongs to its first and last segment"
UNREACHABLE_PADDED = {("segs", "2+eq"): _PAD, ("segs", "2+short"): _PAD}     # bww_bf16_k, any instance, a case with pad != 0


def conv_reach(inst):
    """the (trips, tail, cap) values conv_bf16_k's instance can take with a patch of the sweep extents, by the restated rule"""
    out = dict(trips=set(), tail=set(), cap=set())
    nt = ceil(inst[1], 16)
    for TY in range(1, TY_MAX + 1):
        for TX in range(1, TX_MAX + 1):
            if conv_fits(inst, TY, TX):
                continue
            _, trips, tail = _trips(ceil(TX * TY, 16), 1 if nt >= 4 else 4 // nt)
            out["trips"].add(trips), out["tail"].add(tail)
            out["cap"].add(conv_fits(inst, TY + 1, TX) or conv_fits(inst, TY, TX + 1) or "none")
    return out


def values(case):
    """coordinate -> the values the sweep of the case's kernel instance must take: every one but the listed unreachable.  (The
    padded cases of an instance stand beside unpadded ones, so UNREACHABLE_PADDED narrows a case, not its instance:
    `case_values`.)"""
    f, (ci, co), inst = case.family, case.channels, instance(case)[1:]
    if f == CONV_BF16:
        full = dict(ycut={"one", "div", "rag"}, xcut={"one", "div", "rag"}, wrap={"rows", "wraps"}, trips={"single", "pair", "loop"},
                    tail={False, True}, cap={"none", "regs", "lds"})
        return {c: {x for x in vals if (inst, c, x) not in UNREACHABLE} for c, vals in full.items()}
    if f == CONVT_BF16:
        full = dict(bands={"1", "div", "rag"}, ty={"1", ">1"}, wtiles={"idle", "single", "pair", "loop", "loop+tail"},
                    zpar={"even/p0", "even/p1", "odd/p0", "odd/p1"})
        return {c: {x for x in vals if (inst, c, x) not in UNREACHABLE_CONVT} for c, vals in full.items()}
    full = dict(zrun={"1", "2", "3+", "all"}, zrag={False, True}, t1={"1", "div", "rag"},
                kblk={"1/whole", "1/pad", ">1/whole", ">1/pad"}, segs={"1", "2+eq", "2+short"})
    return {c: {x for x in vals if (inst, c, x) not in UNREACHABLE_BWW} for c, vals in full.items()}


def case_values(case):
    """the values one case can take: its instance's, without what its padding rules out"""
    pad = case.family == BWW_BF16 and case.geom["p"] != 0
    return {c: {x for x in vals if not (pad and (c, x) in UNREACHABLE_PADDED)} for c, vals in values(case).items()}


# ------------------------------------------------------------------------------------------------ cases
# Shapes: OUTPUT extents of conv_bf16_k and bww_bf16_k, INPUT extents of convT_bf16_k; batch.  "small*": the whole feasible list runs,
# of the others one plan per class signature.  What each is there for:
#   conv_bf16_k   (4, 6, 9): 24 plans (TY 1 .. 6, TX 9 | 5 | 3 | 2: a second and a ragged column, bands that divide 6 and do not).
#                 (4, 17, 33): OH = 17 = 16 + a ragged row, OW = 33: nbx 2 -> TX 17 and a ragged 16, nbx 3 -> 11 | 11 | 11, down to
#                 TX 5: 112 plans where everything fits.  (4, 16, 32): TX 32 and 16, tiles that hold whole rows, bands of 2, 4, 8, 16.
#   convT_bf16_k  input (3, 5, 6) and its twin with the output one plane short, as convT_mfma_k's; input (3, 17, 15): output 34 x 30, nQy 18,
#                 nQx 16 (pads 2, 3: 14): a band of TY rows is TY tiles, so TY = 1 .. 18 runs every tile count from an idle wave to
#                 a second trip with and without a lone last tile, in one band to eighteen, whole and ragged
#   bww_bf16_k    (8, 7, 40) x 2: z-runs of 8, 4, 3 (ragged), 2, 1; TY 1 .. 7 over 7 rows; rows of 40 = 2 k-blocks and a padded third,
#                 segments 16 | 16 | 8 and 32 | 8.  (9, 6, 32): z-runs 9, 5 (ragged), 3, 2 (ragged), 1; whole k-blocks, segments 16 | 16;
#                 TY 2, 3, 6 divide 6.  (3, 3, 13) x 2: one padded k-block, a ragged run of 2 planes.  The rest is what
#                 the workload's default plans add to these (the second cover condition): (8, 4, 56): segments 32 | 24 and 16 | 16 | 16 | 8
#                 with bands of 1 .. 4 rows; (9, 3, 20): a padded second k-block on an odd axis; (8, 2, 16) and (8, 2, 32): whole
#                 k-blocks with even z-runs; (8, 2, 1): rows of one voxel (the 74 discriminators' last layers)
SHAPES = {
    CONV_BF16: [("small", (4, 6, 9), 2), ("4x17x33", (4, 17, 33), 2), ("4x16x32", (4, 16, 32), 1)],
    CONVT_BF16: [("small", (3, 5, 6), 2), ("small-odd", (3, 5, 6), 2), ("small-3x17x15", (3, 17, 15), 2)],
    BWW_BF16: [("small", (8, 7, 40), 2), ("9x6x32", (9, 6, 32), 1), ("small-3x3x13", (3, 3, 13), 2), ("8x4x56", (8, 4, 56), 1),
               ("9x3x20", (9, 3, 20), 1), ("small-8x2x16", (8, 2, 16), 1), ("8x2x32", (8, 2, 32), 1), ("small-8x2x1", (8, 2, 1), 1)],
}
# conv_bf16_k's heads and its 32 -> 32 k4 s2 instance also run what the workload gives them alone: a single output voxel (the 74
# discriminators), 6^3 (one patch, one band short), and rows that one column of patches holds in whole bands (12 x 12, 12 x 24) or
# two and more hold raggedly (10 x 20: TX 7 | 7 | 6)
HEAD_SHAPES = SHAPES[CONV_BF16] + [("small-2x1x1", (2, 1, 1), 2), ("2x12x12", (2, 12, 12), 1), ("2x12x24", (2, 12, 24), 1)]
S2_SHAPES = SHAPES[CONV_BF16] + [("small-2x1x1", (2, 1, 1), 2), ("small-2x6x6", (2, 6, 6), 2), ("2x10x20", (2, 10, 20), 1)]
ENTRY = {CONV_BF16: "conv_h", CONVT_BF16: "convT_h", BWW_BF16: "bww_h"}
ADD_OFF = P.ADD_OFF


def _cases(family, variant, ci, co, k, s, p, add_off=None, bias=False, decline=(), shapes=None, **kw):
    out = []
    for tag, dims, N in shapes or SHAPES[family]:
        if family == CONVT_BF16:
            g = _g("convT_h", ci, co, k, s, p, dims, **kw)
            if tag.endswith("odd"):
                od = out_dims(g)
                g["out"] = (od[0] - 1,) + od[1:]
        else:
            g = _g(ENTRY[family], ci, co, k, s, p, tuple((d - 1) * s + k - 2 * p for d in dims), **kw)
            assert out_dims(g) == dims, (variant, dims, out_dims(g))
        c = Bf16Case(f"{ci + kw.get('ci1', 0)}to{co + kw.get('co1', 0)}-k{k}s{s}-{variant}-{tag}", family, g, N, add_off, bias, decline)
        c.small, c.variant = tag.startswith("small"), variant
        out.append(c)
    return out


GATED = dict(slope=1.0, gate=True)
BD = dict(flip=True, slope=1.0, gate=True)               # the input-gradient form of a stride-1 layer: flipped layout, LeakyReLU' gate
CASES = {f: [] for f in FAMILIES}
_conv = lambda *a, **kw: CASES[CONV_BF16].extend(_cases(CONV_BF16, *a, decline=NO_CONV3, **kw))
# one per code path of conv_bf16_k (conv_bf16.hip dispatch()), with the epilogues the workload or the route gives it.  The one-channel
# kernels in front take a 1 -> C 3x3x3 layer whose rows are a multiple of 4 voxels: these extents are not (W = 11 | 35 | 34 + ...)
_conv("plain", 1, 8, 3, 1, 0)                                                               # C_in = 1: the taps as K (g.c0 at 74)
_conv("bd", 1, 16, 3, 1, 2, **BD)                                                           # input-gradient of g.f2's kind
_conv("plain", 8, 8, 3, 1, 0)                                                               # C_in >= 8, fragments in LDS
_conv("cat", 8, 16, 3, 1, 0, ci1=8)                                                         # two inputs
_conv("add", 16, 16, 3, 1, 2, ADD_OFF, add=True, **BD)                                       # skip-gradient window
_conv("keepw", 16, 8, 3, 1, 2, co1=8, keep=1, **BD)                                          # Dropout, keep bits written; two outputs
_conv("keepr", 16, 8, 3, 1, 2, co1=8, keep=2, **BD)                                          # keep bits read
_conv("plain", 32, 32, 3, 1, 0)                                                             # !BLDS, C_in = 32: tap-direct
_conv("plain", 32, 32, 4, 2, 0, shapes=S2_SHAPES)                                            # d.d2b / d.d3b
_conv("plain", 16, 32, 4, 2, 1)                                                             # !BLDS, C_in = 16: table-driven from L2
_conv("bd", 8, 16, 4, 2, 1, ADD_OFF, add=True, **GATED)                                      # stride 2 with fragments in LDS
_conv("plain", 32, 32, 1, 1, 0, shapes=HEAD_SHAPES)                                          # the 1x1x1 head forms
_conv("bd", 32, 32, 1, 1, 0, shapes=HEAD_SHAPES, **BD)
_conv("bd", 1, 32, 1, 1, 0, shapes=HEAD_SHAPES, **BD)
_conv("bias", 32, 1, 1, 1, 0, bias=True, slope=1.0, shapes=HEAD_SHAPES)                                        # C_out = 1: scalar stores
CONVT_PAIRS = [(16, 8), (32, 16), (8, 8), (16, 16), (32, 32)]                                # convT_bf16.hip CT_CASE
for _ci, _co in CONVT_PAIRS:
    CASES[CONVT_BF16] += _cases(CONVT_BF16, "keepw", _ci, _co, 4, 2, 1, keep=1)              # EPM 0: Philox, keep bits written
    CASES[CONVT_BF16] += _cases(CONVT_BF16, "keepr", _ci, _co, 4, 2, 1, keep=2)              # EPM 1
    CASES[CONVT_BF16] += _cases(CONVT_BF16, "plain", _ci, _co, 4, 2, 1)                      # EPM 0
    CASES[CONVT_BF16] += _cases(CONVT_BF16, "bd", _ci, _co, 4, 2, 0, ADD_OFF, slope=1.0, gate=True, add=True)   # EPM 2
for _ci, _co in CONVT_PAIRS[:2]:                                                            # the generator's two on the cycle path
    CASES[CONVT_BF16] += _cases(CONVT_BF16, "keepr2", _ci, _co, 4, 2, 2, keep=2)
    CASES[CONVT_BF16] += _cases(CONVT_BF16, "keepr3", _ci, _co, 4, 2, 3, keep=2)
# what the step's input-gradient and cycle-path launches add: one band of 16 tiles without a lone last one (16 -> 16 at 74), two such
# bands (8 -> 8: nQy 16, nQx 32, TY 8), a single tile (32 -> 32 on a 4^3 output), one band of three tiles with pad 3
_BD = dict(slope=1.0, gate=True, add=True)
CASES[CONVT_BF16] += _cases(CONVT_BF16, "bd", 8, 8, 4, 2, 0, ADD_OFF, shapes=[("small-2x15x31", (2, 15, 31), 1)], **_BD)
CASES[CONVT_BF16] += _cases(CONVT_BF16, "bd", 16, 16, 4, 2, 0, ADD_OFF, shapes=[("small-2x7x15", (2, 7, 15), 1)], **_BD)
CASES[CONVT_BF16] += _cases(CONVT_BF16, "bd", 32, 32, 4, 2, 0, ADD_OFF, shapes=[("small-2x1x1", (2, 1, 1), 2)], **_BD)
CASES[CONVT_BF16] += _cases(CONVT_BF16, "keepr3", 32, 16, 4, 2, 3, shapes=[("small-3x7x7", (3, 7, 7), 1)], keep=2)
for (_ci, _co, _k, _s), _ in BWW_MTG.items():
    if _ci == 1 and _k == 3:                               # bww_c1m_h_k takes rows of an even length: only the odd-row shape is this kernel's
        CASES[BWW_BF16] += _cases(BWW_BF16, "p0", _ci, _co, _k, _s, 0, shapes=[("small-8x7x33", (8, 7, 33), 2)])
        continue
    CASES[BWW_BF16] += _cases(BWW_BF16, "p0", _ci, _co, _k, _s, 0)
CASES[BWW_BF16] += _cases(BWW_BF16, "p0", 32, 32, 4, 2, 0, shapes=[("small-2x3x24", (2, 3, 24), 2)])   # its widest rows: two k-blocks, the second padded
CASES[BWW_BF16] += _cases(BWW_BF16, "cat", 8, 16, 3, 1, 0, ci1=8)                            # two inputs
CASES[BWW_BF16] += _cases(BWW_BF16, "p1T", 8, 16, 4, 2, 1)                                   # a transposed layer's: in := upstream gradient
CASES[BWW_BF16] += _cases(BWW_BF16, "p3T", 16, 32, 4, 2, 3, shapes=SHAPES[BWW_BF16][:1])
ALL_CASES = [c for f in FAMILIES for c in CASES[f]]
