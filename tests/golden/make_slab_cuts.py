"""The cases of tests/test_slab_cuts.py (`cases(U)`) and the recorder of their answers:
    python tests/golden/make_slab_cuts.py [checkout] [out.json]
imports transfer_em_amd.utils from `checkout` (default: this tree) and writes tests/golden/slab_cuts.json,
{cutter: {group: [[number of slabs of every case], SHA-256 of the cases' reprs]}}: a group is the cases of one cutter,
shape, ROI and parameter over all budgets and ranks, in `cases`' order, and its digest is taken over the repr of each
returned list, one per line -- one digest per case would be 400 KB of hex alone, and this one changes with any of them.
A case that raises counts -1 slabs and enters the digest as "ValueError: message".  Run it on the checkout whose cuts are to be KEPT -- the table in the tree was
recorded from the cutters as each pass had them, before they were folded into one; re-record only when a cut changes on
purpose.

Every public slab cutter, over the shapes, the whole volume and an interior ROI, the budgets around each cutter's
thresholds (a row, a section, a section with its halo), three ranks, and each cutter's own parameter at its ends."""
import hashlib
import json
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden", "slab_cuts.json")
SHAPES = ((1, 1, 1), (5, 7, 9), (12, 40, 75))
IMAGE = (7, 9)
RANKS = ((0, 1), (0, 3), (2, 3))


def whole(shape):
    return ((0, 1),) * (3 - len(shape)) + tuple((0, n) for n in shape)


def interior(shape):
    return ((0, 1),) * (3 - len(shape)) + tuple((n // 4, n - n // 4) for n in shape)


def rois(shape):
    return [("whole", whole(shape))] + ([("roi", interior(shape))] if interior(shape) != whole(shape) else [])


def budgets(box, halo, itemsize=1):
    """None, 1, a row's bytes - 1 and exactly, a section - 1 and exactly, (1 + halo) sections - 1, exactly and + 1, far
    more than the volume: the positive ones, each once."""
    (z0, z1), (y0, y1), (x0, x1) = box
    row = (x1 - x0) * itemsize
    sec = (y1 - y0) * row
    cand = [1, row - 1, row, sec - 1, sec, (1 + halo) * sec - 1, (1 + halo) * sec, (1 + halo) * sec + 1, 1 << 40]
    return [None] + sorted({b for b in cand if b >= 1})


def cases(U):
    """(cutter name, case id, thunk) for every case; `U` is the utils module under test."""
    def over(name, shape, tag, box, halo, call, itemsize=1):
        for b in budgets(box, halo, itemsize):
            for rank, world in RANKS:
                yield name, f"{'x'.join(map(str, shape))}|{tag}|b={b}|r={rank}/{world}", \
                    (lambda b=b, rank=rank, world=world: call(b, rank, world))

    for shape in SHAPES + (IMAGE,):
        Z = shape[0] if len(shape) == 3 else 1
        for roi, box in rois(shape):
            for item in (1, 2):
                yield from over("hist_chunks", shape, f"{roi}|itemsize={item}", box, 0,
                                lambda b, r, w, box=box, item=item: U.hist_chunks(box, b, r, w, item), item)
            for win in (3, 11):
                for flat in (False, True):
                    yield from over("ssim_chunks", shape, f"{roi}|win={win}|flat={flat}", box, 0 if flat else win - 1,
                                    lambda b, r, w, box=box, win=win, flat=flat: U.ssim_chunks(box, win, flat, b, r, w))
        box = whole(shape)
        yield from over("zcorr_chunks", shape, "whole", box, 1, lambda b, r, w: U.zcorr_chunks(shape, b, r, w))
        for L in (1, 8):
            yield from over("zlag_chunks", shape, f"whole|max_lag={L}", box, min(L, Z - 1),
                            lambda b, r, w, L=L: U.zlag_chunks(shape, L, b, r, w))
            yield from over("plane_lag_chunks", shape, f"whole|max_lag={L}", box, 0,
                            lambda b, r, w, L=L: U.plane_lag_chunks(shape, L, b, r, w))
        for rad in (1, 8):
            yield from over("zshift_chunks", shape, f"whole|radius={rad}", box, 1,
                            lambda b, r, w, rad=rad: U.zshift_chunks(shape, rad, b, r, w))
            for reach in ((0, 0), (-3, 5)):
                yield from over("zshift_chunks_at", shape, f"whole|radius={rad}|reach={reach}", box, 1,
                                lambda b, r, w, rad=rad, reach=reach: U.zshift_chunks_at(shape, rad, reach, b, r, w))

    for shape in SHAPES:
        Z, Y, X = shape
        skips = [()] + ([(1, 2)] if Z > 4 else [])
        ident = np.tile(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (Z, 1, 1))
        bent = ident + np.array([[0.02, -0.1, 2.5], [0.1, -0.03, -4.25]]) * np.linspace(-1.0, 1.0, Z)[:, None, None]
        maps = [("identity", U.quantize_maps(ident)), ("bent", U.quantize_maps(bent))]
        gy, gx = U.field_grid(shape, 16)
        wave = np.zeros((Z, gy, gx, 2))
        wave[..., 0] = 1.5 * np.sin(np.arange(gy))[None, :, None] * np.linspace(-1.0, 1.0, Z)[:, None, None]
        wave[..., 1] = -1.25 * np.cos(np.arange(gx))[None, None, :]
        fields = [("zero", U.quantize_field(np.zeros((Z, gy, gx, 2)), 16)), ("wave", U.quantize_field(wave, 16))]
        stretched = np.arange(Z, dtype=np.int64) * (U.ZSPACE_UNIT * 7 // 4)
        taps = [("even", U.resample_z_taps(np.arange(Z, dtype=np.int64) * U.ZSPACE_UNIT)),
                ("stretched", U.resample_z_taps(stretched)), ("squeezed", U.resample_z_taps(stretched, nz=max(1, Z // 2)))]
        for roi, box in rois(shape):
            for gap in (1, 32):
                yield from over("repair_chunks", shape, f"{roi}|max_gap={gap}", box, 2 * gap,
                                lambda b, r, w, box=box, gap=gap: U.repair_chunks(box, shape, gap, b, r, w))
            for skip in skips:
                for lag in (1, 8):
                    nbr = U.section_neighbours(Z, skip, lag)
                    for rad in (0, 7):
                        yield from over("outlier_chunks", shape, f"{roi}|skip={skip}|max_lag={lag}|radius={rad}", box, 2,
                                        lambda b, r, w, box=box, nbr=nbr, rad=rad: U.outlier_chunks(box, shape, nbr, rad,
                                                                                                    b, r, w))
            for mname, M in maps:
                yield from over("warp_chunks", shape, f"{roi}|{mname}", box, 1,
                                lambda b, r, w, box=box, M=M: U.warp_chunks(box, shape, M, b, r, w))
                for fname, F in fields:
                    yield from over("field_chunks", shape, f"{roi}|{mname}|{fname}", box, 1,
                                    lambda b, r, w, box=box, M=M, F=F: U.field_chunks(box, shape, M, F, 16, b, r, w))
        for sname, step in (("2", 2), ("1/2", Fraction(1, 2)), ("3/2,2/3,1", (Fraction(3, 2), Fraction(2, 3), 1))):
            grid = U.rescale_shape(shape, step)
            for roi, box in rois(grid):
                yield from over("rescale_chunks", shape, f"{roi}|step={sname}", box, 1,
                                lambda b, r, w, box=box, step=step: U.rescale_chunks(box, shape, step, b, r, w))
        for tname, t in taps:
            for roi, box in rois((t.shape[0], Y, X)):
                yield from over("resample_z_chunks", shape, f"{roi}|{tname}", box, 1,
                                lambda b, r, w, box=box, t=t: U.resample_z_chunks(box, shape, t, b, r, w))
        for skip in skips:
            for lag in (1, 8):
                pairs = U.section_pairs(Z, skip, lag).pairs
                for rad in (1, 8):
                    for reach in ((0, 0), (-3, 5)):
                        yield from over("zshift_chunks_pairs", shape, f"skip={skip}|max_lag={lag}|radius={rad}|reach={reach}",
                                        whole(shape), lag, lambda b, r, w, pairs=pairs, rad=rad, reach=reach:
                                        U.zshift_chunks_pairs(shape, pairs, rad, reach, b, r, w))


def answers(U):
    """{cutter: {group: [[number of slabs per case], digest]}} and {cutter: {group: [case ids]}}."""
    out, ids, text = {}, {}, {}
    for name, cid, thunk in cases(U):
        group = cid[:cid.index("|b=")]
        try:
            got = thunk()
            n, line = len(got), repr(got)
        except ValueError as e:
            n, line = -1, f"ValueError: {e}"
        assert cid not in ids.setdefault(name, {}).setdefault(group, []), (name, cid)
        ids[name][group].append(cid)
        out.setdefault(name, {}).setdefault(group, [[], None])[0].append(n)
        text.setdefault((name, group), []).append(line)
    for (name, group), lines in text.items():
        out[name][group][1] = hashlib.sha256("\n".join(lines).encode()).hexdigest()
    return out, ids


def main():
    sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT)
    from transfer_em_amd import utils
    table, ids = answers(utils)
    out = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(name) + ": {\n" + ",\n".join(
            json.dumps(g) + ": " + json.dumps(v, separators=(",", ":")) for g, v in sorted(table[name].items())) + "\n}"
            for name in sorted(table)) + "\n}\n")
    print(f"{sum(len(c) for v in ids.values() for c in v.values())} cases in {sum(len(v) for v in table.values())} groups of {len(table)} cutters from {os.path.dirname(utils.__file__)} -> {out}")


if __name__ == "__main__":
    main()
