"""The argument structs of tests/test_bf16_routing.py (`cases`, built on import) and the recorder of their answers:
    python tests/golden/make_bf16_routing.py [out.json]
writes tests/golden/bf16_routing.json, {"<return code>|<kernel name>": [case ids]}.  Run it on the library whose routing
is to be KEPT -- the table in the tree was recorded before the bf16 host code was folded into shared helpers;
re-record only when routing changes on purpose."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_bf16_routing as T   # noqa: E402

PTR = {"in0": 0x10000000, "in1": 0x18000000, "out0": 0x20000000, "out1": 0x28000000, "gate": 0x30000000, "add": 0x38000000}
NO_EP = dict(bias=None, slope=1.0, gate=None, gate_slope=1.0, add=None, add_off=[0, 0, 0], dropout=0, keep_mask=None, keep_mode=0,
             drop_org=[0, 0, 0], drop_dims=[0, 0, 0])
cases = []


def view(which, N, D, H, W, C):
    """a contiguous channels-last view"""
    return [PTR[which], N, D, H, W, C, D * H * W * C, H * W * C, W * C, C]


def out_extent(entry, n, k, s, p):
    return (n - 1) * s + k - 2 * p if entry == "convT" else (n + 2 * p - k) // s + 1


def case(cid, entry, nd, ci, co, k, s, n, p=0, N=1, ci1=0, co1=0, ep=None, tags=(), w=0x50000000, w_layout=0, nslab=1024, edit=None):
    """One layer on an n^nd input (ci + ci1 channels in, co + co1 out); `edit(c)` bends the finished case."""
    kk, ss, pp = ([k] * 3, [s] * 3, [p] * 3) if nd == 3 else ([1, k, k], [1, s, s], [0, p, p])
    o = out_extent(entry, n, k, s, p)
    di, do = (n, o) if nd == 3 else (1, 1)
    c = dict(id=cid, entry=entry, k=kk, s=ss, p=pp, w=w, w_layout=w_layout, nslab=nslab, tags=list(tags),
             in0=view("in0", N, di, n, n, ci), in1=view("in1", N, di, n, n, ci1) if ci1 else None,
             out0=view("out0", N, do, o, o, co), out1=view("out1", N, do, o, o, co1) if co1 else None,
             ep=json.loads(json.dumps({**NO_EP, **(ep or {})})))
    if edit:
        edit(c)
    cases.append(c)
    return c


def gate_of(c, C=None):
    return view("gate", *c["out0"][1:5], C or c["out0"][5])


def with_gate(c):
    c["ep"]["gate"] = gate_of(c)
    c["ep"]["gate_slope"] = 0.2


def with_add(off):
    def f(c):                      # a skip-gradient window 4 smaller than the output, placed at `off`
        N, D, H, W, Cc = c["out0"][1:6]
        c["ep"]["add"] = view("add", N, max(D - 4, 1), H - 4, W - 4, Cc)
        c["ep"]["add_off"] = [off if D > 1 else 0, off, off]
    return f


def both(*fs):
    def f(c):
        for g in fs:
            g(c)
    return f


DROP = [dict(dropout=1, keep_mask=None, keep_mode=0), dict(dropout=1, keep_mask=0x60000000, keep_mode=1),
        dict(dropout=1, keep_mask=0x60000000, keep_mode=2)]


def frame(nd):
    return dict(drop_org=[2 if nd == 3 else 0, 3, 5], drop_dims=[300 if nd == 3 else 1, 300, 300])


def set_stride(which, axis, delta):
    def f(c):
        c[which][6 + ["sN", "sD", "sH", "sW"].index(axis)] += delta
    return f


# ---------------------------------------------------------------- the dispatch tables, two sizes each
SIZES = {("conv", 3, 3): (100, 18), ("conv", 3, 4): (100, 18), ("conv", 3, 1): (29, 8), ("conv", 2, 3): (132, 20), ("conv", 2, 4): (132, 20),
         ("convT", 3, 4): (50, 9), ("convT", 2, 4): (66, 9), ("bww", 3, 3): (100, 18), ("bww", 3, 4): (100, 18), ("bww", 3, 1): (29, 8),
         ("bww", 2, 3): (132, 20), ("bww", 2, 4): (132, 20)}
seen = set()
for fname, (entry, nd, table) in T.TABLES.items():
    for ci, co, k, s in table:
        for n in SIZES[entry, nd, k]:
            if n in (100, 132) and max(ci, co) == 32:                          # (32 channels: past the row one band holds -- the "wide" cases below)
                n = 60 if nd == 3 else 68
            p = 1 if entry == "convT" else 0
            if (entry, nd, ci, co, k, s, n) not in seen:                      # the plain layer: the first kernel of the route that takes it
                seen.add((entry, nd, ci, co, k, s, n))
                case(f"{entry}{nd}d_{ci}to{co}_k{k}s{s}_n{n}", entry, nd, ci, co, k, s, n, p=p, N=2 if nd == 2 else 1)
            if fname == "conv_bf16":                                          # past the kernels that are tried first
                if co % 8 == 0:                                               # (a keep mask to draw: conv3_bf16_k and c1_mfma_h_k decline)
                    case(f"conv3d_{ci}to{co}_k{k}s{s}_n{n}_draw", entry, nd, ci, co, k, s, n, ep=DROP[1])
                else:                                                         # (c1out_h_k reads the two plain kernel layouts only)
                    case(f"conv3d_{ci}to{co}_k{k}s{s}_n{n}_layout2", entry, nd, ci, co, k, s, n, w_layout=2)
            if fname == "bww_bf16" and ci == 1 and k == 3:                     # (bww_c1m_h_k wants an even row length)
                case(f"bww3d_{ci}to{co}_k{k}s{s}_n{n + 1}_oddW", entry, nd, ci, co, k, s, n + 1)

# ---------------------------------------------------------------- concat inputs, split outputs, flipped kernels, padding
for nd, n in ((3, 100), (3, 18), (2, 132), (2, 20)):
    case(f"conv{nd}d_concat8+8to8_n{n}", "conv", nd, 8, 8, 3, 1, n, ci1=8)
    case(f"conv{nd}d_16tosplit8+8_n{n}", "conv", nd, 16, 8, 3, 1, n, co1=8)
    case(f"conv{nd}d_concat16+16tosplit8+8_n{n}_draw", "conv", nd, 16, 8, 3, 1, n, ci1=16, co1=8, ep=DROP[1])
    case(f"conv{nd}d_8to8_flip_p2_n{n}", "conv", nd, 8, 8, 3, 1, n, p=2, w_layout=1, edit=with_gate)
    case(f"conv{nd}d_16to8_k4s2_p1_n{n}", "conv", nd, 16, 16, 4, 2, n, p=1)
    case(f"bww{nd}d_concat8+8to8_n{n}", "bww", nd, 8, 8, 3, 1, n, ci1=8)
    case(f"bww{nd}d_concat16+16to16_n{n}_p1", "bww", nd, 16, 16, 3, 1, n, ci1=16, p=1)
    case(f"bww{nd}d_8to8_n{n}_nslab16", "bww", nd, 8, 8, 3, 1, n, nslab=16)
    case(f"bww{nd}d_8to8_n{n}_N4", "bww", nd, 8, 8, 3, 1, n, N=4)
for flip in (0, 1):
    case(f"conv3d_1to8_flip{flip}_gate", "conv", 3, 1, 8, 3, 1, 40, p=2 * flip, w_layout=flip, edit=with_gate)
    case(f"conv3d_8to1_flip{flip}_gate", "conv", 3, 8, 1, 3, 1, 40, p=2 * flip, w_layout=flip, edit=with_gate)
    case(f"conv3d_16to1_flip{flip}_bias", "conv", 3, 16, 1, 3, 1, 40, p=2 * flip, w_layout=flip, ep=dict(bias=0x70000000, slope=0.2))

# ---------------------------------------------------------------- every epilogue form
for entry, nd, ci, co, k, s, n in (("conv", 3, 8, 8, 3, 1, 60), ("conv", 3, 16, 16, 4, 2, 60), ("conv", 2, 8, 8, 3, 1, 132), ("conv", 2, 16, 16, 4, 2, 132),
                                   ("convT", 3, 16, 8, 4, 2, 30), ("convT", 3, 8, 8, 4, 2, 30), ("convT", 2, 16, 8, 4, 2, 66), ("convT", 2, 32, 32, 4, 2, 17)):
    base = f"{entry}{nd}d_{ci}to{co}_k{k}_n{n}_ep_"
    kw = dict(p=1 if entry == "convT" else 0, N=2)
    if entry == "conv":
        case(base + "bias", entry, nd, ci, co, k, s, n, ep=dict(bias=0x70000000, slope=0.2), **kw)
        case(base + "bias_gate_add", entry, nd, ci, co, k, s, n, ep=dict(bias=0x70000000), edit=both(with_gate, with_add(2)), **kw)
    case(base + "lrelu", entry, nd, ci, co, k, s, n, ep=dict(slope=0.2), **kw)
    case(base + "gate", entry, nd, ci, co, k, s, n, edit=with_gate, **kw)
    case(base + "add0", entry, nd, ci, co, k, s, n, edit=with_add(0), **kw)
    case(base + "add2", entry, nd, ci, co, k, s, n, edit=with_add(2), **kw)
    case(base + "gate_add2", entry, nd, ci, co, k, s, n, edit=both(with_gate, with_add(2)), **kw)
    for m, d in enumerate(DROP):
        case(base + f"drop{m}", entry, nd, ci, co, k, s, n, ep={**d, "slope": 0.2}, **kw)
        case(base + f"drop{m}_frame", entry, nd, ci, co, k, s, n, ep={**d, **frame(nd), "slope": 0.2}, **kw)
        case(base + f"drop{m}_gate", entry, nd, ci, co, k, s, n, ep=d, edit=with_gate, **kw)
    case(base + "dropout_without_mask_mode2", entry, nd, ci, co, k, s, n, ep=dict(dropout=1, keep_mask=None, keep_mode=2), **kw)
    case(base + "mask_without_dropout", entry, nd, ci, co, k, s, n, ep=dict(dropout=0, keep_mask=0x60000000, keep_mode=1), **kw)

# ---------------------------------------------------------------- rejections
LAYER = {"conv": (8, 8, 3, 1), "convT": (16, 8, 4, 2), "bww": (8, 8, 3, 1)}
for entry in ("conv", "convT", "bww"):
    ci, co, k, s = LAYER[entry]
    for nd, n in ((3, 40), (2, 40)):
        b = f"{entry}{nd}d_{ci}to{co}_"
        kw = dict(p=1 if entry == "convT" else 0, N=2)
        out = "out0"

        def bump(which, field, delta):
            def f(c):
                c[which][field] += delta
            return f
        case(b + "in_ptr_off16", entry, nd, ci, co, k, s, n, tags=["ptr_off16"], edit=bump("in0", 0, 8), **kw)
        case(b + "in_ptr_off8", entry, nd, ci, co, k, s, n, tags=["ptr_off8"], edit=bump("in0", 0, 4), **kw)
        if entry != "bww":      # (the kernel gradient reads dout in 16-byte chunks, as it reads in0)
            case(b + "out_ptr_off16", entry, nd, ci, co, k, s, n, edit=bump(out, 0, 8), **kw)
            case(b + "out_ptr_off8", entry, nd, ci, co, k, s, n, tags=["ptr_off8"], edit=bump(out, 0, 4), **kw)
        else:
            case(b + "dout_ptr_off16", entry, nd, ci, co, k, s, n, tags=["ptr_off16"], edit=bump(out, 0, 8), **kw)
        case(b + "in_ptr_off2", entry, nd, ci, co, k, s, n, edit=bump("in0", 0, 2), **kw)
        for axis in ("sN", "sD", "sH", "sW"):
            # 8 + 4: a multiple of 4 elements, not of 8 (16-byte input chunks); 4 + 2: not of 4 (8-byte stores); 2-D views carry odd sD
            d_in, d_out = (1, 1) if (nd == 2 and axis == "sD") else (12 if axis != "sW" else 4, 6 if axis != "sW" else 2)
            case(b + f"in_{axis}_plus{d_in}", entry, nd, ci, co, k, s, n, tags=[f"stride_in8_{axis}_{nd}d"], edit=set_stride("in0", axis, d_in), **kw)
            case(b + f"out_{axis}_plus{d_out}", entry, nd, ci, co, k, s, n, tags=[f"stride_out4_{axis}_{nd}d"], edit=set_stride(out, axis, d_out), **kw)
            if entry != "bww":
                case(b + f"out_{axis}_plus4", entry, nd, ci, co, k, s, n, edit=set_stride(out, axis, 4), **kw)
                case(b + f"gate_{axis}_plus2", entry, nd, ci, co, k, s, n, edit=both(with_gate, lambda c, axis=axis: set_stride("gate", axis, 2)(c["ep"])), **kw)
                case(b + f"add_{axis}_plus2", entry, nd, ci, co, k, s, n, edit=both(with_add(2), lambda c, axis=axis: set_stride("add", axis, 2)(c["ep"])), **kw)
        if nd == 2:
            case(b + "odd_sD_everywhere", entry, nd, ci, co, k, s, n, tags=["odd_sD_2d"],
                 edit=both(set_stride("in0", "sD", 1), set_stride(out, "sD", 3)), **kw)
        case(b + "pair_24to8", entry, nd, 24, 8, k, s, n, tags=["pair_outside"], **kw)
        case(b + "pair_8to24", entry, nd, 8, 24, k, s, n, tags=["pair_outside"], **kw)
        case(b + "k5", entry, nd, ci, co, 5, s, n, **kw)
        case(b + "k3s2", entry, nd, ci, co, 3, 2, n, **kw)
        case(b + "N_mismatch", entry, nd, ci, co, k, s, n, tags=["n_mismatch"], edit=bump(out, 1, 1), **kw)
        case(b + "null_in0", entry, nd, ci, co, k, s, n, edit=lambda c: c["in0"].__setitem__(0, None), **kw)
        case(b + "null_out", entry, nd, ci, co, k, s, n, edit=lambda c: c["out0"].__setitem__(0, None), **kw)
        case(b + "zero_extent", entry, nd, ci, co, k, s, n, edit=lambda c: c["in0"].__setitem__(3, 0), **kw)
        # a view whose span sits just below / at 2^31 elements: images 2^31 - (dense image) [- 8] elements apart
        for which in ("in0", "out0"):
            def far(at):
                def f(c, which=which):
                    v = c[which]
                    v[6] = (1 << 31) - v[2] * v[3] * v[4] * v[5] - (0 if at else 8)
                return f
            case(b + f"{which}_span_below_2^31", entry, nd, ci, co, k, s, n, tags=["span_below_2^31"], edit=far(False), **kw)
            case(b + f"{which}_span_at_2^31", entry, nd, ci, co, k, s, n, tags=["span_at_2^31"], edit=far(True), **kw)
        if entry == "bww":
            case(b + "nslab0", entry, nd, ci, co, k, s, n, nslab=0, **kw)
            case(b + "nslab1", entry, nd, ci, co, k, s, n, nslab=1, **kw)
            case(b + "concat_extent", entry, nd, ci, co, k, s, n, ci1=8, edit=bump("in1", 3, 1), **kw)
            continue
        case(b + "null_w", entry, nd, ci, co, k, s, n, w=None, **kw)
        case(b + "gate_extent", entry, nd, ci, co, k, s, n, tags=["gate_extent"], edit=both(with_gate, lambda c: c["ep"]["gate"].__setitem__(3, c["ep"]["gate"][3] + 1)), **kw)
        case(b + "gate_channels", entry, nd, ci, co, k, s, n, tags=["gate_channels"], edit=lambda c: c["ep"].__setitem__("gate", gate_of(c, 4)), **kw)
        case(b + "gate_wider", entry, nd, ci, co, k, s, n, edit=lambda c: c["ep"].__setitem__("gate", gate_of(c, 16)), **kw)
        case(b + "add_channels", entry, nd, ci, co, k, s, n, edit=both(with_add(2), lambda c: c["ep"]["add"].__setitem__(5, 4)), **kw)
        case(b + "add_N", entry, nd, ci, co, k, s, n, edit=both(with_add(2), lambda c: c["ep"]["add"].__setitem__(1, 1)), **kw)
        if nd == 2:
            case(b + "add_off0", entry, nd, ci, co, k, s, n, tags=["add_off0_2d"], edit=both(with_add(2), lambda c: c["ep"]["add_off"].__setitem__(0, 1)), **kw)
            case(b + "add_depth2", entry, nd, ci, co, k, s, n, edit=both(with_add(2), lambda c: c["ep"]["add"].__setitem__(2, 2)), **kw)
        if entry == "conv":     # (every transposed layer has a multiple of 8 output channels: its tables end the query first)
            case(b + "dropout_c_out1", entry, nd, 8, 1, k, s, n, tags=["dropout_c_out"], ep=DROP[1], **kw)
            case(b + "dropout_c_out1_nomask", entry, nd, 16, 1, k, s, n, tags=["dropout_c_out"], ep=DROP[0], **kw)
            case(b + "gate_c_out1_layout2", entry, nd, 8, 1, k, s, n, w_layout=2, edit=with_gate, **kw)
            case(b + "concat_extent", entry, nd, ci, co, k, s, n, ci1=8, edit=bump("in1", 3, 1), **kw)
            case(b + "split_extent", entry, nd, ci, co, k, s, n, co1=8, edit=bump("out1", 3, 1), **kw)
            case(b + "concat_1+8", entry, nd, 1, 8, k, s, n, ci1=8, **kw)
        else:
            case(b + "dropout_c_out4", entry, nd, 16, 4, k, s, n, ep=DROP[1], **kw)
            case(b + "bias", entry, nd, ci, co, k, s, n, ep=dict(bias=0x70000000), **kw)
            case(b + "concat", entry, nd, ci, co, k, s, n, ci1=8, **kw)
        # gate / add spans just below / at 2^30 elements (their buffer loads address bytes below 2^31)
        for which, tag in (("gate", "gate"), ("add", "add")):
            def far(at, which=which):
                def f(c):
                    (with_gate if which == "gate" else with_add(2))(c)
                    v = c["ep"][which]
                    v[6] = (1 << 30) - v[2] * v[3] * v[4] * v[5] - (0 if at else 8)
                return f
            case(b + f"{which}_span_below_2^30", entry, nd, ci, co, k, s, n, tags=[f"{tag}_below_2^30"], edit=far(False), **kw)
            case(b + f"{which}_span_at_2^30", entry, nd, ci, co, k, s, n, tags=[f"{tag}_at_2^30"], edit=far(True), **kw)
        # the keep mask of a dropout frame: 2 images x D x H x W x 8 channels below / at 2^33 elements
        dd = [1024, 1024, 512] if nd == 3 else [1, 1 << 15, 1 << 14]
        below = dd[:2] + [dd[2] - 1]
        case(b + "mask_below_2^33", entry, nd, ci, co, k, s, n, tags=["mask_below_2^33"], ep={**DROP[1], "drop_dims": below}, **kw)
        case(b + "mask_at_2^33", entry, nd, ci, co, k, s, n, tags=["mask_at_2^33"], ep={**DROP[1], "drop_dims": dd}, **kw)
        case(b + "mask_at_2^33_no_dropout", entry, nd, ci, co, k, s, n, ep={"drop_dims": dd}, **kw)

# ---------------------------------------------------------------- kernel gradients of rows wider than one band
# A pad-0 row whose single-row band overflows the loaders' registers is cut into column segments (run() of bww_bf16.hip /
# bww2d_bf16.hip); only the width matters, so the other extents are small (3-D: D 8, H = W; 2-D: H 12).  Per layer form the
# last width that is one launch, the first that is segmented, and the widest at which the 260 model launches the form.
def wide(nd, ci, co, k, s, w, ci1=0, p=0):
    d, h = (8, w) if nd == 3 else (1, 12)
    o = lambda n: (n + 2 * p - k) // s + 1
    kk, ss, pp = ([k] * 3, [s] * 3, [p] * 3) if nd == 3 else ([1, k, k], [1, s, s], [0, p, p])
    cid = f"bww{nd}d_{ci}{'+' + str(ci1) if ci1 else ''}to{co}_k{k}s{s}_wide{w}" + (f"_p{p}" if p else "")
    cases.append(dict(id=cid, entry="bww", k=kk, s=ss, p=pp, w=0x50000000, w_layout=0, nslab=8192, tags=["wide"],
                      in0=view("in0", 1, d, h, w, ci), in1=view("in1", 1, d, h, w, ci1) if ci1 else None,
                      out0=view("out0", 1, o(d) if nd == 3 else 1, o(h), o(w), co), out1=None, ep=json.loads(json.dumps(NO_EP))))


WIDE = [(3, 8, 16, 3, 1, 8, 171, 228), (3, 16, 32, 3, 1, 0, 171, 108), (3, 32, 16, 3, 1, 0, 86, 116), (3, 32, 32, 3, 1, 0, 86, 118),
        (3, 8, 8, 4, 2, 0, 258, 254), (3, 16, 16, 4, 2, 0, 130, 124), (3, 32, 32, 4, 2, 0, 66, 106),
        (2, 32, 16, 3, 1, 0, 171, 116), (2, 32, 32, 3, 1, 0, 171, 118), (2, 16, 16, 4, 2, 0, 258, 124), (2, 32, 32, 4, 2, 0, 130, 220)]
for nd, ci, co, k, s, ci1, limit, model in WIDE:
    for w in (limit - 1, limit, model):
        wide(nd, ci, co, k, s, w, ci1=ci1)
# (the 260 model's cycle cone launches three of the forms at a second width past the limit)
for nd, ci, co, k, s, w, ci1 in ((3, 8, 16, 3, 1, 192, 8), (3, 32, 16, 3, 1, 100, 0), (3, 16, 32, 3, 1, 102, 16)):
    wide(nd, ci, co, k, s, w, ci1=ci1)
wide(3, 32, 32, 3, 1, 86, p=1)                     # a padded row that is too wide stays refused
wide(2, 32, 32, 4, 2, 130, p=1)


def main():
    from transfer_em_amd import _lib
    lib = _lib.load()
    answers = {}
    for c in cases:
        rc, name = T.query(lib, c)
        answers.setdefault(f"{rc}|{name}", []).append(c["id"])
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in sorted(answers.items())) + "\n}\n")
    print(f"{len(cases)} cases, {len(answers)} answers -> {out}")


ids = [c["id"] for c in cases]
assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1]
if __name__ == "__main__":
    main()
