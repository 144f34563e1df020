"""Host routing of the bf16 convolution family against a recorded table (no GPU: the dry queries take made-up pointers
and never dereference them).

tests/golden/bf16_routing.json was recorded by tests/golden/make_bf16_routing.py from the library BEFORE the host code
of the seven bf16 convolution files was folded into shared helpers.  The generator holds the argument struct of every
dry query -- tem_conv_bf16_describe, tem_conv_transpose_bf16_describe or tem_conv_bwd_weight_bf16_nslab -- and the
table its answer: the return code (for kernel gradients the slab count) and the kernel name with the template
arguments the planner chose.  The test rebuilds each struct and asserts the same answer; the coverage conditions below
are asserted over the table itself, so a thinned-out table fails."""
import ctypes as C
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bf16_routing.json")
OK, EINVAL, EUNSUPPORTED, ESHAPE = 0, -1, -2, -3
ENTRIES = {"conv": "tem_conv_bf16_describe", "convT": "tem_conv_transpose_bf16_describe", "bww": "tem_conv_bwd_weight_bf16_nslab"}

# (C_in, C_out, k, s) of the dispatch tables (concat / split channels summed), by file
K3 = [(8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32)]
K4 = [(8, 8), (16, 16), (32, 32), (8, 16), (16, 32)]
C1 = [(1, 8), (8, 1), (1, 16), (16, 1)]
CT = [(16, 8), (32, 16), (8, 8), (16, 16), (32, 32)]
TABLES = {
    "conv_bf16": ("conv", 3, [(i, o, 3, 1) for i, o in C1 + K3] + [(i, o, 4, 2) for i, o in K4] +
                  [(32, 32, 1, 1), (32, 1, 1, 1), (1, 32, 1, 1)]),
    "conv3_bf16": ("conv", 3, [(i, o, 3, 1) for i, o in K3] + [(8, 8, 4, 2), (8, 16, 4, 2), (16, 16, 4, 2), (16, 32, 4, 2)]),
    "conv2d_bf16": ("conv", 2, [(i, o, 3, 1) for i, o in C1 + K3] + [(i, o, 4, 2) for i, o in K4]),
    "convT_bf16": ("convT", 3, [(i, o, 4, 2) for i, o in CT]),
    "convT2d_bf16": ("convT", 2, [(i, o, 4, 2) for i, o in CT]),
    "bww_bf16": ("bww", 3, [(i, o, 3, 1) for i, o in [(1, 8), (1, 16)] + K3] + [(i, o, 4, 2) for i, o in K4] +
                 [(32, 32, 1, 1), (1, 32, 1, 1)]),
    "bww2d_bf16": ("bww", 2, [(i, o, 3, 1) for i, o in [(1, 8), (1, 16)] + K3] + [(i, o, 4, 2) for i, o in K4]),
}
FAMILIES = ["conv2d_bf16_k<", "conv3_bf16_k<", "conv_bf16_k<", "convT_bf16_k<", "convT2d_bf16_k<", "bww_bf16_k<", "bww2d_bf16_k<",
            "c1_mfma_h_k<", "c1out_h_k<", "bww_c1m_h_k<"]


def _view(v, spec):
    """spec: [ptr, N, D, H, W, C, sN, sD, sH, sW] or None (an absent view stays zero)"""
    if spec:
        v.ptr, v.N, v.D, v.H, v.W, v.C, v.sN, v.sD, v.sH, v.sW = spec


def build_args(case):
    from transfer_em_amd import _lib
    k, s, p = case["k"], case["s"], case["p"]
    if case["entry"] == "bww":
        a = _lib.tem_bww_args()
        _view(a.dout, case["out0"])
        a.slabs, a.slab_stride, a.nslab, a.accumulate = 0x40000000, 0, case["nslab"], 0
    else:
        a = _lib.tem_conv_args()
        _view(a.out0, case["out0"])
        _view(a.out1, case["out1"])
        a.w, a.w_layout = case["w"], case["w_layout"]
        e, ep = case["ep"], a.ep
        ep.bias, ep.slope, ep.gate_slope = e["bias"], e["slope"], e["gate_slope"]
        _view(ep.gate, e["gate"])
        _view(ep.add, e["add"])
        ep.add_off[:] = e["add_off"]
        ep.dropout, ep.seed, ep.site, ep.step = e["dropout"], 42, 3, 7
        ep.drop_org[:] = e["drop_org"]
        ep.drop_dims[:] = e["drop_dims"]
        ep.keep_mask, ep.keep_mode = e["keep_mask"], e["keep_mode"]
    _view(a.in0, case["in0"])
    _view(a.in1, case["in1"])
    a.kd, a.kh, a.kw = k
    a.sd, a.sh, a.sw = s
    a.pd, a.ph, a.pw = p
    return a


def query(lib, case):
    """-> (return code or slab count, kernel name)"""
    name = C.create_string_buffer(96)
    rc = getattr(lib, ENTRIES[case["entry"]])(C.byref(build_args(case)), name, 96)
    return rc, name.value.decode()


def _cases():
    """the generator's argument structs, each with its recorded answer (`rc`, `name`)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_bf16_routing", os.path.join(os.path.dirname(GOLDEN), "make_bf16_routing.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    recorded = {cid: key.split("|", 1) for key, ids in json.load(open(GOLDEN)).items() for cid in ids}
    assert sorted(recorded) == sorted(c["id"] for c in gen.cases)          # every case has an answer, no answer lacks its case
    return [dict(c, rc=int(recorded[c["id"]][0]), name=recorded[c["id"]][1]) for c in gen.cases]


def test_routing_matches_the_recorded_table():
    from transfer_em_amd import _lib
    lib = _lib.load()
    bad = []
    for c in _cases():
        rc, name = query(lib, c)
        if (rc, name) != (c["rc"], c["name"]):
            bad.append(f"{c['id']}: recorded ({c['rc']}, {c['name']!r}), now ({rc}, {name!r})")
    assert not bad, "\n".join(bad)


def _dims(c):
    return 2 if (c["k"][0] == 1 and c["in0"][2] == 1 and c["k"][1] > 1) else 3


def _layer(c):
    ci = c["in0"][5] + (c["in1"][5] if c["in1"] else 0)
    co = c["out0"][5] + (c["out1"][5] if c.get("out1") else 0)
    return ci, co, c["k"][2], c["s"][2]


def test_table_covers_every_dispatch_entry_at_two_sizes():
    cases = [c for c in _cases() if c["rc"] >= 0]
    for fname, (entry, nd, table) in TABLES.items():
        for layer in table:
            hits = [c for c in cases if c["entry"] == entry and _dims(c) == nd and _layer(c) == layer and c["name"].startswith(fname + "_k<")]
            sizes = {tuple(c["out0"][1:5]) for c in hits}
            assert len(sizes) >= 2, (fname, layer, sizes)


def test_table_covers_every_kernel_family_and_epilogue_form():
    cases = _cases()
    names = {c["name"] for c in cases if c["rc"] >= 0}
    for fam in FAMILIES:
        assert any(n.startswith(fam) for n in names), fam
    assert any(n.startswith("conv_bf16_k<") and n.endswith("true>") for n in names)      # BLDS
    assert any(n.startswith("conv_bf16_k<") and n.endswith("false>") for n in names)
    for epm in (0, 1, 2):
        assert any(n.startswith("convT_bf16_k<") and n.endswith(f", {epm}>") for n in names), epm
    for epm in (0, 2):          # (the 2-D kernel has no compiled Dropout-read form: keep mode 2 runs its run-time flags)
        assert any(n.startswith("convT2d_bf16_k<") and n.endswith(f", {epm}>") for n in names), epm
    ok = [c for c in cases if c["rc"] >= 0]
    for entry in ("conv", "convT"):
        for nd in (2, 3):
            mine = [c for c in ok if c["entry"] == entry and _dims(c) == nd]
            if entry == "conv":
                assert any(c["ep"]["bias"] for c in mine), (entry, nd, "bias")
                assert any(c["in1"] for c in mine) and any(c["out1"] for c in mine), (entry, nd, "concat / split")
            assert any(c["ep"]["gate"] for c in mine), (entry, nd, "gate")
            assert any(c["ep"]["add"] and any(c["ep"]["add_off"]) for c in mine), (entry, nd, "add with offset")
            for mode in (0, 1, 2):
                assert any(c["ep"]["dropout"] and (c["ep"]["keep_mode"] if c["ep"]["keep_mask"] else 0) == mode for c in mine), (entry, nd, "keep mode", mode)
            assert any(c["ep"]["dropout"] and c["ep"]["drop_dims"][0] for c in mine), (entry, nd, "dropout frame")
    assert any(c["entry"] == "bww" and c["in1"] for c in ok)


def test_table_covers_the_rejections():
    cases = _cases()
    for entry in ENTRIES:
        codes = {c["rc"] for c in cases if c["entry"] == entry}
        assert {EINVAL, EUNSUPPORTED, ESHAPE} <= codes, (entry, codes)
    tags = {}
    for c in cases:
        for t in c.get("tags", []):
            tags.setdefault(t, []).append(c)
    # every named rejection is in the table with the code it must keep ...
    for tag, rc in (("ptr_off16", EUNSUPPORTED), ("ptr_off8", EUNSUPPORTED), ("pair_outside", EUNSUPPORTED), ("n_mismatch", ESHAPE),
                    ("gate_extent", ESHAPE), ("gate_channels", ESHAPE), ("add_off0_2d", ESHAPE), ("dropout_c_out", EUNSUPPORTED),
                    ("span_at_2^31", EUNSUPPORTED), ("gate_at_2^30", EUNSUPPORTED), ("add_at_2^30", EUNSUPPORTED),
                    ("mask_at_2^33", EUNSUPPORTED)):
        assert tags.get(tag), tag
        assert all(c["rc"] == rc for c in tags[tag]), tag
    for axis in ("sN", "sD", "sH", "sW"):
        for what in ("in8", "out4"):
            assert any(c["rc"] == EUNSUPPORTED for c in tags.get(f"stride_{what}_{axis}_3d", [])), (what, axis)
        for what in ("in8", "out4"):
            hit = tags.get(f"stride_{what}_{axis}_2d", [])
            assert hit and all((c["rc"] >= 0 and c["name"]) if axis == "sD" else c["rc"] == EUNSUPPORTED for c in hit), (what, axis)
    # ... and the case just below each limit is accepted, with a kernel name: the pair sits on the boundary
    for tag in ("span_below_2^31", "gate_below_2^30", "add_below_2^30", "mask_below_2^33"):
        assert tags.get(tag), tag
        assert all(c["rc"] >= 0 and c["name"] for c in tags[tag]), tag


def test_rows_wider_than_one_band_are_segmented_not_refused():
    """Kernel gradients whose row overflows a single-row band (tag "wide", tests/golden/make_bf16_routing.py): admitted
    with pad 0 -- on both sides of each form's limit and at the 260 model's widths --, refused with a pad.  And for
    every admitted kernel gradient of the table the count is what the launch will be held to: tem_conv_bwd_weight_bf16
    asks the same query with nslab = that count and refuses any other answer."""
    from transfer_em_amd import _lib
    lib = _lib.load()
    cases = _cases()
    wide = [c for c in cases if "wide" in c.get("tags", [])]
    assert len(wide) >= 30
    for c in wide:
        assert (c["rc"] >= 1 and c["name"]) if not any(c["p"]) else c["rc"] == EUNSUPPORTED, (c["id"], c["rc"])
    for fam in ("bww_bf16_k<", "bww2d_bf16_k<"):
        assert sum(c["name"].startswith(fam) for c in wide) >= 12, fam
    for c in cases:
        if c["entry"] == "bww" and c["rc"] >= 1:
            assert query(lib, dict(c, nslab=c["rc"])) == (c["rc"], c["name"]), c["id"]
