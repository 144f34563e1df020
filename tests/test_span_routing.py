"""Where the convolution entry points stop admitting a view, and what the tile batch of the inference plans may be (no
GPU: the dry queries take made-up pointers and never dereference them).

Every tiled kernel guards its 32-bit address arithmetic with a host-side span check; past it the entry point answers
TEM_EUNSUPPORTED and the call goes to the next kernel, in the end to the 64-bit direct forms.

* `LIMITS` is the table of those checks ("Span limits of the convolution kernels"), derived from the
  dispatch functions and the kernels' address arithmetic.  For every row two argument structs are built, one with the
  limited quantity at the largest admissible value below the limit and one with the smallest at or above it; the first
  must be answered with the family's kernel, the second with the kernel that runs instead (fp32) or TEM_EUNSUPPORTED
  (bf16, which has no direct form).  tests/test_gpu_span_limits.py runs the same structs on the device.
* The plan ladder: for every launch of the dense inference plan, the largest batch N whose kernel is the one of N = 1,
  and utils.stable_tile_batch, the smallest of them, to which predict_cube / predict_volume lower `tile_batch`."""
import pytest
import torch

from span_cases import FAMILIES, LIMITS, OPERANDS, build, query

EUNSUPPORTED = -2


# ------------------------------------------------------------------------------------------------ a. the limit table
@pytest.mark.parametrize("row", LIMITS, ids=lambda r: r.id)
def test_limit_row_admits_below_and_refuses_at(row):
    from transfer_em_amd import _lib
    lib = _lib.load()
    below, at = build(row, "below"), build(row, "at")
    assert below.value < row.limit <= at.value, (below.value, row.limit, at.value)
    # nothing admissible lies between the two: the next step of the alignment grid from `below` is at or past the limit
    assert below.value + below.step >= row.limit and at.value - at.step < row.limit, (below.value, below.step, at.value)
    rc, name = query(lib, row, below)
    assert name.startswith(row.kernel + "<") and rc >= 0, (row.id, "below", rc, name)
    rc, name = query(lib, row, at)
    assert not name.startswith(row.kernel + "<"), (row.id, "at", rc, name)
    if row.fallback is None:                       # bf16 without another bf16 kernel behind it: refused
        assert rc == EUNSUPPORTED and name == "", (row.id, "at", rc, name)
    else:
        assert name.startswith(row.fallback + "<"), (row.id, "at", rc, name)


def test_limit_table_covers_every_family_and_guarded_operand():
    for fam, kernels in FAMILIES.items():
        rows = [r for r in LIMITS if r.family == fam]
        assert {r.kernel for r in rows} == set(kernels), (fam, {r.kernel for r in rows})
        have = {(r.kernel, r.operand, r.quantity) for r in rows}
        for need in OPERANDS[fam]:
            assert need in have, (fam, need)
    assert {r.family for r in LIMITS} == set(FAMILIES)
    assert len({r.id for r in LIMITS}) == len(LIMITS)
    for r in LIMITS:
        assert r.why and r.limit & (r.limit - 1) == 0, r.id           # a reason, and a power of two


@pytest.mark.parametrize("wrap", [None, "unsigned", "signed"])
def test_sentinel_frame_and_comparison_catch_a_truncated_offset(wrap):
    """The checks of tests/test_gpu_span_limits.py on a stand-in of a kernel's store, at a scale where the offset
    register has 16 bits: out[n sN + z sD + y sH + x sW + c] = value, the offset exact or truncated to 16 bits.  The
    exact store passes; a truncated one stays inside the allocation (that is what the head room is for) and is caught
    twice: sentinels outside the view are gone, and elements inside were never written."""
    import numpy as np
    from span_cases import frame_intact, framed, head_room, span, stretch
    v, value, _ = stretch((3, 4, 5, 8), "image", (1 << 16) + 256, "at", 4)    # the last image's tail lies past 2^16
    assert value >= (1 << 16) + 256 and v.N == 3
    head = head_room(span(v), 1 << 15)
    assert head >= 1 << 15
    buf, view = framed(v, torch.float32, "cpu", head)
    n, z, y, x, c = np.meshgrid(*[np.arange(e) for e in (v.N, v.D, v.H, v.W, v.C)], indexing="ij")
    off = n * v.sN + z * v.sD + y * v.sH + x * v.sW + c
    if wrap == "unsigned":
        off = off & 0xFFFF
    elif wrap == "signed":
        off = ((off + 0x8000) & 0xFFFF) - 0x8000
    assert off.min() >= -head and off.max() < span(v)                     # inside the allocation either way: no fault
    values = np.random.default_rng(0).standard_normal(off.shape).astype(np.float32)
    buf[torch.from_numpy(head + off.reshape(-1))] = torch.from_numpy(values.reshape(-1))
    inside, bad = frame_intact(buf, view)
    ok = bad == 0 and bool(torch.isfinite(inside).all()) and np.array_equal(inside.numpy(), values)
    assert ok == (wrap is None), (wrap, bad)


# ------------------------------------------------------------------------------------------------ b. the plan ladder
MODELS = [(74, True), (132, True), (260, True), (74, False), (132, False), (260, False)]
SCAN = {True: 800, False: 4200}       # batches scanned one by one: past every first change of the 3-D models, past the 2-D cap


def _ladder(edge, is3d, dtype):
    """layer -> largest N (< SCAN) whose route is that of N = 1, None where it never changes; and the layers whose
    template arguments change while the route stays"""
    from transfer_em_amd.utils import plan_routes, route_key
    base = plan_routes(edge, 1, is3d, dtype)
    last, vary = {k: None for k in base}, set()
    for n in range(2, SCAN[is3d]):
        cur = plan_routes(edge, n, is3d, dtype)
        for k in base:
            if last[k] is None and route_key(cur[k]) != route_key(base[k]):
                last[k] = n - 1
            elif last[k] is None and cur[k] != base[k]:
                vary.add(k)
    return last, vary


@pytest.fixture(scope="module")
def ladders():
    return {(e, d, t): _ladder(e, d, t) for e, d in MODELS for t in (torch.float32, torch.bfloat16)}


def test_plan_ladder_of_the_3d_fp32_models(ladders):
    """the first route change of each launch: N = 32, 36, 123, 129 on the 132 model, 196, 453, 720, 783 on the 74 model"""
    l132, _ = ladders[(132, True, torch.float32)]
    first = {"d1b": 31, "f2": 35, "c0": 122, "d1a": 122, "f1": 128}
    assert {k: l132[k] for k in first} == first
    assert all(v is None or v > 128 for k, v in l132.items() if k not in first), l132      # the other launches change later
    l74, vary = ladders[(74, True, torch.float32)]
    first = {"d1b": 195, "f2": 452, "c0": 719, "d1a": 719, "f1": 782}
    assert {k: l74[k] for k in first} == first
    assert all(v is None for k, v in l74.items() if k not in first), l74                    # ... or not below 800
    assert vary == {"u2a"}                    # conv_lds_k's tiles per wave (utils.route_key): 1 -> 2 at N = 5
    from transfer_em_amd.utils import plan_routes
    r1, r32 = plan_routes(132, 1), plan_routes(132, 32)
    assert r1["d1b"] == "conv_s2_k<8, 1, 4, true>" and r32["d1b"] == "conv_direct_k<8, 0, 8, 0, false>"
    assert r1["f2"] == "c1out_mfma_k<16, false, false>" and plan_routes(132, 36)["f2"] == "c1_stencil_k<16, 1, false, 6>"
    assert plan_routes(132, 123)["c0"].startswith("conv_rows_k<") and plan_routes(132, 129)["f1"].startswith("conv_direct_k<")


def test_2d_fp32_plans_run_the_direct_kernels_at_every_batch(ladders):
    for edge in (74, 132, 260):
        last, vary = ladders[(edge, False, torch.float32)]
        assert not any(last.values()) and not vary, (edge, last, vary)
    # the transposed layers' direct form, which no query names, as conv_launch spells it in Launch.meta["kernel"]
    # (the 2-D step's launch tables in test_gpu_2d_fullsize_oracle.py; plan_kernels() in test_gpu_model260.py)
    from transfer_em_amd.utils import plan_routes
    r = plan_routes(260, 3, False)
    assert (r["u2b"], r["u1b"]) == ("convT_direct_k<32, 16, 0, 16>", "convT_direct_k<16, 8, 0, 8>")


def test_template_arguments_vary_only_where_audited(ladders):
    """route_key compares kernel functions.  A template argument that changes with N below the stable batch must be one
    that leaves each output's sum order alone: conv_lds_k's MTW (accumulator tiles per wave) on g.u2a of the 74 model
    is the only one."""
    seen = {key: vary for key, (_, vary) in ladders.items() if vary}
    assert seen == {(74, True, torch.float32): {"u2a"}}, seen


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("edge,is3d", MODELS)
def test_stable_tile_batch_is_the_ladders_lowest_rung(ladders, edge, is3d, dtype):
    from transfer_em_amd.utils import STABLE_BATCH_SEARCH_MAX, default_tile_batch, stable_tile_batch
    last, _ = ladders[(edge, is3d, dtype)]
    rungs = [v for v in last.values() if v]
    stable = stable_tile_batch(edge, is3d, dtype)
    if rungs:
        assert stable == min(rungs), (stable, last)
    else:                                             # no change below the scan: the search agrees up to there
        assert stable >= SCAN[is3d] - 1
    assert 1 <= stable <= STABLE_BATCH_SEARCH_MAX
    assert default_tile_batch(edge, is3d) <= stable, (edge, is3d, dtype, default_tile_batch(edge, is3d), stable)


def test_stable_tile_batch_numbers():
    from transfer_em_amd.utils import TILE_BATCH, default_tile_batch, stable_tile_batch
    assert stable_tile_batch(132, True, torch.float32) == 31
    assert stable_tile_batch(74, True, torch.float32) == 195
    assert stable_tile_batch(260, True, torch.float32) == 2        # g.f2 leaves c1out_mfma_k at N = 3
    assert default_tile_batch(132, True) == default_tile_batch(74, True) == TILE_BATCH == 27
    assert default_tile_batch(260, True) == 2
    from transfer_em_amd import utils
    assert (132, True, torch.float32) in utils._STABLE_BATCH       # cached per (edge, is3d, dtype)
    # the bf16 figures of DESIGN.md's plan ladder (74 / 132 / 260); past the 2-D ones the plan fails: bf16 has no direct form
    assert [stable_tile_batch(e, True, torch.bfloat16) for e in (74, 132, 260)] == [359, 35, 2]
    assert [stable_tile_batch(e, False, torch.bfloat16) for e in (74, 132, 260)] == [51781, 13975, 2627]


def test_effective_batch_lowers_a_large_request():
    from transfer_em_amd.utils import _effective_batch
    assert _effective_batch(40, 132, True, 48) == 31
    assert _effective_batch(None, 132, True, 48) == 27
    assert _effective_batch(40, 132, True, 17) == 17
    assert _effective_batch(1, 132, True, 48) == 1
    assert _effective_batch(None, 260, True, 8) == 2
    assert _effective_batch(5000, 132, False, 10000) == 5000        # 2-D fp32: direct kernels, nothing to lower
