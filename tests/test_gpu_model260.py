"""The 260 model against the oracle, layer by layer and through tiling.

The 260 inference plan is not the 132 plan scaled up (plan ladder): g.d1b runs conv_direct_k from N = 1
(conv_s2_k stops at 1024 tiles per plane), g.f2 leaves c1out_mfma_k at N = 3, every Winograd and MFMA layer runs row
counts, z-runs and tile plans that no other size reaches, and the tile kernels see od = 222 (even, no multiple of 4),
tpad = 1 and edge 260 = 4 * 64 + 4.  This module holds every activation of that plan to the oracle over the whole
tensors (3-D at N = 1, 2-D at N = 3, fp32 and bf16), batches to single tiles bit for bit, and predict_cube /
predict_volume with a 260 model to the tile-wise oracle, to each other and to their mip / ensemble definitions.

The price is the oracle's 260^3 forward on the host, twice (fp32 and bf16 storage mode): 260^3 is the smallest input
at which these routes exist.  Both are computed once, in `ref260`; see the figures there.  The module takes 33 s on an
MI355X host with 16 threads, 16 s of it in that fixture; no test spends more than 4 s."""
import ctypes
import os
import time
from collections import namedtuple

import numpy as np
import pytest
import torch

from test_mips_plan import ref_pool
from util import FLIP_BOUND, _GEN_SAVED, failed_bars, forward_stats, l2_err, reference_tile, scaled_params

pytestmark = pytest.mark.gpu

MS_X, MS_Y = (0.02, 0.58), (-0.1, 0.4)           # with f2 * 20: the uint8 output spreads over the range
EDGE = 260
VOL = (262, 266, 540)                             # [z, y, x]: holds tile 0's 260^3 footprint, not the other two tiles'
START, SIZE = (21, 22, 19), (500, 200, 150)       # (x, y, z): 3 tiles of 222 along x -> batches of 2 + 1
START_R = (-30, 100, 19)                          # under "reflect": the request passes the near x and the far y face
VOL2 = (3, 430, 640)                              # 2-D stack
START2, SIZE2 = (-10, 15, 0), (600, 400, 3)       # 3 x 2 tiles of 222 per section, ragged in y and x
BF16_FACTOR = 4                                   # what this suite gives a reference-only measurement (GTOL_F_NOTEBOOK, inorm_f32)

Ref = namedtuple("Ref", "P x y sv y_bf sv_bf bars_bf vol rois tpad")
_LIVE = []                                        # generators whose plans the next part of the module releases


def _host_threads():
    """At most 16 host threads for the oracle (its C kernels run under OpenMP, torch's under its own pool)."""
    n = min(16, len(os.sched_getaffinity(0)))
    torch.set_num_threads(n)
    ctypes.CDLL("libgomp.so.1").omp_set_num_threads(n)
    return n


def _params(is3d):
    from oracle import graph
    P = scaled_params(graph.generator_param_shapes(is3d), 4)
    P["f2"] = P["f2"] * 20
    return P


def _keep(sv):
    return {key: sv[key] for key in _GEN_SAVED.values()}


def _bf16_bars(sv_bf, y_bf, sv, y):
    """Per layer BF16_FACTOR x the L2 distance of the oracle's bf16-mode activation from its own fp32-mode one: what
    bf16 storage itself moves a layer by, measured on the reference alone.  The output keeps its standing bars."""
    own = {layer: l2_err(sv_bf[key], sv[key]) for layer, key in _GEN_SAVED.items()}
    own["y"] = l2_err(y_bf, y)
    return {k: BF16_FACTOR * v for k, v in own.items() if k != "y"}, own


@pytest.fixture(scope="module")
def ref260(oracle_lib):
    """The oracle's 260^3 inference forward of tile 0 of the request, fp32 and bf16 mode, once for the module.
    Measured with 16 host threads: fp32 6.1 s, bf16 6.8 s, 16 s with the L2 figures of the bf16 bars (8 threads: 27 s
    + 30 s); 9.2 GB peak on the host, of which the two sets of saved activations that stay are 2.9 GB each."""
    from oracle import graph
    from transfer_em_amd.models.generator import generator_out
    from transfer_em_amd.utils import tile_plan
    threads = _host_threads()
    P = _params(True)
    vol = np.random.default_rng(260).integers(0, 256, VOL, dtype=np.uint8)
    out = generator_out(EDGE)
    od, buf, tpad, rois, _ = tile_plan(START, SIZE, out, (EDGE - out) // 2)
    assert (od, tpad, od + 2 * buf, len(rois)) == (222, 1, EDGE, 3)
    for lo, n in zip(rois[0], VOL[::-1]):                                    # tile 0's footprint: wholly inside
        assert 0 <= lo and lo + EDGE <= n, (rois[0], VOL)
    x = reference_tile(vol, rois[0], EDGE, MS_X)
    t0 = time.perf_counter()
    y, sv = graph.generator_forward(P, x, True, training=False)
    sv = _keep(sv)
    t1 = time.perf_counter()
    with graph.precision("bf16"):
        y_bf, sv_bf = graph.generator_forward(P, graph.round_bf16(x), True, training=False)
    sv_bf = _keep(sv_bf)
    t2 = time.perf_counter()
    bars, own = _bf16_bars(sv_bf, y_bf, sv, y)
    print(f"oracle 260^3 on {threads} threads: fp32 {t1 - t0:.1f} s, bf16 {t2 - t1:.1f} s; bf16 vs fp32 (L2): "
          + ", ".join(f"{k} {v:.2e}" for k, v in own.items()))
    return Ref(P, x, y, sv, y_bf, sv_bf, bars, vol, rois, tpad)


@pytest.fixture(scope="module")
def model3(tmp_path_factory):
    """EM2EM builds its train steps on the first train_step: a 260 model costs its parameters alone."""
    from transfer_em_amd.cgan import EM2EM
    model = EM2EM(EDGE, "m260", checkpoint_root=str(tmp_path_factory.mktemp("m260")))
    model.generator_g.params.load_dict(_params(True))
    assert not model._steps and (model.outdimsize, model.buffer) == (224, 18)
    _LIVE.append(model.generator_g)
    return model


def _run(gen, x, dtype=torch.float32):
    """Run the cached plan of x's shape on x; the plan (its act buffers hold this run until the next one)."""
    x = torch.as_tensor(x)
    plan = gen.plan(tuple(x.shape), dtype)
    plan.x.copy_(x.to(dtype))
    plan.run()
    torch.cuda.synchronize()
    return plan


def _report(tag, stats):
    worst = max(stats, key=lambda k: stats[k][0])
    worst2 = max(stats, key=lambda k: stats[k][1])
    flips = sum(s[2] for k, s in stats.items() if k != "y")
    total = sum(s[3] for k, s in stats.items() if k != "y")
    print(f"{tag}: worst rel_err {stats[worst][0]:.2e} at {worst}, worst L2 {stats[worst2][1]:.2e} at {worst2}, "
          f"{flips} sign flips of {total} | " + ", ".join(f"{k} {s[0]:.1e}/{s[1]:.1e}" for k, s in stats.items()))


def _check(tag, stats, dtype, bars_bf):
    """fp32: the standing 1e-4 of activation_stats(tol=1e-4) / test_generator_inference_132 on every layer and the
    output, and its flip bound.  bf16: the output's standing bars of test_generator_inference_bf16 (2e-2 of the range,
    5e-3 in L2); the activations' L2 bars from the reference alone (_bf16_bars)."""
    _report(tag, stats)
    if dtype == torch.float32:
        bad = failed_bars(stats, rel_tol=1e-4, flip_bound=FLIP_BOUND)
    else:
        bad = failed_bars(stats, rel_tol={"y": 2e-2}, l2_bars=dict(bars_bf, y=5e-3))
    assert not bad, (tag, bad)


def _routes_agree(gen, edge, is3d, dtype=torch.float32):
    from transfer_em_amd.utils import plan_routes
    ran = gen.plan_kernels()
    for n, kernels in ran.items():
        assert kernels == dict(plan_routes(edge, n, is3d, dtype)), (n, kernels)
    return ran


DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


# ------------------------------------------------------------------------------- 3-D: every layer against the oracle
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_every_layer_of_the_260_plan_matches_the_oracle(ref260, model3, dtype):
    """N = 1, whole tensors, all faces (d2a without its last plane, row and column: 125 is odd, the stride-2 layer
    behind it reads 124 and the plan computes no more).  Reference-only bf16 figures (oracle bf16 mode against its own
    fp32 mode, L2; the bar is 4 x each): c0 2.91e-3, d1a 3.75e-3, d1b 4.00e-3, d2a 4.73e-3, d2b 5.46e-3, u2a 7.06e-3,
    u2b 7.30e-3, mid 6.02e-3, u1a 5.61e-3, u1b 6.70e-3, f1 6.09e-3 (the output, on its standing bars: 7.06e-3)."""
    from transfer_em_amd.utils import route_key
    gen, dt = model3.generator_g, DTYPES[dtype]
    gen.clear_plans()
    x = torch.from_numpy(ref260.x)
    y = gen(x.to(dt))                                                        # the public call; its plan stays cached
    plan = gen.plan(tuple(x.shape), dt)
    assert torch.equal(y, plan.y) and tuple(y.shape) == (1, 224, 224, 224, 1)
    ran = _routes_agree(gen, EDGE, True, dt)
    assert list(ran) == [1]
    print(f"260^3 {dtype} routes at N = 1: {ran[1]}")
    if dtype == "fp32":
        assert route_key(ran[1]["d1b"]) == "conv_direct_k"                   # conv_s2_k: 1024 tiles per plane
        stats = forward_stats(plan, ref260.sv, ref260.y)
    else:
        stats = forward_stats(plan, ref260.sv_bf, ref260.y_bf)
    _check(f"260^3 {dtype} N=1", stats, dt, ref260.bars_bf)


def test_the_bars_see_one_wrong_tap(ref260, model3):
    """One tap of g.d1b (the conv_direct_k layer; the tap of largest magnitude, so that the planted error does not
    depend on a draw) times 1.05 in the HIP model's weights: the layers before it keep their bars, d1b and the output
    lose theirs.  The kernels are untouched."""
    gen = model3.generator_g
    P = dict(ref260.P)
    w = P["d1b"].copy()
    tap = tuple(int(i) for i in np.unravel_index(np.abs(w).argmax(), w.shape))
    w[tap] *= np.float32(1.05)
    P["d1b"] = w
    gen.params.load_dict(P)
    try:
        stats = forward_stats(_run(gen, ref260.x), ref260.sv, ref260.y)
    finally:
        gen.params.load_dict(ref260.P)
    _report(f"260^3 fp32, d1b{tap} x 1.05", stats)
    bad = failed_bars(stats, rel_tol=1e-4)
    print("outside their bars:", bad)
    assert "c0" not in bad and "d1a" not in bad, bad
    assert "d1b" in bad and "y" in bad, (bad, stats)


def test_batch_2_equals_two_batches_of_1(ref260, model3):
    """The only batch the pipeline uses for this model.  Tiles 0 and 1 of the request."""
    from transfer_em_amd.utils import plan_routes, route_key
    gen = model3.generator_g
    gen.clear_plans()
    xs = [ref260.x, reference_tile(ref260.vol, ref260.rois[1], EDGE, MS_X)]
    assert not np.array_equal(xs[0], xs[1])
    singles = []
    for x in xs:
        plan = _run(gen, x)
        singles.append({k: v.clone() for k, v in plan.act.items()})
    plan = _run(gen, np.concatenate(xs))
    ran = _routes_agree(gen, EDGE, True)
    assert sorted(ran) == [1, 2] and ran[2] == dict(plan_routes(EDGE, 2))
    print(f"260^3 fp32 routes at N = 2: {ran[2]}")
    assert [route_key(k) for k in ran[2].values()] == [route_key(k) for k in ran[1].values()]
    assert len(plan.act) == 12 and plan.y is plan.act["f2"]
    for i in range(2):
        for layer, one in singles[i].items():
            assert np.array_equal(plan.act[layer][i].cpu().numpy(), one[0].cpu().numpy()), (i, layer)


# ------------------------------------------------------------------------------------------- 3-D: tiled inference
@pytest.fixture(scope="module")
def pred260(ref260, model3):
    """predict_cube of the 3-tile request with the default batch, and the routes of its two plans."""
    from transfer_em_amd.utils import predict_cube
    gen = model3.generator_g
    gen.clear_plans()
    got = predict_cube(ref260.vol, START, SIZE, model3, MS_X, MS_Y)
    return got, gen.plan_kernels()


def test_predict_is_independent_of_the_batch_and_routed_as_planned(ref260, model3, pred260):
    from transfer_em_amd.utils import default_tile_batch, plan_routes, predict_cube, predict_volume
    got, ran = pred260
    assert got.shape == (150, 200, 500) and got.dtype == np.uint8 and got.std() > 20
    assert sorted(ran) == [1, 2] and default_tile_batch(EDGE, True) == 2
    for n, kernels in ran.items():
        assert kernels == dict(plan_routes(EDGE, n)), (n, kernels)
    for tb in (1, 5):
        assert np.array_equal(predict_cube(ref260.vol, START, SIZE, model3, MS_X, MS_Y, tile_batch=tb), got), tb
    stats = {}
    vol = predict_volume(ref260.vol, START, SIZE, model3, MS_X, MS_Y, stats=stats)
    assert stats["tile_batch"] == 2 and stats["chunks"] == 1 and np.array_equal(vol, got)


def _off_by_one(got, ref):
    """The bars of test_predict_cube_matches_tilewise_oracle: no voxel further than 1 in uint8 wrap distance, fewer
    than 1 % off by one (fp32 against double accumulation at .5 ties: a cap, not a measurement)."""
    d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    d = np.minimum(d, 256 - d)
    share = float((d != 0).mean())
    print(f"off by one: {share:.4%} of {d.size} voxels, further off: {int((d > 1).sum())}")
    assert (d > 1).sum() == 0 and share < 0.01, share


def test_tile_0_matches_the_oracle(oracle_lib, ref260, model3, pred260):
    """Tile 0's block of the request, and all 222^3 voxels of the tile as a request of its own."""
    from transfer_em_amd.utils import predict_cube, tile_plan
    t = ref260.tpad
    ref = oracle_lib.to_u8(ref260.y[:, t:-t, t:-t, t:-t, :], MS_Y)[0, ..., 0]
    assert ref.shape == (222, 222, 222)
    got = pred260[0]
    block = got[:, :, :222]
    _off_by_one(block, ref[:150, :200])
    assert got.std() > 20 and block.std() > 20
    assert tile_plan(START, (222, 222, 222), model3.outdimsize, model3.buffer)[3] == ref260.rois[:1]
    whole = predict_cube(ref260.vol, START, (222, 222, 222), model3, MS_X, MS_Y)
    assert np.array_equal(whole[:150, :200], block)
    _off_by_one(whole, ref)


@pytest.mark.parametrize("boundary", ["zeros", "reflect"])
def test_streaming_equals_the_resident_prediction(ref260, model3, pred260, boundary):
    """chunk_tiles is (kz, ky, kx): (1, 1, 1) and (2, 1, 1) stream the three tiles one by one, (1, 1, 2) as 2 + 1."""
    from transfer_em_amd.utils import chunk_plan, predict_cube, predict_volume
    start = START if boundary == "zeros" else START_R
    if boundary == "zeros":
        ref = pred260[0]
    else:
        lo, hi = start, tuple(s + n for s, n in zip(start, SIZE))
        assert lo[0] < 0 and hi[1] > VOL[1]                                  # the request itself passes two faces
        ref = predict_cube(ref260.vol, start, SIZE, model3, MS_X, MS_Y, boundary=boundary)
        assert ref.std() > 20 and not np.array_equal(
            ref, predict_cube(ref260.vol, start, SIZE, model3, MS_X, MS_Y))
    for ct, nchunk in (((1, 1, 1), 3), ((2, 1, 1), 3), ((1, 1, 2), 2)):
        assert len(chunk_plan(start, SIZE, model3.outdimsize, model3.buffer, VOL, ct, boundary=boundary)) == nchunk
        got = predict_volume(ref260.vol, start, SIZE, model3, MS_X, MS_Y, chunk_tiles=ct, boundary=boundary)
        assert np.array_equal(got, ref), (boundary, ct)


def test_mip_pyramid_of_222_tiles(ref260, model3, pred260):
    """tem_u8_pool2 at od = 222: over the resident (222, 222, 666) buffer and over each streamed 222^3 chunk."""
    from transfer_em_amd.utils import max_mips, predict_cube, predict_volume
    plain = pred260[0]
    assert max_mips(222) == 1
    want = ref_pool(plain, fz=2)                                             # mean of existing children, half up
    assert want.shape == (75, 100, 250)
    for levels in (predict_cube(ref260.vol, START, SIZE, model3, MS_X, MS_Y, mips=1),
                   predict_volume(ref260.vol, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 1), mips=1)):
        assert isinstance(levels, list) and len(levels) == 2
        assert np.array_equal(levels[0], plain)
        assert levels[1].shape == want.shape and np.array_equal(levels[1], want), np.argwhere(levels[1] != want)[:5]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for fn in (predict_cube, predict_volume):
        with pytest.raises(ValueError, match=r"\b1\b"):
            fn(ref260.vol, START, SIZE, model3, MS_X, MS_Y, mips=2)
    assert torch.cuda.memory_allocated() == before                           # raised before any GPU work


def test_one_transposed_member_equals_the_prediction_of_the_transposed_volume(ref260, model3, pred260):
    """The y <-> x transposition moves x, so gather and accumulate go through the 64 x 64 LDS planes: edge 260 leaves
    a ragged last block of 4, the 224-voxel output one of 32.  Tiles map to tiles (no flip), so the generator sees
    the same inputs in both runs."""
    from transfer_em_amd.utils import predict_cube
    s = ((0, 2, 1), (0, 0, 0))
    got = predict_cube(ref260.vol, START, SIZE, model3, MS_X, MS_Y, ensemble=[s])
    tv = np.ascontiguousarray(ref260.vol.swapaxes(1, 2))
    swap = lambda v: (v[1], v[0], v[2])
    want = predict_cube(tv, swap(START), swap(SIZE), model3, MS_X, MS_Y).swapaxes(1, 2)
    assert got.shape == want.shape == (150, 200, 500) and np.array_equal(got, want)
    assert not np.array_equal(got, pred260[0]) and got.std() > 20            # the orientation matters to the network


# ------------------------------------------------------------------------------------------------------------ 2-D
Ref2 = namedtuple("Ref2", "P x y sv y_bf sv_bf bars_bf")


@pytest.fixture(scope="module")
def model2(tmp_path_factory):
    from transfer_em_amd.cgan import EM2EM
    for gen in _LIVE:                                                        # the 3-D plans: a few GB of activations
        gen.clear_plans()
    torch.cuda.empty_cache()
    model = EM2EM(EDGE, "m260_2d", is3d=False, checkpoint_root=str(tmp_path_factory.mktemp("m260_2d")))
    model.generator_g.params.load_dict(_params(False))
    return model


@pytest.fixture(scope="module")
def ref2d(oracle_lib):
    """Three 260 x 260 sections through the oracle's 2-D graph, fp32 and bf16 mode (under a second on the host)."""
    from oracle import graph
    _host_threads()
    P = _params(False)
    u = np.random.default_rng(261).integers(0, 256, (3, 1, EDGE, EDGE), dtype=np.uint8)
    x = oracle_lib.standardize(oracle_lib.scale_u8(u), MS_X)
    y, sv = graph.generator_forward(P, x, False, training=False)
    with graph.precision("bf16"):
        y_bf, sv_bf = graph.generator_forward(P, graph.round_bf16(x), False, training=False)
    bars, own = _bf16_bars(sv_bf, y_bf, sv, y)
    print("oracle 260^2 x 3, bf16 vs fp32 (L2): " + ", ".join(f"{k} {v:.2e}" for k, v in own.items()))
    return Ref2(P, x, y, _keep(sv), y_bf, _keep(sv_bf), bars)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_every_layer_of_the_2d_260_plan_matches_the_oracle(ref2d, model2, dtype):
    """N = 3 against the oracle, and against three runs of N = 1 bit for bit.  Reference-only bf16 figures (oracle
    bf16 mode against its own fp32 mode, L2; the bar is 4 x each): c0 2.82e-3, d1a 3.40e-3, d1b 4.33e-3, d2a 5.16e-3,
    d2b 6.42e-3, u2a 6.83e-3, u2b 7.06e-3, mid 7.33e-3, u1a 8.10e-3, u1b 8.24e-3, f1 7.42e-3 (output: 6.62e-3)."""
    gen, dt = model2.generator_g, DTYPES[dtype]
    gen.clear_plans()
    singles = []
    for i in range(3):
        plan = _run(gen, ref2d.x[i:i + 1], dt)
        singles.append({k: v.clone() for k, v in plan.act.items()})
    plan = _run(gen, ref2d.x, dt)
    ran = _routes_agree(gen, EDGE, False, dt)
    assert sorted(ran) == [1, 3]
    print(f"260^2 {dtype} routes at N = 1: {ran[1]}\n260^2 {dtype} routes at N = 3: {ran[3]}")
    stats = forward_stats(plan, ref2d.sv if dtype == "fp32" else ref2d.sv_bf,
                          ref2d.y if dtype == "fp32" else ref2d.y_bf, False)
    _check(f"260^2 {dtype} N=3", stats, dt, ref2d.bars_bf)
    for i in range(3):
        for layer, one in singles[i].items():
            assert np.array_equal(plan.act[layer][i].float().cpu().numpy(), one[0].float().cpu().numpy()), (i, layer)


def test_predict_cube_2d_260_matches_tilewise_oracle(oracle_lib, ref2d, model2):
    """18 tiles of 222 x 222 over a stack of three sections, every tile against the oracle (the bars of
    test_predict_cube_2d_matches_tilewise_oracle); the batched run equals the tile-by-tile one."""
    from test_gpu_predict2d import _reference_predict_2d
    from transfer_em_amd.utils import predict_cube, tile_plan_2d
    _host_threads()
    vol = np.random.default_rng(262).integers(0, 256, VOL2, dtype=np.uint8)
    od, buf, tpad, rois, _ = tile_plan_2d(START2, SIZE2, model2.outdimsize, model2.buffer)
    assert (od, tpad, len(rois)) == (222, 1, 3 * 2 * 3) and SIZE2[0] % od and SIZE2[1] % od
    got = predict_cube(vol, START2, SIZE2, model2, MS_X, MS_Y)
    assert got.shape == (3, 400, 600) and got.dtype == np.uint8
    assert np.array_equal(predict_cube(vol, START2, SIZE2, model2, MS_X, MS_Y, tile_batch=1), got)
    ref = _reference_predict_2d(vol, START2, SIZE2, ref2d.P, MS_X, MS_Y, model2.outdimsize, model2.buffer)
    _off_by_one(got, ref)
    assert got.std() > 20
