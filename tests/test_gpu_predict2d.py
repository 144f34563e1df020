"""Tiled inference with the 2-D networks: predict_cube / predict_volume / the saved-model entry points over uint8
image stacks [z, y, x] (every section on its own, utils.tile_plan_2d) and single images [y, x], and the two 2-D tile
kernels (tem_u8_tiles2d_to_f32_std, tem_f32_tiles2d_unstd_to_u8) on their own against numpy."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from util import scaled_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS_X, MS_Y = (0.02, 0.58), (-0.1, 0.4)


def _params(seed=4):
    from oracle import graph
    P = scaled_params(graph.generator_param_shapes(False), seed)
    P["f2"] = P["f2"] * 20                                                   # spread outputs over the uint8 range
    return P


def _model(size, tmp_path, name, P=None):
    from transfer_em_amd.cgan import EM2EM
    model = EM2EM(size, name, is3d=False, checkpoint_root=str(tmp_path))
    model.generator_g.params.load_dict(_params() if P is None else P)
    return model


def _memmap(path, shape, seed):
    vol = np.lib.format.open_memmap(str(path), mode="w+", dtype=np.uint8, shape=shape)
    vol[...] = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    vol.flush()
    return np.load(str(path), mmap_mode="r")


def _wrap_diff(a, b):
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    return np.minimum(d, 256 - d)                                            # uint8 wrap distance


def _reference_predict_2d(volume, start, size, P, meanstd_x, meanstd_y, outdim, buffer):
    """Tile by tile on the oracle: tile_plan_2d's tiles, each cut from its section (zeros outside the volume),
    standardized, run through the 2-D generator graph and written back as uint8."""
    from oracle import graph, ops
    from transfer_em_amd.utils import tile_plan_2d
    outdim, buffer, tpad, rois, index = tile_plan_2d(start, size, outdim, buffer)
    edge = outdim + 2 * buffer
    rnd = lambda v: v + ((outdim - v % outdim) if v % outdim else 0)
    out = np.zeros((size[2], rnd(size[1]), rnd(size[0])), np.uint8)
    Z, Y, X = volume.shape
    for (rx, ry, rz), (ix, iy, iz) in zip(rois, index):
        tile = np.zeros((edge, edge), np.uint8)
        if 0 <= rz < Z:
            y0, x0, y1, x1 = max(ry, 0), max(rx, 0), min(ry + edge, Y), min(rx + edge, X)
            if y0 < y1 and x0 < x1:
                tile[y0 - ry:y1 - ry, x0 - rx:x1 - rx] = volume[rz, y0:y1, x0:x1]
        x = ops.standardize(ops.scale_u8(tile), meanstd_x)[None, None]     # (1, 1, edge, edge, 1)
        y, _ = graph.generator_forward(P, x, False, training=False)
        if tpad:
            y = y[:, :, tpad:-tpad, tpad:-tpad, :]
        out[iz, iy:iy + outdim, ix:ix + outdim] = ops.to_u8(y, meanstd_y)[0, 0, ..., 0]
    return out[:, :size[1], :size[0]]


def test_predict_cube_2d_matches_tilewise_oracle(oracle_lib, tmp_path):
    from transfer_em_amd.utils import predict_cube, tile_plan_2d
    rng = np.random.default_rng(0)
    volume = rng.integers(0, 256, (4, 64, 70), dtype=np.uint8)               # [z, y, x]
    P = _params()
    model = _model(74, tmp_path, "tile2d", P)
    start, size = (-5, 6, -1), (60, 50, 5)                                   # (x, y, z): section -1 lies outside
    od, buf, tpad, rois, _ = tile_plan_2d(start, size, model.outdimsize, model.buffer)
    assert tpad > 0 and len(rois) == 2 * 2 * 5                                # seams and tail tiles in y and x
    inp, got = predict_cube(volume, start, size, model, MS_X, MS_Y, fetch_input=True)
    ref = _reference_predict_2d(volume, start, size, P, MS_X, MS_Y, model.outdimsize, model.buffer)
    assert got.shape == (5, 50, 60) and got.dtype == np.uint8
    want = np.zeros((5, 50, 60), np.uint8)
    want[1:5, :, 5:60] = volume[0:4, 6:56, 0:55]
    assert np.array_equal(inp, want)
    diff = _wrap_diff(got, ref)
    assert (diff > 1).sum() == 0 and (diff != 0).mean() < 0.01              # fp32 vs double accumulation at .5 ties
    assert got[1:].std() > 20                                                 # not a degenerate image


def test_predict_cube_2d_batched_equals_per_tile(tmp_path):
    from transfer_em_amd.utils import default_tile_batch, predict_cube, tile_plan_2d
    model = _model(132, tmp_path, "batch2d")
    vol = np.random.default_rng(1).integers(0, 256, (5, 230, 250), dtype=np.uint8)
    start, size = (-7, 3, 0), (250, 220, 5)
    n = len(tile_plan_2d(start, size, model.outdimsize, model.buffer)[3])
    assert n == 45 and default_tile_batch(132, False) > n                    # the default: one batch of all tiles
    got = predict_cube(vol, start, size, model, MS_X, MS_Y)
    one = predict_cube(vol, start, size, model, MS_X, MS_Y, tile_batch=1)
    assert got.shape == (5, 220, 250) and got.std() > 20
    assert np.array_equal(got, one)


def test_predict_cube_2d_translation_property_260(tmp_path):
    """Away from the tile seams, 132-model tiles of a 260x260 section equal what the 260-edge 2-D generator computes
    on the same data in one piece (the VALID network is translation invariant; the stride-2 transposed convolutions'
    zero padding of each tile is what makes the tiling visible next to tile edges)."""
    from transfer_em_amd import hip_ops as H
    from transfer_em_amd.models.generator import unet_generator
    from transfer_em_amd.utils import predict_cube
    V = np.random.default_rng(3).integers(0, 256, (2, 296, 296), dtype=np.uint8)
    P = _params()
    model = _model(132, tmp_path, "c2d", P)
    start, size = (18, 18, 0), (260, 260, 2)
    got = predict_cube(V, start, size, model, MS_X, MS_Y)
    assert got.shape == (2, 260, 260) and got.std() > 20
    big, out_big = unet_generator(260, False)
    assert out_big == 224
    big.params.load_dict(P)
    x = torch.empty((2, 1, 260, 260, 1), dtype=torch.float32, device="cuda")
    H.u8_to_f32_std(torch.from_numpy(np.ascontiguousarray(V[:, :260, :260])).cuda(), x.view(-1), *MS_X)
    yb = big(x)                                                              # (2, 1, 224, 224, 1): pixels 18..241
    ub = torch.zeros((2, 224, 224), dtype=torch.uint8, device="cuda")
    H.f32_unstd_to_u8(yb.view(1, 2, 224, 224, 1), ub, *MS_Y)
    ub = ub.cpu().numpy()
    m = 12                                                                   # seam margin, as in 3-D
    checked = 0
    for y0 in (0, 96):
        for x0 in (0, 96):
            sl = (slice(None), slice(y0 + m, y0 + 96 - m), slice(x0 + m, x0 + 96 - m))
            d = _wrap_diff(got[sl], ub[sl])
            assert (d > 1).sum() == 0 and (d != 0).mean() < 0.02, (y0, x0)
            checked += d.size
    assert checked == 2 * 4 * 72 ** 2


# ---------------------------------------------------------------------------------------------------- the kernels
def _lib():
    from transfer_em_amd import hip_ops as H
    return H.require_gpu(), H.current_stream()


def _gather_ref(vol, org, edge, mean, std):
    Z, Y, X = vol.shape
    r = np.arange(edge)
    zz = org[:, 0][:, None, None] + 0 * r[None, :, None] + 0 * r[None, None, :]
    yy = org[:, 1][:, None, None] + r[None, :, None] + 0 * r[None, None, :]
    xx = org[:, 2][:, None, None] + 0 * r[None, :, None] + r[None, None, :]
    m = (zz >= 0) & (zz < Z) & (yy >= 0) & (yy < Y) & (xx >= 0) & (xx < X)
    v = np.where(m, vol[np.clip(zz, 0, Z - 1), np.clip(yy, 0, Y - 1), np.clip(xx, 0, X - 1)], 0).astype(np.float32)
    v = (v / np.float32(127.5)) - np.float32(1.0)
    return (v - np.float32(mean)) / np.float32(std)


def _gather(vol, org, edge, mean, std, offset=0):
    from transfer_em_amd import _lib as L
    lib, stream = _lib()
    Z, Y, X = vol.shape
    dv = torch.from_numpy(vol).cuda()
    do = torch.from_numpy(np.ascontiguousarray(org, np.int32)).cuda()
    n = len(org)
    buf = torch.full((n * edge * edge + offset,), float("nan"), dtype=torch.float32, device="cuda")
    L.check(lib.tem_u8_tiles2d_to_f32_std(dv.data_ptr(), Z, Y, X, do.data_ptr(), n, edge, buf.data_ptr() + 4 * offset,
                                          float(mean), float(std), stream), "tem_u8_tiles2d_to_f32_std")
    return buf[offset:].view(n, edge, edge).cpu().numpy()


@pytest.mark.parametrize("edge,ntile,offset", [(6, 300, 0), (5, 300, 0), (6, 300, 1), (4, 70001, 0)],
                         ids=["even-dwordx4", "odd", "unaligned-out", "70001-tiles"])
def test_gather_kernel_matches_numpy(edge, ntile, offset):
    rng = np.random.default_rng(edge * 7 + offset)
    vol = rng.integers(0, 256, (3, 20, 22), dtype=np.uint8)
    org = np.stack([rng.integers(-2, 5, ntile), rng.integers(-10, 23, ntile), rng.integers(-10, 25, ntile)], 1)
    org[:4] = [[-1, 0, 0], [3, 0, 0], [1, -30, 2], [1, 5, 40]]                  # wholly outside: zeros
    got = _gather(vol, org, edge, 0.02, 0.58, offset)
    ref = _gather_ref(vol, org, edge, 0.02, 0.58)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))         # bit for bit
    zero = np.float32((np.float32(-1.0) - np.float32(0.02)) / np.float32(0.58))
    assert (got[:4] == zero).all()


def _scatter_ref(y, tpad, idx, shape, mean, std):
    """Op by op in float32.  The kernels fuse y * std + mean into one FMA (elementwise.hip, unstd_u8): the callers
    choose y and std so that the product is exact, where both agree."""
    yedge = y.shape[1]
    od = yedge - 2 * tpad
    v = y[:, tpad:yedge - tpad, tpad:yedge - tpad].astype(np.float32)
    v = ((v * np.float32(std) + np.float32(mean)) + np.float32(1.0)) * np.float32(127.5)
    q = (np.rint(v).astype(np.int64) & 0xFF).astype(np.uint8)
    out = np.zeros(shape, np.uint8)
    r = np.arange(od)
    zz = idx[:, 0][:, None, None] + 0 * r[None, :, None] + 0 * r[None, None, :]
    yy = idx[:, 1][:, None, None] + r[None, :, None] + 0 * r[None, None, :]
    xx = idx[:, 2][:, None, None] + 0 * r[None, :, None] + r[None, None, :]
    m = (zz >= 0) & (zz < shape[0]) & (yy >= 0) & (yy < shape[1]) & (xx >= 0) & (xx < shape[2])
    out[zz[m], yy[m], xx[m]] = q[m]
    return out, v


def _scatter(y, tpad, idx, shape, mean, std):
    from transfer_em_amd import _lib as L
    lib, stream = _lib()
    dy = torch.from_numpy(np.ascontiguousarray(y, np.float32)).cuda()
    di = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).cuda()
    out = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    L.check(lib.tem_f32_tiles2d_unstd_to_u8(dy.data_ptr(), len(idx), y.shape[1], tpad, di.data_ptr(), out.data_ptr(),
                                            *shape, float(mean), float(std), stream), "tem_f32_tiles2d_unstd_to_u8")
    return out.cpu().numpy()


def _disjoint_tiles(rng, od, nz, ny, nx, z0, y0, x0):
    """(z, y, x) origins of an nz x ny x nx grid of od x od interiors starting at (z0, y0, x0), in random order."""
    g = np.stack(np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij"), -1).reshape(-1, 3)
    g = g * [1, od, od] + [z0, y0, x0]
    return g[rng.permutation(len(g))]


@pytest.mark.parametrize("yedge,tpad", [(10, 1), (10, 2), (12, 0), (4, 1)])
def test_scatter_kernel_matches_numpy(yedge, tpad):
    rng = np.random.default_rng(yedge * 3 + tpad)
    od = yedge - 2 * tpad
    if od == 2:                                     # > 65,535 tiles in one launch
        shape = (600, 16, 32)
        idx = _disjoint_tiles(rng, od, 600, 8, 16, 0, 0, 0)
        assert len(idx) > 65535
    else:                                           # OX = 30: rows start on and off 4-byte boundaries; tiles at
        shape = (3, 20, 30)                         # x = 2 + k*od, partly or wholly outside `out` (clipped)
        idx = _disjoint_tiles(rng, od, 5, 4, 5, -1, -4, 2)
    n = len(idx)
    # multiples of 2^-12 times std = 3/8: y * std is exact in float32 (see _scatter_ref)
    y = (np.round(rng.standard_normal((n, yedge, yedge)) * 0.8 * 4096) / 4096).astype(np.float32)
    for mean, std in ((-0.125, 0.375), (0.0, 1.0)):
        if std == 1.0:                              # even integers y: (y + 1) * 127.5 is an exact .5 tie; |y| > 1 wraps
            y.reshape(-1)[::3] = rng.integers(-2, 3, y.size)[::3] * 2
        got = _scatter(y, tpad, idx, shape, mean, std)
        ref, v = _scatter_ref(y, tpad, idx, shape, mean, std)
        assert np.array_equal(got, ref), (mean, std, np.argwhere(got != ref)[:5])
        if std == 1.0:
            assert (v - np.floor(v) == 0.5).any() and ((v < 0) | (v > 255)).any()
    assert got.any()


def test_2d_kernels_equal_3d_kernels():
    """A 3-D tile is a stack of 2-D tiles: on general data (no exact products, arbitrary statistics) the 2-D pair
    gives the 3-D pair's bytes and floats bit for bit -- the same per-voxel arithmetic."""
    from transfer_em_amd import _lib as L
    lib, stream = _lib()
    rng = np.random.default_rng(11)
    vol = rng.integers(0, 256, (30, 40, 50), dtype=np.uint8)
    edge, n = 12, 40
    org3 = np.stack([rng.integers(-8, 30, n), rng.integers(-8, 40, n), rng.integers(-8, 50, n)], 1)
    org2 = (org3[:, None, :] + np.stack([np.arange(edge), 0 * np.arange(edge), 0 * np.arange(edge)], 1)[None])
    dv, do = torch.from_numpy(vol).cuda(), torch.from_numpy(np.ascontiguousarray(org3, np.int32)).cuda()
    t3 = torch.empty((n, edge, edge, edge), dtype=torch.float32, device="cuda")
    L.check(lib.tem_u8_tiles_to_f32_std(dv.data_ptr(), 30, 40, 50, do.data_ptr(), n, edge, t3.data_ptr(), 0.0731,
                                        0.4127, stream), "tem_u8_tiles_to_f32_std")
    t2 = _gather(vol, org2.reshape(-1, 3), edge, 0.0731, 0.4127)
    assert np.array_equal(t3.cpu().numpy().reshape(-1, edge, edge).view(np.uint32), t2.view(np.uint32))
    # scatter: n disjoint yedge^3 tiles (tpad 0) of general floats into a (2*yedge, 2*yedge, 10*yedge) volume
    yedge = 8
    idx3 = _disjoint_tiles(rng, yedge, 2, 2, 10, 0, 0, 0) * [yedge, 1, 1]
    n = len(idx3)
    y = (rng.standard_normal((n, yedge, yedge, yedge)) * 1.7).astype(np.float32)
    shape = (2 * yedge, 2 * yedge, 10 * yedge)
    dy, di = torch.from_numpy(y).cuda(), torch.from_numpy(np.ascontiguousarray(idx3, np.int32)).cuda()
    o3 = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    L.check(lib.tem_f32_tiles_unstd_to_u8(dy.data_ptr(), n, yedge, 0, di.data_ptr(), o3.data_ptr(), *shape, -0.1037,
                                          0.3911, stream), "tem_f32_tiles_unstd_to_u8")
    idx2 = (idx3[:, None, :] + np.stack([np.arange(yedge), 0 * np.arange(yedge), 0 * np.arange(yedge)], 1)[None])
    o2 = _scatter(y.reshape(-1, yedge, yedge), 0, idx2.reshape(-1, 3), shape, -0.1037, 0.3911)
    assert np.array_equal(o3.cpu().numpy(), o2) and o2.std() > 20


# ----------------------------------------------------------------------------------------------- predict_volume
class Recorder:
    """Array-like over a numpy array that records every box read and refuses whole-array conversion."""

    def __init__(self, a):
        self.a, self.shape, self.dtype, self.boxes = a, a.shape, a.dtype, []

    def __getitem__(self, key):
        r = self.a[key]
        self.boxes.append(r.shape)
        return r

    def __array__(self, *args, **kw):
        raise AssertionError("whole-array conversion of the volume")


START, SIZE, SHAPE = (-20, -15, -1), (190, 165, 8), (6, 130, 150)          # sections -1 and 6 lie outside


@pytest.fixture(scope="module")
def case2d(tmp_path_factory):
    from transfer_em_amd.utils import predict_cube
    tmp = tmp_path_factory.mktemp("pv2d")
    model = _model(74, tmp, "pv2d")
    vol = _memmap(tmp / "vol.npy", SHAPE, 1)
    ref = predict_cube(np.array(vol), START, SIZE, model, MS_X, MS_Y)
    return model, vol, ref, tmp


def test_predict_volume_2d_bit_identical_to_predict_cube(case2d):
    from transfer_em_amd.utils import chunk_plan, predict_volume
    model, vol, ref, tmp = case2d
    assert ref.shape == (8, 165, 190) and ref[1:7].std() > 20
    chunks = chunk_plan(START, SIZE, model.outdimsize, model.buffer, SHAPE, (3, 2, 2), is3d=False)
    assert len(chunks) > 20 and len({len(c.tiles) for c in chunks}) > 2       # tails in z, y and x
    out = np.lib.format.open_memmap(str(tmp / "out.npy"), mode="w+", dtype=np.uint8, shape=ref.shape)
    assert predict_volume(vol, START, SIZE, model, MS_X, MS_Y, out=out, chunk_tiles=(3, 2, 2)) is out
    out.flush()
    del out
    assert np.array_equal(np.load(str(tmp / "out.npy")), ref)
    assert np.array_equal(predict_volume(vol, START, SIZE, model, MS_X, MS_Y), ref)                  # default chunks
    assert np.array_equal(predict_volume(vol, START, SIZE, model, MS_X, MS_Y, chunk_tiles=(2, 3, 1), tile_batch=4),
                          ref)


def test_predict_volume_2d_reads_only_footprints(case2d):
    from transfer_em_amd.utils import chunk_plan, predict_cube, predict_volume
    model, _, _, _ = case2d
    big = np.random.default_rng(5).integers(0, 256, (40, 300, 500), dtype=np.uint8)
    start, size = (430, 250, 17), (60, 70, 6)                                 # a corner past two in-plane faces
    rec = Recorder(big)
    got = predict_volume(rec, start, size, model, MS_X, MS_Y, chunk_tiles=(4, 1, 2))
    chunks = chunk_plan(start, size, model.outdimsize, model.buffer, big.shape, (4, 1, 2), is3d=False)
    assert sorted(rec.boxes) == sorted(c.block for c in chunks if min(c.block) > 0)
    for c in chunks:                                                          # no z halo: the chunk's sections only
        assert c.block[0] == len({c.read[0][0] + o[0] for o in c.origins})
    assert sum(int(np.prod(b)) for b in rec.boxes) < big.size // 50                # the footprints: ~0.9 %
    assert np.array_equal(got, predict_cube(big, start, size, model, MS_X, MS_Y))


def test_predict_volume_2d_two_ranks_share_out(case2d):
    from transfer_em_amd.utils import predict_volume
    model, vol, ref, tmp = case2d
    out = np.lib.format.open_memmap(str(tmp / "ranks.npy"), mode="w+", dtype=np.uint8, shape=ref.shape)
    for rank in (0, 1):
        predict_volume(vol, START, SIZE, model, MS_X, MS_Y, out=out, chunk_tiles=(3, 2, 2), rank=rank, world_size=2)
    out.flush()
    assert np.array_equal(np.array(out), ref)
    half = predict_volume(vol, START, SIZE, model, MS_X, MS_Y, chunk_tiles=(3, 2, 2), rank=1, world_size=2)
    assert 0 < (half != 0).mean() < 0.9                                       # one rank alone writes part of it


# ---------------------------------------------------------------------------------------------------- export
def test_export_cli_round_trip_2d(tmp_path):
    """bin/save_model.py (fresh process) -> the saved-model entry points equal the live model; the single-image [y, x]
    form equals section 0 of the stack form."""
    from transfer_em_amd import utils
    model = _model(74, tmp_path, "exp2d")
    ckpt = model.make_checkpoint(1)
    ms_x, ms_y = (0.1, 1.2), (-0.2, 0.9)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "save_model.py"), "exported", ckpt,
                        repr(ms_x[0]), repr(ms_x[1]), repr(ms_y[0]), repr(ms_y[1]), "74", "0"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out_dir = str(tmp_path / "exported")
    vol = _memmap(tmp_path / "vol.npy", (3, 70, 80), 4)
    start, size = (-3, 5, 0), (85, 61, 3)
    live = utils.predict_cube(np.array(vol), start, size, model, ms_x, ms_y)
    assert live.shape == (3, 61, 85) and live.std() > 20
    assert np.array_equal(utils.predict_cube_from_saved_model(np.array(vol), start, size, None, out_dir), live)
    assert np.array_equal(utils.predict_volume_from_saved_model(vol, start, size, out_dir, chunk_tiles=(2, 1, 2)), live)
    assert np.array_equal(utils.predict_ng_cube(np.array(vol), start, size, model, ms_x, ms_y), live)
    img = np.array(vol[0])                                                    # one image [y, x]
    one = utils.predict_cube(img, start[:2], size[:2], model, ms_x, ms_y)
    assert one.shape == (61, 85) and np.array_equal(one, live[0])
    inp, one = utils.predict_cube_from_saved_model(img, start[:2], size[:2], None, out_dir, fetch_input=True)
    assert np.array_equal(one, live[0]) and np.array_equal(inp[:, 3:83], img[5:66]) and not inp[:, :3].any()
    assert np.array_equal(utils.predict_volume_from_saved_model(vol[0], start[:2], size[:2], out_dir), live[0])
    with pytest.raises(ValueError):
        utils.predict_cube(img, start[:2], size, model, ms_x, ms_y)          # 2-element start with 3-element size
