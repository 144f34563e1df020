"""Reflect / edge boundaries of tiled inference (boundary="reflect" | "edge").  The oracle is the zero-mode code on a
host-padded volume: predict_cube(np.pad(vol, P, mode), start + P, size) with P beyond the furthest tile reach, so that
the padded run never reads a zero.  Same tiles, same batches, same kernels behind the gather and identical float
inputs: every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from util import scaled_params

pytestmark = pytest.mark.gpu

MS_X, MS_Y = (0.02, 0.58), (-0.1, 0.4)
MODES = ("reflect", "edge")
# the 74 model: tiles of 36 + a halo of 19.  The ROI's last tile starts at 62 on every axis and ends at 62 + 36 + 19 =
# 117 (z: 67 past the face at 50); its first starts at -20 - 19.  P covers both.
P = 72
VOL, START, SIZE = (50, 61, 45), (-20, -15, -10), (90, 100, 80)            # (z,y,x); (x,y,z): 27 tiles, past all six faces
VOL2, START2, SIZE2 = (3, 50, 45), (-20, -15, -1), (90, 100, 5)             # 2-D: sections -1 and 3 lie outside


def _shift(start):
    return tuple(s + P for s in start)


def _model3(tmp_path, name):
    from oracle import graph
    from transfer_em_amd.cgan import EM2EM
    model = EM2EM(74, name, checkpoint_root=str(tmp_path))
    Pm = scaled_params(graph.generator_param_shapes(True), 4)
    Pm["f2"] = Pm["f2"] * 20                                                 # spread outputs over the uint8 range
    model.generator_g.params.load_dict(Pm)
    return model


def _model2(tmp_path, name):
    from oracle import graph
    from transfer_em_amd.cgan import EM2EM
    model = EM2EM(74, name, is3d=False, checkpoint_root=str(tmp_path))
    Pm = scaled_params(graph.generator_param_shapes(False), 4)
    Pm["f2"] = Pm["f2"] * 20
    model.generator_g.params.load_dict(Pm)
    return model


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


# ---------------------------------------------------------------------------------------------------- the kernels
def _env():
    from transfer_em_amd import _lib as L
    from transfer_em_amd import hip_ops as H
    return L, H.require_gpu(), H.current_stream()


def _mode_id(mode):
    from transfer_em_amd import _lib as L
    return {"reflect": L.TEM_BOUNDARY_REFLECT, "edge": L.TEM_BOUNDARY_EDGE}[mode]


def _gather_zeros(vol, org, edge, is3d):
    """The existing zero-mode gather: tiles of `vol` at `org` as float bits."""
    L, lib, stream = _env()
    name = "tem_u8_tiles_to_f32_std" if is3d else "tem_u8_tiles2d_to_f32_std"
    dv = torch.from_numpy(np.ascontiguousarray(vol)).cuda()
    do = torch.from_numpy(np.ascontiguousarray(org, np.int32)).cuda()
    n, per = len(org), edge ** (3 if is3d else 2)
    out = torch.full((n * per,), float("nan"), dtype=torch.float32, device="cuda")
    L.check(getattr(lib, name)(dv.data_ptr(), *vol.shape, do.data_ptr(), n, edge, out.data_ptr(), MS_X[0], MS_X[1],
                               stream), name)
    return out.cpu().numpy().view(np.uint32).reshape(n, per)


def _gather_bc(blk, lo, vol_shape, mode, org_rel, edge, is3d):
    L, lib, stream = _env()
    name = "tem_u8_tiles_to_f32_std_bc" if is3d else "tem_u8_tiles2d_to_f32_std_bc"
    dv = torch.from_numpy(np.ascontiguousarray(blk)).cuda()
    do = torch.from_numpy(np.ascontiguousarray(org_rel, np.int32)).cuda()
    n, per = len(org_rel), edge ** (3 if is3d else 2)
    out = torch.full((n * per,), float("nan"), dtype=torch.float32, device="cuda")
    L.check(getattr(lib, name)(dv.data_ptr(), *blk.shape, *lo, *vol_shape, _mode_id(mode), do.data_ptr(), n, edge,
                               out.data_ptr(), MS_X[0], MS_X[1], stream), name)
    return out.cpu().numpy().view(np.uint32).reshape(n, per)


KP = 48                                                                       # origins reach -30 and +30 + edge 12


def _padded_ref(vol, org, edge, mode, is3d):
    return _gather_zeros(np.pad(vol, KP, mode=mode), np.asarray(org) + KP, edge, is3d)


@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("edge", [12, 7])
@pytest.mark.parametrize("shape", [(5, 9, 13), (1, 7, 6)])
def test_bc_gather_whole_volume_equals_zero_gather_on_padded(shape, edge, mode, is3d):
    rng = np.random.default_rng(sum(shape) + edge)
    vol = rng.integers(0, 256, shape, dtype=np.uint8)
    org = rng.integers(-30, 31, (40, 3))
    org[:3] = [[0, 0, 0], [-1, 0, 0], [shape[0] - 1, shape[1] - edge, shape[2] - edge]]
    if min(s - edge for s in shape) >= 0:
        org[3] = [s - edge for s in shape]                                   # a tile inside the volume: the plain path
    got = _gather_bc(vol, (0, 0, 0), shape, mode, org, edge, is3d)
    ref = _padded_ref(vol, org, edge, mode, is3d)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    assert len(np.unique(ref)) > 20


@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("edge", [12, 7])
@pytest.mark.parametrize("shape", [(5, 9, 13), (1, 7, 6), (23, 31, 40)])
def test_bc_gather_sub_block_at_its_hull(shape, edge, mode, is3d):
    """Tiles clustered at the far corner, part inside and part past the faces: the block is the hull of their folded
    coordinates (utils.fold), its origin is non-zero on the axes longer than the tiles' reach, and the tile origins
    are relative to it."""
    from transfer_em_amd.utils import fold
    rng = np.random.default_rng(sum(shape) * 3 + edge)
    vol = rng.integers(0, 256, shape, dtype=np.uint8)
    org = np.stack([rng.integers(n - edge - 3, n + 4, 24) for n in shape], 1)
    org[0] = [n - edge - 3 for n in shape]
    ext = (edge, edge, edge) if is3d else (1, edge, edge)
    read = []
    for d in range(3):
        f = fold(np.arange(org[:, d].min(), org[:, d].max() + ext[d]), shape[d], mode)
        read.append((int(f.min()), int(f.max()) + 1))
    lo = tuple(r[0] for r in read)
    if shape == (23, 31, 40):
        assert min(lo) > 0                                                    # a block strictly inside the volume
    blk = vol[tuple(slice(a, b) for a, b in read)]
    got = _gather_bc(blk, lo, shape, mode, org - np.array(lo), edge, is3d)
    ref = _padded_ref(vol, org, edge, mode, is3d)
    assert np.array_equal(got, ref), (read, np.argwhere(got != ref)[:5])


@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
@pytest.mark.parametrize("mode", MODES)
def test_bc_gather_reads_zero_outside_the_block(mode, is3d):
    """A block smaller than the hull (a planner would never make one): folded coordinates outside it read 0.  The block
    touches the volume's near z face and far x face and stops short of the other four, so a clamped or mirrored
    coordinate lands inside it on some axes and outside on others; half the origins are far out (multi-bounce), half
    straddle the faces.  How much of the expected result is the predicate's zero is a property of these inputs and is
    held on `want`, before the kernel runs."""
    from transfer_em_amd.utils import fold
    shape, edge, lo, bshape = (9, 14, 17), 8, (0, 2, 3), (6, 9, 14)
    rng = np.random.default_rng(8)
    vol = rng.integers(1, 256, shape, dtype=np.uint8)                        # no zero byte: a 0 read is the predicate
    blk = vol[tuple(slice(a, a + b) for a, b in zip(lo, bshape))]
    org = np.concatenate([rng.integers(-20, 24, (15, 3)), rng.integers(-6, 10, (15, 3))])
    org[0] = (1, 2, 3)                                                        # inside the volume, partly outside blk
    ext = (edge, edge, edge) if is3d else (1, edge, edge)
    want = np.zeros((len(org),) + ext, np.float32)
    kept = np.zeros((len(org),) + ext, bool)
    for t, o in enumerate(org):
        ix = [fold(o[d] + np.arange(ext[d]), shape[d], mode) for d in range(3)]
        kept[t][np.ix_(*[(i >= l) & (i < l + b) for i, l, b in zip(ix, lo, bshape)])] = True
        want[t] = np.where(kept[t], vol[np.ix_(*ix)], 0)
    per_tile = kept.reshape(len(org), -1).mean(1)
    assert 0.05 < kept.mean() < 0.95                                          # both outcomes are well represented
    assert ((per_tile > 0) & (per_tile < 1)).sum() >= 8                       # and vary within a tile, not only between
    want = ((want / np.float32(127.5) - np.float32(1.0)) - np.float32(MS_X[0])) / np.float32(MS_X[1])
    got = _gather_bc(blk, lo, shape, mode, org - np.array(lo), edge, is3d)
    assert np.array_equal(got, want.reshape(len(org), -1).view(np.uint32))
    zero = np.float32((np.float32(-1.0) - np.float32(MS_X[0])) / np.float32(MS_X[1])).view(np.uint32)
    assert np.array_equal(got == zero, ~kept.reshape(len(org), -1))


def test_bc_entry_points_refuse_bad_arguments():
    L, lib, stream = _env()
    vol = torch.zeros((4, 5, 6), dtype=torch.uint8, device="cuda")
    org = torch.zeros((1, 3), dtype=torch.int32, device="cuda")
    out = torch.zeros((6 ** 3,), dtype=torch.float32, device="cuda")
    for name in ("tem_u8_tiles_to_f32_std_bc", "tem_u8_tiles2d_to_f32_std_bc"):
        fn = getattr(lib, name)

        def call(block=(4, 5, 6), lo=(0, 0, 0), shape=(4, 5, 6), mode=L.TEM_BOUNDARY_REFLECT):
            return fn(vol.data_ptr(), *block, *lo, *shape, mode, org.data_ptr(), 1, 6, out.data_ptr(), 0.0, 1.0, stream)
        assert call() == L.TEM_OK
        for mode in (0, 3, -1):                                              # 0 would be "zeros": not these kernels'
            assert call(mode=mode) == L.TEM_EINVAL
        assert call(shape=(4, 0, 6)) == L.TEM_EINVAL
        assert call(block=(4, 0, 6)) == L.TEM_EINVAL
        assert call(block=(2, 5, 6), lo=(3, 0, 0)) == L.TEM_EINVAL           # the block leaves the volume
        assert call(block=(2, 5, 6), lo=(-1, 0, 0)) == L.TEM_EINVAL
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ predict_cube, 3-D
@pytest.fixture(scope="module")
def case3(tmp_path_factory):
    from transfer_em_amd.utils import predict_cube
    tmp = tmp_path_factory.mktemp("bc3")
    model = _model3(tmp, "bc3")
    vol = np.random.default_rng(1).integers(0, 256, VOL, dtype=np.uint8)
    zeros = predict_cube(vol, START, SIZE, model, MS_X, MS_Y)
    ref = {m: predict_cube(np.pad(vol, P, mode=m), _shift(START), SIZE, model, MS_X, MS_Y) for m in MODES}
    got = {m: predict_cube(vol, START, SIZE, model, MS_X, MS_Y, boundary=m) for m in MODES}
    return model, vol, zeros, ref, got, tmp


def test_padding_covers_every_tile(case3):
    """P is no smaller than the furthest reach of a tile past a face, so the padded oracle reads no zero."""
    from transfer_em_amd.utils import tile_plan, tile_plan_2d
    model = case3[0]
    for plan, start, size, vol in ((tile_plan, START, SIZE, VOL), (tile_plan_2d, START2, SIZE2, VOL2)):
        od, buf, _, rois, _ = plan(start, size, model.outdimsize, model.buffer)
        edge = od + 2 * buf
        for d, n in zip((2, 1, 0), vol):                                      # rois are (x, y, z)
            ext = 1 if (plan is tile_plan_2d and d == 2) else edge
            assert min(r[d] for r in rois) >= -P and max(r[d] for r in rois) + ext <= n + P


@pytest.mark.parametrize("mode", MODES)
def test_predict_cube_equals_padded_oracle(case3, mode):
    from transfer_em_amd.utils import predict_cube, tile_plan
    model, vol, zeros, ref, got, _ = case3
    assert len(tile_plan(START, SIZE, model.outdimsize, model.buffer)[3]) == 27
    assert got[mode].shape == (80, 100, 90) and got[mode].dtype == np.uint8
    assert ref[mode].std() > 20 and not np.array_equal(ref[mode], zeros)
    assert np.array_equal(got[mode], ref[mode])
    inp, out = predict_cube(vol, START, SIZE, model, MS_X, MS_Y, fetch_input=True, boundary=mode, tile_batch=4)
    assert np.array_equal(out, ref[mode])
    want = np.pad(vol, P, mode=mode)[tuple(slice(s + P, s + P + n) for s, n in zip(START[::-1], SIZE[::-1]))]
    assert inp.shape == (80, 100, 90) and np.array_equal(inp, want)


@pytest.mark.parametrize("mode", MODES)
def test_predict_cube_whole_volume_roi(case3, mode):
    from transfer_em_amd.utils import predict_cube
    model, vol = case3[0], case3[1]
    size = VOL[::-1]
    ref = predict_cube(np.pad(vol, P, mode=mode), (P, P, P), size, model, MS_X, MS_Y)
    got = predict_cube(vol, (0, 0, 0), size, model, MS_X, MS_Y, boundary=mode)
    assert ref.std() > 20 and not np.array_equal(ref, predict_cube(vol, (0, 0, 0), size, model, MS_X, MS_Y))
    assert np.array_equal(got, ref)


def test_predict_cube_default_is_zeros_and_bad_arguments_raise(case3):
    from transfer_em_amd.utils import predict_cube, predict_volume
    model, vol, zeros = case3[0], case3[1], case3[2]
    assert np.array_equal(predict_cube(vol, START, SIZE, model, MS_X, MS_Y, boundary="zeros"), zeros)
    for fn in (predict_cube, predict_volume):
        with pytest.raises(ValueError):
            fn(vol, START, SIZE, model, MS_X, MS_Y, boundary="wrap")
        with pytest.raises(ValueError):
            fn(vol[:, :0], START, SIZE, model, MS_X, MS_Y, boundary="reflect")


# ---------------------------------------------------------------------------------------------- predict_volume, 3-D
@pytest.mark.parametrize("mode", MODES)
def test_predict_volume_equals_predict_cube(case3, mode):
    from transfer_em_amd.utils import chunk_plan, predict_volume
    model, vol, _, ref, got, _ = case3
    chunks = chunk_plan(START, SIZE, model.outdimsize, model.buffer, VOL, (1, 2, 2), boundary=mode)
    assert len(chunks) == 12 and len({len(c.tiles) for c in chunks}) > 1
    rec = Recorder(vol)
    streamed = predict_volume(rec, START, SIZE, model, MS_X, MS_Y, chunk_tiles=(1, 2, 2), boundary=mode)
    assert np.array_equal(streamed, got[mode]) and np.array_equal(streamed, ref[mode])
    assert sum(int(np.prod(b)) for b in rec.boxes) == sum(int(np.prod(c.block)) for c in chunks)
    assert sorted(rec.boxes) == sorted(c.block for c in chunks)
    one = predict_volume(vol, START, SIZE, model, MS_X, MS_Y, chunk_tiles=(1, 2, 2), tile_batch=1, boundary=mode)
    assert np.array_equal(one, got[mode])
    dflt = predict_volume(vol, START, SIZE, model, MS_X, MS_Y, boundary=mode)             # default chunk box
    assert np.array_equal(dflt, got[mode])


def test_predict_volume_sub_block_chunks(case3):
    """A volume several tiles long: chunks at the far faces stage blocks with non-zero origins and mirror into them."""
    from transfer_em_amd.utils import chunk_plan, predict_cube, predict_volume
    model = case3[0]
    vol = np.random.default_rng(6).integers(0, 256, (120, 70, 130), dtype=np.uint8)
    start, size = (60, -5, 50), (72, 72, 72)                                 # (x,y,z): 8 tiles past the far x and z faces
    chunks = chunk_plan(start, size, model.outdimsize, model.buffer, vol.shape, (1, 1, 2), boundary="reflect")
    assert any(min(c.read[0][0], c.read[2][0]) > 0 and c.read[2][1] == 130 for c in chunks)
    ref = predict_cube(np.pad(vol, P, mode="reflect"), _shift(start), size, model, MS_X, MS_Y)
    rec = Recorder(vol)
    got = predict_volume(rec, start, size, model, MS_X, MS_Y, chunk_tiles=(1, 1, 2), boundary="reflect")
    assert np.array_equal(got, ref)
    assert sum(int(np.prod(b)) for b in rec.boxes) == sum(int(np.prod(c.block)) for c in chunks)


def test_predict_volume_from_saved_model_reflect(tmp_path):
    from transfer_em_amd import utils
    model = _model3(tmp_path, "bcsave")
    ckpt = model.make_checkpoint(1)
    out_dir = str(tmp_path / "exported")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        utils.save_model(out_dir, ckpt, MS_X, MS_Y, size=74, is3d=True)
    finally:
        os.chdir(cwd)
    vol = np.random.default_rng(4).integers(0, 256, (40, 50, 45), dtype=np.uint8)
    start, size = (-3, 5, -8), (60, 50, 50)
    live = utils.predict_volume(vol, start, size, model, MS_X, MS_Y, chunk_tiles=(1, 2, 2), boundary="reflect")
    saved = utils.predict_volume_from_saved_model(vol, start, size, out_dir, chunk_tiles=(1, 2, 2), boundary="reflect")
    assert live.std() > 20 and np.array_equal(live, saved)
    assert not np.array_equal(live, utils.predict_volume(vol, start, size, model, MS_X, MS_Y, chunk_tiles=(1, 2, 2)))


# ------------------------------------------------------------------------------------------------------ 2-D model
@pytest.fixture(scope="module")
def case2(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bc2")
    model = _model2(tmp, "bc2")
    vol = np.random.default_rng(2).integers(0, 256, VOL2, dtype=np.uint8)
    return model, vol


@pytest.mark.parametrize("mode", MODES)
def test_2d_model_equals_padded_oracle(case2, mode):
    from transfer_em_amd.utils import chunk_plan, predict_cube, predict_volume
    model, vol = case2
    ref = predict_cube(np.pad(vol, P, mode=mode), _shift(START2), SIZE2, model, MS_X, MS_Y)
    zeros = predict_cube(vol, START2, SIZE2, model, MS_X, MS_Y)
    assert ref.shape == (5, 100, 90) and ref.std() > 20 and not np.array_equal(ref, zeros)
    inp, got = predict_cube(vol, START2, SIZE2, model, MS_X, MS_Y, fetch_input=True, boundary=mode)
    assert np.array_equal(got, ref)
    want = np.pad(vol, P, mode=mode)[tuple(slice(s + P, s + P + n) for s, n in zip(START2[::-1], SIZE2[::-1]))]
    assert np.array_equal(inp, want)
    rec = Recorder(vol)
    streamed = predict_volume(rec, START2, SIZE2, model, MS_X, MS_Y, chunk_tiles=(2, 1, 2), boundary=mode)
    assert np.array_equal(streamed, ref)
    chunks = chunk_plan(START2, SIZE2, model.outdimsize, model.buffer, VOL2, (2, 1, 2), is3d=False, boundary=mode)
    assert sorted(rec.boxes) == sorted(c.block for c in chunks)
    assert np.array_equal(predict_volume(vol, START2, SIZE2, model, MS_X, MS_Y, boundary=mode), ref)
    assert np.array_equal(predict_cube(vol, START2, SIZE2, model, MS_X, MS_Y, boundary=mode, tile_batch=5), ref)


@pytest.mark.parametrize("mode", MODES)
def test_2d_single_image_equals_padded_oracle(case2, mode):
    from transfer_em_amd.utils import predict_cube, predict_volume
    model, vol = case2
    img, start, size = vol[1], START2[:2], SIZE2[:2]
    ref = predict_cube(np.pad(img, P, mode=mode), _shift(start), size, model, MS_X, MS_Y)
    assert ref.shape == (100, 90) and ref.std() > 20
    assert not np.array_equal(ref, predict_cube(img, start, size, model, MS_X, MS_Y))
    inp, got = predict_cube(img, start, size, model, MS_X, MS_Y, fetch_input=True, boundary=mode)
    assert np.array_equal(got, ref)
    assert np.array_equal(inp, np.pad(img, P, mode=mode)[P - 15:P + 85, P - 20:P + 70])
    assert np.array_equal(predict_volume(img, start, size, model, MS_X, MS_Y, boundary=mode), ref)
