"""Out-of-core tiled inference (utils.predict_volume): chunks streamed from an array-like volume give predict_cube's
bytes exactly, read only their footprints, and keep device memory bounded by the chunk."""
import numpy as np
import pytest
import torch

from util import scaled_params

pytestmark = pytest.mark.gpu

MS_X, MS_Y = (0.02, 0.58), (-0.1, 0.4)


def _model(size, tmp_path, name):
    from oracle import graph
    from transfer_em_amd.cgan import EM2EM
    model = EM2EM(size, name, checkpoint_root=str(tmp_path))
    P = scaled_params(graph.generator_param_shapes(True), 4)
    P["f2"] = P["f2"] * 20                                                   # spread outputs over the uint8 range
    model.generator_g.params.load_dict(P)
    return model


def _memmap(path, shape, seed):
    vol = np.lib.format.open_memmap(str(path), mode="w+", dtype=np.uint8, shape=shape)
    vol[...] = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    vol.flush()
    return np.load(str(path), mmap_mode="r")


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


START, SIZE, SHAPE = (-20, -15, -10), (190, 165, 135), (110, 130, 150)      # (x,y,z) ROI past all six faces; (z,y,x)


@pytest.fixture(scope="module")
def case74(tmp_path_factory):
    from transfer_em_amd.utils import predict_cube, predict_volume
    tmp = tmp_path_factory.mktemp("pv74")
    model = _model(74, tmp, "pv74")
    vol = _memmap(tmp / "vol.npy", SHAPE, 1)
    ref = predict_cube(np.array(vol), START, SIZE, model, MS_X, MS_Y)
    got = predict_volume(vol, START, SIZE, model, MS_X, MS_Y, chunk_tiles=(1, 2, 2))
    return model, vol, ref, got, tmp


def test_predict_volume_bit_identical_to_predict_cube(case74):
    from transfer_em_amd.utils import chunk_plan, predict_volume
    model, vol, ref, got, _ = case74
    assert got.shape == (135, 165, 190) and got.dtype == np.uint8
    assert ref.std() > 20
    chunks = chunk_plan(START, SIZE, model.outdimsize, model.buffer, SHAPE, (1, 2, 2))
    assert len(chunks) > 20 and len({len(c.tiles) for c in chunks}) > 1        # many seams and tail chunks
    assert np.array_equal(got, ref)
    one = predict_volume(vol, START, SIZE, model, MS_X, MS_Y, chunk_tiles=(1, 2, 2), tile_batch=1)
    assert np.array_equal(one, ref)
    dflt = predict_volume(vol, START, SIZE, model, MS_X, MS_Y)               # default chunk box
    assert np.array_equal(dflt, ref)


def test_predict_volume_reads_only_footprints(case74, tmp_path):
    from transfer_em_amd.utils import chunk_plan, predict_volume
    model, _, _, _, _ = case74
    big = np.random.default_rng(5).integers(0, 256, (400, 300, 500), dtype=np.uint8)
    start, size = (430, 250, -5), (60, 70, 45)                                # a corner reaching past three faces
    rec = Recorder(big)
    got = predict_volume(rec, start, size, model, MS_X, MS_Y, chunk_tiles=(1, 2, 2))
    chunks = chunk_plan(start, size, model.outdimsize, model.buffer, big.shape, (1, 2, 2))
    read = sum(int(np.prod(b)) for b in rec.boxes)
    assert read == sum(int(np.prod(c.block)) for c in chunks)
    assert read < big.size // 50                                             # the footprints: ~1.3 %
    from transfer_em_amd.utils import predict_cube
    assert np.array_equal(got, predict_cube(big, start, size, model, MS_X, MS_Y))


def test_predict_volume_into_file(case74, tmp_path):
    from transfer_em_amd.utils import predict_volume
    model, vol, ref, got, _ = case74
    path = tmp_path / "out.npy"
    out = np.lib.format.open_memmap(str(path), mode="w+", dtype=np.uint8, shape=got.shape)
    assert predict_volume(vol, START, SIZE, model, MS_X, MS_Y, out=out, chunk_tiles=(1, 2, 2)) is out
    out.flush()
    del out
    assert np.array_equal(np.load(str(path)), ref)


def test_predict_volume_device_memory_bounded(case74):
    from transfer_em_amd.utils import predict_volume
    model, _, _, _, _ = case74
    od = model.outdimsize - model.outdimsize % 6                              # 36: tile interior of the 74 model
    vol = np.random.default_rng(2).integers(0, 256, (8 * od, 4 * od, 4 * od), dtype=np.uint8)
    small, large = (2 * od, 2 * od, 4 * od), (4 * od, 4 * od, 8 * od)           # (x,y,z): 16 and 128 tiles
    peaks = []
    for size in (small, small, large):                                        # the first run builds the plan
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        predict_volume(vol, (0, 0, 0), size, model, MS_X, MS_Y, chunk_tiles=(1, 2, 2))
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated())
    assert peaks[2] <= peaks[1] * 1.05, peaks


def test_predict_volume_from_saved_model(tmp_path):
    from transfer_em_amd import utils
    model = _model(74, tmp_path, "pvsave")
    import os
    ckpt = model.make_checkpoint(1)
    out_dir = str(tmp_path / "exported")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        utils.save_model(out_dir, ckpt, MS_X, MS_Y, size=74, is3d=True)
    finally:
        os.chdir(cwd)
    vol = _memmap(tmp_path / "vol.npy", (60, 70, 80), 4)
    start, size = (-3, 5, 2), (85, 61, 50)
    live = utils.predict_volume(vol, start, size, model, MS_X, MS_Y, chunk_tiles=(1, 2, 2))
    saved = utils.predict_volume_from_saved_model(vol, start, size, out_dir, chunk_tiles=(1, 2, 2))
    assert np.array_equal(live, saved)
    assert np.array_equal(live, utils.predict_cube(np.array(vol), start, size, model, MS_X, MS_Y))


def test_predict_volume_132(tmp_path):
    from transfer_em_amd.utils import predict_cube, predict_volume
    model = _model(132, tmp_path, "pv132")
    vol = _memmap(tmp_path / "vol.npy", (240, 300, 340), 7)
    start, size = (10, -20, -5), (300, 260, 200)
    got = predict_volume(vol, start, size, model, MS_X, MS_Y)
    ref = predict_cube(np.array(vol), start, size, model, MS_X, MS_Y)
    assert got.shape == (200, 260, 300) and ref.std() > 20
    assert np.array_equal(got, ref)
