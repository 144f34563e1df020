"""The mip pyramid of tiled inference on the device (mips=L): tem_u8_pool2 against the numpy reference pooling, and
predict_cube / predict_volume with `mips` end to end.  The pooling is integer arithmetic, so every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from test_mips_plan import ref_pool
from util import scaled_params

pytestmark = pytest.mark.gpu

FRAME, FRAME_BYTE, DST_FILL = 64, 0xA5, 0x5A


def _env():
    from transfer_em_amd import _lib as L
    from transfer_em_amd import hip_ops as H
    return L, H.require_gpu(), H.current_stream()


def _half(v, fz):
    return (-(-v[0] // fz), -(-v[1] // 2), -(-v[2] // 2))


def _source(dims, valid, seed):
    """Random bytes inside the valid box, 255 outside it: an unmasked read shows in the mean."""
    src = np.full(dims, 255, np.uint8)
    src[:valid[0], :valid[1], :valid[2]] = np.random.default_rng(seed).integers(0, 256, valid, dtype=np.uint8)
    return src


def _counts(src, valid, fz):
    """(sum, cnt) of the valid children of every pooled voxel."""
    dims = src.shape
    inside = np.zeros(dims, bool)
    inside[:valid[0], :valid[1], :valid[2]] = True
    pad = [(0, -n % k) for n, k in zip(dims, (fz, 2, 2))]
    cells = lambda t: np.pad(t.astype(np.int64), pad).reshape(
        (dims[0] + pad[0][1]) // fz, fz, (dims[1] + pad[1][1]) // 2, 2, (dims[2] + pad[2][1]) // 2, 2).sum(axis=(1, 3, 5))
    return cells(np.where(inside, src, 0)), cells(inside)


def _check_inputs(src, valid, fz, want):
    """Conditions on the inputs, asserted on the expected values before the kernel runs."""
    sums, cnt = _counts(src, valid, fz)
    full = cnt == 8
    if full.any():                              # exact ties among the 8-child voxels: half-up rounding is exercised
        ties = np.count_nonzero(sums[full] % 8 == 4)
        assert ties >= 0.05 * np.count_nonzero(full), (ties, np.count_nonzero(full))
    if (cnt > 1).any():                         # a voxel with one child IS that child: only the others can differ
        pick = src[::fz, ::2, ::2]
        assert want.shape == pick.shape
        differ = np.count_nonzero(want != pick)
        assert differ >= 0.10 * want.size, (differ, want.size)
    pooled = valid[1:] if fz == 1 else valid
    if all(v % 2 == 1 and v >= 3 for v in pooled):      # odd valid extents: every child count occurs
        assert set(np.unique(cnt)) >= ({1, 2, 4, 8} if fz == 2 else {1, 2, 4}), np.unique(cnt)


def _pool(src_dev_ptr, dims, valid, fz):
    """tem_u8_pool2 into a dst inside a 0xA5 frame, itself pre-filled; returns the dst bytes, frame checked."""
    L, lib, stream = _env()
    odims = _half(dims, fz)
    n = int(np.prod(odims))
    buf = torch.full((FRAME + n + FRAME,), FRAME_BYTE, dtype=torch.uint8, device="cuda")
    buf[FRAME:FRAME + n] = DST_FILL
    L.check(lib.tem_u8_pool2(src_dev_ptr, *dims, *valid, fz, buf.data_ptr() + FRAME, stream), "tem_u8_pool2")
    got = buf.cpu().numpy()
    assert (got[:FRAME] == FRAME_BYTE).all() and (got[FRAME + n:] == FRAME_BYTE).all(), "the frame around dst was written"
    return got[FRAME:FRAME + n].reshape(odims)


CASES = [  # (D, H, W), valid
    ((1, 1, 1), (1, 1, 1)),
    ((5, 7, 10), (5, 7, 9)),
    ((4, 6, 16), (4, 6, 16)),                   # rows on 8 bytes: the aligned path
    ((3, 8, 24), (2, 5, 17)),
    ((2, 4, 222), (2, 3, 221)),                 # W % 4 == 2: odd rows are off dword alignment; the last group is cut
    ((6, 10, 72), (6, 10, 0)),                  # nothing valid: all zeros
    ((6, 10, 72), (0, 10, 72)),
    ((2, 2, 2050), (2, 2, 2050)),               # 257 groups per row: more than one workgroup per row
    ((36, 72, 72), (36, 41, 50)),               # a 74-model chunk of 1 x 2 x 2 tiles clipped by the ROI
]


@pytest.mark.parametrize("fz", [2, 1])
@pytest.mark.parametrize("dims, valid", CASES, ids=[f"{d}-{v}".replace(" ", "") for d, v in CASES])
def test_pool2_equals_the_reference(dims, valid, fz):
    src = _source(dims, valid, seed=sum(dims) + fz)
    want = ref_pool(src, valid, fz)
    assert want.shape == _half(dims, fz)
    if min(valid) == 0:
        assert not want.any()
    _check_inputs(src, valid, fz, want)
    dev = torch.from_numpy(src).cuda()
    got = _pool(dev.data_ptr(), dims, valid, fz)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


@pytest.mark.parametrize("fz", [2, 1])
def test_pool2_from_an_unaligned_source(fz):
    """The shape that took the 8-byte loads at offset 0, with the source 1, 2 and 3 bytes into its allocation (2-byte
    loads at 2, byte loads at 1 and 3): the same bytes."""
    dims = valid = (4, 6, 16)
    src = _source(dims, valid, seed=40 + fz)
    want = ref_pool(src, valid, fz)
    _check_inputs(src, valid, fz, want)
    n = src.size
    for off in (0, 1, 2, 3):
        dev = torch.full((n + 8,), 255, dtype=torch.uint8, device="cuda")
        dev[off:off + n] = torch.from_numpy(src.reshape(-1)).cuda()
        assert dev.data_ptr() % 8 == 0
        got = _pool(dev.data_ptr() + off, dims, valid, fz)
        assert np.array_equal(got, want), (off, np.argwhere(got != want)[:5])


@pytest.mark.parametrize("fz", [2, 1])
def test_three_level_cascade(fz):
    """Each level is the kernel on the previous level's output, with the halved valid extents, as the pipeline runs it."""
    L, lib, stream = _env()
    dims, valid = (8, 12, 20), (7, 11, 19)
    src = _source(dims, valid, seed=50 + fz)
    _check_inputs(src, valid, fz, ref_pool(src, valid, fz))
    want, w, v = [], src, valid
    for _ in range(3):
        w, v = ref_pool(w, v, fz), _half(v, fz)
        want.append(w)
    level = torch.from_numpy(src).cuda()
    for l in range(3):
        odims = _half(dims, fz)
        nxt = torch.full(odims, DST_FILL, dtype=torch.uint8, device="cuda")
        L.check(lib.tem_u8_pool2(level.data_ptr(), *dims, *valid, fz, nxt.data_ptr(), stream), "tem_u8_pool2")
        level, dims, valid = nxt, odims, _half(valid, fz)
        assert np.array_equal(level.cpu().numpy(), want[l]), l
    assert dims == ((1, 2, 3) if fz == 2 else (8, 2, 3))


def test_pool2_rejects_malformed_arguments():
    """Host-side checks of the entry point: TEM_EINVAL, and nothing is launched (dst keeps its fill)."""
    L, lib, stream = _env()
    src = torch.zeros(4 * 6 * 8, dtype=torch.uint8, device="cuda")
    dst = torch.full((2 * 3 * 4 * 2,), DST_FILL, dtype=torch.uint8, device="cuda")

    def call(ptr=None, dims=(4, 6, 8), valid=(4, 6, 8), fz=2, out=None):
        return lib.tem_u8_pool2(src.data_ptr() if ptr is None else ptr, *dims, *valid, fz,
                                dst.data_ptr() if out is None else out, stream)
    assert call(ptr=0) == L.TEM_EINVAL and call(out=0) == L.TEM_EINVAL
    for a in range(3):
        at = lambda v, base=(4, 6, 8): tuple(v if d == a else n for d, n in enumerate(base))
        assert call(dims=at(0), valid=at(0)) == L.TEM_EINVAL and call(dims=at(-1), valid=at(0)) == L.TEM_EINVAL
        assert call(valid=at(-1)) == L.TEM_EINVAL and call(valid=at((4, 6, 8)[a] + 1)) == L.TEM_EINVAL
    for fz in (0, 3, -1, 4):
        assert call(fz=fz) == L.TEM_EINVAL
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == DST_FILL).all()
    assert call() == L.TEM_OK and call(fz=1) == L.TEM_OK and call(valid=(0, 0, 0)) == L.TEM_OK
    torch.cuda.synchronize()
    assert not dst.cpu().numpy()[:2 * 3 * 4].any()                          # valid extent 0 is legal: zeros


# ------------------------------------------------------------------------------------------------------- end to end
# the 74 model: tiles of 36 + a halo of 19 (tpad 2); max_mips(36) = 2
MS_X, MS_Y = (0.02, 0.58), (-0.1, 0.4)
VOL, START, SIZE = (60, 70, 90), (-5, 3, -4), (77, 50, 41)          # (z,y,x); (x,y,z): 3 x 2 x 2 tiles, odd extents
VOL2, START2, SIZE2 = (3, 90, 75), (-3, 4, 0), (75, 61, 3)           # 2-D: 3 x 2 tiles in each of 3 sections


def _model(tmp_path, name, is3d):
    from oracle import graph
    from transfer_em_amd.cgan import EM2EM
    model = EM2EM(74, name, is3d=is3d, checkpoint_root=str(tmp_path))
    Pm = scaled_params(graph.generator_param_shapes(is3d), 4)
    Pm["f2"] = Pm["f2"] * 20                                                 # spread outputs over the uint8 range
    model.generator_g.params.load_dict(Pm)
    return model


@pytest.fixture(scope="module")
def model3(tmp_path_factory):
    return _model(tmp_path_factory.mktemp("mips3"), "mips3", True)


@pytest.fixture(scope="module")
def model2(tmp_path_factory):
    return _model(tmp_path_factory.mktemp("mips2"), "mips2", False)


@pytest.fixture(scope="module")
def vol3():
    return np.random.default_rng(21).integers(0, 256, VOL, dtype=np.uint8)


@pytest.fixture(scope="module")
def vol2():
    return np.random.default_rng(22).integers(0, 256, VOL2, dtype=np.uint8)


def _guard(level0):
    """A flat prediction would make every comparison of means vacuous."""
    assert level0.std() > 20 and len(np.unique(level0)) >= 16, (level0.std(), len(np.unique(level0)))


def _is_pyramid(levels, level0, L, fz):
    assert isinstance(levels, list) and len(levels) == L + 1
    assert all(isinstance(v, np.ndarray) and v.dtype == np.uint8 for v in levels)
    assert np.array_equal(levels[0], level0)
    for l in range(L):
        want = ref_pool(levels[l], fz=fz)
        assert levels[l + 1].shape == want.shape
        assert np.array_equal(levels[l + 1], want), (l + 1, np.argwhere(levels[l + 1] != want)[:5])


def _same(a, b):
    assert len(a) == len(b)
    for l, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x, y), (l, np.argwhere(x != y)[:5])


@pytest.fixture(scope="module")
def cube3(model3, vol3):
    """predict_cube's result and its pyramid, per (boundary, ensemble): computed once."""
    from transfer_em_amd.utils import predict_cube
    memo = {}

    def get(boundary="zeros", ensemble=None):
        if (boundary, ensemble) not in memo:
            memo[boundary, ensemble] = predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y, boundary=boundary,
                                                    ensemble=ensemble, mips=2)
        return memo[boundary, ensemble]
    return get


@pytest.fixture(scope="module")
def cube2(model2, vol2):
    from transfer_em_amd.utils import predict_cube
    memo = {}

    def get(boundary="zeros", ensemble=None):
        if (boundary, ensemble) not in memo:
            memo[boundary, ensemble] = predict_cube(vol2, START2, SIZE2, model2, MS_X, MS_Y, boundary=boundary,
                                                    ensemble=ensemble, mips=2)
        return memo[boundary, ensemble]
    return get


def test_no_mips_is_the_plain_result(model3, vol3, model2, vol2):
    from transfer_em_amd.utils import predict_cube, predict_volume
    for model, vol, start, size in ((model3, vol3, START, SIZE), (model2, vol2, START2, SIZE2)):
        plain = predict_cube(vol, start, size, model, MS_X, MS_Y)
        _guard(plain)
        for mips in (None, 0):
            st = {}
            got = predict_cube(vol, start, size, model, MS_X, MS_Y, mips=mips)
            assert isinstance(got, np.ndarray) and np.array_equal(got, plain)
            got = predict_volume(vol, start, size, model, MS_X, MS_Y, chunk_tiles=(1, 1, 2), mips=mips, stats=st)
            assert isinstance(got, np.ndarray) and np.array_equal(got, plain) and st["mips"] == 0
        out = np.zeros(plain.shape, np.uint8)
        assert predict_volume(vol, start, size, model, MS_X, MS_Y, out=out, mips=0) is out and np.array_equal(out, plain)


def test_cube_pyramid_3d(model3, vol3, cube3):
    from transfer_em_amd.utils import mip_shapes, predict_cube
    plain = predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y)
    _guard(plain)
    levels = cube3()
    assert [v.shape for v in levels] == mip_shapes(SIZE, 2) == [(41, 50, 77), (21, 25, 39), (11, 13, 20)]
    _is_pyramid(levels, plain, 2, fz=2)
    inp, res = predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y, fetch_input=True, mips=1)
    assert np.array_equal(inp, predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y, fetch_input=True)[0])
    _same(res, levels[:2])


def test_cube_pyramid_2d_and_one_image(model2, vol2, cube2):
    from transfer_em_amd.utils import mip_shapes, predict_cube, predict_volume
    plain = predict_cube(vol2, START2, SIZE2, model2, MS_X, MS_Y)
    _guard(plain)
    levels = cube2()
    assert [v.shape for v in levels] == mip_shapes(SIZE2, 2, False) == [(3, 61, 75), (3, 31, 38), (3, 16, 19)]
    _is_pyramid(levels, plain, 2, fz=1)                                      # sections are not pooled
    img = predict_cube(vol2[1], START2[:2], SIZE2[:2], model2, MS_X, MS_Y, mips=2)
    assert [v.shape for v in img] == mip_shapes(SIZE2[:2], 2, False)
    _same(img, [v[1] for v in levels])
    st = {}
    streamed = predict_volume(vol2[1], START2[:2], SIZE2[:2], model2, MS_X, MS_Y, chunk_tiles=(1, 1, 2), mips=2, stats=st)
    _same(streamed, img)
    assert st["mips"] == 2
    outs = [np.zeros(s, np.uint8) for s in mip_shapes(SIZE2[:2], 2, False)]
    back = predict_volume(vol2[1], START2[:2], SIZE2[:2], model2, MS_X, MS_Y, out=outs, mips=2)
    assert all(a is b for a, b in zip(back, outs))
    _same(outs, img)


@pytest.mark.parametrize("boundary", ["zeros", "reflect"])
@pytest.mark.parametrize("chunk_tiles", [(1, 1, 2), (2, 1, 1)])
def test_volume_equals_cube_3d(model3, vol3, cube3, chunk_tiles, boundary):
    from transfer_em_amd.utils import chunk_plan, predict_volume
    ref = cube3(boundary)
    _guard(ref[0])
    chunks = chunk_plan(START, SIZE, model3.outdimsize, model3.buffer, VOL, chunk_tiles, boundary=boundary)
    assert len(chunks) == {(1, 1, 2): 8, (2, 1, 1): 6}[chunk_tiles] and any(hi - lo < d for c in chunks for (lo, hi), d in zip(c.out_box, c.dims))
    st = {}
    got = predict_volume(vol3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=chunk_tiles, boundary=boundary, mips=2,
                         stats=st)
    assert st["mips"] == 2 and st["chunks"] == len(chunks)
    _same(got, ref)
    if boundary == "reflect":
        assert not np.array_equal(ref[0], cube3()[0])


@pytest.mark.parametrize("boundary", ["zeros", "reflect"])
@pytest.mark.parametrize("chunk_tiles", [(1, 1, 2), (2, 1, 1)])
def test_volume_equals_cube_2d(model2, vol2, cube2, chunk_tiles, boundary):
    from transfer_em_amd.utils import predict_volume
    ref = cube2(boundary)
    _guard(ref[0])
    got = predict_volume(vol2, START2, SIZE2, model2, MS_X, MS_Y, chunk_tiles=chunk_tiles, boundary=boundary, mips=2)
    _same(got, ref)


def test_under_an_ensemble(model3, vol3, cube3, model2, vol2, cube2):
    from transfer_em_amd.utils import predict_volume
    for model, vol, start, size, cube, fz in ((model3, vol3, START, SIZE, cube3, 2), (model2, vol2, START2, SIZE2, cube2, 1)):
        ref = cube("zeros", "flips")
        _guard(ref[0])
        assert not np.array_equal(ref[0], cube()[0])
        _is_pyramid(ref, ref[0], 2, fz)
        got = predict_volume(vol, start, size, model, MS_X, MS_Y, chunk_tiles=(1, 1, 2), ensemble="flips", mips=2)
        _same(got, ref)


def test_two_ranks_fill_one_list(model3, vol3, cube3):
    from transfer_em_amd.utils import mip_shapes, predict_volume
    ref = cube3()
    outs = [np.zeros(s, np.uint8) for s in mip_shapes(SIZE, 2)]
    for rank in range(2):
        st = {}
        back = predict_volume(vol3, START, SIZE, model3, MS_X, MS_Y, out=outs, chunk_tiles=(1, 1, 2), rank=rank,
                              world_size=2, stats=st, mips=2)
        assert st["chunks"] == 4 and all(a is b for a, b in zip(back, outs))
        if rank == 0:
            assert not any(np.array_equal(a, b) for a, b in zip(outs, ref))   # the other rank's boxes are still empty
    _same(outs, ref)


def test_memmaps_and_the_saved_model(model3, vol3, cube3, tmp_path):
    from transfer_em_amd import utils
    ref = cube3()
    outs = [np.lib.format.open_memmap(str(tmp_path / f"level{l}.npy"), mode="w+", dtype=np.uint8, shape=s)
            for l, s in enumerate(utils.mip_shapes(SIZE, 2))]
    back = utils.predict_volume(vol3, START, SIZE, model3, MS_X, MS_Y, out=outs, chunk_tiles=(2, 1, 1), mips=2)
    assert all(a is b for a, b in zip(back, outs))
    for o in outs:
        o.flush()
    _same([np.load(str(tmp_path / f"level{l}.npy")) for l in range(3)], ref)
    ckpt = model3.make_checkpoint(1)
    out_dir = str(tmp_path / "exported")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        utils.save_model(out_dir, ckpt, MS_X, MS_Y, size=74, is3d=True)
    finally:
        os.chdir(cwd)
    saved = utils.predict_volume_from_saved_model(vol3, START, SIZE, out_dir, chunk_tiles=(1, 2, 2), mips=1)
    _same(saved, ref[:2])


def test_too_many_levels_raise_before_any_allocation(model3, vol3, model2, vol2):
    from transfer_em_amd import utils
    assert utils.max_mips(utils.tile_plan(START, SIZE, model3.outdimsize, model3.buffer)[0]) == 2
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for fn in (utils.predict_cube, utils.predict_volume):
        for model, vol, start, size in ((model3, vol3, START, SIZE), (model2, vol2, START2, SIZE2)):
            with pytest.raises(ValueError, match=r"\b2\b"):
                fn(vol, start, size, model, MS_X, MS_Y, mips=3)
    assert torch.cuda.memory_allocated() == before
