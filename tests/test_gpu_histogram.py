"""Intensity histograms and lookup tables on the device: tem_u8_hist and tem_u8_lut against numpy (np.bincount, fancy
indexing), volume_histogram out of core, and predict_cube / predict_volume with `lut` and `histogram`.  Everything is
integers or bytes, so every comparison is exact."""
import numpy as np
import pytest
import torch

from util import scaled_params

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 64, 0xA5


def _env():
    from transfer_em_amd import _lib as L
    from transfer_em_amd import hip_ops as H
    return L, H.require_gpu(), H.current_stream()


def _upload(a, off=0):
    """The bytes of `a` on the device, `off` bytes into a 256-byte-aligned allocation; (tensor kept alive, pointer)."""
    flat = np.ascontiguousarray(a).reshape(-1)
    t = torch.zeros(flat.size + off + 16, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    t[off:off + flat.size] = torch.from_numpy(flat).cuda()
    return t, t.data_ptr() + off


def _hist(ptr, dims, box, per_section=False, counts=None):
    L, lib, stream = _env()
    (z0, z1), (y0, y1), (x0, x1) = box
    if counts is None:
        counts = torch.zeros(((z1 - z0) if per_section else 1, 256), dtype=torch.int64, device="cuda")
    L.check(lib.tem_u8_hist(ptr, *dims, z0, z1, y0, y1, x0, x1, counts.data_ptr(), int(per_section), stream), "tem_u8_hist")
    return counts


def _bincount(a):
    return np.bincount(a.ravel(), minlength=256).astype(np.int64)


def _boxes(dims):
    """The whole buffer, a one-voxel box, and boxes at an odd x0 of widths 1, 15, 16, 17 (where they fit)."""
    D, H, W = dims
    boxes = [((0, D), (0, H), (0, W)), ((D - 1, D), (H // 2, H // 2 + 1), (W - 1, W))]
    for w in (1, 15, 16, 17):
        for x0 in (1, 3):
            if x0 + w <= W:
                boxes.append(((0, D), (0, H), (x0, x0 + w)))
                boxes.append(((D // 2, D), (H // 3, H - H // 4), (x0, x0 + w)))
    return [b for b in boxes if all(hi > lo for lo, hi in b)]


HIST_DIMS = [(1, 1, 1), (3, 5, 17), (2, 7, 16), (5, 33, 131)]


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("dims", HIST_DIMS, ids=[str(d).replace(" ", "") for d in HIST_DIMS])
def test_hist_equals_bincount(dims, off):
    src = np.random.default_rng(sum(dims)).integers(0, 256, dims, dtype=np.uint8)
    keep, ptr = _upload(src, off)
    for box in _boxes(dims):
        (z0, z1), (y0, y1), (x0, x1) = box
        want = _bincount(src[z0:z1, y0:y1, x0:x1])
        got = _hist(ptr, dims, box).cpu().numpy()[0]
        assert np.array_equal(got, want), (box, np.flatnonzero(got != want)[:5])


def test_hist_calls_add_and_many_workgroups_flush_into_one():
    dims = (7, 64, 300)                                  # 448 rows of 20 segments: 35 workgroups
    src = np.random.default_rng(1).integers(0, 256, dims, dtype=np.uint8)
    keep, ptr = _upload(src)
    whole = ((0, 7), (0, 64), (0, 300))
    counts = _hist(ptr, dims, whole)
    assert np.array_equal(counts.cpu().numpy()[0], _bincount(src))
    _hist(ptr, dims, ((1, 5), (3, 60), (7, 208)), counts=counts)
    assert np.array_equal(counts.cpu().numpy()[0], _bincount(src) + _bincount(src[1:5, 3:60, 7:208]))


@pytest.mark.parametrize("value", [255, 0])
def test_hist_of_a_constant_volume(value):
    """Every lane adds to the same bin: the contention case of the workgroup-private counters."""
    src = np.full((64, 64, 64), value, np.uint8)
    keep, ptr = _upload(src)
    got = _hist(ptr, src.shape, ((0, 64),) * 3).cpu().numpy()[0]
    want = np.zeros(256, np.int64)
    want[value] = 262144
    assert np.array_equal(got, want)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
def test_hist_per_section_reads_nothing_outside_the_box(off):
    """Inside the box every byte is below 200; everything around it is 233, whose bin must stay empty."""
    dims, box = (9, 40, 150), ((2, 8), (5, 37), (3, 140))
    src = np.full(dims, 233, np.uint8)
    (z0, z1), (y0, y1), (x0, x1) = box
    src[z0:z1, y0:y1, x0:x1] = np.random.default_rng(2).integers(0, 200, (z1 - z0, y1 - y0, x1 - x0), dtype=np.uint8)
    keep, ptr = _upload(src, off)
    want = np.stack([_bincount(src[z, y0:y1, x0:x1]) for z in range(z0, z1)])
    assert want[:, 233].sum() == 0 and len({tuple(r) for r in want}) == z1 - z0          # distinct rows
    got = _hist(ptr, dims, box, per_section=True).cpu().numpy()
    assert got.shape == (z1 - z0, 256) and np.array_equal(got, want)
    assert np.array_equal(_hist(ptr, dims, box).cpu().numpy()[0], want.sum(axis=0))
    # many short sections: a workgroup's run of rows crosses sections and flushes at each
    dims2 = (40, 3, 21)
    src2 = np.random.default_rng(3).integers(0, 256, dims2, dtype=np.uint8)
    keep2, ptr2 = _upload(src2, off)
    got = _hist(ptr2, dims2, ((0, 40), (0, 3), (0, 21)), per_section=True).cpu().numpy()
    assert np.array_equal(got, np.stack([_bincount(s) for s in src2]))


def test_hist_rejects_malformed_arguments():
    """TEM_EINVAL from the host-side checks, nothing launched: counts keeps its fill."""
    L, lib, stream = _env()
    src = torch.zeros(4 * 6 * 8, dtype=torch.uint8, device="cuda")
    counts = torch.full((4, 256), 7, dtype=torch.int64, device="cuda")
    base = (4, 6, 8)

    def call(ptr=None, dims=base, box=(0, 4, 0, 6, 0, 8), out=None, per_section=0):
        return lib.tem_u8_hist(src.data_ptr() if ptr is None else ptr, *dims, *box,
                               counts.data_ptr() if out is None else out, per_section, stream)
    assert call(ptr=0) == L.TEM_EINVAL and call(out=0) == L.TEM_EINVAL
    for a in range(3):
        at = lambda v: tuple(v if d == a else n for d, n in enumerate(base))

        def box(lo, hi):
            b = [0, 4, 0, 6, 0, 8]
            b[2 * a], b[2 * a + 1] = lo, hi
            return tuple(b)
        assert call(dims=at(0), box=box(0, 0)) == L.TEM_EINVAL and call(dims=at(-1), box=box(0, 0)) == L.TEM_EINVAL
        assert call(box=box(-1, 2)) == L.TEM_EINVAL and call(box=box(0, base[a] + 1)) == L.TEM_EINVAL
        assert call(box=box(3, 2)) == L.TEM_EINVAL
    # too many voxels for a workgroup's 32-bit counters (the bound of include/tem_hip.h); refused on the host, so the
    # extents need no memory behind them
    M = 2 ** 31 - 1
    for per_section in (0, 1):
        assert call(dims=(1, M, M), box=(0, 1, 0, M, 0, M), per_section=per_section) == L.TEM_EINVAL
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == 7).all()
    for b in ((2, 2, 0, 6, 0, 8), (0, 4, 6, 6, 0, 8), (0, 4, 0, 6, 3, 3)):              # empty boxes: fine, nothing counted
        assert call(box=b) == L.TEM_OK and call(box=b, per_section=1) == L.TEM_OK
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == 7).all()
    assert call() == L.TEM_OK
    torch.cuda.synchronize()
    got = counts.cpu().numpy()
    assert got[0, 0] == 7 + 192 and (got.ravel()[1:] == 7).all()


# -------------------------------------------------------------------------------------------------------- tem_u8_lut
def _lut(buf_np, table, per_section=False, zsec0=0, off=0):
    """tem_u8_lut on a copy of buf_np placed `off` bytes into an aligned allocation between two guards."""
    L, lib, stream = _env()
    n = buf_np.size
    t = torch.full((GUARD + off + n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    t[GUARD + off:GUARD + off + n] = torch.from_numpy(buf_np.reshape(-1)).cuda()
    keep, lut_ptr = _upload(table, off)                                  # the table is as misaligned as the buffer
    L.check(lib.tem_u8_lut(t.data_ptr() + GUARD + off, *buf_np.shape, lut_ptr, int(per_section), zsec0, stream),
            "tem_u8_lut")
    got = t.cpu().numpy()
    assert (got[:GUARD + off] == GUARD_BYTE).all() and (got[GUARD + off + n:] == GUARD_BYTE).all(), "guards were written"
    return got[GUARD + off:GUARD + off + n].reshape(buf_np.shape)


LUT_DIMS = HIST_DIMS + [(3, 50, 1111)]                                   # the last: several workgroups per buffer


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("dims", LUT_DIMS, ids=[str(d).replace(" ", "") for d in LUT_DIMS])
def test_lut_equals_fancy_indexing(dims, off):
    rng = np.random.default_rng(sum(dims) + 1)
    buf = rng.integers(0, 256, dims, dtype=np.uint8)
    perm = rng.permutation(256).astype(np.uint8)
    assert not np.array_equal(perm, np.arange(256))
    assert np.array_equal(_lut(buf, perm, off=off), perm[buf])
    const = np.full(256, 99, np.uint8)
    assert np.array_equal(_lut(buf, const, off=off), const[buf])
    # one table per section, the buffer starting at section 2 of a taller volume
    tables = np.stack([rng.permutation(256).astype(np.uint8) for _ in range(dims[0] + 3)])
    want = np.stack([tables[2 + z][buf[z]] for z in range(dims[0])])
    assert np.array_equal(_lut(buf, tables, per_section=True, zsec0=2, off=off), want)
    if dims[0] > 1:
        assert not np.array_equal(want, np.stack([tables[z][buf[z]] for z in range(dims[0])]))


def test_lut_rejects_malformed_arguments():
    L, lib, stream = _env()
    buf = torch.full((4 * 6 * 8,), 5, dtype=torch.uint8, device="cuda")
    table = torch.zeros(4 * 256, dtype=torch.uint8, device="cuda")

    def call(ptr=None, dims=(4, 6, 8), lut=None, per_section=0, zsec0=0):
        return lib.tem_u8_lut(buf.data_ptr() if ptr is None else ptr, *dims, table.data_ptr() if lut is None else lut,
                              per_section, zsec0, stream)
    assert call(ptr=0) == L.TEM_EINVAL and call(lut=0) == L.TEM_EINVAL
    for a in range(3):
        for v in (0, -1):
            assert call(dims=tuple(v if d == a else n for d, n in enumerate((4, 6, 8)))) == L.TEM_EINVAL
    assert call(zsec0=-1) == L.TEM_EINVAL and call(per_section=1, zsec0=-1) == L.TEM_EINVAL
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 5).all()
    assert call(per_section=1) == L.TEM_OK
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()


# -------------------------------------------------------------------------------------------------- volume_histogram
@pytest.fixture(scope="module")
def memmap(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("hist") / "vol.npy")
    m = np.lib.format.open_memmap(path, mode="w+", dtype=np.uint8, shape=(40, 50, 70))
    m[...] = np.clip(np.random.default_rng(8).normal(120, 30, m.shape), 0, 255).astype(np.uint8)
    m.flush()
    return np.load(path, mmap_mode="r")


def test_volume_histogram(memmap):
    from transfer_em_amd.utils import hist_chunks, volume_histogram
    vol = np.asarray(memmap)
    budget = 3 * 50 * 70 + 100                                           # 3 sections per slab: 14 z-slabs
    st = {}
    got = volume_histogram(memmap, chunk_bytes=budget, stats=st)
    assert got.dtype == np.int64 and got.shape == (256,) and np.array_equal(got, _bincount(vol))
    assert st["chunks"] == 14 and st["read_s"] > 0
    assert np.array_equal(volume_histogram(memmap), _bincount(vol))                     # the default budget: one slab
    start, size = (9, 5, 3), (53, 39, 14)                                               # an inner ROI, (x, y, z)
    roi = vol[3:17, 5:44, 9:62]
    ysplit = 10 * 53 + 7                                                 # below one section of the ROI: split along y
    assert len(hist_chunks(((3, 17), (5, 44), (9, 62)), ysplit)) == 14 * 4
    for budget in (ysplit, 2 * 39 * 53):
        assert np.array_equal(volume_histogram(memmap, start, size, chunk_bytes=budget), _bincount(roi))
        got = volume_histogram(memmap, start, size, per_section=True, chunk_bytes=budget)
        assert got.shape == (14, 256) and np.array_equal(got, np.stack([_bincount(s) for s in roi]))
    parts = [volume_histogram(memmap, start, size, per_section=True, chunk_bytes=ysplit, rank=r, world_size=2, stats=st)
             for r in range(2)]
    assert st["chunks"] == 28 and all(p.any() for p in parts)
    assert np.array_equal(parts[0] + parts[1], np.stack([_bincount(s) for s in roi]))
    parts = [volume_histogram(memmap, chunk_bytes=budget, rank=r, world_size=2) for r in range(2)]
    assert not np.array_equal(parts[0], parts[1]) and np.array_equal(parts[0] + parts[1], _bincount(vol))
    img = vol[7]
    assert np.array_equal(volume_histogram(img), _bincount(img))
    assert np.array_equal(volume_histogram(img, (3, 4), (60, 41), chunk_bytes=500), _bincount(img[4:45, 3:63]))
    assert volume_histogram(img, per_section=True).shape == (1, 256)
    for start, size in (((0, 0, 0), (71, 50, 40)), ((-1, 0, 0), (5, 5, 5)), ((0, 0, 38), (5, 5, 3))):
        with pytest.raises(ValueError):
            volume_histogram(memmap, start, size)
    assert not volume_histogram(memmap, (0, 0, 0), (0, 50, 40)).any()                   # an empty ROI counts nothing


# ------------------------------------------------------------------------------------------------------- end to end
# the 74 model: tiles of 36 + a halo of 19 (tpad 2)
MS_X, MS_Y = (0.02, 0.58), (-0.1, 0.4)
VOL, START, SIZE = (45, 60, 64), (-5, 3, -4), (50, 41, 40)           # (z,y,x); (x,y,z): 2 x 2 x 2 tiles past two faces
VOL2, START2, SIZE2 = (3, 60, 64), (-3, 4, 0), (50, 41, 3)           # 2-D: 2 x 2 tiles in each of 3 sections
THIN, THIN_START, THIN_SIZE = (20, 40, 45), (0, 0, 0), (36, 36, 100)  # tiles at z = 0, 36, 72: the last reads [53, 127)


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
    return _model(tmp_path_factory.mktemp("hist3"), "hist3", True)


@pytest.fixture(scope="module")
def model2(tmp_path_factory):
    return _model(tmp_path_factory.mktemp("hist2"), "hist2", False)


@pytest.fixture(scope="module")
def vol3():
    return np.random.default_rng(31).integers(0, 256, VOL, dtype=np.uint8)


@pytest.fixture(scope="module")
def table():
    """A table that moves every value, 0 included (lut[0] = 255 - 0 = 255 != 0), and is no bijection."""
    t = (255 - (np.arange(256) // 2) * 2).astype(np.uint8)
    assert t[0] != 0
    return t


@pytest.fixture(scope="module")
def tables():
    """One table per section of VOL, all different."""
    rng = np.random.default_rng(32)
    t = np.stack([rng.permutation(256).astype(np.uint8) for _ in range(VOL[0])])
    assert len({r.tobytes() for r in t}) == VOL[0] and (t[:, 0] != 0).any()
    return t


def _guard(pred):
    """A flat prediction would make the comparisons vacuous."""
    assert pred.std() > 20 and len(np.unique(pred)) >= 16, (pred.std(), len(np.unique(pred)))


def _eq(a, b):
    assert a.shape == b.shape and np.array_equal(a, b), np.argwhere(a != b)[:5]


@pytest.mark.parametrize("boundary", ["zeros", "reflect", "edge"])
def test_cube_with_a_lut_equals_cube_on_the_remapped_volume(model3, vol3, table, boundary):
    from transfer_em_amd.utils import predict_cube
    want_in, want = predict_cube(table[vol3], START, SIZE, model3, MS_X, MS_Y, boundary=boundary, fetch_input=True)
    _guard(want)
    got_in, got = predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y, boundary=boundary, lut=table, fetch_input=True)
    _eq(got, want)
    _eq(got_in, want_in)                                 # fetch_input: the remapped bytes, zeros outside under "zeros"
    if boundary == "zeros":
        assert (want_in[:4] == 0).all() and (want_in[:, :, :5] == 0).all()             # outside: 0, not lut[0] = 255
        plain = predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y)
        assert not np.array_equal(plain, want)


@pytest.mark.parametrize("kw", [dict(ensemble="flips"), dict(mips=1), dict(tile_batch=3)], ids=["flips", "mips1", "batch3"])
def test_cube_with_a_lut_composes(model3, vol3, table, kw):
    from transfer_em_amd.utils import predict_cube
    want = predict_cube(table[vol3], START, SIZE, model3, MS_X, MS_Y, **kw)
    got = predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y, lut=table, **kw)
    if "mips" in kw:
        assert len(got) == len(want) == 2
        _guard(want[0])
        for a, b in zip(got, want):
            _eq(a, b)
    else:
        _guard(want)
        _eq(got, want)


def test_cube_with_a_table_per_section_under_reflect(model3, vol3, tables):
    from transfer_em_amd.utils import predict_cube
    remapped = np.stack([tables[z][vol3[z]] for z in range(VOL[0])])
    want_in, want = predict_cube(remapped, START, SIZE, model3, MS_X, MS_Y, boundary="reflect", fetch_input=True)
    _guard(want)
    got_in, got = predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y, boundary="reflect", lut=tables, fetch_input=True)
    _eq(got, want)
    _eq(got_in, want_in)
    assert not np.array_equal(want, predict_cube(tables[0][vol3], START, SIZE, model3, MS_X, MS_Y, boundary="reflect"))


@pytest.mark.parametrize("boundary", ["zeros", "reflect"])
def test_volume_with_a_lut_equals_cube(model3, vol3, table, tables, boundary):
    from transfer_em_amd.utils import predict_cube, predict_volume
    for t in (table, tables):
        want = predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y, boundary=boundary, lut=t)
        _guard(want)
        got = predict_volume(vol3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 2), boundary=boundary, lut=t)
        _eq(got, want)


def test_volume_with_a_lut_and_a_chunk_outside_the_volume(model3, table):
    """A chunk wholly outside the volume gathers from one stand-in zero byte, which must not become lut[0]."""
    from transfer_em_amd.utils import chunk_plan, predict_cube, predict_volume
    thin = np.random.default_rng(33).integers(0, 256, THIN, dtype=np.uint8)
    chunks = chunk_plan(THIN_START, THIN_SIZE, model3.outdimsize, model3.buffer, THIN, (1, 1, 1))
    assert len(chunks) == 3 and sum(min(c.block) == 0 for c in chunks) == 1
    want = predict_cube(table[thin], THIN_START, THIN_SIZE, model3, MS_X, MS_Y)
    _guard(want)
    _eq(predict_cube(thin, THIN_START, THIN_SIZE, model3, MS_X, MS_Y, lut=table), want)
    per_section = np.tile(table, (THIN[0], 1))
    for t in (table, per_section):
        _eq(predict_volume(thin, THIN_START, THIN_SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 1), lut=t), want)


def test_2d_model_with_a_lut(model2, table):
    from transfer_em_amd.utils import predict_cube, predict_volume
    vol = np.random.default_rng(34).integers(0, 256, VOL2, dtype=np.uint8)
    rows = np.stack([table, table[::-1].copy(), np.roll(table, 7)])
    for t, remapped in ((table, table[vol]), (rows, np.stack([rows[z][vol[z]] for z in range(3)]))):
        want = predict_cube(remapped, START2, SIZE2, model2, MS_X, MS_Y)
        _guard(want)
        _eq(predict_cube(vol, START2, SIZE2, model2, MS_X, MS_Y, lut=t), want)
        _eq(predict_volume(vol, START2, SIZE2, model2, MS_X, MS_Y, chunk_tiles=(2, 1, 2), lut=t), want)
    img = predict_cube(vol[1], START2[:2], SIZE2[:2], model2, MS_X, MS_Y, lut=table)     # one image
    _eq(img, predict_cube(table[vol[1]], START2[:2], SIZE2[:2], model2, MS_X, MS_Y))
    _eq(predict_volume(vol[1], START2[:2], SIZE2[:2], model2, MS_X, MS_Y, lut=table[None]), img)


def test_histogram_of_the_prediction(model3, vol3, model2):
    """SIZE is no multiple of the 36-voxel tile: the margin of the rounded-up blocks must not be counted."""
    from transfer_em_amd.utils import predict_cube, predict_volume
    assert all(n % 36 for n in SIZE)
    st = {}
    out = predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y, histogram=True, stats=st)
    _guard(out)
    want = _bincount(out)
    assert st["histogram"].dtype == np.int64 and np.array_equal(st["histogram"], want) and want.sum() == out.size
    st = {}
    _eq(predict_volume(vol3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 2), histogram=True, stats=st), out)
    assert np.array_equal(st["histogram"], want) and st["chunks"] == 4
    st = {}
    levels = predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y, mips=1, histogram=True, stats=st)
    _eq(levels[0], out)
    assert np.array_equal(st["histogram"], want)                                       # level 0 only
    st = {}
    predict_volume(vol3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 2, 1), mips=1, histogram=True, stats=st)
    assert np.array_equal(st["histogram"], want)
    parts = []
    for rank in range(2):                                                              # the ranks' histograms add
        st = {}
        predict_volume(vol3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 2), rank=rank, world_size=2,
                       histogram=True, stats=st)
        parts.append(st["histogram"])
    assert parts[0].sum() + parts[1].sum() == out.size and np.array_equal(parts[0] + parts[1], want)
    vol2 = np.random.default_rng(35).integers(0, 256, VOL2, dtype=np.uint8)
    st, st2 = {}, {}
    out2 = predict_cube(vol2, START2, SIZE2, model2, MS_X, MS_Y, histogram=True, stats=st)
    predict_volume(vol2, START2, SIZE2, model2, MS_X, MS_Y, chunk_tiles=(2, 1, 2), histogram=True, stats=st2)
    assert np.array_equal(st["histogram"], _bincount(out2)) and np.array_equal(st2["histogram"], _bincount(out2))


def test_defaults_are_the_plain_call(model3, vol3):
    from transfer_em_amd.utils import predict_cube, predict_volume
    plain = predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y)
    _guard(plain)
    st = {}
    _eq(predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y, lut=None, histogram=False, stats=st), plain)
    assert st == {}
    _eq(predict_volume(vol3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 2)), plain)
    _eq(predict_volume(vol3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 2), lut=None, histogram=False, stats=st),
        plain)
    assert "histogram" not in st
    identity = np.arange(256, dtype=np.uint8)
    _eq(predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y, lut=identity), plain)


# ------------------------------------------------------------------------- every option at once; launches; read errors
# 3 x 2 x 1 tiles; chunk_tiles (1, 1, 2) cuts them into 4 chunks of 2, 2, 1 and 1 tiles, so with tile_batch = 1 the
# double buffers are reused and two chunks run two batches each
ALL_VOL, ALL_START, ALL_SIZE = (30, 55, 90), (-3, 2, 1), (100, 60, 36)
ALL_ENSEMBLE = (((0, 1, 2), (0, 0, 0)), ((0, 2, 1), (0, 1, 0)))        # the identity, and a member that moves x
ALL_VOL2, ALL_START2, ALL_SIZE2 = (3, 55, 90), (-3, 2, 0), (100, 60, 3)  # 2-D: 3 x 2 tiles in each of 3 sections
ALL_ENSEMBLE2 = (((0, 1), (0, 0)), ((1, 0), (0, 1)))                     # (y, x): the identity and a transposing member


def _counted(fn):
    """fn()'s result and its launches: calls of _lib.check per entry-point name, generator runs under "run"."""
    import collections
    from transfer_em_amd import _lib, hip_ops
    counts = collections.Counter()
    check, run = _lib.check, hip_ops.run

    def counting_check(rc, what):
        counts[what] += 1
        return check(rc, what)

    def counting_run(launches, stream=None):
        counts["run"] += 1
        return run(launches, stream)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, "check", counting_check)
        mp.setattr(hip_ops, "run", counting_run)
        return fn(), counts


@pytest.fixture(scope="module")
def all3(model3):
    """The 3-D case under every option, resident and streamed, each once and with its launches counted."""
    from transfer_em_amd.utils import predict_cube, predict_volume
    rng = np.random.default_rng(36)
    vol = rng.integers(0, 256, ALL_VOL, dtype=np.uint8)
    lut = np.stack([rng.permutation(256).astype(np.uint8) for _ in range(ALL_VOL[0])])
    kw = dict(boundary="reflect", ensemble=ALL_ENSEMBLE, mips=2, lut=lut, histogram=True, tile_batch=1)
    st_c, st_v = {}, {}
    cube, n_cube = _counted(lambda: predict_cube(vol, ALL_START, ALL_SIZE, model3, MS_X, MS_Y, stats=st_c, **kw))
    streamed, n_vol = _counted(lambda: predict_volume(vol, ALL_START, ALL_SIZE, model3, MS_X, MS_Y,
                                                      chunk_tiles=(1, 1, 2), stats=st_v, **kw))
    return dict(vol=vol, kw=kw, cube=cube, streamed=streamed, n_cube=n_cube, n_vol=n_vol, st_cube=st_c, st_vol=st_v)


def test_every_option_at_once_streamed_equals_resident(all3, model3):
    from transfer_em_amd.utils import chunk_plan, mip_shapes
    chunks = chunk_plan(ALL_START, ALL_SIZE, model3.outdimsize, model3.buffer, ALL_VOL, (1, 1, 2), boundary="reflect")
    assert [len(c.tiles) for c in chunks] == [2, 2, 1, 1]
    cube, streamed = all3["cube"], all3["streamed"]
    assert len(cube) == len(streamed) == 3 and [c.shape for c in cube] == mip_shapes(ALL_SIZE, 2)
    _guard(cube[0])
    for a, b in zip(streamed, cube):
        _eq(a, b)
    assert all3["st_vol"]["chunks"] == 4 and all3["st_vol"]["tile_batch"] == 1
    want = _bincount(cube[0])
    assert np.array_equal(all3["st_vol"]["histogram"], want) and np.array_equal(all3["st_cube"]["histogram"], want)


def test_every_option_at_once_2d(model2):
    from transfer_em_amd.utils import chunk_plan, predict_cube, predict_volume
    chunks = chunk_plan(ALL_START2, ALL_SIZE2, model2.outdimsize, model2.buffer, ALL_VOL2, (2, 1, 2), is3d=False,
                        boundary="reflect")
    assert [len(c.tiles) for c in chunks] == [4, 4, 2, 2, 2, 2, 1, 1]
    rng = np.random.default_rng(37)
    vol = rng.integers(0, 256, ALL_VOL2, dtype=np.uint8)
    lut = np.stack([rng.permutation(256).astype(np.uint8) for _ in range(ALL_VOL2[0])])
    kw = dict(boundary="reflect", ensemble=ALL_ENSEMBLE2, mips=2, lut=lut, histogram=True, tile_batch=3)
    st_c, st_v = {}, {}
    cube = predict_cube(vol, ALL_START2, ALL_SIZE2, model2, MS_X, MS_Y, stats=st_c, **kw)
    streamed = predict_volume(vol, ALL_START2, ALL_SIZE2, model2, MS_X, MS_Y, chunk_tiles=(2, 1, 2), stats=st_v, **kw)
    assert len(cube) == len(streamed) == 3 and st_v["chunks"] == 8 and st_v["tile_batch"] == 3
    _guard(cube[0])
    for a, b in zip(streamed, cube):
        _eq(a, b)
    want = _bincount(cube[0])
    assert np.array_equal(st_v["histogram"], want) and np.array_equal(st_c["histogram"], want)


GATHER, GATHER_BC, GATHER_SYM = "tem_u8_tiles_to_f32_std", "tem_u8_tiles_to_f32_std_bc", "tem_u8_tiles_to_f32_std_sym"
ACCUM, SCATTER = "tem_f32_tiles_sym_accum", "tem_f32_tiles_unstd_to_u8"


def test_launch_counts_follow_the_plan(all3, model3):
    """6 tiles in batches of 1 under 2 members: 12 gathers, runs and accumulates and 6 scatters, resident or streamed;
    the table, the 2 pooled levels and the histogram once for the resident result and once per chunk (4) streamed."""
    from transfer_em_amd.utils import predict_cube, predict_volume
    per_call = {"predict_cube": 1, "predict_volume": 4}
    for name, n in (("predict_cube", all3["n_cube"]), ("predict_volume", all3["n_vol"])):
        got = {k: n[k] for k in (GATHER_SYM, ACCUM, "run", SCATTER, "tem_u8_lut", "tem_u8_pool2", "tem_u8_hist", GATHER,
                                 GATHER_BC)}
        want = {GATHER_SYM: 12, ACCUM: 12, "run": 12, SCATTER: 6, "tem_u8_lut": per_call[name],
                "tem_u8_pool2": 2 * per_call[name], "tem_u8_hist": per_call[name], GATHER: 0, GATHER_BC: 0}
        assert got == want, name
    kw = dict(all3["kw"], ensemble=None)
    calls = {"predict_cube": lambda: predict_cube(all3["vol"], ALL_START, ALL_SIZE, model3, MS_X, MS_Y, stats={}, **kw),
             "predict_volume": lambda: predict_volume(all3["vol"], ALL_START, ALL_SIZE, model3, MS_X, MS_Y,
                                                      chunk_tiles=(1, 1, 2), stats={}, **kw)}
    levels = {}
    for name, fn in calls.items():
        levels[name], n = _counted(fn)
        got = {k: n[k] for k in (GATHER_BC, GATHER_SYM, ACCUM, GATHER, "run", SCATTER)}
        assert got == {GATHER_BC: 6, GATHER_SYM: 0, ACCUM: 0, GATHER: 0, "run": 6, SCATTER: 6}, name
    for a, b in zip(levels["predict_volume"], levels["predict_cube"]):
        _eq(a, b)


class FailingReads:
    """Array-like over a numpy array whose third read raises OSError: a host error, nothing faults on the device."""

    def __init__(self, a):
        self.a, self.shape, self.dtype, self.reads = a, a.shape, a.dtype, 0

    def __getitem__(self, key):
        self.reads += 1
        if self.reads == 3:
            raise OSError("the third read fails")
        return self.a[key]


def test_a_failing_read_surfaces_and_leaves_nothing_behind(all3, model3):
    import threading
    from transfer_em_amd.utils import hist_box, hist_chunks, predict_cube, predict_volume, volume_histogram
    vol = all3["vol"]
    threads = threading.active_count()
    bad = FailingReads(vol)
    with pytest.raises(OSError, match="the third read fails"):
        predict_volume(bad, ALL_START, ALL_SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 2), tile_batch=1)
    assert bad.reads >= 3 and threading.active_count() == threads               # the reader thread has ended
    got = predict_volume(vol, ALL_START, ALL_SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 2), tile_batch=1)
    _guard(got)
    _eq(got, predict_cube(vol, ALL_START, ALL_SIZE, model3, MS_X, MS_Y, tile_batch=1))
    budget = 8 * 55 * 90                                                        # 8 of 30 sections per slab
    assert len(hist_chunks(hist_box(ALL_VOL), budget)) == 4
    bad = FailingReads(vol)
    with pytest.raises(OSError, match="the third read fails"):
        volume_histogram(bad, chunk_bytes=budget)
    assert bad.reads >= 3 and threading.active_count() == threads
    assert np.array_equal(volume_histogram(vol, chunk_bytes=budget), _bincount(vol))


class FailingWrites:
    """Array-like over a numpy array whose third write raises OSError: a host error, nothing faults on the device."""

    def __init__(self, a):
        self.a, self.shape, self.dtype, self.writes = a, a.shape, a.dtype, 0

    def __setitem__(self, key, value):
        self.writes += 1
        if self.writes == 3:
            raise OSError("the third write fails")
        self.a[key] = value


def test_a_failing_write_surfaces_and_leaves_nothing_behind(all3, model3):
    """4 chunks / 4 slabs, so the failing write is that of a reused pinned buffer and writes are queued behind it."""
    import threading
    from clahe_ref import ref_remap, ref_tables, ref_tile_hist
    from transfer_em_amd.utils import (clahe_fit, clahe_volume, hist_box, hist_chunks, mip_shapes, predict_cube,
                                       predict_volume)
    vol = all3["vol"]
    shape = (ALL_SIZE[2], ALL_SIZE[1], ALL_SIZE[0])
    threads = threading.active_count()
    bad = FailingWrites(np.zeros(shape, np.uint8))
    with pytest.raises(OSError, match="the third write fails"):
        predict_volume(vol, ALL_START, ALL_SIZE, model3, MS_X, MS_Y, out=bad, chunk_tiles=(1, 1, 2), tile_batch=1)
    assert bad.writes >= 3 and threading.active_count() == threads              # the host thread has ended
    want = predict_cube(vol, ALL_START, ALL_SIZE, model3, MS_X, MS_Y, tile_batch=1)
    _guard(want)
    _eq(predict_volume(vol, ALL_START, ALL_SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 2), tile_batch=1), want)
    levels = [np.zeros(s, np.uint8) for s in mip_shapes(ALL_SIZE, 2)]           # the per-level write loop
    bad = levels[1] = FailingWrites(levels[1])
    with pytest.raises(OSError, match="the third write fails"):
        predict_volume(vol, ALL_START, ALL_SIZE, model3, MS_X, MS_Y, out=levels, chunk_tiles=(1, 1, 2), tile_batch=1,
                       mips=2)
    assert bad.writes >= 3 and threading.active_count() == threads
    _eq(predict_volume(vol, ALL_START, ALL_SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 2), tile_batch=1), want)
    budget = 8 * 55 * 90                                                        # 8 of 30 sections per slab
    assert len(hist_chunks(hist_box(ALL_VOL), budget)) == 4
    c = clahe_fit(vol, tile=32)
    T = ref_tables(ref_tile_hist(vol, 32, 32), 3.0)
    assert np.array_equal(c.tables, T)
    bad = FailingWrites(np.zeros(ALL_VOL, np.uint8))
    with pytest.raises(OSError, match="the third write fails"):
        clahe_volume(vol, c, out=bad, chunk_bytes=budget)
    assert bad.writes >= 3 and threading.active_count() == threads
    fresh = np.zeros(ALL_VOL, np.uint8)
    assert clahe_volume(vol, c, out=fresh, chunk_bytes=budget) is fresh
    assert np.array_equal(fresh, ref_remap(vol, T, 32, 32))
