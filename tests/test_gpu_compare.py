"""Two uint8 volumes held against each other on the device: tem_u8_hist2 against numpy (np.bincount of 256 a + b),
volume_joint_histogram out of core, and predict_cube / predict_volume with `compare`.  Everything is integers, so
every comparison is exact.  Helpers, volumes and the 74-model fixtures are those of test_gpu_histogram.py."""
import numpy as np
import pytest
import torch

from test_gpu_histogram import (MS_X, MS_Y, SIZE, SIZE2, START, START2, THIN, THIN_SIZE, THIN_START, VOL, VOL2, HIST_DIMS,
                                FailingReads, _boxes, _counted, _env, _eq, _guard, _hist, _upload,
                                model2, model3, table, vol3)  # noqa: F401  (the last four are fixtures)

pytestmark = pytest.mark.gpu


def _joint(a, b):
    return np.bincount(a.ravel().astype(np.int64) * 256 + b.ravel(), minlength=65536).reshape(256, 256)


def _hist2(pa, da, oa, pb, db, ob, n, counts=None):
    """tem_u8_hist2 of the box of extents n at origin oa of block (pa, da) against origin ob of block (pb, db)."""
    L, lib, stream = _env()
    if counts is None:
        counts = torch.zeros((256, 256), dtype=torch.int64, device="cuda")
    L.check(lib.tem_u8_hist2(pa, *da, *oa, pb, *db, *ob, *n, counts.data_ptr(), stream), "tem_u8_hist2")
    return counts


def _whole(a, b, off=(0, 0)):
    """The joint histogram of two whole blocks of one shape."""
    ka, pa = _upload(a, off[0])
    kb, pb = _upload(b, off[1])
    return _hist2(pa, a.shape, (0, 0, 0), pb, b.shape, (0, 0, 0), a.shape).cpu().numpy()


# ------------------------------------------------------------------------------------------------------ tem_u8_hist2
OFFS = [(0, 0), (1, 0), (0, 1), (1, 3)]


@pytest.mark.parametrize("off", OFFS, ids=[f"off{a}{b}" for a, b in OFFS])
@pytest.mark.parametrize("dims", HIST_DIMS, ids=[str(d).replace(" ", "") for d in HIST_DIMS])
def test_hist2_equals_bincount(dims, off):
    """`b` once in a block of another width and at other origins than `a` (rows misaligned differently modulo 16),
    once in a block of a's geometry (both rows aligned alike)."""
    rng = np.random.default_rng(sum(dims) + 2)
    D, H, W = dims
    a = rng.integers(0, 256, dims, dtype=np.uint8)
    other = (D + 1, H + 2, W + 5)
    b_other, b_same = rng.integers(0, 256, other, dtype=np.uint8), rng.integers(0, 256, dims, dtype=np.uint8)
    ka, pa = _upload(a, off[0])
    ko, po = _upload(b_other, off[1])
    ks, ps = _upload(b_same, off[1])
    for box in _boxes(dims):
        (z0, z1), (y0, y1), (x0, x1) = box
        n = (z1 - z0, y1 - y0, x1 - x0)
        want = _joint(a[z0:z1, y0:y1, x0:x1], b_other[z0 + 1:z1 + 1, y0 + 2:y1 + 2, x0 + 5:x1 + 5])
        got = _hist2(pa, dims, (z0, y0, x0), po, other, (z0 + 1, y0 + 2, x0 + 5), n).cpu().numpy()
        assert np.array_equal(got, want), (box, np.argwhere(got != want)[:5])
        want = _joint(a[z0:z1, y0:y1, x0:x1], b_same[z0:z1, y0:y1, x0:x1])
        got = _hist2(pa, dims, (z0, y0, x0), ps, dims, (z0, y0, x0), n).cpu().numpy()
        assert np.array_equal(got, want), (box, np.argwhere(got != want)[:5])


def test_hist2_index_order_and_marginals():
    """J(a, b) == J(b, a).T on an asymmetric pair (a swapped index would pass a symmetric one), and the row sums are
    tem_u8_hist of a's box."""
    dims, box = (5, 33, 131), ((1, 5), (2, 30), (3, 120))
    rng = np.random.default_rng(3)
    a = rng.integers(0, 100, dims, dtype=np.uint8)
    b = (a // 2 + rng.integers(100, 110, dims)).astype(np.uint8)
    (z0, z1), (y0, y1), (x0, x1) = box
    org, n = (z0, y0, x0), (z1 - z0, y1 - y0, x1 - x0)
    ka, pa = _upload(a, 1)
    kb, pb = _upload(b)
    ab = _hist2(pa, dims, org, pb, dims, org, n).cpu().numpy()
    ba = _hist2(pb, dims, org, pa, dims, org, n).cpu().numpy()
    assert not np.array_equal(ab, ab.T) and np.array_equal(ab, ba.T)
    assert np.array_equal(ab, _joint(a[z0:z1, y0:y1, x0:x1], b[z0:z1, y0:y1, x0:x1]))
    assert np.array_equal(ab.sum(axis=1), _hist(pa, dims, box).cpu().numpy()[0])
    assert np.array_equal(ab.sum(axis=0), _hist(pb, dims, box).cpu().numpy()[0])


@pytest.mark.parametrize("pair", [(0, 0), (255, 255), (0, 255), (255, 0), (127, 128), (128, 127)], ids=str)
def test_hist2_of_a_constant_pair(pair):
    """Every lane of every wave adds to one counter: the contention case, at the corner bins and on both sides of the
    seam of the split by the high bit of `a`."""
    a, b = np.full((64, 64, 64), pair[0], np.uint8), np.full((64, 64, 64), pair[1], np.uint8)
    want = np.zeros((256, 256), np.int64)
    want[pair] = 262144
    assert np.array_equal(_whole(a, b), want)


# (13, 128, 128): 1,664 rows of 9 segments, 4 workgroups per half of the table.  (65, 128, 1024): 8,320 rows of 66
# segments = 549,120 items, past the 524,288 at which the grid is capped: 128 workgroups per half, each with a run of
# 65 rows = 66,560 voxels that walks every bin, so every bin of the table takes 128 flushes
EVERY_BIN = [(13, 128, 128), (65, 128, 1024)]


@pytest.mark.parametrize("dims", EVERY_BIN, ids=[str(d).replace(" ", "") for d in EVERY_BIN])
def test_hist2_with_every_bin_occupied(dims):
    """All sections but the last walk all 65,536 (a, b) pairs in order, a whole number of times; the last repeats the
    first quarter of the walk, so the bins hold two different counts."""
    D, H, W = dims
    assert ((D - 1) * H * W) % 65536 == 0 and (H * W) % 16384 == 0
    i = np.concatenate([np.arange((D - 1) * H * W) % 65536, np.arange(H * W) % 16384])
    a, b = (i >> 8).astype(np.uint8).reshape(dims), (i & 255).astype(np.uint8).reshape(dims)
    want = _joint(a, b)
    assert (want > 0).all() and len(np.unique(want)) == 2
    got = _whole(a, b, off=(0, 1))
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_hist2_splits_rows_and_segments_exactly_for_wide_rows():
    """129 rows of 1,330,409 bytes: 83,152 segments per row and runs of 2 rows per workgroup.  At this width the
    multiply-high by ceil(2^32 / S) alone is one too large for the last items of a run (asserted below on the host,
    among them segments that certainly hold 16 bytes), which would drop their bytes: the kernel has to correct it.  `a`
    and `b` are two boxes of ONE buffer, two bytes apart, so the rows of the two sides are misaligned differently."""
    ny, nx = 129, 1330409
    S, W = (nx + 30) // 16, nx + 2
    magic = (2 ** 32 + S - 1) // S
    i = np.arange(2 * S, dtype=np.uint64)
    wrong = i[((i * np.uint64(magic)) >> np.uint64(32)) != i // np.uint64(S)]
    assert len(wrong) >= 2 and int((wrong % np.uint64(S)).min()) <= S - 3
    buf = np.random.default_rng(6).integers(0, 256, (1, ny, W), dtype=np.uint8)
    keep, ptr = _upload(buf, 1)
    got = _hist2(ptr, buf.shape, (0, 0, 0), ptr, buf.shape, (0, 0, 2), (1, ny, nx)).cpu().numpy()
    want = np.zeros((256, 256), np.int64)
    for y in range(0, ny, 16):                                           # in pieces: the index array is 8 bytes a voxel
        want += _joint(buf[0, y:y + 16, :nx], buf[0, y:y + 16, 2:])
    assert want.sum() == ny * nx
    assert got.sum() == want.sum(), (int(got.sum()), int(want.sum()))
    assert np.array_equal(got, want)


def test_hist2_calls_add_and_many_workgroups_flush_into_one():
    dims = (7, 64, 300)                                  # 448 rows of 20 segments: 3 workgroups per half of the table
    rng = np.random.default_rng(4)
    a, b = rng.integers(0, 256, dims, dtype=np.uint8), rng.integers(0, 256, dims, dtype=np.uint8)
    ka, pa = _upload(a)
    kb, pb = _upload(b, 2)
    counts = torch.full((256, 256), 7, dtype=torch.int64, device="cuda")
    _hist2(pa, dims, (0, 0, 0), pb, dims, (0, 0, 0), dims, counts=counts)
    assert np.array_equal(counts.cpu().numpy(), 7 + _joint(a, b))
    _hist2(pa, dims, (1, 3, 7), pb, dims, (1, 3, 7), (4, 57, 201), counts=counts)
    assert np.array_equal(counts.cpu().numpy(), 7 + _joint(a, b) + _joint(a[1:5, 3:60, 7:208], b[1:5, 3:60, 7:208]))


@pytest.mark.parametrize("off", [(0, 0), (1, 3)], ids=["aligned", "off13"])
def test_hist2_counts_nothing_outside_the_boxes(off):
    """Inside the boxes every byte is below 200; everything around them is 233, whose row and column must stay empty."""
    da, oa, db, ob, n = (9, 40, 150), (2, 5, 3), (8, 45, 161), (1, 9, 14), (6, 32, 137)
    rng = np.random.default_rng(5)
    a, b = np.full(da, 233, np.uint8), np.full(db, 233, np.uint8)
    sa = tuple(slice(o, o + e) for o, e in zip(oa, n))
    sb = tuple(slice(o, o + e) for o, e in zip(ob, n))
    a[sa], b[sb] = rng.integers(0, 200, n, dtype=np.uint8), rng.integers(0, 200, n, dtype=np.uint8)
    ka, pa = _upload(a, off[0])
    kb, pb = _upload(b, off[1])
    got = _hist2(pa, da, oa, pb, db, ob, n).cpu().numpy()
    assert not got[233].any() and not got[:, 233].any() and got.sum() == np.prod(n)
    assert np.array_equal(got, _joint(a[sa], b[sb]))


def test_hist2_rejects_malformed_arguments():
    """TEM_EINVAL from the host-side checks, nothing launched: counts keeps its fill."""
    L, lib, stream = _env()
    a = torch.zeros(4 * 6 * 8, dtype=torch.uint8, device="cuda")
    b = torch.ones(5 * 7 * 9, dtype=torch.uint8, device="cuda")
    counts = torch.full((256 * 256 + 1,), 7, dtype=torch.int64, device="cuda")

    def call(pa=None, da=(4, 6, 8), oa=(0, 0, 0), pb=None, db=(5, 7, 9), ob=(1, 1, 1), n=(4, 6, 8), out=None):
        return lib.tem_u8_hist2(a.data_ptr() if pa is None else pa, *da, *oa, b.data_ptr() if pb is None else pb, *db,
                                *ob, *n, counts.data_ptr() if out is None else out, stream)
    assert call(pa=0) == L.TEM_EINVAL and call(pb=0) == L.TEM_EINVAL and call(out=0) == L.TEM_EINVAL
    assert call(out=counts.data_ptr() + 4) == L.TEM_EINVAL                             # off 8-byte alignment
    at = lambda t, d, v: tuple(v if i == d else e for i, e in enumerate(t))
    for d in range(3):
        for v in (0, -1):                                                               # a dim below 1
            assert call(da=at((4, 6, 8), d, v), n=at((4, 6, 8), d, 0)) == L.TEM_EINVAL
            assert call(db=at((5, 7, 9), d, v), ob=(0, 0, 0), n=at((4, 6, 8), d, 0)) == L.TEM_EINVAL
        assert call(oa=at((0, 0, 0), d, -1)) == L.TEM_EINVAL and call(ob=at((1, 1, 1), d, -1)) == L.TEM_EINVAL
        assert call(n=at((4, 6, 8), d, -1)) == L.TEM_EINVAL                             # a negative extent
        assert call(oa=at((0, 0, 0), d, 1)) == L.TEM_EINVAL                             # the box leaves a
        assert call(ob=at((1, 1, 1), d, 2)) == L.TEM_EINVAL                             # ... leaves b
        assert call(n=at((4, 6, 8), d, (5, 7, 9)[d]), ob=(0, 0, 0)) == L.TEM_EINVAL     # fits b, leaves a
    # too many voxels for a workgroup's 32-bit counters (the bound of include/tem_hip.h); refused on the host, so the
    # extents need no memory behind them
    M = 2 ** 31 - 1
    assert call(da=(1, M, M), db=(1, M, M), ob=(0, 0, 0), n=(1, M, M)) == L.TEM_EINVAL
    assert call(da=(M, M, 16), db=(M, M, 16), ob=(0, 0, 0), n=(M, M, 16)) == L.TEM_EINVAL
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == 7).all()
    for d in range(3):                                                                  # empty boxes: fine, nothing counted
        assert call(n=at((4, 6, 8), d, 0)) == L.TEM_OK
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == 7).all()
    assert call() == L.TEM_OK
    torch.cuda.synchronize()
    got = counts.cpu().numpy()
    assert got[1] == 7 + 192 and (np.delete(got, 1) == 7).all()                         # all of (0, 1); the 65537th kept


# -------------------------------------------------------------------------------------------- volume_joint_histogram
@pytest.fixture(scope="module")
def memmaps(tmp_path_factory):
    """An EM-like (40, 50, 70) memmap and a noisy copy of it inside a larger (43, 56, 77) one, at (z, y, x) (2, 4, 6)."""
    tmp = tmp_path_factory.mktemp("joint")
    rng = np.random.default_rng(9)
    a = np.lib.format.open_memmap(str(tmp / "a.npy"), mode="w+", dtype=np.uint8, shape=(40, 50, 70))
    a[...] = np.clip(rng.normal(120, 30, a.shape), 0, 255).astype(np.uint8)
    b = np.lib.format.open_memmap(str(tmp / "b.npy"), mode="w+", dtype=np.uint8, shape=(43, 56, 77))
    b[...] = rng.integers(0, 256, b.shape, dtype=np.uint8)
    b[2:42, 4:54, 6:76] = np.clip(a.astype(np.int64) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    a.flush(), b.flush()
    return np.load(str(tmp / "a.npy"), mmap_mode="r"), np.load(str(tmp / "b.npy"), mmap_mode="r")


def test_volume_joint_histogram(memmaps):
    import threading
    from transfer_em_amd.utils import hist_chunks, volume_joint_histogram
    ma, mb = memmaps
    a, b = np.asarray(ma), np.asarray(mb)
    whole = _joint(a, b[2:42, 4:54, 6:76])
    budget = 3 * 50 * 70 + 100                                           # 3 sections per slab: 14 z-slabs
    st = {}
    got = volume_joint_histogram(ma, mb, b_start=(6, 4, 2), chunk_bytes=budget, stats=st)
    assert got.dtype == np.int64 and got.shape == (256, 256) and np.array_equal(got, whole)
    assert st["chunks"] == 14 and st["read_s"] > 0
    assert np.array_equal(volume_joint_histogram(ma, mb, b_start=(6, 4, 2)), whole)     # the default budget: one slab
    assert np.array_equal(volume_joint_histogram(ma, mb), _joint(a, b[:40, :50, :70]))  # b_start=None: a's start
    start, size, b_start = (9, 5, 3), (53, 39, 14), (20, 1, 7)                          # an inner ROI, (x, y, z)
    want = _joint(a[3:17, 5:44, 9:62], b[7:21, 1:40, 20:73])
    assert np.array_equal(volume_joint_histogram(ma, mb, start, size), _joint(a[3:17, 5:44, 9:62], b[3:17, 5:44, 9:62]))
    ysplit = 10 * 53 + 7                                                 # below one section of the ROI: split along y
    assert len(hist_chunks(((3, 17), (5, 44), (9, 62)), ysplit)) == 14 * 4
    for budget in (ysplit, 2 * 39 * 53):
        assert np.array_equal(volume_joint_histogram(ma, mb, start, size, b_start, chunk_bytes=budget), want)
    parts = [volume_joint_histogram(ma, mb, start, size, b_start, chunk_bytes=ysplit, rank=r, world_size=2, stats=st)
             for r in range(2)]
    assert st["chunks"] == 28 and all(p.any() for p in parts) and not np.array_equal(parts[0], parts[1])
    assert np.array_equal(parts[0] + parts[1], want)
    ia, ib = a[7], b[9]                                                  # one image
    assert np.array_equal(volume_joint_histogram(ia, ib), _joint(ia, ib[:50, :70]))
    assert np.array_equal(volume_joint_histogram(ia, ib, (3, 4), (60, 41), (11, 2), chunk_bytes=500),
                          _joint(ia[4:45, 3:63], ib[2:43, 11:71]))
    for kw in (dict(start=(0, 0, 0), size=(71, 50, 40)), dict(start=(-1, 0, 0), size=(5, 5, 5)),
               dict(start=(0, 0, 38), size=(5, 5, 3)), dict(b_start=(8, 0, 0)), dict(b_start=(0, 0, -1)),
               dict(size=(5, 5, -1)), dict(start=(0, 0), size=(5, 5))):
        with pytest.raises(ValueError):
            volume_joint_histogram(ma, mb, **kw)
    for bad in ((a.astype(np.uint16), b), (a, b.astype(np.int8)), (a, ib)):
        with pytest.raises(ValueError):
            volume_joint_histogram(*bad)
    assert not volume_joint_histogram(ma, mb, (0, 0, 0), (0, 50, 40)).any()             # an empty ROI counts nothing
    # a failing read: a host error that surfaces, ends the reader thread and leaves the next call right
    threads = threading.active_count()
    bad = FailingReads(a)
    with pytest.raises(OSError, match="the third read fails"):
        volume_joint_histogram(bad, mb, chunk_bytes=8 * 50 * 70)                        # 5 slabs
    assert bad.reads >= 3 and threading.active_count() == threads
    assert np.array_equal(volume_joint_histogram(ma, mb, chunk_bytes=8 * 50 * 70), _joint(a, b[:40, :50, :70]))


# ------------------------------------------------------------------------------------------------------- end to end
def _inside(vol_shape, start, size):
    """(slices of the volume, slices of the result) of the ROI voxels that lie inside the volume; start / size (x, y, z)."""
    lo = [max(s, 0) for s in start[::-1]]
    hi = [min(s + n, v) for s, n, v in zip(start[::-1], size[::-1], vol_shape)]
    return (tuple(slice(l, h) for l, h in zip(lo, hi)),
            tuple(slice(l - s, h - s) for l, h, s in zip(lo, hi, start[::-1])))


@pytest.fixture(scope="module")
def gt3():
    return np.random.default_rng(38).integers(0, 256, VOL, dtype=np.uint8)


@pytest.fixture(scope="module")
def cube3(model3, vol3, gt3):
    """The resident prediction of the 3-D case with its joint histogram, the reference of the streamed forms."""
    from transfer_em_amd.utils import predict_cube
    st = {}
    (out, n) = _counted(lambda: predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y, compare=gt3, stats=st))
    _guard(out)
    return out, st, n


def test_cube_compare_equals_numpy_on_the_inside_voxels(cube3, gt3):
    out, st, n = cube3
    in_vol, in_out = _inside(VOL, START, SIZE)
    J = st["joint_histogram"]
    assert J.dtype == np.int64 and J.shape == (256, 256) and set(st) == {"joint_histogram"}
    assert J.sum() == gt3[in_vol].size == 36 * 41 * 45 and J.sum() < out.size       # the ROI passes two faces
    assert np.array_equal(J, _joint(gt3[in_vol], out[in_out]))
    assert n["tem_u8_hist2"] == 1 and n["tem_u8_hist"] == 0


def test_volume_compare_equals_cube(cube3, model3, vol3, gt3):
    from transfer_em_amd.utils import predict_cube, predict_volume
    out, st_c, _ = cube3
    want = st_c["joint_histogram"]
    st = {}
    got, n = _counted(lambda: predict_volume(vol3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 2), compare=gt3,
                                             stats=st))
    _eq(got, out)
    assert st["chunks"] == 4 and n["tem_u8_hist2"] == 4 and np.array_equal(st["joint_histogram"], want)
    st = {}
    _eq(predict_volume(vol3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(2, 1, 1), tile_batch=1, compare=gt3,
                       stats=st), out)
    assert np.array_equal(st["joint_histogram"], want)
    parts = []
    for rank in range(2):                                                              # the ranks' tables add
        st = {}
        predict_volume(vol3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 2), rank=rank, world_size=2,
                       compare=gt3, stats=st)
        parts.append(st["joint_histogram"])
    assert parts[0].any() and parts[1].any() and np.array_equal(parts[0] + parts[1], want)
    for fn, kw in ((predict_cube, {}), (predict_volume, dict(chunk_tiles=(1, 2, 1)))):  # mips: level 0 is compared
        st = {}
        levels = fn(vol3, START, SIZE, model3, MS_X, MS_Y, mips=1, compare=gt3, stats=st, **kw)
        _eq(levels[0], out)
        assert np.array_equal(st["joint_histogram"], want)


def test_compare_composes_streamed_equals_resident(model3, vol3, gt3, table):
    from transfer_em_amd.utils import predict_cube, predict_volume
    kw = dict(lut=table, ensemble="flips", boundary="reflect", histogram=True, compare=gt3)
    st_c, st_v = {}, {}
    cube = predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y, stats=st_c, **kw)
    _guard(cube)
    streamed, n = _counted(lambda: predict_volume(vol3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 2),
                                                  stats=st_v, **kw))
    _eq(streamed, cube)
    in_vol, in_out = _inside(VOL, START, SIZE)
    want = _joint(gt3[in_vol], cube[in_out])                             # mirrored voxels outside are not compared
    assert want.sum() < cube.size and n["tem_u8_hist2"] == 4 and n["tem_u8_hist"] == 4
    assert np.array_equal(st_c["joint_histogram"], want) and np.array_equal(st_v["joint_histogram"], want)
    assert np.array_equal(st_c["histogram"], st_v["histogram"]) and st_c["histogram"].sum() == cube.size


def test_compare_with_chunks_outside_the_volume(model3):
    """THIN's ROI runs far past the volume's last section: a chunk without ground truth launches nothing."""
    from transfer_em_amd.utils import chunk_plan, predict_cube, predict_volume
    rng = np.random.default_rng(39)
    thin, gt = rng.integers(0, 256, THIN, dtype=np.uint8), rng.integers(0, 256, THIN, dtype=np.uint8)
    chunks = chunk_plan(THIN_START, THIN_SIZE, model3.outdimsize, model3.buffer, THIN, (1, 1, 1))
    assert len(chunks) == 3 and sum(min(c.block) == 0 for c in chunks) == 1
    assert sum(c.out_box[0][0] < THIN[0] for c in chunks) == 1           # one chunk's result lies inside the volume
    st_c, st_v = {}, {}
    cube = predict_cube(thin, THIN_START, THIN_SIZE, model3, MS_X, MS_Y, compare=gt, stats=st_c)
    _guard(cube)
    streamed, n = _counted(lambda: predict_volume(thin, THIN_START, THIN_SIZE, model3, MS_X, MS_Y,
                                                  chunk_tiles=(1, 1, 1), compare=gt, stats=st_v))
    _eq(streamed, cube)
    want = _joint(gt[:, :36, :36], cube[:20])
    assert n["tem_u8_hist2"] == 1 and want.sum() == 20 * 36 * 36
    assert np.array_equal(st_c["joint_histogram"], want) and np.array_equal(st_v["joint_histogram"], want)


def test_compare_with_a_2d_model_and_one_image(model2):
    from transfer_em_amd.utils import predict_cube, predict_volume
    rng = np.random.default_rng(40)
    vol, gt = rng.integers(0, 256, VOL2, dtype=np.uint8), rng.integers(0, 256, VOL2, dtype=np.uint8)
    st_c, st_v = {}, {}
    cube = predict_cube(vol, START2, SIZE2, model2, MS_X, MS_Y, compare=gt, stats=st_c)
    _guard(cube)
    _eq(predict_volume(vol, START2, SIZE2, model2, MS_X, MS_Y, chunk_tiles=(2, 1, 2), compare=gt, stats=st_v), cube)
    in_vol, in_out = _inside(VOL2, START2, SIZE2)
    want = _joint(gt[in_vol], cube[in_out])
    assert 0 < want.sum() < cube.size
    assert np.array_equal(st_c["joint_histogram"], want) and np.array_equal(st_v["joint_histogram"], want)
    st_c, st_v = {}, {}
    img = predict_cube(vol[1], START2[:2], SIZE2[:2], model2, MS_X, MS_Y, compare=gt[1], stats=st_c)     # one image
    _eq(img, cube[1])
    _eq(predict_volume(vol[1], START2[:2], SIZE2[:2], model2, MS_X, MS_Y, compare=gt[1], stats=st_v), img)
    want = _joint(gt[1][in_vol[1:]], img[in_out[1:]])
    assert np.array_equal(st_c["joint_histogram"], want) and np.array_equal(st_v["joint_histogram"], want)


def test_without_compare_the_launches_are_the_plain_call(cube3, model3, vol3):
    from transfer_em_amd.utils import predict_cube, predict_volume
    out, _, n_with = cube3
    st = {}
    plain, n = _counted(lambda: predict_cube(vol3, START, SIZE, model3, MS_X, MS_Y, compare=None, stats=st))
    _eq(plain, out)
    assert st == {} and n["tem_u8_hist2"] == 0
    assert {k: v for k, v in n_with.items() if k != "tem_u8_hist2"} == dict(n)       # compare adds its one launch only
    bare, n_bare = _counted(lambda: predict_volume(vol3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 2)))
    st = {}
    streamed, n = _counted(lambda: predict_volume(vol3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 2),
                                                  compare=None, stats=st))
    _eq(streamed, out)
    _eq(bare, out)
    assert "joint_histogram" not in st and n["tem_u8_hist2"] == 0 and dict(n) == dict(n_bare)
