"""The 16-bit ingest on the device: tem_u16_hist against np.bincount, tem_u16_lut_u8 and its _direct form against
fancy indexing, volume_histogram16 / volume_to_u8 out of core, and the seeded fixture through the whole route.
Everything is integers or bytes, so every comparison is exact."""
import threading

import numpy as np
import pytest
import torch

import u16_ref as R
from test_gpu_histogram import GUARD, GUARD_BYTE, FailingReads, _boxes, _env, _upload

pytestmark = pytest.mark.gpu

BINS = 65536


def _upload16(a, off=0):
    """The voxels of `a` on the device, `off` ELEMENTS into a 256-byte-aligned allocation."""
    return _upload(np.ascontiguousarray(a).view(np.uint8), 2 * off)


def _hist(ptr, dims, box, signed, per_section=False, counts=None):
    L, lib, stream = _env()
    (z0, z1), (y0, y1), (x0, x1) = box
    if counts is None:
        counts = torch.zeros(((z1 - z0) if per_section else 1, BINS), dtype=torch.int64, device="cuda")
    L.check(lib.tem_u16_hist(ptr, *dims, z0, z1, y0, y1, x0, x1, counts.data_ptr(), int(per_section), int(signed),
                             stream), "tem_u16_hist")
    return counts


def _random16(rng, dims, dtype):
    """Values on both sides of 32768, the ends of the range included."""
    a = rng.integers(0, BINS, dims, dtype=np.uint16)
    flat = a.reshape(-1)
    k = max(1, flat.size // 8)
    flat[rng.integers(0, flat.size, k)] = rng.choice([0, 0x7FFF, 0x8000, 0xFFFF], k)
    return a.view(dtype) if dtype == np.int16 else a


HIST_DIMS = [(3, 5, 1), (2, 7, 9), (3, 9, 37), (2, 33, 131)]


@pytest.mark.parametrize("dtype", [np.uint16, np.int16], ids=["uint16", "int16"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("dims", HIST_DIMS, ids=[str(d).replace(" ", "") for d in HIST_DIMS])
def test_hist_equals_bincount(dims, off, dtype):
    src = _random16(np.random.default_rng(sum(dims)), dims, dtype)
    assert (R.index(src) < 32768).any() and (R.index(src) >= 32768).any()
    keep, ptr = _upload16(src, off)
    for box in _boxes(dims):
        (z0, z1), (y0, y1), (x0, x1) = box
        want = R.ref_hist(src[z0:z1, y0:y1, x0:x1])
        got = _hist(ptr, dims, box, dtype == np.int16).cpu().numpy()[0]
        assert np.array_equal(got, want), (box, np.flatnonzero(got != want)[:5])
        want = R.ref_hist_sections(src[z0:z1, y0:y1, x0:x1])
        got = _hist(ptr, dims, box, dtype == np.int16, per_section=True).cpu().numpy()
        assert np.array_equal(got, want), (box, np.argwhere(got != want)[:5])


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
def test_hist_per_section_runs_cross_sections_and_read_nothing_outside_the_box(off):
    """Inside the box every index is below 50,000; everything around it is 60,000, whose bin must stay empty."""
    dims, box = (9, 40, 150), ((2, 8), (5, 37), (3, 140))
    src = np.full(dims, 60000, np.uint16)
    (z0, z1), (y0, y1), (x0, x1) = box
    src[z0:z1, y0:y1, x0:x1] = np.random.default_rng(2).integers(0, 50000, (z1 - z0, y1 - y0, x1 - x0), dtype=np.uint16)
    keep, ptr = _upload16(src, off)
    want = R.ref_hist_sections(src[z0:z1, y0:y1, x0:x1])
    assert want[:, 60000].sum() == 0
    got = _hist(ptr, dims, box, False, per_section=True).cpu().numpy()
    assert got.shape == (z1 - z0, BINS) and np.array_equal(got, want)
    assert np.array_equal(_hist(ptr, dims, box, False).cpu().numpy()[0], want.sum(axis=0))
    # 300 short sections: more than the workgroups of a class, so each workgroup chains whole sections and flushes at each
    dims2 = (300, 3, 21)
    src2 = np.random.default_rng(3).integers(0, BINS, dims2, dtype=np.uint16)
    keep2, ptr2 = _upload16(src2, off)
    got = _hist(ptr2, dims2, ((0, 300), (0, 3), (0, 21)), False, per_section=True).cpu().numpy()
    assert np.array_equal(got, R.ref_hist_sections(src2))
    # 3 sections of 600 rows: each is cut into pieces, and no piece crosses into the next section
    dims3 = (3, 600, 130)
    src3 = np.random.default_rng(4).integers(0, BINS, dims3, dtype=np.uint16).view(np.int16)
    keep3, ptr3 = _upload16(src3, off)
    got = _hist(ptr3, dims3, ((0, 3), (1, 600), (0, 129)), True, per_section=True).cpu().numpy()
    assert np.array_equal(got, R.ref_hist_sections(src3[:, 1:600, :129]))


def test_hist_calls_add_and_many_workgroups_flush_into_one():
    dims = (7, 64, 300)
    src = np.random.default_rng(1).integers(0, BINS, dims, dtype=np.uint16)
    keep, ptr = _upload16(src)
    counts = _hist(ptr, dims, ((0, 7), (0, 64), (0, 300)), False)
    assert np.array_equal(counts.cpu().numpy()[0], R.ref_hist(src))
    _hist(ptr, dims, ((1, 5), (3, 60), (7, 208)), False, counts=counts)
    assert np.array_equal(counts.cpu().numpy()[0], R.ref_hist(src) + R.ref_hist(src[1:5, 3:60, 7:208]))


def test_hist_of_a_permutation_fills_every_bin_once():
    src = np.random.default_rng(5).permutation(BINS).astype(np.uint16).reshape(1, 256, 256)
    keep, ptr = _upload16(src)
    for signed in (False, True):
        got = _hist(ptr, src.shape, ((0, 1), (0, 256), (0, 256)), signed).cpu().numpy()[0]
        assert (got == 1).all()


@pytest.mark.parametrize("value", [0, 0x7FFF, 0x8000, 0xFFFF])
def test_hist_of_a_constant_block(value):
    """Every lane adds to the same counter: the contention case of the workgroup's shared counters."""
    src = np.full((16, 64, 64), value, np.uint16)
    keep, ptr = _upload16(src)
    for signed in (False, True):
        got = _hist(ptr, src.shape, ((0, 16), (0, 64), (0, 64)), signed).cpu().numpy()[0]
        want = np.zeros(BINS, np.int64)
        want[value ^ (0x8000 if signed else 0)] = src.size
        assert np.array_equal(got, want)


def test_hist_rejects_malformed_arguments():
    """TEM_EINVAL from the host-side checks, nothing launched: counts keeps its fill."""
    L, lib, stream = _env()
    src = torch.zeros(4 * 6 * 8 + 8, dtype=torch.int16, device="cuda")
    counts = torch.full((4, BINS), 7, dtype=torch.int64, device="cuda")
    base = (4, 6, 8)

    def call(ptr=None, dims=base, box=(0, 4, 0, 6, 0, 8), out=None, per_section=0, signed=0):
        return lib.tem_u16_hist(src.data_ptr() if ptr is None else ptr, *dims, *box,
                                counts.data_ptr() if out is None else out, per_section, signed, stream)
    assert call(ptr=0) == L.TEM_EINVAL and call(out=0) == L.TEM_EINVAL
    assert call(ptr=src.data_ptr() + 1) == L.TEM_EINVAL and call(out=counts.data_ptr() + 4) == L.TEM_EINVAL
    for flag in (-1, 2):
        assert call(per_section=flag) == L.TEM_EINVAL and call(signed=flag) == L.TEM_EINVAL
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
    assert call(dims=(M, M, 2), box=(0, M, 0, M, 0, 2), per_section=1) == L.TEM_EINVAL      # one section: 2^32 voxels
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == 7).all()
    for b in ((2, 2, 0, 6, 0, 8), (0, 4, 6, 6, 0, 8), (0, 4, 0, 6, 3, 3)):              # empty boxes: fine, nothing counted
        assert call(box=b) == L.TEM_OK and call(box=b, per_section=1) == L.TEM_OK
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == 7).all()
    assert call(ptr=src.data_ptr() + 2) == L.TEM_OK                                     # any 2-byte alignment
    torch.cuda.synchronize()
    got = counts.cpu().numpy()
    assert got[0, 0] == 7 + 192 and (got.ravel()[1:] == 7).all()


# ---------------------------------------------------------------------------------------------------- tem_u16_lut_u8
def _convert(entry, src_np, table, per_section=False, zsec0=0, src_off=0, dst_off=0):
    """`entry` on src_np placed src_off elements into an aligned allocation, into a dst dst_off bytes into another one,
    between two guards."""
    L, lib, stream = _env()
    n = src_np.size
    t = torch.full((GUARD + dst_off + n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    keep_s, src_ptr = _upload16(src_np, src_off)
    keep_t, lut_ptr = _upload(table, dst_off)                            # the table is as misaligned as dst
    L.check(getattr(lib, entry)(src_ptr, *src_np.shape, t.data_ptr() + GUARD + dst_off, lut_ptr, int(per_section), zsec0,
                                int(src_np.dtype == np.int16), stream), entry)
    got = t.cpu().numpy()
    assert (got[:GUARD + dst_off] == GUARD_BYTE).all() and (got[GUARD + dst_off + n:] == GUARD_BYTE).all(), "guards"
    return got[GUARD + dst_off:GUARD + dst_off + n].reshape(src_np.shape)


@pytest.fixture(scope="module")
def tables():
    """Eight distinct random tables: rows 5, 6, 7 serve the per-section case."""
    t = np.random.default_rng(11).integers(0, 256, (8, BINS), dtype=np.uint8)
    assert len({r.tobytes() for r in t}) == 8
    return t


@pytest.mark.parametrize("src_off", [0, 1], ids=["src0", "src1"])
@pytest.mark.parametrize("W", [1, 7, 8, 9, 37, 64])
def test_lut_equals_fancy_indexing(W, src_off, tables):
    rng = np.random.default_rng(W)
    for dtype in (np.uint16, np.int16):
        src = _random16(rng, (3, 5, W), dtype)
        for dst_off in range(4):
            want = R.ref_convert(src, tables[0])
            got = _convert("tem_u16_lut_u8", src, tables[0], src_off=src_off, dst_off=dst_off)
            assert np.array_equal(got, want), (dtype, dst_off)
            direct = _convert("tem_u16_lut_u8_direct", src, tables[0], src_off=src_off, dst_off=dst_off)
            assert np.array_equal(direct, got)
            want = R.ref_convert(src, tables, zsec0=5)                   # D = 3 at section 5: rows 5, 6, 7
            assert not np.array_equal(want, R.ref_convert(src, tables, zsec0=0)) or W == 1
            for entry in ("tem_u16_lut_u8", "tem_u16_lut_u8_direct"):
                got = _convert(entry, src, tables, per_section=True, zsec0=5, src_off=src_off, dst_off=dst_off)
                assert np.array_equal(got, want), (entry, dtype, dst_off)


def test_lut_of_several_workgroups_per_section(tables):
    src = _random16(np.random.default_rng(12), (3, 300, 1111), np.uint16)            # 333,300 voxels per section
    for entry in ("tem_u16_lut_u8", "tem_u16_lut_u8_direct"):
        assert np.array_equal(_convert(entry, src, tables[1], src_off=1, dst_off=3), R.ref_convert(src, tables[1]))
        assert np.array_equal(_convert(entry, src, tables, per_section=True, zsec0=2), R.ref_convert(src, tables, zsec0=2))


def test_lut_rejects_malformed_arguments():
    L, lib, stream = _env()
    src = torch.zeros(4 * 6 * 8 + 8, dtype=torch.int16, device="cuda")
    dst = torch.full((4 * 6 * 8,), 5, dtype=torch.uint8, device="cuda")
    table = torch.full((4 * BINS,), 9, dtype=torch.uint8, device="cuda")
    for entry in (lib.tem_u16_lut_u8, lib.tem_u16_lut_u8_direct):
        def call(ptr=None, dims=(4, 6, 8), out=None, lut=None, per_section=0, zsec0=0, signed=0):
            return entry(src.data_ptr() if ptr is None else ptr, *dims, dst.data_ptr() if out is None else out,
                         table.data_ptr() if lut is None else lut, per_section, zsec0, signed, stream)
        assert call(ptr=0) == L.TEM_EINVAL and call(out=0) == L.TEM_EINVAL and call(lut=0) == L.TEM_EINVAL
        assert call(ptr=src.data_ptr() + 1) == L.TEM_EINVAL
        for a in range(3):
            for v in (0, -1):
                assert call(dims=tuple(v if d == a else n for d, n in enumerate((4, 6, 8)))) == L.TEM_EINVAL
        assert call(zsec0=-1) == L.TEM_EINVAL and call(per_section=1, zsec0=-1) == L.TEM_EINVAL
        for flag in (-1, 2):
            assert call(per_section=flag) == L.TEM_EINVAL and call(signed=flag) == L.TEM_EINVAL
        torch.cuda.synchronize()
        assert (dst.cpu().numpy() == 5).all()
        assert call(per_section=1, ptr=src.data_ptr() + 2) == L.TEM_OK
        torch.cuda.synchronize()
        assert (dst.cpu().numpy() == 9).all()
        dst.fill_(5)


# ------------------------------------------------------------------------------------------------------- out of core
VOL, START, SIZE = (9, 50, 70), (9, 5, 2), (53, 39, 6)                   # the ROI: [2:8, 5:44, 9:62]


@pytest.fixture(scope="module")
def vol16():
    return _random16(np.random.default_rng(21), VOL, np.uint16)


@pytest.fixture(scope="module")
def memmap16(tmp_path_factory, vol16):
    path = str(tmp_path_factory.mktemp("u16") / "vol.npy")
    m = np.lib.format.open_memmap(path, mode="w+", dtype=np.uint16, shape=VOL)
    m[...] = vol16
    m.flush()
    return np.load(path, mmap_mode="r")


# bytes: three sections per slab; rows of one section; below one row (one-row slabs)
BUDGETS = {"sections": 2 * 3 * 39 * 53 + 100, "rows": 2 * 10 * 53 + 7, "one_row": 50}


@pytest.mark.parametrize("source", ["ndarray", "memmap"])
def test_volume_histogram16(vol16, memmap16, source):
    from transfer_em_amd.utils import hist_chunks, volume_histogram16
    vol = vol16 if source == "ndarray" else memmap16
    st = {}
    got = volume_histogram16(vol, chunk_bytes=2 * 2 * 50 * 70 + 100, stats=st)           # 2 sections per slab: 5 slabs
    assert got.dtype == np.int64 and got.shape == (BINS,) and np.array_equal(got, R.ref_hist(vol16))
    assert st["chunks"] == 5 and st["read_s"] > 0
    assert np.array_equal(volume_histogram16(vol), R.ref_hist(vol16))                    # the default budget: one slab
    roi = vol16[2:8, 5:44, 9:62]
    box = ((2, 8), (5, 44), (9, 62))
    assert [len(hist_chunks(box, b, itemsize=2)) for b in BUDGETS.values()] == [2, 6 * 4, 6 * 39]
    for budget in BUDGETS.values():
        assert np.array_equal(volume_histogram16(vol, START, SIZE, chunk_bytes=budget), R.ref_hist(roi))
        got = volume_histogram16(vol, START, SIZE, per_section=True, chunk_bytes=budget)
        assert got.shape == (6, BINS) and np.array_equal(got, R.ref_hist_sections(roi))
    parts = [volume_histogram16(vol, START, SIZE, per_section=True, chunk_bytes=BUDGETS["rows"], rank=r, world_size=2,
                                stats=st) for r in range(2)]
    assert st["chunks"] == 12 and all(p.any() for p in parts)
    assert np.array_equal(parts[0] + parts[1], R.ref_hist_sections(roi))
    assert not volume_histogram16(vol, (0, 0, 0), (0, 50, 9)).any()                      # an empty ROI counts nothing


def test_volume_histogram16_signed_image_and_slab_accumulators(vol16, monkeypatch):
    from transfer_em_amd import utils
    signed = vol16.view(np.int16)
    assert np.array_equal(utils.volume_histogram16(signed, chunk_bytes=BUDGETS["rows"]), R.ref_hist(signed))
    img = signed[7]
    assert np.array_equal(utils.volume_histogram16(img), R.ref_hist(img))
    assert np.array_equal(utils.volume_histogram16(img, (3, 4), (60, 41), chunk_bytes=500), R.ref_hist(img[4:45, 3:63]))
    assert utils.volume_histogram16(img, per_section=True).shape == (1, BINS)
    # past CLAHE_ACC_BYTES the accumulator holds one slab's sections and is read back per slab
    monkeypatch.setattr(utils, "CLAHE_ACC_BYTES", 3 * BINS * 8)
    for budget in (BUDGETS["sections"], BUDGETS["rows"]):
        got = utils.volume_histogram16(vol16, START, SIZE, per_section=True, chunk_bytes=budget)
        assert np.array_equal(got, R.ref_hist_sections(vol16[2:8, 5:44, 9:62]))


@pytest.mark.parametrize("source", ["ndarray", "memmap"])
def test_volume_to_u8(vol16, memmap16, tables, source, tmp_path):
    from transfer_em_amd.utils import volume_to_u8
    vol = vol16 if source == "ndarray" else memmap16
    luts = np.concatenate([tables, tables[:1]])                                          # 9 rows: one per section
    st = {}
    got = volume_to_u8(vol, tables[0], chunk_bytes=2 * 2 * 50 * 70 + 100, histogram=True, stats=st)
    assert got.dtype == np.uint8 and np.array_equal(got, R.ref_convert(vol16, tables[0]))
    assert st["chunks"] == 5 and st["read_s"] > 0 and st["write_s"] > 0
    assert np.array_equal(st["histogram"], np.bincount(got.ravel(), minlength=256))
    roi = vol16[2:8, 5:44, 9:62]
    want = R.ref_convert(roi, luts, zsec0=2)                                             # rows belong to the volume
    assert not np.array_equal(want, R.ref_convert(roi, luts, zsec0=0))
    for budget in BUDGETS.values():
        assert np.array_equal(volume_to_u8(vol, luts, start=START, size=SIZE, chunk_bytes=budget), want)
        assert np.array_equal(volume_to_u8(vol, tables[3], start=START, size=SIZE, chunk_bytes=budget),
                              R.ref_convert(roi, tables[3]))
    out = np.lib.format.open_memmap(str(tmp_path / "out.npy"), mode="w+", dtype=np.uint8, shape=(6, 39, 53))
    hists = []
    for r in range(2):                                                                   # two ranks: disjoint boxes of `out`
        st = {}
        assert volume_to_u8(vol, luts, out=out, start=START, size=SIZE, chunk_bytes=BUDGETS["rows"], rank=r,
                            world_size=2, histogram=True, stats=st) is out
        assert st["chunks"] == 12
        hists.append(st["histogram"])
        if r == 0:
            assert not np.array_equal(out, want) and 0 < hists[0].sum() < want.size
    assert np.array_equal(out, want)
    assert np.array_equal(hists[0] + hists[1], np.bincount(want.ravel(), minlength=256))


def test_volume_to_u8_signed_and_one_image(vol16, tables):
    from transfer_em_amd.utils import volume_to_u8
    signed = vol16.view(np.int16)
    assert np.array_equal(volume_to_u8(signed, tables[2], chunk_bytes=BUDGETS["rows"]), R.ref_convert(signed, tables[2]))
    img = signed[7]
    got = volume_to_u8(img, tables[4])
    assert got.shape == img.shape and np.array_equal(got, R.ref_convert(img[None], tables[4])[0])
    got = volume_to_u8(img, tables[4:5], start=(3, 4), size=(60, 41), chunk_bytes=500)
    assert np.array_equal(got, R.ref_convert(img[None, 4:45, 3:63], tables[4])[0])


def test_a_failing_read_surfaces_and_leaves_nothing_behind(vol16, tables):
    from transfer_em_amd.utils import hist_box, hist_chunks, volume_histogram16, volume_to_u8
    budget = 2 * 2 * 50 * 70
    assert len(hist_chunks(hist_box(VOL), budget, itemsize=2)) == 5
    threads = threading.active_count()
    bad = FailingReads(vol16)
    with pytest.raises(OSError, match="the third read fails"):
        volume_histogram16(bad, chunk_bytes=budget)
    assert bad.reads >= 3 and threading.active_count() == threads               # the reader thread has ended
    bad = FailingReads(vol16)
    with pytest.raises(OSError, match="the third read fails"):
        volume_to_u8(bad, tables[0], chunk_bytes=budget)
    assert bad.reads >= 3 and threading.active_count() == threads
    assert np.array_equal(volume_histogram16(vol16, chunk_bytes=budget), R.ref_hist(vol16))
    assert np.array_equal(volume_to_u8(vol16, tables[0], chunk_bytes=budget), R.ref_convert(vol16, tables[0]))


# ------------------------------------------------------------------------------------------------------- the fixture
def test_the_fixture_through_the_device_route():
    """Per-section volume_histogram16 -> match_lut16 -> volume_to_u8 equals the numpy route byte for byte, and that
    route is the best of the four."""
    from transfer_em_amd.utils import match_lut16, volume_histogram, volume_histogram16, volume_to_u8
    G, raw = R.fixture_stack()
    want_luts, want = R.route_match16_sections(raw, G)
    h = volume_histogram16(raw, per_section=True, chunk_bytes=2 * 96 * 128 * 5)          # 5 sections per slab
    assert np.array_equal(h, R.ref_hist_sections(raw))
    h_ref = volume_histogram(G, per_section=True)
    luts = match_lut16(h, h_ref)
    assert np.array_equal(luts, want_luts)
    st = {}
    got = volume_to_u8(raw, luts, chunk_bytes=2 * 96 * 100, histogram=True, stats=st)    # rows of a section per slab
    assert np.array_equal(got, want)
    assert np.array_equal(st["histogram"], np.bincount(got.ravel(), minlength=256))
    routes = R.fixture_routes(raw, G)
    assert np.array_equal(routes[0], got)
    maes = [R.mae(r, G) for r in routes]
    print("MAE (grey levels): per-section 16-bit match %.4f, per-section window + per-section 8-bit match %.4f, "
          "global window + per-section 8-bit match %.4f, global window + global 8-bit match %.4f" % tuple(maes))
    assert maes[0] < maes[1] < maes[2] < maes[3]
