"""CLAHE on the device: tem_u8_hist_tiles and tem_u8_clahe against the in-test numpy reference (clahe_ref),
clahe_histograms / clahe_volume out of core, and predict_cube / predict_volume with `clahe`.  Everything is integers or
bytes, so every comparison is exact."""
import collections

import numpy as np
import pytest
import torch

from clahe_ref import assert_input_condition, ramp_volume, ref_grid, ref_remap, ref_tables, ref_tile_hist
from util import scaled_params

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 64, 233
BLOCKS = [(1, 1, 1), (3, 5, 17), (2, 7, 16), (5, 33, 131)]
TILES = [(1, 1), (7, 19), (16, 16), (16, 24), (2048, 2048)]
IDS = [str(d).replace(" ", "") for d in BLOCKS]


def _env():
    from transfer_em_amd import _lib as L
    from transfer_em_amd import hip_ops as H
    return L, H.require_gpu(), H.current_stream()


def _origins(th, tw):
    """(0, 0), an odd one, and one that puts the block's first row and column on the last pixel of a tile."""
    return [(0, 0), (3, 2), (th - 1, tw - 1)]


def _guarded(a, off, fill=GUARD_BYTE):
    """The bytes of `a`, `off` bytes past GUARD bytes of `fill` in a 256-byte-aligned allocation that ends in GUARD
    more of them; (tensor, pointer to the first byte of `a`)."""
    flat = np.ascontiguousarray(a).reshape(-1)
    t = torch.full((GUARD + off + flat.size + GUARD,), fill, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    t[GUARD + off:GUARD + off + flat.size] = torch.from_numpy(flat).cuda()
    return t, t.data_ptr() + GUARD + off


def _ref_counts(block, y_org, x_org, th, tw, gy, gx):
    D, H, W = block.shape
    d, y, x = np.arange(D)[:, None, None], np.arange(H)[None, :, None], np.arange(W)[None, None, :]
    idx = ((d * gy + (y_org + y) // th) * gx + (x_org + x) // tw) * 256 + block
    return np.bincount(idx.ravel(), minlength=D * gy * gx * 256).reshape(D, gy, gx, 256).astype(np.int64)


def _hist_tiles(ptr, dims, y_org, x_org, th, tw, gy, gx, counts=None):
    L, lib, stream = _env()
    if counts is None:
        counts = torch.zeros((dims[0], gy, gx, 256), dtype=torch.int32, device="cuda")
    L.check(lib.tem_u8_hist_tiles(ptr, *dims, y_org, x_org, th, tw, gy, gx, counts.data_ptr(), stream), "tem_u8_hist_tiles")
    return counts


def _u32(counts):
    return counts.cpu().numpy().view(np.uint32).astype(np.int64)


# ------------------------------------------------------------------------------------------------- tem_u8_hist_tiles
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("dims", BLOCKS, ids=IDS)
def test_hist_tiles_equals_bincount_per_tile(dims, off):
    """The block holds values below 200 between guards of 233: nothing outside the block is read while bin 233 stays
    empty."""
    block = np.random.default_rng(sum(dims)).integers(0, 200, dims, dtype=np.uint8)
    keep, ptr = _guarded(block, off)
    D, H, W = dims
    for th, tw in TILES:
        for y_org, x_org in _origins(th, tw):
            gy, gx = ref_grid(y_org + H, x_org + W, th, tw)
            gx += 1                                                      # a column of tiles the block does not reach
            want = _ref_counts(block, y_org, x_org, th, tw, gy, gx)
            got = _u32(_hist_tiles(ptr, dims, y_org, x_org, th, tw, gy, gx))
            assert got[..., GUARD_BYTE].sum() == 0 and got.sum() == block.size, (th, tw, y_org, x_org)
            assert np.array_equal(got, want), (th, tw, y_org, x_org, np.argwhere(got != want)[:5])


def test_hist_tiles_calls_add():
    """Two slabs that cut the tiles between rows accumulate into the same counters; the second call starts at a row
    that is no tile boundary."""
    dims, th, tw = (4, 50, 300), 16, 24
    block = np.random.default_rng(3).integers(0, 256, dims, dtype=np.uint8)
    gy, gx = ref_grid(50, 300, th, tw)
    want = ref_tile_hist(block, th, tw)
    keep, ptr = _guarded(block, 0)
    assert np.array_equal(_u32(_hist_tiles(ptr, dims, 0, 0, th, tw, gy, gx)), want)
    counts = torch.zeros((4, gy, gx, 256), dtype=torch.int32, device="cuda")
    for y0, y1 in ((0, 21), (21, 50)):
        keep2, ptr2 = _guarded(block[:, y0:y1], 1)
        _hist_tiles(ptr2, (4, y1 - y0, 300), y0, 0, th, tw, gy, gx, counts=counts)
    assert np.array_equal(_u32(counts), want)
    _hist_tiles(ptr, dims, 0, 0, th, tw, gy, gx, counts=counts)
    assert np.array_equal(_u32(counts), 2 * want)


@pytest.mark.parametrize("value", [255, 0])
def test_hist_tiles_of_a_constant_block(value):
    """Every lane adds to the same bin: the contention case of the workgroup-private counters."""
    block = np.full((64, 64, 64), value, np.uint8)
    keep, ptr = _guarded(block, 0, fill=7)
    got = _u32(_hist_tiles(ptr, block.shape, 0, 0, 16, 16, 4, 4))
    want = np.zeros((64, 4, 4, 256), np.int64)
    want[..., value] = 256
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------ tem_u8_clahe
def _clahe(block, T, th, tw, zsec0=0, y_org=0, x_org=0, off=0):
    """tem_u8_clahe on a copy of `block` between two guards, the tables as misaligned as the buffer."""
    L, lib, stream = _env()
    t, ptr = _guarded(block, off)
    keep, tptr = _guarded(T, off)
    L.check(lib.tem_u8_clahe(ptr, *block.shape, zsec0, y_org, x_org, tptr, T.shape[1], T.shape[2], th, tw, stream),
            "tem_u8_clahe")
    got, n = t.cpu().numpy(), block.size
    assert (got[:GUARD + off] == GUARD_BYTE).all() and (got[GUARD + off + n:] == GUARD_BYTE).all(), "guards were written"
    assert np.array_equal(keep.cpu().numpy()[GUARD + off:GUARD + off + T.size], T.reshape(-1))
    return got[GUARD + off:GUARD + off + n].reshape(block.shape)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("dims", BLOCKS, ids=IDS)
def test_clahe_equals_the_reference_remap(dims, off):
    rng = np.random.default_rng(sum(dims) + 1)
    block = rng.integers(0, 256, dims, dtype=np.uint8)
    D, H, W = dims
    for th, tw in TILES:
        for y_org, x_org in _origins(th, tw):
            gy, gx = ref_grid(y_org + H, x_org + W, th, tw)
            gx += 1
            T = rng.integers(0, 256, (D + 3, gy, gx, 256), dtype=np.uint8)      # random tables: no two alike
            for zsec0 in (0, 2):
                want = ref_remap(block, T, th, tw, zsec0, y_org, x_org)
                got = _clahe(block, T, th, tw, zsec0, y_org, x_org, off)
                assert np.array_equal(got, want), (th, tw, y_org, x_org, zsec0, np.argwhere(got != want)[:5])
            if D > 1 or H > 1:
                assert not np.array_equal(want, ref_remap(block, T, th, tw, 0, y_org, x_org))      # zsec0 picks the rows


def test_clahe_on_a_grid_of_one_tile_is_the_plain_lookup():
    rng = np.random.default_rng(5)
    block = rng.integers(0, 256, (3, 40, 150), dtype=np.uint8)
    T = rng.integers(0, 256, (3, 1, 1, 256), dtype=np.uint8)
    want = np.stack([T[z, 0, 0][block[z]] for z in range(3)])
    for th, tw in ((40, 150), (64, 256), (2048, 2048)):
        assert np.array_equal(_clahe(block, T, th, tw), want)
    assert np.array_equal(_clahe(block[:, 5:30, 11:140], T, 40, 150, 0, 5, 11, off=1), want[:, 5:30, 11:140])


def test_clahe_numerator_at_the_32_bit_bound():
    """Tile (2048, 2048) with tables of 0 and 255 only: the numerator reaches 255 * 4 * 2048^2 + 2 * 2048^2 = 4 286 578 688.
    8 x 8 blocks sit where the weights wy, wx pass 0 | 1, 2047 | 2048 and 4095: with an even tile f = 2 y + 1 - th is
    odd, so the weights are the odd numbers and the blocks straddle the even targets (wy = 4095 at y = 1023 is followed
    by wy = 1 of the next cell at y = 1024; 2047 at y = 2047, 2049 at y = 2048; 4095 at y = 3071)."""
    rng = np.random.default_rng(6)
    t = 2048
    T = rng.choice(np.array([0, 255], np.uint8), (2, 2, 2, 256))
    full = np.full((2, 2, 2, 256), 255, np.uint8)
    block = rng.integers(0, 256, (2, 8, 8), dtype=np.uint8)
    orgs = [0, 1023 - 3, 1024 - 3, 2047 - 3, 3071 - 3, 4096 - 8]
    seen = set()
    for y_org in orgs:
        for x_org in orgs:
            f = 2 * (y_org + np.arange(8)) + 1 - t
            seen |= set((f - (f // (2 * t)) * 2 * t).tolist())
            want = ref_remap(block, T, t, t, 0, y_org, x_org)
            got = _clahe(block, T, t, t, 0, y_org, x_org)
            assert np.array_equal(got, want), (y_org, x_org, np.argwhere(got != want)[:5])
            assert (_clahe(block, full, t, t, 0, y_org, x_org) == 255).all(), (y_org, x_org)
    assert {1, 2047, 2049, 4095} <= seen


def test_both_kernels_reject_malformed_arguments():
    """TEM_EINVAL from the host-side checks, nothing launched: the buffers keep their fill."""
    L, lib, stream = _env()
    buf = torch.full((4 * 6 * 8,), 5, dtype=torch.uint8, device="cuda")
    counts = torch.full((4, 1, 1, 256), 7, dtype=torch.int32, device="cuda")
    tables = torch.zeros((4, 1, 1, 256), dtype=torch.uint8, device="cuda")
    base = dict(buf=buf.data_ptr(), D=4, H=6, W=8, zsec0=0, y_org=0, x_org=0, th=16, tw=16, gy=1, gx=1,
                counts=counts.data_ptr(), tables=tables.data_ptr())

    def hist(**kw):
        a = dict(base, **kw)
        return lib.tem_u8_hist_tiles(a["buf"], a["D"], a["H"], a["W"], a["y_org"], a["x_org"], a["th"], a["tw"], a["gy"],
                                     a["gx"], a["counts"], stream)

    def remap(**kw):
        a = dict(base, **kw)
        return lib.tem_u8_clahe(a["buf"], a["D"], a["H"], a["W"], a["zsec0"], a["y_org"], a["x_org"], a["tables"],
                                a["gy"], a["gx"], a["th"], a["tw"], stream)
    bad = [dict(buf=0)] + [{k: v} for k in ("D", "H", "W") for v in (0, -1)] + \
          [{k: v} for k in ("th", "tw") for v in (0, -1, 2049)] + [dict(y_org=-1), dict(x_org=-1)] + \
          [dict(y_org=11), dict(x_org=9), dict(th=5), dict(tw=7), dict(gy=0), dict(gx=0)]       # past the grid
    for kw in bad:
        assert hist(**kw) == L.TEM_EINVAL, kw
        assert remap(**kw) == L.TEM_EINVAL, kw
    assert hist(counts=0) == L.TEM_EINVAL and remap(tables=0) == L.TEM_EINVAL and remap(zsec0=-1) == L.TEM_EINVAL
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 5).all() and (counts.cpu().numpy() == 7).all()
    assert hist(y_org=10, x_org=8) == L.TEM_OK and remap(y_org=10, x_org=8) == L.TEM_OK      # exactly to the grid's end
    torch.cuda.synchronize()
    got = counts.cpu().numpy()
    assert (got[..., 5] == 7 + 48).all() and (np.delete(got, 5, axis=-1) == 7).all()
    assert not buf.cpu().numpy().any()                                   # tables of zeros


# ---------------------------------------------------------------------------------- clahe_histograms and clahe_volume
TILE = (16, 24)
MM = (9, 70, 150)
BUDGETS = [None, 30 * 150 + 11, 150]         # the default (one slab); below one section (row slabs cut tiles); one row


@pytest.fixture(scope="module")
def memmap(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("clahe") / "vol.npy")
    m = np.lib.format.open_memmap(path, mode="w+", dtype=np.uint8, shape=MM)
    m[...] = ramp_volume(MM, 41)
    m.flush()
    return np.load(path, mmap_mode="r")


@pytest.fixture(scope="module")
def mm_ref(memmap):
    """(volume, tile histograms, tables, equalised volume) of the memmap by the reference; the input condition holds."""
    vol = np.asarray(memmap)
    h = ref_tile_hist(vol, *TILE)
    T = ref_tables(h, 3.0)
    return vol, h, T, assert_input_condition(vol, T, *TILE)


def test_clahe_histograms(memmap, mm_ref, monkeypatch):
    from transfer_em_amd import utils
    from transfer_em_amd.utils import clahe_histograms, hist_box, hist_chunks
    vol, h, _, _ = mm_ref
    assert [len(hist_chunks(hist_box(MM), b)) for b in BUDGETS] == [1, 9 * 3, 9 * 70]
    for budget in BUDGETS:
        st = {}
        got = clahe_histograms(memmap, TILE, chunk_bytes=budget, stats=st)
        assert got.dtype == np.uint32 and got.shape == (9, 5, 7, 256) and np.array_equal(got, h), budget
        assert st["chunks"] == len(hist_chunks(hist_box(MM), budget)) and st["read_s"] > 0
    parts = [clahe_histograms(memmap, TILE, chunk_bytes=BUDGETS[1], rank=r, world_size=2) for r in range(2)]
    assert all(p.any() for p in parts) and np.array_equal(parts[0].astype(np.int64) + parts[1], h)
    monkeypatch.setattr(utils, "CLAHE_ACC_BYTES", 1000)                  # one accumulator per slab, added on the host
    assert np.array_equal(clahe_histograms(memmap, TILE, chunk_bytes=BUDGETS[1]), h)
    assert np.array_equal(clahe_histograms(memmap, TILE, chunk_bytes=2 * 70 * 150), h)
    monkeypatch.undo()
    img = vol[4]
    got = clahe_histograms(img, TILE, chunk_bytes=1000)                  # one image
    assert got.shape == (1, 5, 7, 256) and np.array_equal(got[0], h[4])
    assert np.array_equal(clahe_histograms(vol, 2048)[:, 0, 0], np.stack([np.bincount(s.ravel(), minlength=256) for s in vol]))


@pytest.mark.parametrize("budget", BUDGETS, ids=["default", "rows", "one_row"])
def test_clahe_volume(memmap, mm_ref, tmp_path, budget):
    from transfer_em_amd.utils import ClaheTables, clahe_fit, clahe_volume
    vol, _, T, ref = mm_ref
    c = clahe_fit(memmap, TILE, chunk_bytes=budget)
    assert isinstance(c, ClaheTables) and c.tile == TILE and np.array_equal(c.tables, T)
    out = np.lib.format.open_memmap(str(tmp_path / "out.npy"), mode="w+", dtype=np.uint8, shape=MM)
    st = {}
    assert clahe_volume(memmap, c, out=out, chunk_bytes=budget, histogram=True, stats=st) is out
    assert np.array_equal(np.asarray(out), ref)
    assert st["histogram"].dtype == np.int64 and np.array_equal(st["histogram"], np.bincount(ref.ravel(), minlength=256))
    assert st["chunks"] == {None: 1, 150: 630}.get(budget, 27) and st["write_s"] > 0
    start, size = (13, 9, 2), (121, 50, 6)                              # an inner ROI, (x, y, z): origins off the grid
    roi = ref[2:8, 9:59, 13:134]
    st = {}
    got = clahe_volume(memmap, c, start=start, size=size, chunk_bytes=budget, histogram=True, stats=st)
    assert got.shape == roi.shape and np.array_equal(got, roi)
    assert np.array_equal(st["histogram"], np.bincount(roi.ravel(), minlength=256))


def test_clahe_volume_ranks_and_one_image(memmap, mm_ref):
    from transfer_em_amd.utils import ClaheTables, clahe_volume
    vol, _, T, ref = mm_ref
    c = ClaheTables(T, TILE)
    out, hists = np.zeros(MM, np.uint8), []
    for rank in range(2):
        st = {}
        clahe_volume(memmap, c, out=out, chunk_bytes=BUDGETS[1], rank=rank, world_size=2, histogram=True, stats=st)
        hists.append(st["histogram"])
        assert st["chunks"] in (13, 14) and (rank == 1 or not np.array_equal(out, ref))
    assert np.array_equal(out, ref) and np.array_equal(hists[0] + hists[1], np.bincount(ref.ravel(), minlength=256))
    c1 = ClaheTables(T[4:5], TILE)
    assert np.array_equal(clahe_volume(vol[4], c1, chunk_bytes=1000), ref[4])
    assert np.array_equal(clahe_volume(vol[4], c1, start=(13, 9), size=(121, 50)), ref[4, 9:59, 13:134])


# ------------------------------------------------------------------------------------------------------- prediction
# the 74 model: tiles of 36 + a halo of 19 (tpad 2); the volumes and ROIs of test_gpu_histogram.py.  Tile (16, 24) puts
# several tiles and the partial edge tiles (60 = 3 * 16 + 12, 64 = 2 * 24 + 16) into every footprint.
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
    return _model(tmp_path_factory.mktemp("clahe3"), "clahe3", True)


@pytest.fixture(scope="module")
def model2(tmp_path_factory):
    return _model(tmp_path_factory.mktemp("clahe2"), "clahe2", False)


Case = collections.namedtuple("Case", "vol clahe eq")


def _case(shape, seed, z_radius=0):
    """A volume under the input condition, its tables from the device pipeline -- equal to the reference's -- and the
    reference-equalised volume (computed once, shared, left unchanged)."""
    from transfer_em_amd.utils import clahe_fit
    vol = ramp_volume(shape, seed)
    T = ref_tables(ref_tile_hist(vol, *TILE), 3.0, z_radius)
    eq = assert_input_condition(vol, T, *TILE)
    c = clahe_fit(vol, TILE, z_radius=z_radius)
    assert np.array_equal(c.tables, T)
    return Case(vol, c, eq)


@pytest.fixture(scope="module")
def case3():
    return _case(VOL, 51)


@pytest.fixture(scope="module")
def case2():
    return _case(VOL2, 52)


@pytest.fixture(scope="module")
def thin():
    return _case(THIN, 53)


def _streamed(vol, model, start=START, size=SIZE, chunk_tiles=(1, 1, 1), **kw):
    """predict_volume in chunks of one tile: every axis is cut."""
    from transfer_em_amd.utils import predict_volume
    return predict_volume(vol, start, size, model, MS_X, MS_Y, chunk_tiles=chunk_tiles, **kw)


def _guard(pred):
    """A flat prediction would make the comparisons vacuous."""
    assert pred.std() > 20 and len(np.unique(pred)) >= 16, (pred.std(), len(np.unique(pred)))


def _eq(a, b):
    assert a.shape == b.shape and np.array_equal(a, b), np.argwhere(a != b)[:5]


@pytest.mark.parametrize("boundary", ["zeros", "reflect", "edge"])
def test_cube_with_clahe_equals_cube_on_the_equalised_volume(model3, case3, boundary):
    from transfer_em_amd.utils import predict_cube
    want_in, want = predict_cube(case3.eq, START, SIZE, model3, MS_X, MS_Y, boundary=boundary, fetch_input=True)
    _guard(want)
    got_in, got = predict_cube(case3.vol, START, SIZE, model3, MS_X, MS_Y, boundary=boundary, clahe=case3.clahe,
                               fetch_input=True)
    _eq(got, want)
    _eq(got_in, want_in)                                 # fetch_input: what the network saw
    if boundary == "zeros":
        assert (want_in[:4] == 0).all() and (want_in[:, :, :5] == 0).all()             # outside the volume: still 0
        assert not np.array_equal(predict_cube(case3.vol, START, SIZE, model3, MS_X, MS_Y), want)


@pytest.mark.parametrize("kw", [dict(ensemble="flips"), dict(mips=1), dict(tile_batch=1), dict(histogram=True)],
                         ids=["flips", "mips1", "batch1", "histogram"])
def test_cube_with_clahe_composes(model3, case3, kw):
    from transfer_em_amd.utils import predict_cube
    st_w, st_g = {}, {}
    want = predict_cube(case3.eq, START, SIZE, model3, MS_X, MS_Y, stats=st_w, **kw)
    got = predict_cube(case3.vol, START, SIZE, model3, MS_X, MS_Y, clahe=case3.clahe, stats=st_g, **kw)
    if "mips" in kw:
        assert len(got) == len(want) == 2
        _eq(got[1], want[1])
        want, got = want[0], got[0]
    _guard(want)
    _eq(got, want)
    if "histogram" in kw:
        assert np.array_equal(st_g["histogram"], st_w["histogram"])
        assert np.array_equal(st_g["histogram"], np.bincount(want.ravel(), minlength=256))


def test_cube_with_clahe_and_a_lut_runs_clahe_first(model3, case3):
    from transfer_em_amd.utils import predict_cube
    t = (255 - (np.arange(256) // 2) * 2).astype(np.uint8)
    want_in, want = predict_cube(t[case3.eq], START, SIZE, model3, MS_X, MS_Y, fetch_input=True)
    _guard(want)
    got_in, got = predict_cube(case3.vol, START, SIZE, model3, MS_X, MS_Y, clahe=case3.clahe, lut=t, fetch_input=True)
    _eq(got, want)
    _eq(got_in, want_in)
    rows = np.stack([np.roll(t, z) for z in range(VOL[0])])                # one table per section
    want = predict_cube(np.stack([rows[z][case3.eq[z]] for z in range(VOL[0])]), START, SIZE, model3, MS_X, MS_Y)
    _eq(predict_cube(case3.vol, START, SIZE, model3, MS_X, MS_Y, clahe=case3.clahe, lut=rows), want)
    _eq(_streamed(case3.vol, model3, clahe=case3.clahe, lut=rows), want)


@pytest.mark.parametrize("boundary", ["zeros", "reflect"])
def test_volume_with_clahe_equals_cube(model3, case3, boundary):
    """chunk_tiles (1, 1, 1) cuts every axis: 8 chunks whose footprints start off the tile grid."""
    from transfer_em_amd.utils import chunk_plan, predict_cube
    chunks = chunk_plan(START, SIZE, model3.outdimsize, model3.buffer, VOL, (1, 1, 1), boundary=boundary)
    assert len(chunks) == 8 and len({c.read for c in chunks}) == 8
    assert any(c.read[1][0] % TILE[0] for c in chunks) and any(c.read[2][0] % TILE[1] for c in chunks)
    want = predict_cube(case3.eq, START, SIZE, model3, MS_X, MS_Y, boundary=boundary)
    _guard(want)
    _eq(_streamed(case3.vol, model3, boundary=boundary, clahe=case3.clahe), want)
    _eq(_streamed(case3.vol, model3, chunk_tiles=(2, 1, 2), boundary=boundary, clahe=case3.clahe), want)


def test_volume_with_clahe_and_a_chunk_outside_the_volume(model3, thin):
    """A chunk wholly outside the volume gathers from one stand-in zero byte, which is not remapped."""
    from transfer_em_amd.utils import chunk_plan, predict_cube
    case = thin
    chunks = chunk_plan(THIN_START, THIN_SIZE, model3.outdimsize, model3.buffer, THIN, (1, 1, 1))
    assert len(chunks) == 3 and sum(min(c.block) == 0 for c in chunks) == 1
    assert (case.clahe.tables[:, :, :, 0] != 0).any()                      # T[0] != 0 somewhere: a remapped 0 would show
    want = predict_cube(case.eq, THIN_START, THIN_SIZE, model3, MS_X, MS_Y)
    _guard(want)
    _eq(predict_cube(case.vol, THIN_START, THIN_SIZE, model3, MS_X, MS_Y, clahe=case.clahe), want)
    _eq(_streamed(case.vol, model3, THIN_START, THIN_SIZE, clahe=case.clahe), want)


def test_2d_model_with_clahe(model2, case2):
    from transfer_em_amd.utils import ClaheTables, predict_cube, predict_volume
    want = predict_cube(case2.eq, START2, SIZE2, model2, MS_X, MS_Y)
    _guard(want)
    _eq(predict_cube(case2.vol, START2, SIZE2, model2, MS_X, MS_Y, clahe=case2.clahe), want)
    _eq(_streamed(case2.vol, model2, START2, SIZE2, chunk_tiles=(2, 1, 2), clahe=case2.clahe), want)
    one = ClaheTables(case2.clahe.tables[1:2], TILE)                       # one image: the tables of its section
    img = predict_cube(case2.eq[1], START2[:2], SIZE2[:2], model2, MS_X, MS_Y)
    _eq(predict_cube(case2.vol[1], START2[:2], SIZE2[:2], model2, MS_X, MS_Y, clahe=one), img)
    _eq(predict_volume(case2.vol[1], START2[:2], SIZE2[:2], model2, MS_X, MS_Y, clahe=one), img)


def test_tables_of_a_z_radius_go_through_unchanged(model3, case3):
    from transfer_em_amd.utils import predict_cube
    case = _case(VOL, 51, z_radius=1)
    assert np.array_equal(case.vol, case3.vol) and not np.array_equal(case.clahe.tables, case3.clahe.tables)
    want = predict_cube(case.eq, START, SIZE, model3, MS_X, MS_Y)
    _guard(want)
    _eq(predict_cube(case.vol, START, SIZE, model3, MS_X, MS_Y, clahe=case.clahe), want)
    _eq(_streamed(case.vol, model3, clahe=case.clahe), want)


def _counted(fn):
    """fn()'s result and its launches: calls of _lib.check per entry-point name, generator runs under "run"."""
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


def test_clahe_none_is_the_plain_call_and_launches_follow_the_plan(model3, case3, thin):
    """clahe=None runs the plain call's launches and bytes; clahe=c adds exactly one tem_u8_clahe per non-empty
    footprint: one for the resident volume, one per streamed chunk that touches the volume."""
    from transfer_em_amd.utils import predict_cube
    calls = {
        "cube": (lambda **kw: predict_cube(case3.vol, START, SIZE, model3, MS_X, MS_Y, **kw), 1),
        "volume": (lambda **kw: _streamed(case3.vol, model3, **kw), 8),
        "thin": (lambda **kw: _streamed(thin.vol, model3, THIN_START, THIN_SIZE, **kw), 2),
    }
    for name, (fn, footprints) in calls.items():
        plain, n_plain = _counted(fn)
        none, n_none = _counted(lambda: fn(clahe=None))
        _eq(none, plain)
        assert n_none == n_plain and n_plain["tem_u8_clahe"] == 0 and n_plain["run"] > 0, name
        c = thin.clahe if name == "thin" else case3.clahe
        got, n = _counted(lambda: fn(clahe=c))
        assert not np.array_equal(got, plain)
        assert dict(n) == dict(n_plain, tem_u8_clahe=footprints), (name, n, n_plain)
