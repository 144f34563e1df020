"""Resampling along z on the device: tem_u8_resample_z against the numpy reference (zspace_ref) for every kind of
table, volume_resample_z out of core on the fixture with planted section positions, and the chain section_lag_sums ->
section_spacing -> volume_resample_z held to the fixture's conditions.  Every comparison of bytes is exact.  The kernel
reads src and writes dst between guards of fill bytes; src and all guards must come back untouched.  Helpers are those
of test_gpu_histogram.py."""
import functools

import numpy as np
import pytest
import torch

import zspace_ref as ZR
from test_gpu_histogram import _counted, _env

pytestmark = pytest.mark.gpu

GUARD, FILL, DFILL = 64, 0xA5, 0x3C
BLOCKS = [(1, 5, 7), (3, 5, 7), (4, 33, 70), (9, 64, 257)]


@functools.lru_cache(maxsize=None)
def _data(shape):
    a = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    a[0, 0, :3] = (0, 255, 254)                                                     # the extremes meet every weight
    if shape[0] > 1:
        a[1, 0, :3] = (255, 0, 255)
    a.setflags(write=False)
    return a


def _tables(D):
    """name -> taps [NZ, 2] over a volume of D sections that the block holds whole."""
    t = {"identity": [(z, 0) for z in range(D)],
         "the_last_section": [(D - 1, 0)] * 3}
    if D > 1:
        t["every_weight"] = [(0, w) for w in range(256)] + [(1, 0)]
        t["many_outputs_per_pair"] = [(z, w) for z in range(D - 1) for w in (0, 3, 100, 127, 128, 200, 255)] + [(D - 1, 0)]
        t["non_monotone"] = [(D - 1, 0), (0, 77), (D - 2, 255), (0, 0), (D - 2, 1), (0, 77), (D - 1, 0), (D - 2, 128)]
    if D > 3:
        t["jumps"] = [(0, 10), (2, 200), (2, 0), (D - 2, 128), (D - 1, 0)] + ([(0, 9), (3, 9), (6, 9)] if D > 7 else [])
        t["plane_by_plane"] = [(z, 64 + z) for z in range(D - 1)]                  # z0 = the held one plus 1, every time
    return {k: np.array(v, np.int32).reshape(-1, 2) for k, v in t.items()}


class _Dev:
    """`n` bytes on the device `off` bytes into an aligned allocation between guards: a copy of `data`, or `fill`."""

    def __init__(self, n, off, fill, data=None):
        self.n, self.off, self.fill = n, off, fill
        self.t = torch.full((n + off + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 256 == 0
        if data is not None:
            self.t[GUARD + off:GUARD + off + n] = torch.from_numpy(np.ascontiguousarray(data).reshape(-1).copy()).cuda()
        self.ptr = self.t.data_ptr() + GUARD + off

    def body(self):
        """The n bytes, after the guards were found untouched."""
        got, lo = self.t.cpu().numpy(), GUARD + self.off
        assert (got[:lo] == self.fill).all() and (got[lo + self.n:] == self.fill).all()
        return got[lo:lo + self.n]


def _call(src, dims, sz0, VZ, dst, OD, oz0, table, nearest, dev_table=None):
    """One tem_u8_resample_z call; returns its code.  The device's copy of the table is `dev_table` where given."""
    L, lib, stream = _env()
    host = np.ascontiguousarray(table, np.int32)
    devt = torch.from_numpy(np.ascontiguousarray(host if dev_table is None else dev_table, np.int32)).cuda()
    rc = lib.tem_u8_resample_z(src.ptr, *dims, sz0, VZ, dst.ptr, OD, oz0, host.shape[0], host.ctypes.data,
                               devt.data_ptr(), int(nearest), stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("shape", BLOCKS, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_reference(shape):
    """Every table, blended and nearest, at byte offsets 0...3 of src and of dst independently."""
    L = _env()[0]
    D, H, W = shape
    vol = _data(shape)
    srcs = [_Dev(vol.size, off, FILL, vol) for off in range(4)]
    for name, table in _tables(D).items():
        NZ = table.shape[0]
        for nearest in (False, True):
            want = ZR.resample(vol, table, nearest).reshape(-1)
            if name == "identity":
                assert np.array_equal(want, vol.reshape(-1))                        # identity taps reproduce the source
            for soff in range(4):
                for doff in range(4):
                    dst = _Dev(NZ * H * W, doff, DFILL)
                    L.check(_call(srcs[soff], shape, 0, D, dst, NZ, 0, table, nearest), "tem_u8_resample_z")
                    got = dst.body()
                    assert np.array_equal(got, want), (name, nearest, soff, doff, np.flatnonzero(got != want)[:5])
    for s in srcs:
        assert np.array_equal(s.body(), vol.reshape(-1))


def test_tables_cover_what_they_claim():
    t = _tables(9)
    assert sorted(t["every_weight"][:256, 1].tolist()) == list(range(256))
    assert (np.diff(t["jumps"][:, 0]) >= 2).any() and (np.diff(t["non_monotone"][:, 0]) < 0).any()
    assert (np.diff(t["plane_by_plane"][:, 0]) == 1).all() and (t["plane_by_plane"][:, 1] > 0).all()
    vol = _data((3, 5, 7))
    got = ZR.resample(vol, t["every_weight"])                                       # the blend's extremes, by hand
    assert got[255, 0, 0] == (1 * 0 + 255 * 255 + 128) >> 8 == 254 and got[128, 0, 1] == (128 * 255 + 128) >> 8 == 128
    assert got[1, 0, 2] == (255 * 254 + 255 + 128) >> 8 == 254 and got[0, 0, 1] == 255
    near = ZR.resample(vol, t["every_weight"], True)
    assert np.array_equal(near[127], vol[0]) and np.array_equal(near[128], vol[1])


def test_sub_blocks_of_a_volume_and_of_the_output():
    """A source block that starts at sz0 > 0 and holds only the hull of the taps, an output block at oz0 > 0; the tap of
    weight 0 above the block's last plane need not lie in it."""
    L = _env()[0]
    VZ, H, W = 12, 33, 70
    vol = _data((VZ, H, W))
    table = np.array([(0, 0), (0, 200), (3, 9), (4, 100), (5, 255), (6, 0), (6, 0), (8, 31), (10, 128), (11, 0), (11, 0)],
                     np.int32)
    for nearest in (False, True):
        want = ZR.resample(vol, table, nearest)
        for (o0, o1), (s0, s1) in (((2, 6), (3, 7)), ((2, 7), (3, 7)), ((5, 7), (6, 7)), ((7, 11), (8, 12)),
                                   ((0, 11), (0, 12)), ((1, 2), (0, 2)), ((9, 11), (11, 12))):
            for soff, doff in ((0, 0), (1, 3), (2, 1), (3, 2)):
                src = _Dev((s1 - s0) * H * W, soff, FILL, vol[s0:s1])
                dst = _Dev((o1 - o0) * H * W, doff, DFILL)
                L.check(_call(src, (s1 - s0, H, W), s0, VZ, dst, o1 - o0, o0, table, nearest), "tem_u8_resample_z")
                assert np.array_equal(dst.body(), want[o0:o1].reshape(-1)), (nearest, o0, o1, s0, s1, soff, doff)
                assert np.array_equal(src.body(), vol[s0:s1].reshape(-1))


def test_a_large_plane_and_long_runs():
    """More than one workgroup per plane, runs of several output planes, a plane that ends inside a piece."""
    L = _env()[0]
    shape = (6, 301, 1731)
    assert (shape[1] * shape[2]) % 16 == 7
    vol = _data(shape)
    Q = np.concatenate([[0], np.cumsum(np.random.default_rng(4).integers(9000, 20000, 5) * 64)])
    table = ZR.taps(Q, 90)                                                          # dense outputs, then the last section
    assert table.shape[0] == 90 and (table[:, 1] > 0).sum() > 10 and table[-1].tolist() == [5, 0]
    want = ZR.resample(vol, table).reshape(-1)
    for soff, doff in ((0, 0), (3, 1)):
        src, dst = _Dev(vol.size, soff, FILL, vol), _Dev(want.size, doff, DFILL)
        L.check(_call(src, shape, 0, 6, dst, 90, 0, table, False), "tem_u8_resample_z")
        assert np.array_equal(dst.body(), want), (soff, doff)


def test_kernel_refuses_bad_arguments():
    """TEM_EINVAL from the host-side checks, nothing launched: dst keeps its fill."""
    L = _env()[0]
    VZ, NZ, H, W = 6, 5, 4, 8
    vol = _data((VZ, H, W))
    src, dst = _Dev(3 * H * W, 0, FILL, vol[1:4]), _Dev(2 * H * W, 0, DFILL)
    table = np.array([(0, 0), (1, 128), (2, 255), (3, 0), (5, 0)], np.int32)        # outputs 1...3 lie in sections 1...3
    good = dict(dims=(3, H, W), sz0=1, VZ=VZ, OD=2, oz0=1, table=table, nearest=0)

    def call(**kw):
        a = dict(good, **kw)
        return _call(a.get("src", src), a["dims"], a["sz0"], a["VZ"], a.get("dst", dst), a["OD"], a["oz0"], a["table"],
                     a["nearest"])

    class _Null:
        ptr = None

    def tab(j, z0, w):
        t = table.copy()
        t[j] = (z0, w)
        return t

    for kw in (dict(src=_Null), dict(dst=_Null), dict(dims=(0, H, W)), dict(dims=(3, 0, W)), dict(dims=(3, H, 0)),
               dict(OD=0), dict(VZ=0), dict(sz0=-1), dict(sz0=4), dict(oz0=-1), dict(oz0=4), dict(OD=5), dict(nearest=2),
               dict(nearest=-1), dict(table=tab(1, -1, 0)), dict(table=tab(1, 6, 0)), dict(table=tab(2, 2, 256)),
               dict(table=tab(2, 2, -1)), dict(table=tab(1, 0, 0)), dict(table=tab(2, 3, 1)), dict(table=tab(2, 4, 0)),
               dict(oz0=2, OD=3), dict(oz0=0, OD=2)):
        assert call(**kw) == L.TEM_EINVAL, kw
    Lb, lib, stream = _env()
    devt = torch.from_numpy(table).cuda()
    assert lib.tem_u8_resample_z(src.ptr, 3, H, W, 1, VZ, dst.ptr, 2, 1, NZ, None, devt.data_ptr(), 0, stream) == L.TEM_EINVAL
    assert lib.tem_u8_resample_z(src.ptr, 3, H, W, 1, VZ, dst.ptr, 2, 1, NZ, table.ctypes.data, None, 0, stream) == L.TEM_EINVAL
    assert (dst.body() == DFILL).all()
    # rows of the table outside the block's are not looked at; a tap of weight 0 above the block is no tap
    assert call(table=tab(4, 99, 999)) == 0 and call(table=tab(2, 3, 0)) == 0
    assert call(oz0=1, OD=2) == 0
    assert np.array_equal(dst.body(), ZR.resample(vol, table)[1:3].reshape(-1))
    # a device table that disagrees with the host's: wrong bytes, clamped into the block, never a fault
    wild = np.array([(0, 0), (-5, 300), (1 << 30, -7), (3, 0), (5, 0)], np.int32)
    assert call(table=table) == 0
    assert _call(src, (3, H, W), 1, VZ, dst, 2, 1, table, 0, dev_table=wild) == 0
    clamped = np.array([(0, 0), (1, 255), (3, 0), (3, 0), (5, 0)], np.int32)        # z0 into [1, 3], w into [0, 255]
    assert np.array_equal(dst.body(), ZR.resample(vol, clamped)[1:3].reshape(-1))
    assert np.array_equal(src.body(), vol[1:4].reshape(-1))


# ------------------------------------------------------------------------------------------------ volume_resample_z
Z, Y, X = ZR.FIX_SHAPE


@pytest.fixture(scope="module")
def vmap(tmp_path_factory):
    path = tmp_path_factory.mktemp("resamplez") / "vol.u8"
    m = np.memmap(path, np.uint8, "w+", shape=ZR.FIX_SHAPE)
    m[...] = ZR.fixture().volume
    m.flush()
    return np.memmap(path, np.uint8, "r", shape=ZR.FIX_SHAPE)


@functools.lru_cache(maxsize=None)
def _planted():
    """The planted positions, their reference table and the reference output."""
    fx = ZR.fixture()
    table = ZR.taps(ZR.quantize(fx.positions))
    want = ZR.resample(fx.volume, table)
    want.setflags(write=False)
    return fx.positions, table, want


BUDGETS = {"whole": 1 << 30, "sections": 7 * Y * X, "rows": 3 * 20 * X}


@pytest.mark.parametrize("budget", list(BUDGETS), ids=list(BUDGETS))
def test_volume_resample_z_equals_the_reference_however_it_is_cut(vmap, budget):
    from transfer_em_amd.utils import resample_z_chunks, volume_resample_z
    P, table, want = _planted()
    st = {}
    got, counts = _counted(lambda: volume_resample_z(vmap, P, chunk_bytes=BUDGETS[budget], stats=st))
    assert got.dtype == np.uint8 and got.shape == ZR.FIX_SHAPE and np.array_equal(got, want)
    chunks = resample_z_chunks(((0, Z), (0, Y), (0, X)), ZR.FIX_SHAPE, table, BUDGETS[budget])
    assert st["chunks"] == len(chunks) == counts["tem_u8_resample_z"] and st["read_s"] >= 0 and st["write_s"] >= 0
    assert {"whole": len(chunks) == 1, "sections": 1 < len(chunks) <= Z and all(o[1] == (0, Y) for o, _ in chunks),
            "rows": len(chunks) > Z and all(o[1] != (0, Y) for o, _ in chunks)}[budget]
    assert np.array_equal(np.asarray(vmap), ZR.fixture().volume)                    # the input: read only


def test_volume_resample_z_roi_ranks_out_nz_and_a_mask(vmap, tmp_path):
    from transfer_em_amd.utils import quantize_positions, volume_resample_z
    fx = ZR.fixture()
    P, table, want = _planted()
    roi = volume_resample_z(vmap, P, start=(8, 5, 3), size=(60, 41, 30), chunk_bytes=4 * 41 * 60)
    assert np.array_equal(roi, want[3:33, 5:46, 8:68])
    assert np.array_equal(roi, ZR.resample(fx.volume, table, box=((3, 33), (5, 46), (8, 68))))
    out = np.memmap(tmp_path / "out.u8", np.uint8, "w+", shape=ZR.FIX_SHAPE)        # two ranks write one output
    for r in (1, 0):
        assert volume_resample_z(vmap, quantize_positions(P), out=out, chunk_bytes=5 * Y * X, rank=r, world_size=2) is out
        assert np.array_equal(np.asarray(out), want) == (r == 0)
    more = volume_resample_z(fx.volume, P, nz=Z + 3)                                # past the end: the last section
    assert np.array_equal(more[:Z], want) and all(np.array_equal(more[Z + k], fx.volume[-1]) for k in range(3))
    mask = volume_resample_z(fx.mask, P, nearest=True, chunk_bytes=6 * Y * X)       # nearest moves a mask
    assert np.array_equal(mask, ZR.resample(fx.mask, table, nearest=True)) and set(np.unique(mask)) == {0, 255}
    assert not np.array_equal(mask, fx.mask)
    blended = volume_resample_z(fx.mask, P)
    assert len(np.unique(blended)) > 2                                              # which the blend would smear


def test_the_chain_meets_the_fixtures_conditions(vmap):
    """section_lag_sums -> section_spacing -> volume_resample_z on the device: the spacing error and the RMSE of the
    fixture's conditions, with the reference's values."""
    from transfer_em_amd.utils import quantize_positions, resample_z_taps, section_lag_sums, section_spacing, volume_resample_z
    fx = ZR.fixture()
    P_ref, _, e_ref, even_ref, raw_ref, res_ref = ZR.check_fixture()
    sp = section_spacing(section_lag_sums(vmap, ZR.FIX_TILE, ZR.FIX_LAGS, chunk_bytes=9 * Y * X), fx.skip)
    assert sp.clipped == [] and sp.unresolved == [] and np.abs(sp.positions - P_ref).max() < 1e-9
    table = resample_z_taps(quantize_positions(sp.positions))
    assert np.array_equal(table, ZR.taps(ZR.quantize(P_ref)))
    got = volume_resample_z(vmap, sp.positions, chunk_bytes=9 * Y * X)
    e_est, e_even, r_raw, r_res = ZR.conditions(sp.positions, got, table)
    print(f"spacing error {e_est:.4f} (even spacing {e_even:.4f}), RMSE raw {r_raw:.4f} resampled {r_res:.4f}")
    assert e_even >= 1.0 and e_est <= 0.25 and r_res <= 0.5 * r_raw
    assert abs(e_est - e_ref) < 1e-9 and e_even == even_ref and r_raw == raw_ref and r_res == res_ref
