"""Per-voxel spread of the self-ensemble as a uint8 map (spread= of predict_cube / predict_volume).

The map is pinned so that numpy reproduces every byte: moments about the first member, every operation one rounded fp32
operation in a fixed order (include/tem_hip.h).  So the kernels are held to a numpy float32 restatement bit for bit,
and, where the moments come from real members, to the float64 np.std form within 1.  End to end the reference is rebuilt
from the generator's own member outputs, as test_gpu_ensemble.py rebuilds the mean."""
import os

import numpy as np
import pytest
import torch

from util import scaled_params

pytestmark = pytest.mark.gpu

MS_X, MS_Y = (0.02, 0.58), (-0.1, 0.4)
ID3 = ((0, 1, 2), (0, 0, 0))
f32 = np.float32


# ------------------------------------------------------------------------------------------- the numpy restatement
def ref_moments(members):
    """(ref, s1, s2) of the members (float32 arrays, in the ensemble's order), op by op."""
    r = members[0]
    s1, s2 = np.zeros_like(r), np.zeros_like(r)
    for y in members[1:]:
        d = y - r
        s1 = s1 + d
        p = d * d
        s2 = s2 + p
    assert s1.dtype == s2.dtype == np.float32
    return r, s1, s2


def ref_finish(s1, s2, k, std_y, gain):
    k = f32(k)
    t = (s1 * s1) / k
    v = np.maximum(s2 - t, f32(0)) / k
    sd = np.sqrt(v)
    x = np.minimum(((sd * f32(abs(std_y))) * f32(127.5)) * f32(gain), f32(255))
    assert x.dtype == np.float32
    return np.rint(x).astype(np.uint8)


def ref_float64(members, std_y, gain):
    """The definition in float64: rint(min(255, gain 127.5 |std_y| np.std(members)))."""
    sd = np.std(np.stack([m.astype(np.float64) for m in members]), axis=0)
    return np.rint(np.minimum(255.0, float(f32(gain)) * 127.5 * abs(float(f32(std_y))) * sd)).astype(np.uint8)


def within_one(a, b):
    return np.abs(a.astype(np.int16) - b.astype(np.int16)).max() <= 1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def Tinv(v, s, lead=0):
    perm, flips = s
    v = np.flip(v, [lead + a for a, f in enumerate(flips) if f])
    return np.transpose(v, tuple(range(lead)) + tuple(lead + int(p) for p in np.argsort(perm)))


def _syms(is3d, kind="all"):
    """3-axis members with int flags, as the C ABI takes them."""
    from transfer_em_amd.utils import symmetries
    if is3d:
        return [(tuple(p), tuple(int(f) for f in fl)) for p, fl in symmetries(True, kind)]
    return [((0, p[0] + 1, p[1] + 1), (0, int(fl[0]), int(fl[1]))) for p, fl in symmetries(False, kind)]


def _env():
    from transfer_em_amd import _lib as L
    from transfer_em_amd import hip_ops as H
    return L, H.require_gpu(), H.current_stream()


def _tile_shape(n, edge, is3d):
    return (n, edge, edge, edge) if is3d else (n, 1, edge, edge)


def _nan(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


# --------------------------------------------------------------------------------------------------- the accumulate
def _accum(y, s, acc, first, divisor, is3d, moments=None):
    L, lib, stream = _env()
    name = ("tem_f32_tiles_sym_accum" if is3d else "tem_f32_tiles2d_sym_accum") + ("_spread" if moments else "")
    mom = tuple(m.data_ptr() for m in moments) if moments else ()
    L.check(getattr(lib, name)(y.data_ptr(), y.shape[0], y.shape[2], *s[0], *s[1], acc.data_ptr(), int(first), divisor,
                               *mom, stream), name)


# yedge 13 and 40: one ragged LDS window; 70: a full 64-wide window plus a remainder of 6 (every fifth symmetry)
@pytest.mark.parametrize("yedge, step", [(13, 1), (40, 1), (70, 5)])
@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
def test_accumulate_three_members_equals_numpy(is3d, yedge, step):
    """3 tiles, 3 members: first, middle, last with divisor 3, for every symmetry in every one of the three roles.  All
    four destinations start as NaN: `first` reads none of them."""
    syms = _syms(is3d)
    k, n = len(syms), 3
    rng = np.random.default_rng(yedge)
    ys = [rng.standard_normal(_tile_shape(n, yedge, is3d)).astype(np.float32) * f32(3) + f32(j) for j in range(3)]
    dys = [torch.from_numpy(y).cuda() for y in ys]
    for i in range(0, k, step):
        members = [syms[i], syms[(i + 7) % k], syms[(i + 13) % k]]
        plain, acc = _nan(dys[0].shape), _nan(dys[0].shape)
        mom = [_nan(dys[0].shape) for _ in range(3)]
        for j, (first, div) in enumerate([(True, 1), (False, 1), (False, 3)]):
            _accum(dys[j], members[j], plain, first, div, is3d)
            _accum(dys[j], members[j], acc, first, div, is3d, mom)
        back = [np.ascontiguousarray(Tinv(ys[j], members[j], 1)) for j in range(3)]   # a 2-D tile is [1, E, E]: z stays
        want = ((back[0] + back[1]) + back[2]) / f32(3)
        got = acc.cpu().numpy()
        assert np.array_equal(bits(got), bits(plain.cpu().numpy())), members
        assert np.array_equal(bits(got), bits(want)), members
        for name, g, w in zip(("ref", "s1", "s2"), mom, ref_moments(back)):
            assert np.array_equal(bits(g.cpu().numpy()), bits(w)), (name, members)


@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
def test_accumulate_first_member_resets_the_moments(is3d):
    y = torch.from_numpy(np.random.default_rng(3).standard_normal(_tile_shape(2, 21, is3d)).astype(np.float32)).cuda()
    for s in _syms(is3d)[:: 7 if is3d else 3]:
        acc, mom = _nan(y.shape), [_nan(y.shape) for _ in range(3)]
        _accum(y, s, acc, True, 1, is3d, mom)
        want = np.ascontiguousarray(Tinv(y.cpu().numpy(), s, 1))
        assert np.array_equal(bits(acc.cpu().numpy()), bits(want)), s
        assert np.array_equal(bits(mom[0].cpu().numpy()), bits(want)), s
        assert not mom[1].cpu().numpy().view(np.uint32).any() and not mom[2].cpu().numpy().view(np.uint32).any(), s


# ---------------------------------------------------------------------------------------------- the finishing scatter
# members ~ N(offset, scale): (scale, offset, gain).  std_y = 0.4 makes one unit of the members 51 grey levels, so the
# gains put the bulk of each map at 20 to 50 grey steps; scale 3 at gain 0.5 also saturates a share of the voxels
PAIRS = [(1.0, 0.0, 1.0), (0.05, 2.5, 8.0), (3.0, 0.0, 0.5), (1e-3, 100.0, 1000.0)]
# (s1, s2) by hand: s2 - s1^2 / k < 0 for every count used (-> 0), an exact zero, one that saturates
HAND = [(f32(4.0), f32(1.9)), (f32(0.0), f32(0.0)), (f32(0.0), f32(1e6))]
HAND_U8 = [0, 0, 255]


def _scatter_case(is3d, tpad):
    """(yedge, the two tiles' (z, y, x) index, the destination's shape)"""
    if is3d:
        return 21, [(1, 2, 3), (5, 11, 30)], (27, 33, 53)
    # od 131 / 127: rows end in a group of fewer than 4; tile 0 lands on odd addresses, tile 1 on 4-byte boundaries
    return 131, [(0, 2, 3), (2, 5, 160)], (3, 140, 300)


@pytest.mark.parametrize("count", [1, 2, 3, 8])
@pytest.mark.parametrize("tpad", [0, 2])
@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
def test_finishing_scatter_equals_numpy(is3d, tpad, count):
    L, lib, stream = _env()
    yedge, index, oshape = _scatter_case(is3d, tpad)
    od, shape = yedge - 2 * tpad, _tile_shape(2, yedge, is3d)
    name = "tem_f32_tiles_spread_to_u8" if is3d else "tem_f32_tiles2d_spread_to_u8"
    didx = torch.tensor(index, dtype=torch.int32).cuda()
    hand = [(0, 0 if not is3d else tpad + 1, tpad + 1, tpad + 1 + j) for j in range(len(HAND))]   # interior of tile 0
    for scale, offset, gain in PAIRS:
        rng = np.random.default_rng(count * 7 + tpad)
        members = [(rng.standard_normal(shape) * scale + offset).astype(np.float32) for _ in range(count)]
        _, s1, s2 = ref_moments(members)
        for at, (a, b) in zip(hand, HAND):
            s1[at], s2[at] = a, b
        out = torch.full(oshape, 0xA5, dtype=torch.uint8, device="cuda")
        d1, d2 = torch.from_numpy(s1).cuda(), torch.from_numpy(s2).cuda()
        L.check(getattr(lib, name)(d1.data_ptr(), d2.data_ptr(), 2, yedge, tpad, didx.data_ptr(), out.data_ptr(), *oshape,
                                   count, MS_Y[1], gain, stream), name)
        got = out.cpu().numpy()
        want = np.full(oshape, 0xA5, np.uint8)
        want64 = want.copy()
        fin, fin64 = ref_finish(s1, s2, count, MS_Y[1], gain), ref_float64(members, MS_Y[1], gain)
        inner = slice(tpad, yedge - tpad)
        real = np.zeros(oshape, bool)                                        # voxels whose moments come from members
        for t, (iz, iy, ix) in enumerate(index):
            box = (slice(iz, iz + (od if is3d else 1)), slice(iy, iy + od), slice(ix, ix + od))
            zin = inner if is3d else slice(None)
            want[box], want64[box], real[box] = fin[t][zin, inner, inner], fin64[t][zin, inner, inner], True
        for (t, z, y, x), u8 in zip(hand, HAND_U8):
            p = (index[t][0] + z - (tpad if is3d else 0), index[t][1] + y - tpad, index[t][2] + x - tpad)
            real[p] = False
            assert want[p] == u8, (p, want[p], u8)
        assert real.sum() == 2 * od ** (3 if is3d else 2) - len(HAND)
        assert np.array_equal(got, want), (scale, offset, gain, np.argwhere(got != want)[:5])
        assert (got[~real & (want == 0xA5)] == 0xA5).all()                   # nothing outside the interiors is touched
        assert within_one(got[real], want64[real]), (scale, offset, gain)
        if count > 1:                                                        # the maps are maps, not constants
            assert len(np.unique(got[real])) > 15, (scale, offset, gain)
        else:
            assert not got[real].any()


# ----------------------------------------------------------------------------------------------------- the arguments
def test_entry_points_refuse_bad_arguments():
    L, lib, stream = _env()
    n = 6 ** 3
    buf = torch.zeros((6 * n,), dtype=torch.float32, device="cuda")
    ptr = [buf.data_ptr() + 4 * n * i for i in range(6)]                     # six disjoint arrays of one 6^3 tile
    idx = torch.zeros((1, 3), dtype=torch.int32, device="cuda")
    out = torch.zeros((6, 6, 6), dtype=torch.uint8, device="cuda")
    bad_syms = [((0, 0, 2), (0, 0, 0)), ((0, 1, 3), (0, 0, 0)), ((-1, 1, 2), (0, 0, 0)), ((1, 1, 1), (0, 0, 0)),
                ((0, 1, 2), (0, 2, 0)), ((0, 1, 2), (0, 0, -1))]
    z_syms = [((1, 0, 2), (0, 0, 0)), ((2, 1, 0), (0, 0, 0)), ((0, 1, 2), (1, 0, 0)), ((1, 2, 0), (0, 1, 1))]
    for is3d in (True, False):
        sfx = "" if is3d else "2d"
        afn, ffn = getattr(lib, f"tem_f32_tiles{sfx}_sym_accum_spread"), getattr(lib, f"tem_f32_tiles{sfx}_spread_to_u8")
        per = n if is3d else 36                                              # elements of one tile

        def accum(p=ptr[:5], sym=ID3, first=1, divisor=1, ntile=1, yedge=6):
            return afn(p[0], ntile, yedge, *sym[0], *sym[1], p[1], first, divisor, p[2], p[3], p[4], stream)

        def finish(s1=ptr[0], s2=ptr[1], ntile=1, yedge=6, tpad=1, index=idx.data_ptr(), o=out.data_ptr(), dims=(6, 6, 6),
                   count=3, gain=8.0):
            return ffn(s1, s2, ntile, yedge, tpad, index, o, *dims, count, 0.4, gain, stream)
        assert accum() == L.TEM_OK and accum(first=0, divisor=3) == L.TEM_OK
        assert accum(sym=((0, 2, 1), (0, 1, 1))) == L.TEM_OK
        assert accum(first=2) == L.TEM_EINVAL and accum(divisor=0) == L.TEM_EINVAL and accum(yedge=0) == L.TEM_EINVAL
        assert accum(ntile=-1) == L.TEM_EINVAL and accum(yedge=46341) == L.TEM_EINVAL
        for i in range(5):                                                   # a null pointer, each of the five
            assert accum(p=ptr[:i] + [0] + ptr[i + 1:5]) == L.TEM_EINVAL, i
            assert accum(p=ptr[:i] + [0] + ptr[i + 1:5], ntile=0) == L.TEM_EINVAL, i
        for i in range(5):                                                   # any two of y, acc, ref, s1, s2 alias
            for j in range(i):
                p = list(ptr[:5])
                p[i] = p[j]
                assert accum(p=p) == L.TEM_EINVAL, (i, j)
                p[i] = p[j] + 4 * (per - 1)                                  # ... or overlap in one element
                assert accum(p=p) == L.TEM_EINVAL, (i, j)
                p[i] = p[j] + 4 * per                                        # back to back is fine
                if all(abs(p[i] - q) >= 4 * per for m, q in enumerate(p) if m != i):
                    assert accum(p=p) == L.TEM_OK, (i, j)
        for s in bad_syms:
            assert accum(sym=s) == L.TEM_EINVAL, s
        for s in z_syms:                                                     # fine for a cube, refused for a section
            assert accum(sym=s) == (L.TEM_OK if is3d else L.TEM_EINVAL), s
        assert finish() == L.TEM_OK and finish(count=1) == L.TEM_OK and finish(tpad=0) == L.TEM_OK
        assert finish(ntile=0) == L.TEM_OK
        assert finish(count=0) == L.TEM_EINVAL and finish(count=-3) == L.TEM_EINVAL
        for g in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
            assert finish(gain=g) == L.TEM_EINVAL, g
        assert finish(s1=0) == L.TEM_EINVAL and finish(s2=0) == L.TEM_EINVAL
        assert finish(index=0) == L.TEM_EINVAL and finish(o=0) == L.TEM_EINVAL
        assert finish(ntile=-1) == L.TEM_EINVAL and finish(yedge=0) == L.TEM_EINVAL
        assert finish(tpad=-1) == L.TEM_EINVAL and finish(tpad=3) == L.TEM_EINVAL
        for dims in ((0, 6, 6), (6, 0, 6), (6, 6, 0)):
            assert finish(dims=dims) == L.TEM_EINVAL, dims
        if not is3d:
            assert finish(yedge=46341) == L.TEM_EINVAL
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------- end to end
# the 74 model: tiles of 36 + a halo of 19 (tpad 2); the volumes of test_gpu_ensemble.py
VOL, START, SIZE = (50, 90, 61), (-20, -15, -10), (90, 100, 80)            # (z,y,x); (x,y,z): 27 tiles, past all six faces
VOL2, START2, SIZE2 = (3, 50, 45), (-20, -15, -1), (90, 100, 5)             # 2-D: sections -1 and 3 lie outside
CUBE = 72
ENS2 = [((0, 1), (False, False)), ((1, 0), (False, True)), ((0, 2, 1), (0, 1, 1))]    # both spellings of a 2-D member
ENS2_ABI = [ID3, ((0, 2, 1), (0, 0, 1)), ((0, 2, 1), (0, 1, 1))]


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
    return _model(tmp_path_factory.mktemp("spr3"), "spr3", True)


@pytest.fixture(scope="module")
def model2(tmp_path_factory):
    return _model(tmp_path_factory.mktemp("spr2"), "spr2", False)


@pytest.fixture(scope="module")
def ragged3():
    return np.random.default_rng(1).integers(0, 256, VOL, dtype=np.uint8)


@pytest.fixture(scope="module")
def ragged2():
    return np.random.default_rng(2).integers(0, 256, VOL2, dtype=np.uint8)


@pytest.fixture(scope="module")
def cube3():
    return np.random.default_rng(3).integers(0, 256, (CUBE,) * 3, dtype=np.uint8)


class Rebuilt:
    """predict_cube(..., ensemble=syms, spread=S) rebuilt step by step (a copy of test_gpu_ensemble's _manual_mean):
    per member the sym gather, the generator plan and Tinv; then the numpy restatement of the mean and of the moments.
    mean() goes through the existing scatter kernel; maps(gain) are stitched in numpy: (float32 form, float64 form)."""

    def __init__(self, model, vol, start, size, syms, mode, is3d):
        from transfer_em_amd import _lib as L
        from transfer_em_amd.utils import tile_plan, tile_plan_2d
        _, lib, stream = _env()
        self.od, buf, self.tpad, rois, self.index = (tile_plan if is3d else tile_plan_2d)(start, size, model.outdimsize,
                                                                                          model.buffer)
        edge, n = self.od + 2 * buf, len(rois)
        self.is3d, self.size, self.k = is3d, size, len(syms)
        dv = torch.from_numpy(np.ascontiguousarray(vol)).cuda()
        do = torch.tensor([(r[2], r[1], r[0]) for r in rois], dtype=torch.int32).cuda()
        lo, shape = ((0, 0, 0), vol.shape)
        mode_id = {"zeros": 0, "reflect": L.TEM_BOUNDARY_REFLECT, "edge": L.TEM_BOUNDARY_EDGE}[mode]
        name = f"tem_u8_tiles{'' if is3d else '2d'}_to_f32_std_sym"
        plan = model.generator_g.plan(_tile_shape(n, edge, is3d) + (1,))
        self.members = []
        for s in syms:
            L.check(getattr(lib, name)(dv.data_ptr(), *vol.shape, *lo, *shape, mode_id, do.data_ptr(), n, edge, *s[0],
                                       *s[1], plan.x.data_ptr(), MS_X[0], MS_X[1], stream), name)
            y = plan.run().clone().cpu().numpy()[..., 0]                     # [n, D, ye, ye]
            self.members.append(np.ascontiguousarray(Tinv(y, s, 1)))
        _, self.s1, self.s2 = ref_moments(self.members)
        rnd = lambda v: -(-v // self.od) * self.od
        self.oshape = (rnd(size[2]) if is3d else size[2], rnd(size[1]), rnd(size[0]))

    def _crop(self, a):
        return a[:self.size[2], :self.size[1], :self.size[0]]

    def mean(self):
        L, lib, stream = _env()
        acc = self.members[0]
        for m in self.members[1:]:
            acc = acc + m
        acc = acc / f32(self.k) if self.k > 1 else acc
        assert acc.dtype == np.float32 and acc.shape[2] - 2 * self.tpad == self.od
        out = torch.zeros(self.oshape, dtype=torch.uint8, device="cuda")
        dacc = torch.from_numpy(np.ascontiguousarray(acc)).cuda()
        idx = torch.tensor([[i[2], i[1], i[0]] for i in self.index], dtype=torch.int32).cuda()
        name = "tem_f32_tiles_unstd_to_u8" if self.is3d else "tem_f32_tiles2d_unstd_to_u8"
        L.check(getattr(lib, name)(dacc.data_ptr(), len(self.index), acc.shape[2], self.tpad, idx.data_ptr(),
                                   out.data_ptr(), *self.oshape, MS_Y[0], MS_Y[1], stream), name)
        return self._crop(out.cpu().numpy())

    def _stitch(self, tiles):
        out, od, tp = np.zeros(self.oshape, np.uint8), self.od, self.tpad
        inner = slice(tp, tp + od)
        for t, (ix, iy, iz) in enumerate(self.index):
            if self.is3d:
                out[iz:iz + od, iy:iy + od, ix:ix + od] = tiles[t][inner, inner, inner]
            else:
                out[iz, iy:iy + od, ix:ix + od] = tiles[t][0, inner, inner]
        return self._crop(out)

    def map32(self, gain):
        return self._stitch(ref_finish(self.s1, self.s2, self.k, MS_Y[1], gain))

    def maps(self, gain):
        return self.map32(gain), self._stitch(ref_float64(self.members, MS_Y[1], gain))

    def gain(self):
        """The degeneracy guard, computed from the reference alone: the largest gain 1, 1/2, 1/4, ... at which under 1 %
        of the reference map is 255; the map then has more than 50 distinct values."""
        g = 1.0
        while (self.map32(g) == 255).mean() >= 0.01 and g > 2.0 ** -10:
            g /= 2
        ref = self.map32(g)
        print(f"spread reference: gain {g}, {len(np.unique(ref))} distinct values, max {ref.max()}, "
              f"mean {ref.mean():.1f}, share at 255 {(ref == 255).mean():.4f}")
        assert len(np.unique(ref)) > 50 and (ref == 255).mean() < 0.01
        return g


def _check_against(rb, got_map, gain):
    want, want64 = rb.maps(gain)
    print(f"map vs float32 reference: {(got_map != want).sum()} voxels differ; vs float64: max "
          f"{np.abs(got_map.astype(np.int16) - want64.astype(np.int16)).max()}, {(got_map != want64).sum()} differ")
    assert np.array_equal(got_map, want)
    assert within_one(got_map, want64)


@pytest.mark.parametrize("case", ["flips on the cube", "all 48 on one tile"])
def test_map_equals_the_rebuilt_reference_3d(model3, cube3, ragged3, case):
    from transfer_em_amd.utils import predict_cube
    if case == "flips on the cube":
        vol, start, size, ens, mode = cube3, (0, 0, 0), (CUBE,) * 3, "flips", "zeros"
    else:
        vol, start, size, ens, mode = ragged3, (3, 30, 8), (36, 36, 36), "all", "reflect"   # past the near z and x faces
    rb = Rebuilt(model3, vol, start, size, _syms(True, ens), mode, True)
    gain = rb.gain()
    plain = predict_cube(vol, start, size, model3, MS_X, MS_Y, boundary=mode, ensemble=ens)
    assert np.array_equal(plain, rb.mean())
    for tb in (None, 3):
        S, st = np.full(plain.shape, 0xA5, np.uint8), {}
        got = predict_cube(vol, start, size, model3, MS_X, MS_Y, boundary=mode, ensemble=ens, tile_batch=tb, spread=S,
                           spread_gain=gain, stats=st)
        assert np.array_equal(got, plain)                                    # the prediction does not notice
        _check_against(rb, S, gain)
        assert st["spread_histogram"].dtype == np.int64
        assert np.array_equal(st["spread_histogram"], np.bincount(S.ravel(), minlength=256))
        assert "histogram" not in st
    S2 = np.zeros(plain.shape, np.uint8)                                     # twice the gain: another map, same moments
    predict_cube(vol, start, size, model3, MS_X, MS_Y, boundary=mode, ensemble=ens, spread=S2, spread_gain=2 * gain)
    assert np.array_equal(S2, rb.map32(2 * gain)) and not np.array_equal(S2, S)


def test_predict_volume_equals_predict_cube(model3, ragged3, tmp_path):
    """Chunks of 2 x 2 x 2 tiles over a 3 x 3 x 3 grid (tails on every axis, past all six faces), batches of 3 tiles,
    two ranks into one shared `out` and one shared map, boundary reflect; with a pyramid; and the saved-model form."""
    from transfer_em_amd import utils
    rb = Rebuilt(model3, ragged3, START, SIZE, _syms(True, "flips"), "reflect", True)
    gain = rb.gain()
    kw = dict(boundary="reflect", ensemble="flips")
    S_ref, st_ref = np.zeros(SIZE[::-1], np.uint8), {}
    ref = utils.predict_cube(ragged3, START, SIZE, model3, MS_X, MS_Y, spread=S_ref, spread_gain=gain, stats=st_ref,
                             histogram=True, **kw)
    _check_against(rb, S_ref, gain)
    assert np.array_equal(ref, utils.predict_cube(ragged3, START, SIZE, model3, MS_X, MS_Y, **kw))
    assert np.array_equal(st_ref["histogram"], np.bincount(ref.ravel(), minlength=256))
    assert np.array_equal(st_ref["spread_histogram"], np.bincount(S_ref.ravel(), minlength=256))
    out, S, hist = np.zeros(ref.shape, np.uint8), np.zeros(ref.shape, np.uint8), np.zeros(256, np.int64)
    for rank in range(2):
        st = {}
        utils.predict_volume(ragged3, START, SIZE, model3, MS_X, MS_Y, out=out, chunk_tiles=(2, 2, 2), tile_batch=3,
                             rank=rank, world_size=2, stats=st, spread=S, spread_gain=gain, **kw)
        assert st["chunks"] == 4 and st["spread_histogram"].sum() > 0
        hist += st["spread_histogram"]
        if rank == 0:
            assert not np.array_equal(S, S_ref)                              # the other rank's boxes are still empty
    assert np.array_equal(out, ref) and np.array_equal(S, S_ref)
    assert np.array_equal(hist, st_ref["spread_histogram"])
    pyr = utils.predict_volume(ragged3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(2, 2, 2), tile_batch=3, mips=1, **kw)
    S1 = np.zeros(ref.shape, np.uint8)
    got = utils.predict_volume(ragged3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(2, 2, 2), tile_batch=3, mips=1,
                               spread=S1, spread_gain=gain, **kw)
    assert len(got) == 2 and all(np.array_equal(a, b) for a, b in zip(got, pyr)) and np.array_equal(got[0], ref)
    assert np.array_equal(S1, S_ref)
    ckpt = model3.make_checkpoint(1)
    out_dir = str(tmp_path / "exported")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        utils.save_model(out_dir, ckpt, MS_X, MS_Y, size=74, is3d=True)
    finally:
        os.chdir(cwd)
    S2 = np.zeros(ref.shape, np.uint8)
    saved = utils.predict_volume_from_saved_model(ragged3, START, SIZE, out_dir, chunk_tiles=(2, 2, 2), tile_batch=3,
                                                  spread=S2, spread_gain=gain, **kw)
    assert np.array_equal(saved, ref) and np.array_equal(S2, S_ref)


def test_stack_and_single_image_2d(model2, ragged2):
    """A member list that mixes the 2-axis and the 3-axis spelling; the stack and the single-image form, each through
    predict_cube and predict_volume, against the rebuilt reference."""
    from transfer_em_amd.utils import predict_cube, predict_volume
    rb = Rebuilt(model2, ragged2, START2, SIZE2, ENS2_ABI, "reflect", False)
    gain = rb.gain()
    kw = dict(boundary="reflect", ensemble=ENS2)
    plain = predict_cube(ragged2, START2, SIZE2, model2, MS_X, MS_Y, **kw)
    assert np.array_equal(plain, rb.mean())
    S, st = np.zeros(plain.shape, np.uint8), {}
    assert np.array_equal(predict_cube(ragged2, START2, SIZE2, model2, MS_X, MS_Y, spread=S, spread_gain=gain, stats=st,
                                       **kw), plain)
    _check_against(rb, S, gain)
    assert np.array_equal(st["spread_histogram"], np.bincount(S.ravel(), minlength=256))
    Sv, stv = np.zeros(plain.shape, np.uint8), {}
    got = predict_volume(ragged2, START2, SIZE2, model2, MS_X, MS_Y, chunk_tiles=(2, 1, 2), tile_batch=5, spread=Sv,
                         spread_gain=gain, stats=stv, **kw)
    assert np.array_equal(got, plain) and np.array_equal(Sv, S)
    assert np.array_equal(stv["spread_histogram"], st["spread_histogram"])
    img, start, size = ragged2[1], START2[:2], SIZE2[:2]                     # the single-image forms
    rb1 = Rebuilt(model2, img[None], start + (0,), size + (1,), ENS2_ABI, "reflect", False)
    plain1 = predict_cube(img, start, size, model2, MS_X, MS_Y, **kw)
    assert plain1.shape == (100, 90) and np.array_equal(plain1, rb1.mean()[0])
    for fn in (predict_cube, predict_volume):
        S1, st1 = np.zeros(plain1.shape, np.uint8), {}
        assert np.array_equal(fn(img, start, size, model2, MS_X, MS_Y, spread=S1, spread_gain=gain, stats=st1, **kw), plain1)
        _check_against(rb1, S1[None], gain)
        assert np.array_equal(st1["spread_histogram"], np.bincount(S1.ravel(), minlength=256))


def test_one_member_gives_an_all_zero_map(model3, cube3):
    from transfer_em_amd.utils import predict_cube, predict_volume, symmetries
    start, size = (0, 0, 0), (CUBE,) * 3
    plain = predict_cube(cube3, start, size, model3, MS_X, MS_Y)
    for fn in (predict_cube, predict_volume):
        S, st = np.full(plain.shape, 0xA5, np.uint8), {}
        got = fn(cube3, start, size, model3, MS_X, MS_Y, ensemble=[symmetries(True, "flips")[0]], spread=S, stats=st)
        assert np.array_equal(got, plain) and not S.any()
        assert st["spread_histogram"][0] == S.size and st["spread_histogram"].sum() == S.size


def test_paths_without_spread_are_unchanged(model3, cube3):
    """ensemble="flips" without `spread` and ensemble=None, run behind a call with `spread` on the same model, against
    values this run computes through the existing keywords and kernels only."""
    from transfer_em_amd.utils import predict_cube
    start, size = (0, 0, 0), (CUBE,) * 3
    rb = Rebuilt(model3, cube3, start, size, _syms(True, "flips"), "zeros", True)
    none_before = predict_cube(cube3, start, size, model3, MS_X, MS_Y)
    predict_cube(cube3, start, size, model3, MS_X, MS_Y, ensemble="flips", spread=np.zeros((CUBE,) * 3, np.uint8))
    st = {}
    flips = predict_cube(cube3, start, size, model3, MS_X, MS_Y, ensemble="flips", stats=st, histogram=True)
    assert np.array_equal(flips, rb.mean()) and "spread_histogram" not in st
    assert np.array_equal(predict_cube(cube3, start, size, model3, MS_X, MS_Y), none_before)
    assert np.array_equal(predict_cube(cube3, start, size, model3, MS_X, MS_Y, ensemble=[ID3]), none_before)
    assert not np.array_equal(flips, none_before)
