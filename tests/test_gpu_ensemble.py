"""Self-ensemble of tiled inference over the training symmetries (ensemble="flips" | "all" | [symmetries]).

Kernels: the symmetry gather is a pure permutation of the existing gather's output and the accumulate is one fp32
addition (and one division) per voxel, so both are held to numpy bit for bit.  End to end: the generator sees
bit-identical tiles whether a symmetry is applied by the gather or to the volume beforehand, and the mean is rebuilt in
numpy from the generator's own outputs, so every comparison of uint8 results is exact as well."""
import os

import numpy as np
import pytest
import torch

from util import scaled_params

pytestmark = pytest.mark.gpu

MS_X, MS_Y = (0.02, 0.58), (-0.1, 0.4)
MODES = ("zeros", "reflect", "edge")
ID3 = ((0, 1, 2), (0, 0, 0))


def T(v, s, lead=0):
    """T_s over the last 3 (2) axes of v; `lead` leading axes (tiles, sections) stay."""
    perm, flips = s
    v = np.transpose(v, tuple(range(lead)) + tuple(lead + p for p in perm))
    return np.flip(v, [lead + a for a, f in enumerate(flips) if f])


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


def _mode_id(mode):
    from transfer_em_amd import _lib as L
    return {"zeros": 0, "reflect": L.TEM_BOUNDARY_REFLECT, "edge": L.TEM_BOUNDARY_EDGE}[mode]


def _tile_shape(n, edge, is3d):
    return (n, edge, edge, edge) if is3d else (n, 1, edge, edge)


# ------------------------------------------------------------------------------------------------------- the gather
class Gather:
    """One uploaded block and its tile origins; existing(mode) and sym(mode, s) return float bits [n, D, E, E]."""

    def __init__(self, blk, lo, vol_shape, org_rel, edge, is3d):
        self.L, self.lib, self.stream = _env()
        self.blk, self.lo, self.vol_shape, self.edge, self.is3d = blk, lo, vol_shape, edge, is3d
        self.dv = torch.from_numpy(np.ascontiguousarray(blk)).cuda()
        self.do = torch.from_numpy(np.ascontiguousarray(org_rel, np.int32)).cuda()
        self.n = len(org_rel)
        self.shape = _tile_shape(self.n, edge, is3d)

    def _out(self):
        return torch.full(self.shape, float("nan"), dtype=torch.float32, device="cuda")

    def _bits(self, out):
        return out.cpu().numpy().view(np.uint32)

    def existing(self, mode):
        out, sfx = self._out(), "" if self.is3d else "2d"
        if mode == "zeros":
            name = f"tem_u8_tiles{sfx}_to_f32_std"
            rc = getattr(self.lib, name)(self.dv.data_ptr(), *self.blk.shape, self.do.data_ptr(), self.n, self.edge,
                                         out.data_ptr(), MS_X[0], MS_X[1], self.stream)
        else:
            name = f"tem_u8_tiles{sfx}_to_f32_std_bc"
            rc = getattr(self.lib, name)(self.dv.data_ptr(), *self.blk.shape, *self.lo, *self.vol_shape, _mode_id(mode),
                                         self.do.data_ptr(), self.n, self.edge, out.data_ptr(), MS_X[0], MS_X[1],
                                         self.stream)
        self.L.check(rc, name)
        return self._bits(out)

    def sym(self, mode, s):
        out, name = self._out(), f"tem_u8_tiles{'' if self.is3d else '2d'}_to_f32_std_sym"
        lo, shape = ((0, 0, 0), self.blk.shape) if mode == "zeros" else (self.lo, self.vol_shape)
        self.L.check(getattr(self.lib, name)(self.dv.data_ptr(), *self.blk.shape, *lo, *shape, _mode_id(mode),
                                             self.do.data_ptr(), self.n, self.edge, *s[0], *s[1], out.data_ptr(),
                                             MS_X[0], MS_X[1], self.stream), name)
        return self._bits(out)


GVOL = (50, 41, 45)
# (z, y, x) origins per edge: one tile inside the volume, one across the near faces, one across the far faces
ORG = {37: [(5, 2, 4), (-10, -7, -12), (30, 20, 25)], 70: [(-10, -15, -12), (-40, -3, -60), (20, 11, 30)]}
ORG2 = {37: [(1, 2, 4), (0, -7, -12), (49, 20, 25), (-1, 1, 1)], 70: [(2, -15, -12), (3, -3, -60), (50, 11, 30)]}


@pytest.fixture(scope="module")
def gvol():
    return np.random.default_rng(11).integers(0, 256, GVOL, dtype=np.uint8)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("edge", [37, 70])
@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
def test_gather_is_the_permuted_existing_gather(gvol, is3d, edge, mode):
    """All 48 (8) symmetries.  Edge 37 fits one LDS tile with a ragged remainder; edge 70 has a full 64-wide tile and a
    remainder of 6 in both directions of the transposed plane."""
    org = (ORG if is3d else ORG2)[edge]
    if edge == 37:
        o, ext = org[0], ((edge,) * 3 if is3d else (1, edge, edge))
        assert all(0 <= a and a + e <= n for a, e, n in zip(o, ext, GVOL))   # the first tile lies inside the volume
    g = Gather(gvol, (0, 0, 0), GVOL, org, edge, is3d)
    ref = g.existing(mode)
    assert len(np.unique(ref)) > 200
    syms = _syms(is3d)
    assert len(syms) == (48 if is3d else 8)
    for s in syms:
        got = g.sym(mode, s)
        want = T(ref, s, 1)                                                  # a 2-D tile is [1, E, E]: z stays
        want = np.ascontiguousarray(want)
        if s == ID3:
            assert np.array_equal(want, ref)
        assert np.array_equal(got, want), (s, np.argwhere(got != want)[:5])


@pytest.mark.parametrize("mode", ["reflect", "edge"])
@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
def test_gather_from_a_sub_block(is3d, mode):
    """The staging block of a streamed chunk: the hull of the tiles' folded coordinates, with a non-zero origin."""
    from transfer_em_amd.utils import fold
    shape, edge = (23, 31, 40), 12
    rng = np.random.default_rng(5)
    vol = rng.integers(0, 256, shape, dtype=np.uint8)
    org = np.stack([rng.integers(n - edge - 3, n + 4, 6) for n in shape], 1)
    ext = (edge, edge, edge) if is3d else (1, edge, edge)
    read = []
    for d in range(3):
        f = fold(np.arange(org[:, d].min(), org[:, d].max() + ext[d]), shape[d], mode)
        read.append((int(f.min()), int(f.max()) + 1))
    lo = tuple(r[0] for r in read)
    assert min(lo) > 0
    g = Gather(vol[tuple(slice(a, b) for a, b in read)], lo, shape, org - np.array(lo), edge, is3d)
    ref = g.existing(mode)
    for s in _syms(is3d)[::5]:
        want = T(ref, s, 1)                                                  # a 2-D tile is [1, E, E]: z stays
        assert np.array_equal(g.sym(mode, s), want), s


# --------------------------------------------------------------------------------------------------- the accumulate
def _accum(y, s, acc, first, divisor, is3d):
    L, lib, stream = _env()
    name = "tem_f32_tiles_sym_accum" if is3d else "tem_f32_tiles2d_sym_accum"
    L.check(getattr(lib, name)(y.data_ptr(), y.shape[0], y.shape[2], *s[0], *s[1], acc.data_ptr(), int(first), divisor,
                               stream), name)


@pytest.mark.parametrize("yedge", [13, 40])
@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
def test_accumulate_three_members_equals_numpy(is3d, yedge):
    """first, middle, last with divisor 3, for every symmetry in every one of the three roles."""
    syms = _syms(is3d)
    k, n = len(syms), 3
    rng = np.random.default_rng(yedge)
    ys = [rng.standard_normal(_tile_shape(n, yedge, is3d)).astype(np.float32) * np.float32(3) for _ in range(3)]
    dys = [torch.from_numpy(y).cuda() for y in ys]
    inv = lambda v, s: Tinv(v, s, 1)                                         # a 2-D tile is [1, E, E]: z stays
    for i in range(k):
        members = [syms[i], syms[(i + 7) % k], syms[(i + 13) % k]]
        acc = torch.full(dys[0].shape, float("nan"), dtype=torch.float32, device="cuda")   # `first` never reads it
        _accum(dys[0], members[0], acc, True, 1, is3d)
        _accum(dys[1], members[1], acc, False, 1, is3d)
        _accum(dys[2], members[2], acc, False, 3, is3d)
        want = inv(ys[0], members[0])
        want = want + inv(ys[1], members[1])
        want = (want + inv(ys[2], members[2])) / np.float32(3)
        assert want.dtype == np.float32
        got = acc.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), members


@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
def test_accumulate_first_with_divisor_one_writes_y_through(is3d):
    y = torch.from_numpy(np.random.default_rng(3).standard_normal(_tile_shape(2, 21, is3d)).astype(np.float32)).cuda()
    for s in _syms(is3d)[:: 7 if is3d else 3]:
        acc = torch.full(y.shape, float("nan"), dtype=torch.float32, device="cuda")
        _accum(y, s, acc, True, 1, is3d)
        want = Tinv(y.cpu().numpy(), s, 1)
        assert np.array_equal(acc.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), s


# ----------------------------------------------------------------------------------------------------- the arguments
def test_entry_points_refuse_bad_arguments():
    L, lib, stream = _env()
    vol = torch.zeros((4, 5, 6), dtype=torch.uint8, device="cuda")
    org = torch.zeros((1, 3), dtype=torch.int32, device="cuda")
    out = torch.zeros((6 ** 3,), dtype=torch.float32, device="cuda")
    y = torch.zeros((6 ** 3,), dtype=torch.float32, device="cuda")
    bad_syms = [((0, 0, 2), (0, 0, 0)), ((0, 1, 3), (0, 0, 0)), ((-1, 1, 2), (0, 0, 0)), ((1, 1, 1), (0, 0, 0)),
                ((0, 1, 2), (0, 2, 0)), ((0, 1, 2), (0, 0, -1))]
    z_syms = [((1, 0, 2), (0, 0, 0)), ((2, 1, 0), (0, 0, 0)), ((0, 1, 2), (1, 0, 0)), ((1, 2, 0), (0, 1, 1))]
    for is3d in (True, False):
        sfx = "" if is3d else "2d"
        gfn, afn = getattr(lib, f"tem_u8_tiles{sfx}_to_f32_std_sym"), getattr(lib, f"tem_f32_tiles{sfx}_sym_accum")

        def gather(block=(4, 5, 6), lo=(0, 0, 0), shape=(4, 5, 6), mode=0, sym=ID3, ntile=1, edge=6, ptr=None):
            return gfn(vol.data_ptr() if ptr is None else ptr, *block, *lo, *shape, mode, org.data_ptr(), ntile, edge,
                       *sym[0], *sym[1], out.data_ptr(), 0.0, 1.0, stream)

        def accum(sym=ID3, first=1, divisor=1, ntile=1, yedge=6, acc=None):
            return afn(y.data_ptr(), ntile, yedge, *sym[0], *sym[1], out.data_ptr() if acc is None else acc, first,
                       divisor, stream)
        for mode in (0, L.TEM_BOUNDARY_REFLECT, L.TEM_BOUNDARY_EDGE):
            assert gather(mode=mode) == L.TEM_OK
        assert gather(sym=((0, 2, 1), (0, 1, 1))) == L.TEM_OK
        for mode in (3, -1):
            assert gather(mode=mode) == L.TEM_EINVAL
        assert gather(shape=(4, 0, 6)) == L.TEM_EINVAL
        assert gather(block=(4, 0, 6)) == L.TEM_EINVAL
        assert gather(block=(2, 5, 6), lo=(3, 0, 0), mode=L.TEM_BOUNDARY_EDGE) == L.TEM_EINVAL   # leaves the volume
        assert gather(block=(2, 5, 6), lo=(-1, 0, 0)) == L.TEM_EINVAL
        assert gather(ntile=-1) == L.TEM_EINVAL and gather(edge=0) == L.TEM_EINVAL and gather(ptr=0) == L.TEM_EINVAL
        assert accum() == L.TEM_OK and accum(first=0, divisor=3) == L.TEM_OK
        assert accum(first=2) == L.TEM_EINVAL and accum(divisor=0) == L.TEM_EINVAL and accum(yedge=0) == L.TEM_EINVAL
        assert accum(ntile=-1) == L.TEM_EINVAL and accum(acc=0) == L.TEM_EINVAL
        assert accum(acc=y.data_ptr()) == L.TEM_EINVAL                       # in place
        for s in bad_syms:
            assert gather(sym=s) == L.TEM_EINVAL and accum(sym=s) == L.TEM_EINVAL, s
        for s in z_syms:                                                     # fine for a cube, refused for a section
            want = L.TEM_OK if is3d else L.TEM_EINVAL
            assert gather(sym=s) == want and accum(sym=s) == want, s
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------- end to end
# the 74 model: tiles of 36 + a halo of 19 (tpad 2)
VOL, START, SIZE = (50, 90, 61), (-20, -15, -10), (90, 100, 80)            # (z,y,x); (x,y,z): 27 tiles, past all six faces
VOL2, START2, SIZE2 = (3, 50, 45), (-20, -15, -1), (90, 100, 5)             # 2-D: sections -1 and 3 lie outside
CUBE = 72


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
    return _model(tmp_path_factory.mktemp("ens3"), "ens3", True)


@pytest.fixture(scope="module")
def model2(tmp_path_factory):
    return _model(tmp_path_factory.mktemp("ens2"), "ens2", False)


@pytest.fixture(scope="module")
def ragged3():
    return np.random.default_rng(1).integers(0, 256, VOL, dtype=np.uint8)


@pytest.fixture(scope="module")
def ragged2():
    return np.random.default_rng(2).integers(0, 256, VOL2, dtype=np.uint8)


@pytest.fixture(scope="module")
def cube3():
    return np.random.default_rng(3).integers(0, 256, (CUBE,) * 3, dtype=np.uint8)


@pytest.fixture(scope="module")
def stack2():
    return np.random.default_rng(4).integers(0, 256, (3, CUBE, CUBE), dtype=np.uint8)


@pytest.mark.parametrize("mode", MODES)
def test_identity_member_equals_no_ensemble_3d(model3, ragged3, mode):
    from transfer_em_amd.utils import predict_cube, predict_volume, symmetries, tile_plan
    assert len(tile_plan(START, SIZE, model3.outdimsize, model3.buffer)[3]) == 27
    ref = predict_cube(ragged3, START, SIZE, model3, MS_X, MS_Y, boundary=mode)
    assert ref.shape == (80, 100, 90) and ref.std() > 20
    ident = [symmetries(True, "flips")[0]]
    assert np.array_equal(predict_cube(ragged3, START, SIZE, model3, MS_X, MS_Y, boundary=mode, ensemble=ident), ref)
    got = predict_volume(ragged3, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(2, 2, 2), boundary=mode, ensemble=ident)
    assert np.array_equal(got, ref)
    inp, out = predict_cube(ragged3, START, SIZE, model3, MS_X, MS_Y, fetch_input=True, boundary=mode, ensemble=ident,
                            tile_batch=4)
    assert np.array_equal(out, ref)
    assert np.array_equal(inp, predict_cube(ragged3, START, SIZE, model3, MS_X, MS_Y, fetch_input=True, boundary=mode)[0])


@pytest.mark.parametrize("mode", MODES)
def test_identity_member_equals_no_ensemble_2d(model2, ragged2, mode):
    from transfer_em_amd.utils import predict_cube, predict_volume
    ref = predict_cube(ragged2, START2, SIZE2, model2, MS_X, MS_Y, boundary=mode)
    assert ref.shape == (5, 100, 90) and ref.std() > 20
    for ident in ([((0, 1), (False, False))], [ID3]):                        # the 2-axis and the 3-axis spelling
        assert np.array_equal(predict_cube(ragged2, START2, SIZE2, model2, MS_X, MS_Y, boundary=mode, ensemble=ident), ref)
    got = predict_volume(ragged2, START2, SIZE2, model2, MS_X, MS_Y, chunk_tiles=(2, 1, 2), boundary=mode, ensemble=[ID3])
    assert np.array_equal(got, ref)
    img, start, size = ragged2[1], START2[:2], SIZE2[:2]                     # the single-image forms
    ref1 = predict_cube(img, start, size, model2, MS_X, MS_Y, boundary=mode)
    ident = [((0, 1), (False, False))]
    assert np.array_equal(predict_cube(img, start, size, model2, MS_X, MS_Y, boundary=mode, ensemble=ident), ref1)
    assert np.array_equal(predict_volume(img, start, size, model2, MS_X, MS_Y, boundary=mode, ensemble=ident), ref1)


# one pure flip, two transpositions (one keeps x innermost, one moves it), two 3-cycles with flips
SINGLE_3D = [((0, 1, 2), (1, 0, 1)), ((1, 0, 2), (0, 1, 0)), ((0, 2, 1), (0, 0, 0)), ((1, 2, 0), (1, 0, 1)),
             ((2, 0, 1), (0, 1, 1))]


@pytest.mark.parametrize("mode", ["zeros", "reflect"])
def test_single_member_equals_prediction_of_the_transformed_cube_3d(model3, cube3, mode):
    """8 tiles on a grid that every symmetry maps onto itself: the generator sees the same tiles in both runs."""
    from transfer_em_amd.utils import predict_cube
    start, size = (0, 0, 0), (CUBE,) * 3
    plain = predict_cube(cube3, start, size, model3, MS_X, MS_Y, boundary=mode)
    for s in SINGLE_3D:
        want = Tinv(predict_cube(np.ascontiguousarray(T(cube3, s)), start, size, model3, MS_X, MS_Y, boundary=mode), s)
        got = predict_cube(cube3, start, size, model3, MS_X, MS_Y, boundary=mode, ensemble=[s])
        assert np.array_equal(got, want), s
        assert not np.array_equal(got, plain), s                             # the orientation matters to the network


@pytest.mark.parametrize("mode", ["zeros", "reflect"])
def test_single_member_equals_prediction_of_the_transformed_stack_2d(model2, stack2, mode):
    from transfer_em_amd.utils import predict_cube, symmetries
    start, size = (0, 0, 0), (CUBE, CUBE, 3)
    plain = predict_cube(stack2, start, size, model2, MS_X, MS_Y, boundary=mode)
    syms = symmetries(False, "all")
    assert len(syms) == 8
    for s in syms:
        want = Tinv(predict_cube(np.ascontiguousarray(T(stack2, s, 1)), start, size, model2, MS_X, MS_Y, boundary=mode),
                    s, 1)
        got = predict_cube(stack2, start, size, model2, MS_X, MS_Y, boundary=mode, ensemble=[s])
        assert np.array_equal(got, want), s
        assert (s == syms[0]) == np.array_equal(got, plain), s


def _spread(a, k):
    """The guard against a degenerate (constant or saturated) result, for a mean over k members.  One run of these
    models on random bytes spreads over the uint8 range with a standard deviation above 20 (held where `k` is 1).  The
    random network is far from equivariant, so the members' outputs at a voxel are only partly correlated and their
    mean is narrower: by at most sqrt(k), the factor for k uncorrelated members of equal spread."""
    return a.std() > 20 / np.sqrt(k)


def _manual_mean(model, vol, start, size, syms, mode, is3d):
    """predict_cube(..., ensemble=syms) rebuilt step by step: the new gather and the generator plan per member, the
    inverse transform, the fp32 accumulation and the division in numpy, then the existing scatter kernel."""
    from transfer_em_amd.utils import tile_plan, tile_plan_2d
    L, lib, stream = _env()
    od, buf, tpad, rois, index = (tile_plan if is3d else tile_plan_2d)(start, size, model.outdimsize, model.buffer)
    edge, n = od + 2 * buf, len(rois)
    g = Gather(vol, (0, 0, 0), vol.shape, [(r[2], r[1], r[0]) for r in rois], edge, is3d)
    plan = model.generator_g.plan(_tile_shape(n, edge, is3d) + (1,))
    acc = None
    for s in syms:
        tiles = torch.from_numpy(g.sym(mode, s).view(np.float32)).cuda()
        plan.x.copy_(tiles.reshape(plan.x.shape))
        y = plan.run().clone().cpu().numpy()[..., 0]                         # [n, D, ye, ye]
        back = Tinv(y, s, 1)
        acc = back.copy() if acc is None else acc + back
    acc = acc / np.float32(len(syms))
    assert acc.dtype == np.float32
    yedge = acc.shape[2]
    assert yedge - 2 * tpad == od
    rnd = lambda v: -(-v // od) * od
    oshape = (rnd(size[2]) if is3d else size[2], rnd(size[1]), rnd(size[0]))
    out = torch.zeros(oshape, dtype=torch.uint8, device="cuda")
    dacc = torch.from_numpy(np.ascontiguousarray(acc)).cuda()
    idx = torch.tensor([[i[2], i[1], i[0]] for i in index], dtype=torch.int32).cuda()
    name = "tem_f32_tiles_unstd_to_u8" if is3d else "tem_f32_tiles2d_unstd_to_u8"
    L.check(getattr(lib, name)(dacc.data_ptr(), n, yedge, tpad, idx.data_ptr(), out.data_ptr(), *oshape, MS_Y[0], MS_Y[1],
                               stream), name)
    return out[:size[2], :size[1], :size[0]].cpu().numpy()


def test_mean_over_all_48_on_one_tile(model3, ragged3):
    from transfer_em_amd.utils import predict_cube
    start, size = (3, 30, 8), (36, 36, 36)                                   # one tile, past the near z and x faces
    syms = _syms(True)
    want = _manual_mean(model3, ragged3, start, size, syms, "reflect", True)
    got = predict_cube(ragged3, start, size, model3, MS_X, MS_Y, boundary="reflect", ensemble="all")
    plain = predict_cube(ragged3, start, size, model3, MS_X, MS_Y, boundary="reflect")
    assert _spread(plain, 1) and _spread(want, 48)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, plain)


def test_mean_over_the_flips_on_the_cube(model3, cube3):
    from transfer_em_amd.utils import predict_cube
    start, size = (0, 0, 0), (CUBE,) * 3
    want = _manual_mean(model3, cube3, start, size, _syms(True, "flips"), "zeros", True)
    got = predict_cube(cube3, start, size, model3, MS_X, MS_Y, ensemble="flips")
    assert _spread(want, 8) and np.array_equal(got, want)
    assert np.array_equal(predict_cube(cube3, start, size, model3, MS_X, MS_Y, ensemble="flips", tile_batch=3), want)


def test_mean_over_all_8_on_a_stack_2d(model2, stack2):
    from transfer_em_amd.utils import predict_cube
    start, size = (0, 0, 0), (CUBE, CUBE, 3)
    want = _manual_mean(model2, stack2, start, size, _syms(False), "edge", False)
    got = predict_cube(stack2, start, size, model2, MS_X, MS_Y, boundary="edge", ensemble="all")
    assert _spread(want, 8) and np.array_equal(got, want)


def test_predict_volume_equals_predict_cube_under_flips(model3, ragged3, tmp_path):
    """Chunks of 2 x 2 x 2 tiles over a 3 x 3 x 3 grid (tails on every axis), batches of 3 tiles inside a chunk, two
    ranks writing one `out`, boundary reflect; and the saved-model form."""
    from transfer_em_amd import utils
    ref = utils.predict_cube(ragged3, START, SIZE, model3, MS_X, MS_Y, boundary="reflect", ensemble="flips")
    assert _spread(ref, 8)
    assert not np.array_equal(ref, utils.predict_cube(ragged3, START, SIZE, model3, MS_X, MS_Y, boundary="reflect"))
    chunks = utils.chunk_plan(START, SIZE, model3.outdimsize, model3.buffer, VOL, (2, 2, 2), boundary="reflect")
    assert len(chunks) == 8 and sorted({len(c.tiles) for c in chunks}) == [1, 2, 4, 8]
    out = np.zeros(ref.shape, np.uint8)
    for rank in range(2):
        st = {}
        utils.predict_volume(ragged3, START, SIZE, model3, MS_X, MS_Y, out=out, chunk_tiles=(2, 2, 2), tile_batch=3,
                             rank=rank, world_size=2, stats=st, boundary="reflect", ensemble="flips")
        assert st["chunks"] == 4
        if rank == 0:
            assert not np.array_equal(out, ref)                              # the other rank's boxes are still empty
    assert np.array_equal(out, ref)
    dflt = utils.predict_volume(ragged3, START, SIZE, model3, MS_X, MS_Y, boundary="reflect", ensemble="flips")
    assert np.array_equal(dflt, ref)
    ckpt = model3.make_checkpoint(1)
    out_dir = str(tmp_path / "exported")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        utils.save_model(out_dir, ckpt, MS_X, MS_Y, size=74, is3d=True)
    finally:
        os.chdir(cwd)
    saved = utils.predict_volume_from_saved_model(ragged3, START, SIZE, out_dir, chunk_tiles=(2, 2, 2), tile_batch=3,
                                                  boundary="reflect", ensemble="flips")
    assert np.array_equal(saved, ref)


def test_predict_volume_equals_predict_cube_under_an_ensemble_2d(model2, ragged2):
    from transfer_em_amd.utils import predict_cube, predict_volume
    ens = [((0, 1), (False, False)), ((1, 0), (False, True)), ((0, 2, 1), (0, 1, 1))]
    ref = predict_cube(ragged2, START2, SIZE2, model2, MS_X, MS_Y, boundary="reflect", ensemble=ens)
    got = predict_volume(ragged2, START2, SIZE2, model2, MS_X, MS_Y, chunk_tiles=(2, 1, 2), tile_batch=5,
                         boundary="reflect", ensemble=ens)
    assert _spread(ref, 3) and np.array_equal(got, ref)
    assert not np.array_equal(ref, predict_cube(ragged2, START2, SIZE2, model2, MS_X, MS_Y, boundary="reflect"))
