"""The rescale on the device: tem_u8_rescale against the integer numpy reference (rescale_ref), and volume_rescale out
of core.  The contract is integers with one rounding, so every comparison is exact: np.array_equal with the reference.
Every call writes into a buffer between odd guards of fill bytes, which must come back untouched.  Helpers are those of
test_gpu_histogram.py."""
import functools
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import rescale_ref as R
from test_gpu_histogram import FailingReads, _counted, _env, _upload

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "transfer_em_amd", "csrc",
                         "rescale_u8.hip")).read()
TY, TX = (int(v) for v in re.search(r"RESCALE_TY = (\d+), RESCALE_TX = (\d+);", _SRC).groups())      # the kernel's tile
ZRUN = int(re.search(r"RESCALE_ZRUN = (\d+);", _SRC).group(1))                                       # ... and its z-run
PREFETCH = int(re.search(r"RESCALE_PREFETCH = (\d+);", _SRC).group(1))   # bytes per thread of a footprint held in registers

GUARD, FILL = 61, 0xA5                                                   # an odd guard: dst starts misaligned
STEPS = [(2, 1), (3, 2), (7, 3), (8, 1), (1, 2), (2, 3), (1, 5), (1, 8)]
ALL = [(s, s, s) for s in STEPS] + [((1, 5), (2, 1), (2, 1))]            # (z, y, x); the last: ssTEM onto an isotropic grid
ALL_IDS = [f"{p}_{q}" for p, q in STEPS] + ["mixed"]


def _vol(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _hull(obox, vshape, steps):
    """The tight source box (lo, hi) per axis of the output box `obox`."""
    return tuple(R.hull(lo, hi, n, p, q) for (lo, hi), n, (p, q) in zip(obox, vshape, steps))


def _cut(v, box):
    return np.array(v[tuple(slice(lo, hi) for lo, hi in box)])           # a copy: the cached cases stay read-only


def _call(psrc, sdims, s0, vshape, steps, pdst, odims, o0):
    L, lib, stream = _env()
    return lib.tem_u8_rescale(psrc, *sdims, *s0, *vshape, *(v for s in steps for v in s), pdst, *odims, *o0, stream)


def _rescale(v, steps, obox, sbox=None, off=0):
    """tem_u8_rescale of the output box `obox` of volume `v` from its source block `sbox` (default: the tight hull of
    its taps), uploaded `off` bytes off alignment; the guards around dst must be untouched."""
    L = _env()[0]
    sbox = _hull(obox, v.shape, steps) if sbox is None else sbox
    keep, psrc = _upload(_cut(v, sbox), off)
    odims = tuple(hi - lo for lo, hi in obox)
    n = int(np.prod(odims))
    dst = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    L.check(_call(psrc, tuple(hi - lo for lo, hi in sbox), tuple(lo for lo, _ in sbox), v.shape, steps,
                  dst.data_ptr() + GUARD, odims, tuple(lo for lo, _ in obox)), "tem_u8_rescale")
    got = dst.cpu().numpy()
    assert (got[:GUARD] == FILL).all() and (got[GUARD + n:] == FILL).all()
    return got[GUARD:GUARD + n].reshape(odims)


@functools.lru_cache(maxsize=None)
def _case(shape, steps, seed=100):
    """A random volume and its reference, computed once and left unchanged."""
    v = _vol(shape, seed)
    want = R.reference(v, steps)
    v.setflags(write=False), want.setflags(write=False)
    return v, want


def _whole(shape):
    return tuple((0, n) for n in shape)


# ---------------------------------------------------------------------------------------------------- tem_u8_rescale
@pytest.mark.parametrize("steps", ALL, ids=ALL_IDS)
def test_one_voxel_and_one_more_on_each_axis(steps):
    """One output voxel, then one more on each axis in turn, at a non-zero origin of the grid, from the tight hull of its
    taps: a block at a non-zero origin of a larger volume, src and dst at odd addresses."""
    shape = tuple(max(4, -(-6 * p // q)) for p, q in steps)              # at least 6 outputs per axis
    v, want = _case(shape, steps)
    o = (1, 2, 3)
    for extra in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        obox = tuple((lo, lo + 1 + e) for lo, e in zip(o, extra))
        got = _rescale(v, steps, obox, off=1)
        assert got.size == 1 + sum(extra) and np.array_equal(got, _cut(want, obox)), (extra, got, _cut(want, obox))


@pytest.mark.parametrize("steps", [ALL[0], ALL[1], ALL[3], ALL[5], ALL[8]], ids=[ALL_IDS[i] for i in (0, 1, 3, 5, 8)])
def test_extents_around_the_tile_and_the_z_run(steps):
    """Output blocks one below, equal to and one above the kernel's tile in y and x and its run length in z.  At 8/1
    a full tile's footprint is staged directly; at the other steps it travels through registers."""
    most = (ZRUN + 1, TY + 1, TX + 1)
    shape = tuple(-(-n * p // q) for n, (p, q) in zip(most, steps))
    v, want = _case(shape, steps)
    assert all(a >= b for a, b in zip(want.shape, most))
    for oz in (ZRUN - 1, ZRUN, ZRUN + 1):
        for oy in (TY - 1, TY, TY + 1):
            for ox in (TX - 1, TX, TX + 1):
                obox = ((0, oz), (0, oy), (0, ox))
                assert np.array_equal(_rescale(v, steps, obox), _cut(want, obox)), obox


def test_footprints_around_the_register_path():
    """A tile's footprint of one byte per thread and prefetch register less, exactly as many, and more: at step 4/1 a
    tile of TY rows and c columns has a footprint of 4 TY x 4 c bytes, and c = PREFETCH x TX / 16 fills the registers."""
    c = PREFETCH * TX // 16
    assert 4 * TY * 4 * c == PREFETCH * TY * TX and c + 1 <= TX
    steps = ((4, 1),) * 3
    v, want = _case((4 * 5 + 1, 4 * TY, 4 * (c + 1)), steps, 106)
    for cols in (c - 1, c, c + 1):
        for rows in (TY - 1, TY):
            obox = ((0, 6), (0, rows), (0, cols))                        # 6 planes: the last is the far face's
            assert np.array_equal(_rescale(v, steps, obox), _cut(want, obox)), obox


FACES = [((2, 1), (7, 9, 11)), ((3, 2), (7, 8, 10)), ((7, 3), (8, 9, 10)), ((8, 1), (9, 17, 67)), ((64, 63), (5, 6, 70)),
         ((5, 4), (6, 7, 9)), ((1, 2), (3, 4, 5)), ((2, 3), (1, 2, 5)), ((1, 5), (2, 1, 3)), ((1, 8), (3, 2, 5)),
         ((63, 64), (2, 3, 66)), ((1, 3), (3, 4, 5)), ((1, 1), (3, 9, 35))]


@pytest.mark.parametrize("step,shape", FACES, ids=[f"{p}_{q}" for (p, q), _ in FACES])
def test_whole_volumes_with_their_faces(step, shape):
    """Whole small volumes.  Shrinking: n q mod p != 0 on every axis, so the last output of every axis has a reduced
    denominator.  Growing: the clamped taps at the near and the far face, extents of 1 and 2 included, and at 1/3 the
    outputs whose second tap has weight 0."""
    p, q = step
    if p > q:
        assert all((n * q) % p for n in shape)
    steps = (step,) * 3
    v, want = _case(shape, steps, 101)
    assert want.shape == tuple(R.grid(n, p, q) for n in shape)
    assert np.array_equal(_rescale(v, steps, _whole(want.shape), off=3), want)


def test_mixed_steps_and_a_far_face_per_axis():
    for steps, shape in ((((1, 5), (2, 1), (2, 1)), (3, 7, 9)), (((2, 1), (1, 5), (3, 2)), (7, 3, 9)),
                         (((7, 3), (8, 1), (2, 3)), (8, 70, 45))):
        v, want = _case(shape, steps, 102)
        assert np.array_equal(_rescale(v, steps, _whole(want.shape), off=1), want), steps


@pytest.mark.parametrize("step", [(63, 64), (64, 63)], ids=["63_64", "64_63"])
def test_constant_255_reaches_the_32_bit_bound(step):
    """2 S + Den = 511 x 128^3 at 63/64: the largest numerator there is."""
    v = np.full((3, 3, 70), 255, np.uint8)
    steps = (step,) * 3
    got = _rescale(v, steps, _whole(tuple(R.grid(n, *step) for n in v.shape)))
    assert (got == 255).all() and got.shape == ((4, 4, 72) if step == (63, 64) else (3, 3, 69))
    z = np.zeros((3, 3, 70), np.uint8)
    assert (_rescale(z, steps, _whole(got.shape)) == 0).all()


@pytest.mark.parametrize("steps", [ALL[1], ALL[5], ALL[8]], ids=[ALL_IDS[i] for i in (1, 5, 8)])
def test_nothing_outside_the_hull_matters(steps):
    """The same output block from the whole volume as its source block, before and after every byte outside the hull
    of its taps has changed."""
    shape = tuple(-(-n * p // q) for n, (p, q) in zip((12, 14, 40), steps))
    v, want = _case(shape, steps, 103)
    obox = ((2, 9), (3, 12), (5, 38))
    hull = _hull(obox, v.shape, steps)
    inside = tuple(slice(lo, hi) for lo, hi in hull)
    v2 = (255 - v).astype(np.uint8)
    v2[inside] = v[inside]
    assert (v2 != v).sum() == v.size - np.prod([hi - lo for lo, hi in hull]) > 0
    for off in (0, 1):
        a = _rescale(v, steps, obox, sbox=_whole(v.shape), off=off)
        b = _rescale(v2, steps, obox, sbox=_whole(v.shape), off=off)
        assert np.array_equal(a, _cut(want, obox)) and np.array_equal(a, b)


@pytest.mark.parametrize("steps", [ALL[1], ALL[2], ALL[5], ALL[8]], ids=[ALL_IDS[i] for i in (1, 2, 5, 8)])
def test_a_block_does_not_depend_on_how_it_is_cut(steps):
    """A block computed whole equals the same block computed as z-cut and y-cut sub-blocks, each from its own tight
    hull, the far faces included."""
    shape = tuple(-(-n * p // q) - 1 for n, (p, q) in zip((ZRUN + 8, 21, 40), steps))
    v, want = _case(shape, steps, 104)
    gz, gy, gx = want.shape
    whole = _rescale(v, steps, _whole(want.shape), sbox=_whole(v.shape))
    assert np.array_equal(whole, want)
    parts = np.zeros_like(want)
    for z0, z1 in ((0, 1), (1, 7), (7, gz - 1), (gz - 1, gz)):
        for y0, y1 in ((0, 5), (5, 6), (6, gy)):
            obox = ((z0, z1), (y0, y1), (0, gx))
            parts[z0:z1, y0:y1] = _rescale(v, steps, obox)
    assert np.array_equal(parts, want)
    obox = ((3, gz - 2), (2, gy - 3), (7, gx - 1))                       # cut along x as well
    assert np.array_equal(_rescale(v, steps, obox), _cut(want, obox))


def test_rejects_malformed_arguments():
    """TEM_EINVAL from the host-side checks for every refusal of the contract; nothing is launched: dst keeps its fill."""
    L, lib, stream = _env()
    src = torch.zeros(8 * 10 * 12 + 16, dtype=torch.uint8, device="cuda")
    dst = torch.full((4 * 5 * 6 + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    S2 = ((2, 1),) * 3

    def call(psrc=None, sd=(8, 10, 12), s0=(0, 0, 0), V=(8, 10, 12), steps=S2, pdst=None, od=(4, 5, 6), o0=(0, 0, 0)):
        return _call(src.data_ptr() if psrc is None else psrc, sd, s0, V, steps, dst.data_ptr() + GUARD if pdst is None
                     else pdst, od, o0)
    at = lambda t, d, v: tuple(v if i == d else e for i, e in enumerate(t))
    assert call(psrc=0) == L.TEM_EINVAL and call(pdst=0) == L.TEM_EINVAL
    for d in range(3):
        for bad in (0, -1):                                              # a dimension below 1
            assert call(sd=at((8, 10, 12), d, bad)) == L.TEM_EINVAL
            assert call(V=at((8, 10, 12), d, bad)) == L.TEM_EINVAL
            assert call(od=at((4, 5, 6), d, bad)) == L.TEM_EINVAL
        for bad in ((0, 1), (1, 0), (-2, 1), (2, -1), (65, 64), (64, 65), (9, 1), (1, 9), (17, 2), (4, 2), (2, 2), (6, 3)):
            assert call(steps=at(S2, d, bad)) == L.TEM_EINVAL, bad       # p, q outside 1...64; past 8; not reduced
        assert call(s0=at((0, 0, 0), d, -1)) == L.TEM_EINVAL and call(o0=at((0, 0, 0), d, -1)) == L.TEM_EINVAL
        assert call(s0=at((0, 0, 0), d, 1)) == L.TEM_EINVAL              # the source block leaves the volume
        assert call(V=at((8, 10, 12), d, (7, 9, 11)[d])) == L.TEM_EINVAL
        assert call(od=at((4, 5, 6), d, (5, 6, 7)[d])) == L.TEM_EINVAL   # the output block leaves the grid
        assert call(o0=at((0, 0, 0), d, 1)) == L.TEM_EINVAL
        # a tap outside the source block: the block's last plane / row / column is missing, or its first
        assert call(sd=at((8, 10, 12), d, (7, 9, 11)[d])) == L.TEM_EINVAL
        assert call(sd=at((8, 10, 12), d, (7, 9, 11)[d]), s0=at((0, 0, 0), d, 1)) == L.TEM_EINVAL
    # growing: output 0 of step 1/2 clamps onto voxel 0, output 1 reads voxels 0 and 1
    G = ((1, 2),) * 3
    assert call(sd=(1, 1, 1), V=(4, 5, 6), steps=G, od=(1, 1, 2)) == L.TEM_EINVAL
    # more workgroups than a launch holds (the bound of include/tem_hip.h); refused on the host, so the extents need
    # no memory behind them
    M, one = 2 ** 31 - 1, ((1, 1),) * 3
    assert call(sd=(M, M, M), V=(M, M, M), steps=one, od=(M, M, M)) == L.TEM_EINVAL
    over = (ZRUN * 2 ** 12, TY * 2 ** 6, TX * 2 ** 6)                    # 2^24 workgroups: one too many
    assert (over[0] // ZRUN) * (over[1] // TY) * (over[2] // TX) == 2 ** 24
    assert call(sd=over, V=over, steps=one, od=over) == L.TEM_EINVAL
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == FILL).all()
    # the block without its first plane holds the taps of outputs 1...3 (output 1 starts at source plane 2): a good call;
    # so are the clamped output alone, and the plain call
    assert call(sd=(7, 10, 12), s0=(1, 0, 0), od=(3, 5, 6), o0=(1, 0, 0)) == L.TEM_OK
    assert call(sd=(1, 1, 1), V=(4, 5, 6), steps=G, od=(1, 1, 1)) == L.TEM_OK
    assert call() == L.TEM_OK
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[:GUARD] == FILL).all() and (got[GUARD + 120:] == FILL).all() and (got[GUARD:GUARD + 120] == 0).all()


# ---------------------------------------------------------------------------------------------------- volume_rescale
VSTEP = (Fraction(3, 2), 2, Fraction(1, 5))                              # (x, y, z)
VSTEPS = ((1, 5), (2, 1), (3, 2))                                        # the same, (z, y, x) pairs


@pytest.fixture(scope="module")
def memmap(tmp_path_factory):
    """An EM-like (40, 50, 60) memmap and its reference at VSTEP, (200, 25, 40); left unchanged."""
    tmp = tmp_path_factory.mktemp("rescale")
    rng = np.random.default_rng(105)
    a = np.lib.format.open_memmap(str(tmp / "a.npy"), mode="w+", dtype=np.uint8, shape=(40, 50, 60))
    a[...] = np.clip(rng.normal(120, 40, a.shape), 0, 255).astype(np.uint8)
    a.flush()
    want = R.reference(np.asarray(a), VSTEPS)
    want.setflags(write=False)
    return np.load(str(tmp / "a.npy"), mmap_mode="r"), want


def test_volume_rescale_under_every_cut(memmap, tmp_path):
    from transfer_em_amd.utils import rescale_chunks, rescale_shape, volume_rescale
    vol, want = memmap
    assert rescale_shape(vol.shape, VSTEP) == want.shape == (200, 25, 40)
    box = _whole(want.shape)
    st = {}
    got, n = _counted(lambda: volume_rescale(vol, VSTEP, stats=st))     # out=None, the default budget: one slab
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    assert st["chunks"] == 1 == n["tem_u8_rescale"] and st["read_s"] > 0 and st["write_s"] > 0
    # 3500 bytes: a source plane's 3000 fit once, so outputs with one z tap go in runs of whole planes and outputs
    # with two are cut into rows; 12005: runs of whole planes only
    for budget, zcut, ycut in ((3500, True, True), (12005, True, False)):
        chunks = rescale_chunks(box, vol.shape, VSTEP, budget)
        cut_y = [o for o, _ in chunks if o[1] != (0, 25)]
        assert bool(cut_y) == ycut and (len(chunks) - len(cut_y) > 1) == zcut
        out = np.lib.format.open_memmap(str(tmp_path / f"out{budget}.npy"), mode="w+", dtype=np.uint8, shape=want.shape)
        st = {}
        ret, n = _counted(lambda: volume_rescale(vol, VSTEP, out=out, chunk_bytes=budget, stats=st))
        assert ret is out and np.array_equal(out, want), budget
        assert st["chunks"] == len(chunks) == n["tem_u8_rescale"] and st["chunks"] > 10
    # an off-origin ROI of the output grid, (x, y, z)
    start, size = (7, 3, 41), (30, 19, 120)
    out = np.full((120, 19, 30), 3, np.uint8)
    volume_rescale(vol, VSTEP, out=out, start=start, size=size, chunk_bytes=3500)
    assert np.array_equal(out, want[41:161, 3:22, 7:37])
    assert np.array_equal(volume_rescale(vol, VSTEP, start=start, size=size), out)


def test_volume_rescale_ranks_images_and_the_way_back(memmap):
    from transfer_em_amd.utils import volume_rescale
    vol, want = memmap
    shared = np.zeros(want.shape, np.uint8)
    counts = []
    for rank in range(2):                                                # two ranks into one shared out
        st = {}
        volume_rescale(vol, VSTEP, out=shared, chunk_bytes=3500, rank=rank, world_size=2, stats=st)
        counts.append(st["chunks"])
        assert np.array_equal(shared, want) == (rank == 1)
    assert abs(counts[0] - counts[1]) <= 1 and min(counts) > 10
    img = np.asarray(vol[7])                                             # one image [y, x] with a 2-element step
    istep = (2, (2, 3))
    iwant = R.reference2d(img, ((2, 3), (2, 1)))
    assert iwant.shape == (75, 30)
    assert np.array_equal(volume_rescale(img, istep), iwant)
    out = np.zeros((40, 21), np.uint8)
    volume_rescale(img, istep, out=out, start=(4, 11), size=(21, 40), chunk_bytes=50)
    assert np.array_equal(out, iwant[11:51, 4:25])
    down = volume_rescale(vol, 2)                                        # step 2, then 1/2: the way back
    assert down.shape == (20, 25, 30) and np.array_equal(down, R.pool2(np.asarray(vol)))
    back = volume_rescale(down, Fraction(1, 2))
    assert back.shape == vol.shape and np.array_equal(back, R.reference(down, ((1, 2),) * 3))


def test_a_failing_read_surfaces_and_leaves_the_device_usable(memmap):
    import threading
    from transfer_em_amd.utils import volume_rescale
    vol, want = memmap
    threads = threading.active_count()
    bad = FailingReads(np.asarray(vol))
    with pytest.raises(OSError, match="the third read fails"):
        volume_rescale(bad, VSTEP, chunk_bytes=12005)
    assert bad.reads >= 3 and threading.active_count() == threads
    assert np.array_equal(volume_rescale(vol, VSTEP, chunk_bytes=12005), want)
