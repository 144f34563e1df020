"""The warp= keyword of predict_cube / predict_volume on the device: the call on the raw stack equals, bit for bit, the
same call without it on the aligned volume A = volume_warp_field(volume, ...) (volume_warp without fields), resident and
streamed, for 3-D and 2-D models, every boundary, and together with repair (a mask in the raw frame, sections in the
aligned one), clahe, lut, an ensemble with its spread, and mips.  The 74 model (tiles of 36, halo 19) on stacks of
30 x 110 x 150 and 7 x 110 x 150; the model is test_gpu_clahe.py's."""
import numpy as np
import pytest

import warp_box_cases as C
from clahe_ref import ramp_volume
from test_gpu_clahe import _model
from test_gpu_histogram import _counted

pytestmark = pytest.mark.gpu

MS_X, MS_Y = (0.02, 0.58), (-0.1, 0.4)
FILL, GAP = 37, 3
VOL, START, SIZE = (30, 110, 150), (-5, 3, -4), (140, 100, 30)              # 3-D: 4 x 3 x 1 tiles, the ROI leaves the volume
VOL2, START2, SIZE2 = (7, 110, 150), (-5, 3, 1), (140, 100, 5)              # 2-D: 4 x 3 tiles in each of 5 sections
BOUNDARIES = ("zeros", "reflect", "edge")


class Case:
    """A raw stack, its Warp, the aligned volume A, and a Repair in both frames: the mask as the caller has it (raw) and
    as volume_warp_field(mask, nearest=True) moves it (aligned)."""

    def __init__(self, shape, seed, sections, field=True):
        from transfer_em_amd.utils import Repair, Warp, volume_warp, volume_warp_field
        self.shape, self.vol = shape, ramp_volume(shape, seed)
        self.M, self.U = C.stack(shape, seed=seed, field=field)
        self.W = Warp(self.M, self.U, C.SPACING if field else None, fill=FILL)
        mask = np.zeros(shape, np.uint8)
        mask[shape[0] // 3:shape[0] // 3 + 2 * GAP + 2, 30:70, 50:110] = 9    # a blob thicker than 2 GAP: a middle stays
        mask[:, 5, 6] = 1
        align = (lambda v, **kw: volume_warp_field(v, self.M, self.U, C.SPACING, **kw)) if field else \
            (lambda v, **kw: volume_warp(v, self.M, **kw))
        self.A, self.mask, self.mask_A = align(self.vol, fill=FILL), mask, align(mask, nearest=True)
        assert np.array_equal(self.A, C.warp(self.vol, self.M, self.U, fill=FILL))
        assert np.array_equal(self.mask_A, C.warp(mask, self.M, self.U, nearest=True)) and (self.mask_A != mask).mean() > 0.002
        inside = np.stack([C.positions(self.M[z], None if self.U is None else self.U[z], ((0, shape[1]), (0, shape[2])),
                                       shape[1:])[2] for z in range(shape[0])])
        assert 50 < (~inside).sum() < inside.size // 20 and (self.A[~inside] == FILL).all()      # some voxels receive fill
        self.raw = Repair(sections=sections, mask=mask, max_gap=GAP)
        self.aligned = Repair(sections=sections, mask=self.mask_A, max_gap=GAP)


@pytest.fixture(scope="module")
def model3(tmp_path_factory):
    return _model(tmp_path_factory.mktemp("warp3"), "warp3", True)


@pytest.fixture(scope="module")
def model2(tmp_path_factory):
    return _model(tmp_path_factory.mktemp("warp2"), "warp2", False)


@pytest.fixture(scope="module")
def case3():
    return Case(VOL, 91, [0, 11, 12, 29])


@pytest.fixture(scope="module")
def case2():
    return Case(VOL2, 92, [0, 3, 6])


def _eq(a, b):
    assert a.shape == b.shape and np.array_equal(a, b), np.argwhere(a != b)[:5]


def _levels(r):
    return r if isinstance(r, list) else [r]


STREAMED = (((1, 1, 1), None), ((1, 2, 3), 5), (None, None))                 # (chunk_tiles, tile_batch)


def _all_ways(model, case, start, size, repair=False, spread=False, **kw):
    """predict_cube(warp=W) on the raw stack against predict_cube on A -- fetch_input is A's ROI --, and
    predict_volume(warp=W) in chunks of one tile, of 2 x 3 tiles in batches of 5, and with its default chunks against
    the same.  `repair`: the raw-frame Repair with the keyword, the aligned one without.  `spread`: the map too."""
    from transfer_em_amd.utils import predict_cube, predict_volume
    shape = (size[2], size[1], size[0])
    raw_kw, aligned_kw = dict(kw), dict(kw)
    if repair:
        raw_kw["repair"], aligned_kw["repair"] = case.raw, case.aligned
    maps = []

    def more(d):                                # a fresh spread map per call
        if spread:
            maps.append(np.full(shape, 255, np.uint8))
            return dict(d, spread=maps[-1])
        return d
    want_in, want = predict_cube(case.A, start, size, model, MS_X, MS_Y, fetch_input=True, **more(aligned_kw))
    got_in, got = predict_cube(case.vol, start, size, model, MS_X, MS_Y, fetch_input=True, warp=case.W, **more(raw_kw))
    first = _levels(want)[0]
    # not the check, its precondition: a flat prediction, or one that the warp does not reach, would make it vacuous
    assert first.std() > 10 and len(np.unique(first)) >= 16
    assert not np.array_equal(_levels(predict_cube(case.vol, start, size, model, MS_X, MS_Y, **raw_kw))[0], first)
    _eq(got_in, want_in)
    for g, w in zip(_levels(got), _levels(want)):
        _eq(g, w)
    for chunk_tiles, tile_batch in STREAMED:
        st = {}
        res = predict_volume(case.vol, start, size, model, MS_X, MS_Y, chunk_tiles=chunk_tiles, tile_batch=tile_batch,
                             warp=case.W, stats=st, **more(raw_kw))
        assert len(_levels(res)) == len(_levels(want))
        for g, w in zip(_levels(res), _levels(want)):
            _eq(g, w)
        assert st["warp_read_voxels"] >= st["footprint_voxels"] > 0           # equal where one chunk is the whole volume
        if chunk_tiles == (1, 1, 1):            # cut boxes: the taps' margin is read on top of the footprint
            assert st["chunks"] == 12 * (1 if model.generator_g.is3d else size[2])
            assert st["warp_read_voxels"] > st["footprint_voxels"]
    for m in maps[1:]:
        _eq(m, maps[0])
    assert not spread or (len(maps) == 5 and maps[0].std() > 1)               # the map was written, and is not flat
    return want_in


# ------------------------------------------------------------------------------------------------------- equalities
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_predict_3d_with_warp_equals_predict_on_the_aligned_volume(model3, case3, boundary):
    want_in = _all_ways(model3, case3, START, SIZE, boundary=boundary)
    if boundary == "zeros":
        z0, y0, x0 = -START[2], START[1], -START[0]
        _eq(want_in[z0:, :, x0:], case3.A[:SIZE[2] - z0, y0:y0 + SIZE[1], :SIZE[0] - x0])     # A's ROI ...
        assert (want_in[:z0] == 0).all() and (want_in[:, :, :x0] == 0).all()                  # ... and 0 outside, not fill


def _combined(case, boundary):
    """repair in both frames, a per-section lut, the CLAHE tables of the aligned and repaired volume, the flips ensemble
    with its spread map, and one mip level."""
    from transfer_em_amd.utils import clahe_fit, volume_repair
    Z = case.shape[0]
    t = (255 - (np.arange(256) // 2) * 2).astype(np.uint8)
    return dict(boundary=boundary, ensemble="flips", mips=1, lut=np.stack([np.roll(t, z) for z in range(Z)]),
                clahe=clahe_fit(volume_repair(case.A, case.aligned), (16, 24)), repair=True, spread=True)


def test_predict_3d_with_warp_composes(model3, case3):
    _all_ways(model3, case3, START, SIZE, **_combined(case3, "reflect"))


def test_predict_3d_with_warp_and_repair(model3, case3):
    """The mask is given in the raw frame and moved with nearest; the sections are the aligned volume's."""
    from transfer_em_amd.utils import Repair, predict_cube
    _all_ways(model3, case3, START, SIZE, repair=True)
    wrong = predict_cube(case3.A, START, SIZE, model3, MS_X, MS_Y, repair=Repair(sections=[0, 11, 12, 29], mask=case3.mask, max_gap=GAP))
    right = predict_cube(case3.A, START, SIZE, model3, MS_X, MS_Y, repair=case3.aligned)
    assert not np.array_equal(wrong, right)                                    # the other frame gives another result


def test_predict_3d_with_maps_alone(model3):
    """No fields: A is volume_warp's, and the launches are the affine form's."""
    _all_ways(model3, Case(VOL, 93, [2], field=False), START, SIZE, boundary="edge")


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_predict_2d_with_warp_equals_predict_on_the_aligned_volume(model2, case2, boundary):
    _all_ways(model2, case2, START2, SIZE2, boundary=boundary)


def test_predict_2d_with_warp_composes(model2, case2):
    _all_ways(model2, case2, START2, SIZE2, **_combined(case2, "edge"))


def test_single_image(model2, case2):
    """One image [y, x] takes one map and one field; a quantised map [6] and a float map [2, 3] are the same call."""
    from transfer_em_amd.utils import Warp, predict_cube, predict_volume
    z, (start, size) = 4, (START2[:2], SIZE2[:2])
    want_in, want = predict_cube(case2.A[z], start, size, model2, MS_X, MS_Y, fetch_input=True, boundary="reflect")
    assert want.std() > 10
    for W in (Warp(case2.M[z], case2.U[z], C.SPACING, FILL),
              Warp(case2.M[z].reshape(2, 3) / 65536.0, case2.U[z] / 65536.0, (C.SPACING, C.SPACING), FILL)):
        got_in, got = predict_cube(case2.vol[z], start, size, model2, MS_X, MS_Y, fetch_input=True, boundary="reflect", warp=W)
        _eq(got_in, want_in), _eq(got, want)
        for chunk_tiles in ((1, 1, 1), None):
            _eq(predict_volume(case2.vol[z], start, size, model2, MS_X, MS_Y, boundary="reflect", chunk_tiles=chunk_tiles,
                               warp=W), want)


def test_predict_volume_with_warp_across_ranks_and_with_compare(model3, case3, tmp_path):
    """Two ranks write disjoint chunks of one memmap from a memmap; the ground truth lives in the aligned frame."""
    from transfer_em_amd.utils import predict_cube, predict_volume
    gt = ramp_volume(VOL, 94)
    st_w = {}
    want = predict_cube(case3.A, START, SIZE, model3, MS_X, MS_Y, compare=gt, stats=st_w, repair=case3.aligned)
    src = np.memmap(tmp_path / "raw.u8", np.uint8, "w+", shape=VOL)
    src[...] = case3.vol
    out = np.memmap(tmp_path / "out.u8", np.uint8, "w+", shape=want.shape)
    joint, read, foot = np.zeros((256, 256), np.int64), 0, 0
    for rank in (0, 1):
        st = {}
        predict_volume(src, START, SIZE, model3, MS_X, MS_Y, out=out, chunk_tiles=(1, 1, 2), tile_batch=1, rank=rank,
                       world_size=2, warp=case3.W, repair=case3.raw, compare=gt, stats=st)
        joint, read, foot = joint + st["joint_histogram"], read + st["warp_read_voxels"], foot + st["footprint_voxels"]
        assert st["chunks"] == 3
    _eq(np.asarray(out), want)
    assert np.array_equal(joint, st_w["joint_histogram"]) and read > foot > 0


# -------------------------------------------------------------------------------------------- what the cases cover
def _chunk_boxes(case, start, size, is3d, chunk_tiles=(1, 1, 1)):
    from transfer_em_amd import utils
    chunks = utils.chunk_plan(start, size, 36, 19, case.shape, chunk_tiles, is3d=is3d)
    return chunks, utils._warp_footprints(chunks, 0, utils._check_warp(case.W, case.shape), case.shape, False)


@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
def test_the_cases_are_not_vacuous(case3, case2, is3d):
    """From the planner, on the host: with chunks of one tile some source box is cut on both sides in x (and in y), one
    touches each face of the section, at least half of the chunks read more than their footprint, and no box is more
    than 16 columns wider than its footprint: a fraction of the section's width, which whole rows would read."""
    case, start, size = (case3, START, SIZE) if is3d else (case2, START2, SIZE2)
    Y, X = case.shape[1:]
    chunks, (foot, sbox, _) = _chunk_boxes(case, start, size, is3d)
    assert len(chunks) == 12 * (1 if is3d else SIZE2[2]) and all(f is not None and s is not None for f, s in zip(foot, sbox))
    assert any(x0 > 0 and x1 < X for _, (x0, x1) in sbox) and any(y0 > 0 and y1 < Y for (y0, y1), _ in sbox)
    assert any(x0 == 0 for _, (x0, _) in sbox) and any(x1 == X for _, (_, x1) in sbox)
    assert any(y0 == 0 for (y0, _), _ in sbox) and any(y1 == Y for (_, y1), _ in sbox)
    area = lambda b: (b[0][1] - b[0][0]) * (b[1][1] - b[1][0])
    larger = [area(s) > area(f[1:]) for f, s in zip(foot, sbox)]
    assert sum(larger) >= len(chunks) // 2
    for f, s in zip(foot, sbox):                # a footprint's width against the section's: what whole rows would read
        assert (s[1][1] - s[1][0]) <= (f[2][1] - f[2][0]) + 2 * 8 < X


def test_a_footprint_without_a_source_is_filled(model2):
    """Sections moved wholly out of themselves have no source box: predict_volume reads nothing for them and the
    network sees `fill`; the call still equals the one on the aligned volume."""
    from transfer_em_amd.utils import Warp, predict_cube, predict_volume, volume_warp
    vol = ramp_volume(VOL2, 95)
    M = C.stack(VOL2, seed=95, field=False)[0].copy()
    M[2:5, 5] = 400 << 16                                                  # sections 2...4: 400 columns to the right
    W = Warp(M, fill=FILL)
    A = volume_warp(vol, M, fill=FILL)
    assert (A[2:5] == FILL).all() and A[1].std() > 10
    want = predict_cube(A, START2, SIZE2, model2, MS_X, MS_Y)
    st = {}
    reads = []

    class Spy:                                  # the volume as an array-like that records what is read
        shape, dtype = vol.shape, vol.dtype

        def __getitem__(self, key):
            reads.append(key)
            return vol[key]
    got = predict_volume(Spy(), START2, SIZE2, model2, MS_X, MS_Y, chunk_tiles=(1, 1, 1), warp=W, stats=st)
    _eq(got, want)
    assert st["chunks"] == 60 and len(reads) == 12 * 2                     # sections 1...5 of the ROI: only 1 and 5 are read
    assert all(k[0] in (slice(1, 2), slice(5, 6)) for k in reads)


def test_predict_without_warp_runs_the_unchanged_launches(model3, case3):
    """warp=None is the plain call; warp=W adds one tem_u8_warp_box per chunk, two with a mask, and nothing else; the
    resident call adds one per volume."""
    from transfer_em_amd.utils import predict_cube, predict_volume
    run = lambda **kw: predict_volume(case3.vol, START, SIZE, model3, MS_X, MS_Y, chunk_tiles=(1, 1, 1), **kw)
    _, plain = _counted(run)
    _, with_w = _counted(lambda: run(warp=case3.W))
    assert "tem_u8_warp_box" not in plain and with_w.pop("tem_u8_warp_box") == 12
    assert with_w == plain
    _, plain_r = _counted(lambda: run(repair=case3.raw))
    _, both = _counted(lambda: run(repair=case3.raw, warp=case3.W))
    assert both.pop("tem_u8_warp_box") == 24 and both == plain_r
    res = lambda **kw: predict_cube(case3.vol, START, SIZE, model3, MS_X, MS_Y, **kw)
    _, plain_c = _counted(res)
    _, with_c = _counted(lambda: res(warp=case3.W))
    assert with_c.pop("tem_u8_warp_box") == 1 and with_c == plain_c
    _, rep_c = _counted(lambda: res(repair=case3.raw))
    _, both_c = _counted(lambda: res(repair=case3.raw, warp=case3.W))
    assert both_c.pop("tem_u8_warp_box") == 2 and both_c == rep_c


def test_saved_model_form_takes_the_keyword(model3, case3, tmp_path):
    import os
    from transfer_em_amd import utils
    ckpt = model3.make_checkpoint(1)
    out_dir = str(tmp_path / "exported")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        utils.save_model(out_dir, ckpt, MS_X, MS_Y, size=74, is3d=True)
    finally:
        os.chdir(cwd)
    live = utils.predict_cube(case3.A, START, SIZE, model3, MS_X, MS_Y, boundary="edge")
    saved = utils.predict_volume_from_saved_model(case3.vol, START, SIZE, out_dir, chunk_tiles=(1, 2, 2), boundary="edge",
                                                  warp=case3.W)
    _eq(saved, live)
