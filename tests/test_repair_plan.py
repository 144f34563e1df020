"""Host side of the repair along z: the vectorised reference (repair_ref) against a per-voxel triple loop written here,
the locality claim on the slabs of repair_chunks, the slab plan itself, _check_repair's errors, flat_sections, and the
place of the `repair` keyword in the signatures.  No GPU is needed."""
import inspect
import itertools
from fractions import Fraction

import numpy as np
import pytest

import repair_ref as RR
from transfer_em_amd import utils as U
from transfer_em_amd.utils import Repair, _check_repair, flat_sections, repair_chunks


def naive(vol, sections, mask, missing, R):
    """The definition, voxel by voxel: (repaired copy, repaired, unrepaired)."""
    Z, Y, X = vol.shape
    bad = np.zeros(vol.shape, bool)
    for z, y, x in itertools.product(range(Z), range(Y), range(X)):
        bad[z, y, x] = ((sections is not None and z in sections) or (mask is not None and mask[z, y, x] != 0) or
                        (missing is not None and vol[z, y, x] == missing))
    out, rep, unrep = vol.copy(), 0, 0
    for z, y, x in itertools.product(range(Z), range(Y), range(X)):
        if not bad[z, y, x]:
            continue
        d0 = next((d for d in range(1, R + 1) if z - d >= 0 and not bad[z - d, y, x]), None)
        d1 = next((d for d in range(1, R + 1) if z + d <= Z - 1 and not bad[z + d, y, x]), None)
        if d0 is None and d1 is None:
            unrep += 1
            continue
        rep += 1
        if d0 is not None and d1 is not None:
            a, b, n = int(vol[z - d0, y, x]), int(vol[z + d1, y, x]), d0 + d1
            out[z, y, x] = (2 * (a * d1 + b * d0) + n) // (2 * n)
        else:
            out[z, y, x] = vol[z - d0, y, x] if d0 is not None else vol[z + d1, y, x]
    return out, rep, unrep


def run_mask(shape, R, seed):
    """A mask of bad runs along z of every length up to 2 R + 3, at random places."""
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, np.uint8)
    for _ in range(shape[1] * shape[2] * 2):
        y, x, n = rng.integers(shape[1]), rng.integers(shape[2]), rng.integers(1, 2 * R + 4)
        z = rng.integers(-n + 1, shape[0])
        m[max(z, 0):z + n, y, x] = rng.integers(1, 256)
    return m


SOURCES = [c for n in (1, 2, 3) for c in itertools.combinations(("sections", "mask", "missing"), n)]


@pytest.mark.parametrize("srcs", SOURCES, ids=["+".join(s) for s in SOURCES])
def test_reference_equals_the_definition_voxel_by_voxel(srcs):
    for seed, (shape, R) in enumerate([((1, 2, 3), 1), ((9, 3, 4), 1), ((14, 3, 3), 2), ((23, 2, 5), 3), ((12, 2, 2), 32)]):
        rng = np.random.default_rng(seed)
        vol = rng.integers(0, 4, shape, dtype=np.uint8) * 60 + rng.integers(0, 20, shape, dtype=np.uint8)
        sections = sorted(set(rng.integers(0, shape[0], 3).tolist())) if "sections" in srcs else None
        mask = run_mask(shape, R, seed + 50) if "mask" in srcs else None
        missing = int(vol[0, 0, 0]) if "missing" in srcs else None
        want = naive(vol, sections, mask, missing, R)
        got = RR.repair(vol, sections, mask, missing, R, counts=True)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (shape, R)
        assert np.array_equal(RR.repair(vol, sections, mask, missing, R), want[0])
        good = ~RR.bad_voxels(vol, sections, mask, missing)
        assert np.array_equal(got[0][good], vol[good])                      # good voxels are never changed


def test_reference_rounds_half_up_and_weights_the_nearer_voxel_more():
    col = lambda *v: np.array(v, np.uint8).reshape(-1, 1, 1)
    assert RR.repair(col(10, 0, 0, 0, 50), missing_value=0).ravel().tolist() == [10, 20, 30, 40, 50]
    assert RR.repair(col(0, 9, 1), sections=[1]).ravel().tolist() == [0, 1, 1]              # 0.5 -> 1
    assert RR.repair(col(0, 7, 7, 1), sections=[1, 2]).ravel().tolist() == [0, 0, 1, 1]      # 1/3 -> 0, 2/3 -> 1
    # max_gap 1: a run of 3 keeps its middle; of 2 is copied from each side
    assert RR.repair(col(10, 0, 0, 0, 50), missing_value=0, max_gap=1, counts=True)[1:] == (2, 1)
    assert RR.repair(col(10, 0, 0, 0, 50), missing_value=0, max_gap=1).ravel().tolist() == [10, 10, 0, 50, 50]
    assert RR.repair(col(10, 0, 0, 50), missing_value=0, max_gap=1).ravel().tolist() == [10, 10, 50, 50]
    assert RR.repair(col(0, 0, 50, 0), missing_value=0, max_gap=3).ravel().tolist() == [50, 50, 50, 50]
    assert RR.repair(col(0, 0, 0), missing_value=0, counts=True)[1:] == (0, 3)              # a wholly bad column


@pytest.mark.parametrize("R", [1, 2, 5])
def test_a_slab_cropped_to_its_core_is_the_whole_result(R):
    """The locality claim: a voxel needs the sections [z - R, z + R] of its column only."""
    shape = (40, 6, 7)
    rng = np.random.default_rng(R)
    vol = rng.integers(1, 256, shape, dtype=np.uint8)
    mask = run_mask(shape, R, 70 + R)
    longest = max(len(list(g)) for y in range(6) for x in range(7)
                  for k, g in itertools.groupby(mask[:, y, x] != 0) if k)
    assert longest > 2 * R, longest                                         # runs that keep an untouched middle
    sections = [0, 17, 18, shape[0] - 1]
    whole = RR.repair(vol, sections, mask, None, R)
    box = ((3, 38), (1, 6), (0, 7))
    for budget in (10 ** 9, (2 * R + 3) * 35, 60, 1):                       # one slab; section runs; row cuts; one row
        chunks = repair_chunks(box, shape, R, budget)
        assert len(chunks) >= (1 if budget == 10 ** 9 else 2)
        for core, read in chunks:
            sl = tuple(slice(lo, hi) for lo, hi in read)
            sec = [z - read[0][0] for z in sections if read[0][0] <= z < read[0][1]]
            part = RR.repair(vol[sl], sec or None, mask[sl], None, R)
            c = tuple(slice(lo - r[0], hi - r[0]) for (lo, hi), r in zip(core, read))
            assert np.array_equal(part[c], whole[tuple(slice(lo, hi) for lo, hi in core)]), (budget, core)


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("budget", [None, 800, 300, 40, 1])
def test_cores_partition_the_roi_and_read_slabs_hold_their_halo(budget, world):
    shape, R = (30, 9, 11), 3
    box = ((2, 29), (1, 8), (3, 11))
    count = np.zeros(shape, int)
    total = 0
    for rank in range(world):
        chunks = repair_chunks(box, shape, R, budget, rank, world)
        total += len(chunks)
        for core, read in chunks:
            count[tuple(slice(lo, hi) for lo, hi in core)] += 1
            assert read[0] == (max(core[0][0] - R, 0), min(core[0][1] + R, shape[0])) and read[1:] == core[1:]
            assert core[2] == box[2]                                        # x is never cut
            nbytes = int(np.prod([hi - lo for lo, hi in read]))
            one_row = (read[0][1] - read[0][0]) * (box[2][1] - box[2][0])
            if budget is not None:
                assert nbytes <= budget or (core[1][1] - core[1][0] == 1 and nbytes == one_row), (core, read)
    want = np.zeros(shape, int)
    want[tuple(slice(lo, hi) for lo, hi in box)] = 1
    assert np.array_equal(count, want)
    everything = repair_chunks(box, shape, R, budget)
    assert total == len(everything)
    assert [c for r in range(world) for c in repair_chunks(box, shape, R, budget, r, world)] == \
        [c for r in range(world) for c in everything[r::world]]
    if budget == 300:                                                       # 7 x 8 = 56 bytes a plane: 5 planes, no core
        assert all(c[0][1] - c[0][0] == 1 and c[1] != box[1] for c, _ in everything)       # ... rows of one section
    if budget == 800:                                                       # 14 planes: cores of 8 sections
        assert all(c[1] == box[1] for c, _ in everything) and len(everything) > 1


def test_repair_chunks_refuses_what_hist_chunks_refuses():
    box = ((0, 4), (0, 4), (0, 4))
    assert repair_chunks(((2, 2), (0, 4), (0, 4)), (4, 4, 4), 2) == []
    for kw in (dict(chunk_bytes=0), dict(rank=2, world_size=2), dict(rank=-1)):
        with pytest.raises(ValueError):
            repair_chunks(box, (4, 4, 4), 2, **kw)
    for gap in (0, 33, 1.5, True):
        with pytest.raises(ValueError, match="max_gap"):
            repair_chunks(box, (4, 4, 4), gap)


def test_check_repair():
    shape = (6, 4, 5)
    mask = np.zeros(shape, np.uint8)
    assert _check_repair(None, shape) is None
    spec = _check_repair(Repair(sections=(4, 1, 4), mask=mask, missing_value=np.uint8(255), max_gap=np.int64(32)), shape)
    assert spec.flags.dtype == np.uint8 and spec.flags.tolist() == [0, 1, 0, 0, 1, 0]
    assert spec.mask is mask and spec.missing == 255 and spec.max_gap == 32
    spec = _check_repair(Repair(missing_value=0), shape)
    assert spec.flags is None and spec.mask is None and spec.missing == 0 and spec.max_gap == 8
    assert _check_repair(spec, shape) is spec
    assert Repair() == (None, None, None, 8)
    bad = [(Repair(), "no bad voxel"),
           (Repair(max_gap=3), "no bad voxel"),
           (Repair(sections=[1], max_gap=0), "max_gap"), (Repair(sections=[1], max_gap=33), "max_gap"),
           (Repair(sections=[1], max_gap=2.0), "max_gap"), (Repair(sections=[1], max_gap=True), "max_gap"),
           (Repair(sections=[6]), "outside"), (Repair(sections=[-1]), "outside"), (Repair(sections=[1.5]), "section"),
           (Repair(sections=3), "sections"),
           (Repair(mask=np.zeros((6, 4, 4), np.uint8)), "shape"), (Repair(mask=mask.astype(bool)), "uint8"),
           (Repair(mask=mask.tolist()), "uint8"),
           (Repair(missing_value=256), "missing_value"), (Repair(missing_value=-1), "missing_value"),
           (Repair(missing_value=0.0), "missing_value"),
           ("sections", "Repair"), ((1, 2), "Repair")]
    for rp, msg in bad:
        with pytest.raises(ValueError, match=msg):
            _check_repair(rp, shape)
    with pytest.raises(ValueError, match="z"):                              # one image has no z
        _check_repair(Repair(missing_value=0), (4, 5))
    assert _check_repair(Repair(sections=[]), shape).flags.tolist() == [0] * 6          # an empty list is a source


def test_volume_repair_checks_come_before_any_gpu_work(monkeypatch):
    from transfer_em_amd import hip_ops
    monkeypatch.setattr(hip_ops, "require_gpu", lambda: pytest.fail("GPU work before the checks"))
    vol = np.zeros((6, 4, 5), np.uint8)
    for args, kw in [((vol, Repair()), {}), ((vol, None), {}), ((vol.astype(np.int16), Repair(missing_value=0)), {}),
                     ((vol, Repair(missing_value=0)), dict(start=(0, 0, 4), size=(5, 4, 3))),
                     ((vol, Repair(missing_value=0)), dict(out=np.zeros((6, 4, 4), np.uint8))),
                     ((vol, Repair(missing_value=0)), dict(out=np.zeros((6, 4, 5), np.int8))),
                     ((vol, Repair(missing_value=0)), dict(chunk_bytes=0)),
                     ((vol[0], Repair(missing_value=0)), {})]:
        with pytest.raises(ValueError):
            U.volume_repair(*args, **kw)


def test_flat_sections():
    h = np.zeros((7, 256), np.int64)
    h[0, 0] = 100                                       # blank
    h[1, 255], h[1, 3] = 51, 49                         # saturated, above one half
    h[2, 7], h[2, 8] = 50, 50                           # a tie exactly at one half: flagged
    h[3, 7], h[3, 8], h[3, 9] = 49, 49, 2               # just below
    h[4, :100] = 1                                      # ordinary
    h[6, 200] = 1                                       # one pixel  (5: an empty section, not flagged)
    assert flat_sections(h) == [0, 1, 2, 6]
    assert flat_sections(h, Fraction(51, 100)) == [0, 1, 6]
    assert flat_sections(h, (49, 100)) == [0, 1, 2, 3, 6]
    assert flat_sections(h, 1) == [0, 6]
    assert flat_sections(h.astype(np.uint32)[:0]) == []
    big = np.zeros((1, 256), np.int64)
    big[0, 1], big[0, 2] = 2 ** 62 // 3 + 1, 2 ** 62 // 3          # Python integers: no overflow in max * den
    assert flat_sections(big, Fraction(1, 2)) == [0] and flat_sections(big, Fraction(2, 3)) == []
    for bad in (h[0], h.astype(float), h[:, :255], -h):
        with pytest.raises(ValueError):
            flat_sections(bad)
    for f in (0, Fraction(3, 2), 0.5, "1/2", (1, 0), True):
        with pytest.raises(ValueError, match="fraction"):
            flat_sections(h, f)


def test_repair_keyword_in_the_signatures():
    for fn in (U.predict_cube, U.predict_volume):
        params = inspect.signature(fn).parameters
        assert params["repair"].default is None
        names = list(params)
        assert names[-2:] == ["spread", "spread_gain"] and names[-3] == "repair" and names[-4] == "compare"
    for fn in (U.predict_ng_cube, U.predict_cube_from_saved_model):
        assert "repair" not in inspect.signature(fn).parameters
    assert list(inspect.signature(U.volume_repair).parameters) == [
        "volume", "repair", "out", "start", "size", "chunk_bytes", "stats", "rank", "world_size", "device"]
    assert Repair._fields == ("sections", "mask", "missing_value", "max_gap")
