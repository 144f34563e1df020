"""The host side of the shift measurement over a list of section pairs, without a GPU: section_pairs, the chunk plan
zshift_chunks_pairs, chain_pairs, suspect_sections, the `_pairs` verdicts against their `_at` siblings, and the pair-list
driver's logic run on the host with the numpy reference (zshift_pairs_ref) in place of the device passes, on the
fixture of drifting sections with a black section and two noise sections among them."""
import inspect
import os

import numpy as np
import pytest

import zshift_at_ref as AR
import zshift_pairs_ref as PR
from transfer_em_amd import utils
from transfer_em_amd.utils import (HIST_CHUNK_BYTES, BridgedShifts, SectionPairs, Shifts, chain_pairs, section_pairs,
                                   section_shift_sums_pairs, section_shifts_at, section_shifts_bridged,
                                   section_shifts_pairs, shift_counts_at, shift_counts_pairs, shift_positions,
                                   shift_scores_at, shift_scores_pairs, shift_subpixel_at, shift_subpixel_pairs,
                                   suspect_sections, zshift_chunks_at, zshift_chunks_pairs)


# ---------------------------------------------------------------------------------------------------- section_pairs
def test_section_pairs_bridge_the_skipped_sections():
    got = section_pairs(5)
    assert isinstance(got, SectionPairs) and got.pairs.dtype == np.int64 and got.broken == []
    assert got.pairs.tolist() == [[0, 1], [1, 2], [2, 3], [3, 4]]
    assert section_pairs(1).pairs.shape == (0, 2) and section_pairs(0).pairs.shape == (0, 2)
    assert section_pairs(6, [0]).pairs.tolist() == [[1, 2], [2, 3], [3, 4], [4, 5]]            # a skip at either end
    assert section_pairs(6, [5]).pairs.tolist() == [[0, 1], [1, 2], [2, 3], [3, 4]]
    assert section_pairs(6, (0, 1, 5)).pairs.tolist() == [[2, 3], [3, 4]]
    assert section_pairs(8, [3, 5, 6]).pairs.tolist() == [[0, 1], [1, 2], [2, 4], [4, 7]]      # runs of one and two
    assert section_pairs(8, np.array([6, 5, 3, 3])).pairs.tolist() == [[0, 1], [1, 2], [2, 4], [4, 7]]
    got = section_pairs(12, [2, 3, 4, 5, 8], max_lag=4)                                       # 1 -> 6 is lag 5
    assert got.pairs.tolist() == [[0, 1], [6, 7], [7, 9], [9, 10], [10, 11]] and got.broken == [(1, 6)]
    assert section_pairs(12, [2, 3, 4, 5, 8], max_lag=5).broken == []
    assert section_pairs(12, [2, 3, 4, 5, 8], max_lag=1).broken == [(1, 6), (7, 9)]
    assert section_pairs(4, range(4)).pairs.shape == (0, 2)
    far = section_pairs(20, range(1, 9), max_lag=8)
    assert far.broken == [(0, 9)] and section_pairs(20, range(1, 8), max_lag=8).pairs[0].tolist() == [0, 8]
    for a, kw in (((5, [5]), {}), ((5, [-1]), {}), ((5, [1.0]), {}), ((5, [True]), {}), ((5, 3), {}), ((5.0,), {}),
                  ((-1,), {}), ((5,), dict(max_lag=0)), ((5,), dict(max_lag=9)), ((5,), dict(max_lag=2.0))):
        with pytest.raises(ValueError):
            section_pairs(*a, **kw)
    assert utils.SHIFT_MAX_LAG == 8


# ---------------------------------------------------------------------------------------------- zshift_chunks_pairs
def _size(box):
    return int(np.prod([hi - lo for lo, hi in box]))


LISTS = {"chain": ((9, ()), None), "skips": ((9, (3, 6, 7)), None), "bridges": (None, [(2, 4), (5, 8)]),
         "fan": (None, [(0, 1), (0, 3), (1, 2), (1, 9), (4, 5), (8, 9)])}


@pytest.mark.parametrize("name", list(LISTS))
def test_chunks_hold_every_pair_once_with_its_reach_within_the_budget(name):
    Z, Y, X = shape = (10, 9, 5)
    plan, explicit = LISTS[name]
    pairs = np.array(explicit, np.int64) if plan is None else section_pairs(*plan).pairs
    for r, (lo, hi) in ((1, (0, 0)), (2, (-3, 0)), (2, (0, 5)), (8, (-2, 1)), (1, (-1024, 1024))):
        for budget in (None, Z * Y * X, 4 * Y * X, 3 * Y * X, 2 * Y * X, 2 * Y * X - 1, Y * X, 14 * X, 7 * X, 2 * X, X, 1):
            b = HIST_CHUNK_BYTES if budget is None else budget
            chunks = zshift_chunks_pairs(shape, pairs, r, (lo, hi), budget)
            rows = np.zeros((len(pairs), Y), np.int32)
            for (k0, k1), (y0, y1), (rz, ry, rx) in chunks:
                assert 0 <= k0 < k1 <= len(pairs) and 0 <= y0 < y1 <= Y and rx == (0, X)
                rows[k0:k1, y0:y1] += 1
                assert rz == (int(pairs[k0, 0]), int(pairs[k0:k1, 1].max()) + 1)   # the dense box of the run's sections
                assert all(rz[0] <= a and c < rz[1] for a, c in pairs[k0:k1].tolist())
                if (y0, y1) == (0, Y):                                              # whole sections: all rows
                    assert ry == (0, Y) and _size((rz, ry, rx)) <= b
                    top = pairs[k0, 1]
                    for a, c in pairs[k0 + 1:k1].tolist():                         # a chain: no gap in z inside a run
                        assert a <= top
                        top = max(top, c)
                else:                                                               # one pair's rows, with the reach
                    assert k1 == k0 + 1 and ry == (max(y0 - r + lo, 0), min(y1 + r + hi, Y))
                    assert _size((rz, ry, rx)) <= b or y1 - y0 == 1                 # one core row at the least
                    assert (rz[1] - rz[0]) * Y * X > b                              # only where the pair does not fit
            assert (rows == 1).all()                                                # once, or in row runs that tile it
            order = [(k0, y0) for (k0, _), (y0, _), _ in chunks]
            assert order == sorted(order)


def test_chunks_end_a_run_at_a_gap_and_cut_rows_where_a_pair_does_not_fit():
    shape = (12, 10, 4)
    pairs = [(0, 1), (1, 3), (3, 4), (6, 7), (7, 11)]
    assert zshift_chunks_pairs(shape, pairs, 1) == [((0, 3), (0, 10), ((0, 5), (0, 10), (0, 4))),
                                                    ((3, 5), (0, 10), ((6, 12), (0, 10), (0, 4)))]  # 5 is never read
    got = zshift_chunks_pairs(shape, pairs, 1, (-1, 2), 4 * 40)                    # four sections: (7, 11) needs five
    assert got[:3] == [((0, 2), (0, 10), ((0, 4), (0, 10), (0, 4))), ((2, 3), (0, 10), ((3, 5), (0, 10), (0, 4))),
                       ((3, 4), (0, 10), ((6, 8), (0, 10), (0, 4)))]
    # 160 bytes over 5 planes of 4 bytes: 8 rows, of which 2 r + hi - lo = 5 are halo: 3 core rows
    assert got[3:] == [((4, 5), (0, 3), ((7, 12), (0, 6), (0, 4))), ((4, 5), (3, 6), ((7, 12), (1, 9), (0, 4))),
                       ((4, 5), (6, 9), ((7, 12), (4, 10), (0, 4))), ((4, 5), (9, 10), ((7, 12), (7, 10), (0, 4)))]
    everything = zshift_chunks_pairs(shape, pairs, 1, (-1, 2), 4 * 40)
    for world in (1, 2, 3, 4):                                                      # round-robin over the ranks
        parts = [zshift_chunks_pairs(shape, pairs, 1, (-1, 2), 4 * 40, rk, world) for rk in range(world)]
        assert all(p == everything[rk::world] for rk, p in enumerate(parts))
    assert zshift_chunks_pairs(shape, np.zeros((0, 2), np.int64), 1) == []


def test_chunks_of_the_lag_1_chain_read_what_the_sibling_reads():
    for shape in ((7, 9, 5), (2, 9, 5), (10, 6, 8)):
        Z = shape[0]
        pairs = section_pairs(Z).pairs
        for r, reach in ((1, (0, 0)), (2, (-3, 1)), (8, (0, 4))):
            for budget in (None, 4 * shape[1] * shape[2], 3 * shape[1] * shape[2], 2 * shape[1] * shape[2],
                           2 * shape[1] * shape[2] - 1, 5 * shape[2], 1):
                at = zshift_chunks_at(shape, r, reach, budget)
                got = zshift_chunks_pairs(shape, pairs, r, reach, budget)
                # the sibling's cores cover the last section too, which has no pair: those slabs alone are missing
                want = [(core[1], read) for core, read in at if core[0][0] < Z - 1]
                assert [(rows, read) for _, rows, read in got] == want and want
                cores = [core[0] for core, _ in at if core[0][0] < Z - 1]      # a chunk's pairs: its core's sections
                assert [ks for ks, _, _ in got] == [(z0, min(z1, Z - 1)) for z0, z1 in cores]


def test_chunks_refuse_bad_arguments():
    ok = [(0, 1), (1, 3)]
    for kw in (dict(chunk_bytes=0), dict(chunk_bytes=-5), dict(rank=1), dict(rank=-1), dict(rank=2, world_size=2),
               dict(world_size=0), dict(reach=(1, 2)), dict(reach=(0, 1025)), dict(reach=None)):
        with pytest.raises(ValueError):
            zshift_chunks_pairs((4, 4, 4), ok, 2, **kw)
    for r in (0, 9, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            zshift_chunks_pairs((4, 4, 4), ok, r)
    for bad in ([(1, 3), (0, 1)], [(0, 1), (0, 1)], [(0, 2), (0, 1)], [(1, 1)], [(2, 1)], [(-1, 1)], [(0, 4)], [(0, 1, 2)],
                [0, 1], np.array(ok, np.float64), np.array(ok) == 0, None):
        with pytest.raises(ValueError):
            zshift_chunks_pairs((4, 4, 4), bad, 2)
    with pytest.raises(ValueError, match=r"pairs\[1\] = \(1, 10\)"):
        zshift_chunks_pairs((12, 4, 4), [(0, 8), (1, 10)], 2)                      # lag 9
    assert zshift_chunks_pairs((12, 4, 4), [(0, 8), (1, 9)], 2)
    for shape in ((4,), (1, 2, 3, 4)):
        with pytest.raises(ValueError):
            zshift_chunks_pairs(shape, ok, 2)


# ------------------------------------------------------------------------------------- chain_pairs, suspect_sections
def test_chain_pairs_spreads_every_kind_of_value_by_one_rule():
    pairs = section_pairs(8, [3, 5, 6]).pairs                                       # (0,1) (1,2) (2,4) (4,7)
    shifts = np.array([[1, -1], [2, -2], [30, -30], [4, -4]], np.int64)
    got = chain_pairs(pairs, shifts, 8)
    assert got.dtype == np.int64 and got.tolist() == [[1, -1], [2, -2], [30, -30], [0, 0], [4, -4], [0, 0], [0, 0]]
    P = shift_positions(got)                                     # a skipped section sits where the good one above it sits
    assert P[3].tolist() == P[4].tolist() == [33, -33] and P[5].tolist() == P[6].tolist() == P[7].tolist() == [37, -37]
    ident = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    maps = np.stack([ident + k for k in range(1, 5)])
    got = chain_pairs(pairs, maps, 8)
    assert got.dtype == np.float64 and got.shape == (7, 2, 3)
    assert all(np.array_equal(got[z], maps[k]) for k, z in enumerate((0, 1, 2, 4)))
    assert all(np.array_equal(got[z], ident) for z in (3, 5, 6))
    fields = np.random.default_rng(3).standard_normal((4, 3, 5, 2)).astype(np.float32)
    got = chain_pairs(pairs, fields, 8)
    assert got.dtype == np.float32 and got.shape == (7, 3, 5, 2)
    assert np.array_equal(got[[0, 1, 2, 4]], fields) and not got[[3, 5, 6]].any()
    base = np.arange(14, dtype=np.int64).reshape(7, 2) + 100
    got = chain_pairs(pairs[2:3], shifts[2:3], 8, base=base)                        # one bridge mends an alignment
    want = base.copy()
    want[2], want[3] = (30, -30), (0, 0)
    assert np.array_equal(got, want) and base[2].tolist() == [104, 105]             # a new array
    plan = section_pairs(12, [2, 3, 4, 5, 8], max_lag=4)                            # a broken gap keeps the base
    vals = np.arange(1, 11, dtype=np.int64).reshape(5, 2)
    got = chain_pairs(plan.pairs, vals, 12)
    assert got[[0, 6, 7, 9, 10]].tolist() == vals.tolist() and not got[[1, 2, 3, 4, 5, 8]].any()
    got = chain_pairs(plan.pairs, vals, 12, base=np.full((11, 2), 7, np.int64))
    assert (got[1:6] == 7).all() and got[8].tolist() == [0, 0]
    keep = np.array([0, 2, 3])                                                      # unresolved pairs: their rows dropped
    assert chain_pairs(pairs[keep], shifts[keep], 8).tolist() == [[1, -1], [0, 0], [30, -30], [0, 0], [4, -4], [0, 0], [0, 0]]
    assert chain_pairs(np.zeros((0, 2), np.int64), np.zeros((0, 2), np.int64), 3).tolist() == [[0, 0], [0, 0]]
    for bp, bv, kw in ((pairs, shifts[:3], {}), (pairs, shifts[:, :1], {}), (pairs, maps[:, :, :2], {}),
                       (pairs, shifts, dict(base=base[:6])), (pairs, shifts, dict(base=base.astype(np.float64))),
                       (pairs[::-1], shifts, {}), (pairs, shifts == 0, {}), (pairs, np.zeros((4, 2, 2, 3)), {})):
        with pytest.raises(ValueError):
            chain_pairs(bp, bv, 8, **kw)
    with pytest.raises(ValueError):
        chain_pairs(pairs, shifts, 7)                                               # (4, 7) is outside a stack of 7


def test_suspect_sections():
    assert suspect_sections([], 8) == []
    assert suspect_sections([2, 3], 8) == [3] and suspect_sections([2], 8) == []
    assert suspect_sections([2, 3, 4], 8) == [3, 4] and suspect_sections(np.array([4, 2, 3, 3]), 8) == [3, 4]
    assert suspect_sections([0], 8) == [0] and suspect_sections([6], 8) == [7] and suspect_sections([0, 6], 8) == [0, 7]
    assert suspect_sections([0], 2) == [0, 1] and suspect_sections([], 1) == [] and suspect_sections([], 0) == []
    assert suspect_sections([2, 3, 6, 7, 8], 12) == [3, 7, 8]
    for u, Z in (([7], 8), ([-1], 8), ([1.5], 8), ([True], 8), ([0], 1)):
        with pytest.raises(ValueError):
            suspect_sections(u, Z)


# ----------------------------------------------------------------------------------- the `_pairs` verdicts, host only
def test_the_pairs_verdicts_are_the_at_verdicts_row_for_row():
    got = AR.host_driver()                                       # the sibling's fixture: q[10], n[9], centers[9]
    q, n, C = got.q[:-1], got.n, got.centers
    assert np.array_equal(shift_counts_pairs(AR.BIG_SHAPE, AR.BIG_TILE, AR.BIG_RADIUS, C), n)
    assert shift_scores_pairs(q, n).tobytes() == shift_scores_at(got.q, n).tobytes()
    s, s_at = section_shifts_pairs(q, n, C), section_shifts_at(got.q, n, C)
    assert isinstance(s, Shifts) and s.unresolved == s_at.unresolved
    for a, b in zip(s[:4], s_at[:4]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    for a, b in zip(shift_subpixel_pairs(q, n, C), shift_subpixel_at(got.q, n, C)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    pick = [7, 2, 2]                                             # any rows, in any order: a row speaks of its own pair
    s3 = section_shifts_pairs(q[pick], n[pick], C[pick], min_corr=0.3)
    assert np.array_equal(s3.tiles, section_shifts_at(got.q, n, C, min_corr=0.3).tiles[pick])
    per_pair = np.array([[3, -2], [0, 5]], np.int64)             # one centre per pair broadcasts over the tiles
    n2 = shift_counts_pairs((9, 40, 50), 16, 2, per_pair)
    assert n2.shape == (2, 3, 4, 5, 5) and np.array_equal(n2, shift_counts_at((3, 40, 50), 16, 2, per_pair))
    assert shift_scores_pairs(np.zeros((0, 3, 4, 5, 5, 5), np.int64), np.zeros((0, 3, 4, 5, 5), np.int64)).shape == (0, 3, 4, 5, 5)
    for bq, bn, bc in ((q, n[:-1], C), (q, n.astype(np.float64), C), (q[..., :4], n, C), (q, n, C[:-1]),
                       (q, n, C.astype(np.float64)), (got.q, n, C), (q.astype(np.float32), n, C)):
        with pytest.raises(ValueError):
            section_shifts_pairs(bq, bn, bc)
        with pytest.raises(ValueError):
            shift_subpixel_pairs(bq, bn, bc)
    with pytest.raises(ValueError):
        shift_scores_pairs(got.q, n)
    with pytest.raises(ValueError):
        section_shifts_pairs(q, n, C, min_corr=0)
    with pytest.raises(ValueError):
        shift_counts_pairs(AR.BIG_SHAPE, AR.BIG_TILE, AR.BIG_RADIUS, C + 2000)


# ------------------------------------------------------------------------------------------- the driver, on the host
def test_the_fixture_is_what_it_claims():
    v, pairs = PR.bad_volume(), PR.bad_pairs()
    assert v.shape == PR.BAD_SHAPE == (12, 160, 192) and v.dtype == np.uint8
    assert not v[PR.BAD_BLACK].any() and PR.BAD_SKIP == (PR.BAD_BLACK,) + PR.BAD_NOISE
    assert {z: tuple(pairs[z]) for z in PR.BAD_JUMP} == PR.BAD_JUMP
    assert (np.abs(np.delete(pairs, list(PR.BAD_JUMP), axis=0) - np.array(PR.BAD_DRIFT)) <= 1).all()
    P = PR.bad_positions()
    for a, b in PR.chain_list().tolist():                        # section b at (y + dy, x + dx) is section a at (y, x)
        dy, dx = P[b] - P[a]
        va = v[a, max(0, -dy):160 - max(0, dy), max(0, -dx):192 - max(0, dx)].astype(np.int64)
        vb = v[b, max(0, dy):160 + min(0, dy), max(0, dx):192 + min(0, dx)].astype(np.int64)
        assert np.corrcoef(va.ravel(), vb.ravel())[0, 1] > (0.9 if b - a == 1 else 0.4), (a, b)
    for z in PR.BAD_NOISE:                                       # the noise resembles nothing, its neighbour included
        assert abs(np.corrcoef(v[z].ravel().astype(np.float64), v[z + 1].ravel().astype(np.float64))[0, 1]) < 0.05
    assert PR.chain_list().tolist() == [[0, 1], [1, 2], [2, 4], [4, 5], [5, 6], [6, 9], [9, 10], [10, 11]]
    assert [tuple(p) for p in PR.chain_list().tolist() if p[1] - p[0] > 1] == list(PR.BAD_BRIDGES)


def test_the_chain_alone_loses_the_displacement_across_every_bad_section():
    """The defect: the pairs around the bad sections are unresolved, get (0, 0), and every section above sits off by
    what they carried."""
    s = PR.host_plain().shifts
    assert s.unresolved == [2, 3, 6, 7, 8] and not s.pairs[s.unresolved].any()
    assert suspect_sections(s.unresolved, 12) == list(PR.BAD_SKIP)
    good = [z for z in range(11) if z not in s.unresolved]
    assert np.array_equal(s.pairs[good], PR.bad_pairs()[good])
    true = PR.bad_positions()
    off = shift_positions(s.pairs) - true
    lost24, lost69 = true[4] - true[2], true[9] - true[6]
    assert not off[:3].any() and (np.abs(lost24) > 12).all() and (np.abs(lost69) > 4).all()
    assert (off[4:7] == -lost24).all() and (off[9:] == -(lost24 + lost69)).all()


def test_the_bridged_driver_measures_across_the_bad_sections_exactly():
    got = PR.host_bridged()
    assert isinstance(got, BridgedShifts) and isinstance(got.shifts, Shifts)
    pairs, s, true = PR.chain_list(), got.shifts, PR.bad_positions()
    assert np.array_equal(got.pairs, pairs) and got.pairs.dtype == np.int64
    assert s.pairs.shape == (8, 2) and s.tiles.shape == (8, 5, 6, 2) and got.q.shape == (8, 5, 6, 9, 9, 5)
    assert got.n.shape == (8, 5, 6, 9, 9) and got.centers.shape == (8, 5, 6, 2)
    for k, (a, b) in enumerate(pairs.tolist()):
        print((a, b), "decided", int(s.decided[k].sum()), "of 30; smallest decided peak",
              float(s.peak[k][s.decided[k]].min()) if s.decided[k].any() else None)
        assert s.decided[k].sum() >= 0.5 * 30, (a, b)                               # min_decided, of every bridge too
    assert s.unresolved == []
    assert np.array_equal(s.pairs, np.array([true[b] - true[a] for a, b in pairs.tolist()]))
    P = shift_positions(chain_pairs(pairs, s.pairs, 12))
    good = [z for z in range(12) if z not in PR.BAD_SKIP]
    assert np.array_equal(P[good], true[good])                                      # every good section: exact
    assert all(P[z].tolist() == P[z + 1].tolist() for z in (3, 8)) and P[7].tolist() == P[9].tolist()
    # the verdict is section_shifts_pairs' on the returned sums, counts and centres
    again = section_shifts_pairs(got.q, got.n, got.centers)
    assert np.array_equal(again.pairs, s.pairs) and np.array_equal(again.tiles, s.tiles)
    assert np.array_equal(got.n, shift_counts_pairs(PR.BAD_SHAPE, PR.BAD_TILE, PR.BAD_RADIUS, got.centers))
    assert np.array_equal(got.q, PR.volume_sums_pairs(PR.bad_volume(), pairs, got.centers, (32, 32), 4))
    sub = shift_subpixel_pairs(got.q, got.n, got.centers)
    assert np.abs(sub.offsets - s.tiles)[s.decided].max() <= 0.5


def test_the_bridges_alone_give_the_same_rows_and_read_only_their_sections(monkeypatch):
    full, only = PR.host_bridged(), PR.host_bridged(True)
    rows = [2, 5]
    assert np.array_equal(only.pairs, np.array(PR.BAD_BRIDGES)) and only.shifts.unresolved == []
    assert np.array_equal(only.shifts.pairs, full.shifts.pairs[rows]) and np.array_equal(only.q, full.q[rows])
    assert np.array_equal(only.centers, full.centers[rows]) and np.array_equal(only.shifts.tiles, full.shifts.tiles[rows])
    base = PR.host_plain().shifts.pairs                          # an alignment that exists, mended by the bridges
    P = shift_positions(chain_pairs(only.pairs, only.shifts.pairs, 12, base=base))
    good = [z for z in range(12) if z not in PR.BAD_SKIP]
    assert np.array_equal(P[good], PR.bad_positions()[good])
    seen = []                                                    # the sections the rescales are asked for

    def rescale(volume, step, out=None, start=None, size=None, **kw):
        seen.append((start[2], start[2] + size[2]))
        return PR.host_rescale(volume, step, out, start, size)
    monkeypatch.setattr(utils, "volume_rescale", rescale)
    monkeypatch.setattr(utils, "section_shift_sums_pairs", PR.host_sums_pairs)
    coarse = [np.full((12, 160 >> l, 192 >> l), 9, np.uint8) for l in (1, 2, 3)]
    st = {}
    again = section_shifts_bridged(PR.bad_volume(), PR.BAD_BRIDGES, 32, 4, 3, coarse=coarse, stats=st)
    assert seen == [(2, 5), (6, 10)] * 3 and set(st) == {"read_s", "chunks"}
    assert np.array_equal(again.q, only.q) and np.array_equal(again.pairs, only.pairs)
    for c in coarse:                                             # the other sections of `coarse`: left as they are
        assert (c[[0, 1, 5, 10, 11]] == 9).all() and not (c[[2, 4, 6, 9]] == 9).all()
    assert np.array_equal(coarse[0][2:5], PR.halve(PR.bad_volume()[2:5]))
    assert [s for _, _, s in zshift_chunks_pairs(PR.BAD_SHAPE, PR.BAD_BRIDGES, 4)] == \
        [((2, 5), (0, 160), (0, 192)), ((6, 10), (0, 160), (0, 192))]


def test_the_lag_1_list_is_the_existing_driver_bit_for_bit():
    for v, levels in ((AR.big_jump_volume(), AR.BIG_LEVELS), (PR.bad_volume(), PR.BAD_LEVELS), (PR.bad_volume()[:, :64, :96], 2)):
        Z = v.shape[0]
        want = PR.host_run(utils.section_shifts_coarse_to_fine, v, 32, 4, levels)
        got = PR.host_run(section_shifts_bridged, v, section_pairs(Z).pairs, 32, 4, levels)
        for a, b in zip(got.shifts[:4], want.shifts[:4]):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        assert got.shifts.unresolved == want.shifts.unresolved
        assert got.q.tobytes() == want.q[:-1].tobytes() and not want.q[-1].any()
        assert got.n.tobytes() == want.n.tobytes() and got.centers.tobytes() == want.centers.tobytes()
    want = AR.host_driver()                                      # and the sibling's own host stand-ins agree with these
    got = PR.host_run(utils.section_shifts_coarse_to_fine, AR.big_jump_volume(), 32, 4, 3)
    assert got.q.tobytes() == want.q.tobytes() and got.shifts.unresolved == want.shifts.unresolved == [8]


def test_the_driver_and_the_pass_refuse_bad_arguments_on_the_host():
    v = np.zeros((5, 64, 80), np.uint8)
    ok = [(0, 1), (1, 3)]
    for a, kw in (((v.astype(np.int16), ok), {}), ((v[0], ok), {}), ((v, ok), dict(tile=0)), ((v, ok), dict(radius=9)),
                  ((v, ok), dict(levels=0)), ((v, ok), dict(levels=7)), ((v, ok), dict(levels=3)),
                  ((v, ok), dict(min_corr=0)), ((v, ok), dict(min_decided=1.5)), ((v, ok), dict(chunk_bytes=0)),
                  ((v, ok), dict(levels=1, coarse=[np.zeros((5, 32, 41), np.uint8)])),
                  ((v, [(1, 3), (0, 1)]), {}), ((v, [(0, 5)]), {}), ((v, [(0, 0)]), {}), ((v, None), {}),
                  ((v, np.array(ok, np.float32)), {}), ((np.zeros((12, 64, 80), np.uint8), [(0, 9)]), {})):
        with pytest.raises(ValueError):
            section_shifts_bridged(*a, **kw)
    zero = np.zeros((2, 2), np.int64)
    for a, kw in (((v.astype(np.int16), ok), {}), ((v, ok), dict(tile=0)), ((v, ok), dict(radius=9)),
                  ((v, ok), dict(chunk_bytes=0)), ((v, ok), dict(rank=1)), ((v, ok, zero[:1]), {}),
                  ((v, ok, zero.astype(np.float64)), {}), ((v, ok, zero + 1025), {}), ((v[0], ok), {}),
                  ((v, [(1, 3), (0, 1)]), {}), ((v, [(0, 1), (0, 1)]), {}), ((v, [(3, 5)]), {}), ((v, [(2, 1)]), {}),
                  ((v, np.zeros((2, 3), np.int64)), {}), ((v, ok, np.zeros((2, 2, 1, 2), np.int64)), {})):
        with pytest.raises(ValueError):
            section_shift_sums_pairs(*a, **kw)
    none = section_shift_sums_pairs(v, np.zeros((0, 2), np.int64), tile=32)         # no pairs: no sums, no GPU work
    assert none.shape == (0, 2, 3, 9, 9, 5) and none.dtype == np.int64


def test_signatures_the_reference_alias_and_the_export():
    import transfer_em.utils as alias
    from transfer_em_amd import _lib
    names = ("section_pairs", "SectionPairs", "zshift_chunks_pairs", "shift_counts_pairs", "section_shift_sums_pairs",
             "shift_scores_pairs", "section_shifts_pairs", "shift_subpixel_pairs", "section_shifts_bridged",
             "BridgedShifts", "suspect_sections", "chain_pairs", "SHIFT_MAX_LAG")
    for name in names:
        assert getattr(alias, name) is getattr(utils, name)
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(section_pairs) == ["Z", "skip", "max_lag"] and inspect.signature(section_pairs).parameters["max_lag"].default == 4
    assert sig(zshift_chunks_pairs) == ["vol_shape", "pairs", "radius", "reach", "chunk_bytes", "rank", "world_size"]
    assert sig(section_shift_sums_pairs) == ["volume", "pairs", "centers", "tile", "radius", "chunk_bytes", "rank",
                                             "world_size", "device", "stats"]
    assert sig(shift_scores_pairs) == ["q", "n"]
    assert sig(section_shifts_pairs) == sig(shift_subpixel_pairs) == ["q", "n", "centers", "min_corr"]
    assert sig(section_shifts_bridged) == ["volume", "pairs", "tile", "radius", "levels", "min_corr", "min_decided",
                                           "coarse", "chunk_bytes", "device", "stats"]
    d = {k: p.default for k, p in inspect.signature(section_shifts_bridged).parameters.items()}
    assert (d["tile"], d["radius"], d["levels"], d["min_corr"], d["min_decided"]) == (128, 4, 3, 0.1, 0.5)
    assert sig(suspect_sections) == ["unresolved", "Z"] and sig(chain_pairs) == ["pairs", "values", "Z", "base"]
    assert BridgedShifts._fields == ("pairs", "shifts", "q", "n", "centers")
    assert len(_lib._SIGS["tem_u8_zshift_tiles_pairs"]) == 22
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtem_hip.so is not built")
    import ctypes
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "tem_u8_zshift_tiles_pairs")
