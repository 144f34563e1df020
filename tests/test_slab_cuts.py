"""Every public slab cutter still cuts as it did when each pass restated the rule for itself.

tests/golden/slab_cuts.json was recorded by tests/golden/make_slab_cuts.py from the cutters BEFORE they were folded into
one private cutter and one budget check: per case the number of slabs, and per group of cases -- one cutter, shape, ROI
and parameter over all budgets and ranks -- a SHA-256 over the repr of every returned list.  The cases -- shapes, ROIs,
the budgets around every threshold, ranks, each cutter's own parameter at its ends -- are that script's; this test
recomputes them and compares.  CPU only."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slab_cuts.json")
CUTTERS = ("hist_chunks", "ssim_chunks", "zcorr_chunks", "zlag_chunks", "plane_lag_chunks", "zshift_chunks",
           "zshift_chunks_at", "repair_chunks", "outlier_chunks", "warp_chunks", "field_chunks", "rescale_chunks",
           "resample_z_chunks", "zshift_chunks_pairs")


@pytest.fixture(scope="module")
def tables():
    """(recorded, recomputed, case ids): {cutter: {group: ...}}, each once."""
    from transfer_em_amd import utils
    spec = importlib.util.spec_from_file_location("make_slab_cuts", os.path.join(os.path.dirname(GOLDEN), "make_slab_cuts.py"))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    with open(GOLDEN) as f:
        return (json.load(f),) + make.answers(utils)


def test_every_cutter_is_recorded(tables):
    recorded, got, ids = tables
    assert sorted(recorded) == sorted(got) == sorted(CUTTERS)
    assert sum(len(counts) for groups in recorded.values() for counts, _ in groups.values()) > 6000      # cases


@pytest.mark.parametrize("cutter", CUTTERS)
def test_cuts_are_the_recorded_ones(tables, cutter):
    recorded, got, ids = tables
    assert sorted(recorded[cutter]) == sorted(got[cutter])              # the same groups of cases
    for group, (counts, digest) in recorded[cutter].items():
        now, sha = got[cutter][group]
        assert len(now) == len(counts), f"{cutter} {group}: {len(now)} cases, {len(counts)} recorded"
        differ = [cid for cid, a, b in zip(ids[cutter][group], now, counts) if a != b]
        assert not differ, f"{cutter}: another number of slabs in {len(differ)} cases, first: {differ[:3]}"
        assert sha == digest, f"{cutter} {group}: the slab counts are the recorded ones, the slabs are not"
