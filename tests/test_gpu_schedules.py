"""Every stream schedule cgan._CompiledStep can build, held to the flat launch order bit for bit.

Which schedule a process gets depends on its environment (GPU_MAX_HW_QUEUES, TEM_SIDE_SPLIT, TEM_BWW_TAIL, use_graph); the
rest of the suite runs under the queue count it inherits and so executes one of them.  Each test here starts
tests/tools/step_schedules.py as a fresh process with GPU_MAX_HW_QUEUES=8 (the count has to be in place before HIP
initialises) and compares what it dumped.  The child asserts which schedule was built and runs the structural checks of
the lists (every launch once, one record per waited event, every kernel gradient of a tail behind a wait for the event of
the launch that wrote its gradient); it exits non-zero with the offending item named, and the test prints its output.

Every kernel is deterministic and every variant runs the same launches on the same buffers, so ANY difference from the
flat order is a missing or wrong event.  The linearisations run a schedule's lists serially under every priority
permutation of the lists (util.linearise): a dependency no event declares is broken by the order that ranks the consumer's
list first -- no reliance on a race showing up by chance.  The control drops one wait and must differ.

Wall time of each job on the MI355X box, whole child process (python and torch start-up included); the limits below are
about 3 x these:
    eager 74^3 fp32 (5 variants)                3.2 s        graph 74^3 fp32 (3 variants)       2.8 s
    linearisations 74^3 fp32 (54 orders + control) 4.8 s     74^3 bf16 (2 variants + 24 orders) 3.7 s
    74^2 batch 2 (2 variants)                   2.5 s        132^3 fp32 (2 variants)            2.7 s
(of which the child's own work -- building the plans, the steps, the dumps -- is 0.6 .. 1.6 s).
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "tools", "step_schedules.py")
KEYS = ["losses", "grad_all"] + [f"{net}.{which}" for net in ("g", "f", "dx", "dy") for which in ("theta", "m", "v")]


def _job(rank_launcher, tmp_path, timeout, *args):
    res = rank_launcher([sys.executable, TOOL, str(tmp_path)] + list(args), ranks=1, env={"GPU_MAX_HW_QUEUES": "8"},
                        timeout=timeout)
    print(res["tail"][0])
    assert res["rc"] == [0], res["tail"][0]
    return lambda name: np.load(os.path.join(tmp_path, name + ".npz"))


def _variants_equal_flat(load, tags, nlists):
    flat = load("flat")
    assert flat["losses"].shape == (3, 7) and np.isfinite(flat["losses"]).all()
    assert not np.array_equal(flat["g.theta"][0], flat["g.theta"][2])            # the three steps did move the state
    for tag in tags:
        got = load(tag)
        assert int(got["nlists"]) == nlists[tag], tag
        for key in KEYS:                       # the losses: float64 accumulators read back as fp32, compared exactly
            assert np.array_equal(got[key], flat[key]), (tag, key, [bool(np.array_equal(a, b)) for a, b in zip(got[key], flat[key])])
    return flat


def _linearisations_equal_flat(load, tag, flat, nlists):
    lin = load("lin_" + tag)
    perms = sorted({k.split("/")[0] for k in lin.files})
    assert len(perms) == {3: 6, 4: 24}[nlists] and all(len(p) == nlists for p in perms), perms
    bad = [(p, key) for p in perms for key in KEYS if not np.array_equal(lin[f"{p}/{key}"], flat[key][0])]
    assert not bad, (tag, bad[:8])


NLISTS = dict(five=4, tail1=4, tail0=4, three=3, graph=3, graph_split=4)
T_EAGER, T_GRAPH, T_LIN, T_BF16, T_2D, T_132 = 10, 9, 15, 12, 8, 9       # s, per child job: 3 x the docstring's figures


def test_eager_schedules_74_fp32(tmp_path, rank_launcher):
    """3-D 74^3, batch 1, fp32 (72^3, 70^3 and 32^3 are Winograd layers: forward, kernel gradients and the slab split all
    run): five lists with all / the last / no kernel gradients in the tails, and three lists."""
    load = _job(rank_launcher, tmp_path, T_EAGER, "variants=flat,five,tail1,tail0,three")
    _variants_equal_flat(load, ("five", "tail1", "tail0", "three"), NLISTS)


def test_graph_schedules_74_fp32(tmp_path, rank_launcher):
    """use_graph at 8 queues: the default (three branches) and TEM_SIDE_SPLIT=1 (four; the kernel gradients stay in the
    chains under capture).  Step 0 eager, step 1 captured and replayed, step 2 replayed; the child asserts the graph exists."""
    load = _job(rank_launcher, tmp_path, T_GRAPH, "variants=flat,graph,graph_split")
    _variants_equal_flat(load, ("graph", "graph_split"), NLISTS)


def test_linearisations_74_fp32(tmp_path, rank_launcher):
    """Every priority permutation of five (24), tail1 (24) and three (6) gives flat's step 0; the control -- five without
    the wait in front of g1's first kernel gradient, that list first -- does not."""
    load = _job(rank_launcher, tmp_path, T_LIN, "variants=flat", "lin=five,tail1,three", "teeth")
    flat = load("flat")
    for tag in ("five", "tail1", "three"):
        _linearisations_equal_flat(load, tag, flat, NLISTS[tag])
    teeth, ng = load("teeth"), int(flat["counts"][0])
    assert np.isfinite(teeth["grad_all"]).all()
    assert not np.array_equal(teeth["grad_all"][:ng], flat["grad_all"][0][:ng])


def test_schedules_74_bf16(tmp_path, rank_launcher):
    load = _job(rank_launcher, tmp_path, T_BF16, "precision=bf16", "variants=flat,five", "lin=five")
    flat = _variants_equal_flat(load, ("five",), NLISTS)
    _linearisations_equal_flat(load, "five", flat, 4)


def test_schedules_74_2d_batch2(tmp_path, rank_launcher):
    load = _job(rank_launcher, tmp_path, T_2D, "dim=2", "batch=2", "variants=flat,five")
    _variants_equal_flat(load, ("five",), NLISTS)


def test_schedules_132_fp32(tmp_path, rank_launcher):
    """The benchmark's size: the large grids overlap most here, and the early slab sum has its full row count."""
    load = _job(rank_launcher, tmp_path, T_132, "n=132", "variants=flat,five")
    _variants_equal_flat(load, ("five",), NLISTS)
