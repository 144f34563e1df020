"""The product's data-parallel train step, two replicas (the MirroredStrategy the reference lists as TODO,
cgan.py:8-11,55-57): EM2EM with a process group runs the bucketed gradient exchange on the step's streams,
`grad_scale = 1/world` inside the Adam kernel, the parameter broadcast at construction, one dropout stream per
replica and rank-0-only checkpoints.  Both ranks share the one card of the GPU box and talk over gloo (RCCL wants
one GPU per rank; the driver's 8-GPU run covers that transport) -- every line of the product's DP path is the same.

Checked against the oracle step by step, at the bars of the single-replica step (test_gpu_step.py): per-replica gradients
(dropout seed + rank, the replica's own LeakyReLU branches, the state the replicas entered the step with) averaged, then
ONE Keras-Adam update.  The inputs are conditioned, not the bars: standardized uint8 volumes at half amplitude keep the
cycle / identity terms away from their pole (util.dp_inputs; the oracle's own margin is asserted)."""
import os
import sys

import numpy as np
import pytest

from util import DP_OUTPUTS, FLIP_BOUND, _pole_margin, dp_inputs, gates_from_masks, rel_err, unpack_masks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = ("g", "f", "dx", "dy")


def _shapes(is3d):
    from oracle import graph
    gs, ds = graph.generator_param_shapes(is3d), graph.discriminator_param_shapes(is3d)
    return dict(g=gs, f=gs, dx=ds, dy=ds)


def _unflat(vec, shapes):
    from collections import OrderedDict
    out, o = OrderedDict(), 0
    for k, s in shapes.items():
        n = int(np.prod(s))
        out[k] = np.asarray(vec[o:o + n]).reshape(s)
        o += n
    assert o == vec.size
    return out


def _step_matches_oracle(recs, k, is3d):
    """Step k of the two replicas against the oracle, at the bars of test_gpu_step._step_matches_oracle: per replica the
    oracle's gradients from the replicas' own state before the step (no drift to amplify), that replica's inputs, dropout
    seed 42 + rank, step k and the LeakyReLU branches of that replica's forward; their mean; ONE Keras-Adam update, t = k + 1."""
    from oracle import graph, ops
    shapes = _shapes(is3d)
    r0 = recs[0]
    for net in NETS:                             # the replicas enter the step with the same state, bit for bit
        for which in ("theta", "m", "v"):
            assert np.array_equal(r0[f"s{k}.pre.{net}.{which}"], recs[1][f"s{k}.pre.{net}.{which}"]), (k, net, which)
    pre = {which: {net: _unflat(r0[f"s{k}.pre.{net}.{which}"], shapes[net]) for net in NETS} for which in ("theta", "m", "v")}
    P = pre["theta"]
    crop_by = (lambda t, c: t[:, c:-c, c:-c, c:-c, :]) if is3d else (lambda t, c: t[:, :, c:-c, c:-c, :])
    per_rank = []
    for r, rec in enumerate(recs):
        rx, ry = dp_inputs(r, is3d)
        gates = gates_from_masks(unpack_masks(rec, f"s{k}.gate"), is3d)
        losses, grads, aux = graph.train_step_grads(P["g"], P["f"], P["dx"], P["dy"], rx, ry, is3d, 2.0, 42 + r, k, gates=gates)
        per_rank.append(grads)
        b = aux["buffer"]
        margin = _pole_margin(aux, rx, ry, b, crop_by)
        nflip, total = (sum(v[i] for v in gates.flips.values()) for i in range(2))
        print(f"step {k} rank {r}: smallest 1 - |a - b| / 2 of the cycle / identity terms (oracle) {margin:.3g}; {nflip} gate "
              f"flips of {total} activations: " + ", ".join(f"{c} {v[0]}" for c, v in gates.flips.items() if v[0]))
        assert margin >= 0.05, (k, r, margin)
        assert set(gates.flips) == set(aux["saved"]) and total > 0
        for call, (nf, tot) in gates.flips.items():
            assert nf <= max(2, FLIP_BOUND * tot), (k, r, call, nf, tot)
        assert nflip <= max(2, FLIP_BOUND * total), (k, r, nflip, total)
        assert rel_err(rec[f"s{k}.losses"], losses) < 1e-5, (k, r, rec[f"s{k}.losses"], losses)
        for key, _ in DP_OUTPUTS:
            ref = crop_by(aux[key], b) if key.startswith("cyc") else aux[key]    # cycled_*: only the cropped window exists
            assert rel_err(rec[f"s{k}.out.{key}"], ref) < 1e-4, (k, r, key)
    gmean = {net: {name: (np.asarray(per_rank[0][net][name], np.float64) + np.asarray(per_rank[1][net][name], np.float64)) / 2
                   for name in shapes[net]} for net in NETS}
    # grad_all is the SUM over the replicas: grad_scale = 1/2 lives in the Adam kernel
    assert np.array_equal(r0[f"s{k}.grad_all"], recs[1][f"s{k}.grad_all"])
    gtol, o = (2e-4 if is3d else 1e-4), 0
    for net in NETS:
        count = r0[f"s{k}.pre.{net}.theta"].size
        got = _unflat(r0[f"s{k}.grad_all"][o:o + count] / np.float32(2), shapes[net])
        o += count
        scale = max(np.abs(v).max() for v in gmean[net].values())
        worst = max(np.abs(got[name] - ref).max() / np.abs(ref).max() for name, ref in gmean[net].items())
        print(f"step {k}: network {net}: worst error of the mean gradient {worst:.2e} of a layer's largest entry, bar {gtol:g}")
        for name, ref in gmean[net].items():
            err = np.abs(got[name] - ref).max()
            # the bias gradient is a sum of logit gradients of both signs: absolute floor from fp32 dz
            floor = 1e-7 * scale + (3e-8 if name.endswith("_bias") else 0.0)
            assert err <= gtol * np.abs(ref).max() + floor, (k, net, name, err, np.abs(ref).max())
        want = {"theta": {}, "m": {}, "v": {}}
        for name in shapes[net]:
            want["theta"][name], want["m"][name], want["v"][name] = ops.adam_keras(
                P[net][name], gmean[net][name], pre["m"][net][name], pre["v"][net][name], k + 1)
        for which, tol in (("m", gtol), ("v", 2 * gtol)):
            got_s = _unflat(r0[f"s{k}.post.{net}.{which}"], shapes[net])
            scale_s = max(np.abs(v).max() for v in want[which].values())
            for name, ref in want[which].items():
                floor = 1e-6 * scale_s + ((2e-8 if which == "m" else 1e-13) if name.endswith("_bias") else 0.0)
                assert np.abs(got_s[name] - ref).max() <= tol * np.abs(ref).max() + floor, (k, net, which, name)
        th = _unflat(r0[f"s{k}.post.{net}.theta"], shapes[net])
        for name in th:
            # entries whose gradient is a sizeable fraction of the layer's largest move by +-lr whatever the 1e-4 error; near
            # g == 0 rounding decides the sign of the whole +-lr step on either side (test_gpu_step.py)
            gref = np.abs(gmean[net][name])
            big = gref >= 0.01 * gref.max()
            assert np.abs(th[name] - want["theta"][name])[big].max() < 0.15 * 2e-4, (k, net, name)
            assert np.abs(th[name] - want["theta"][name]).max() <= 2.05 * 2e-4, (k, net, name)


def _inherited_lists():
    """Stream lists of the step under the queue count this session runs with: a stream per discriminator from 6 queues on."""
    return 4 if int(os.environ.get("GPU_MAX_HW_QUEUES") or 4) >= 6 else 3


@pytest.mark.parametrize("is3d,queues", [(False, None), (True, None), (True, 8)])
def test_two_rank_step_matches_oracle(tmp_path, rank_launcher, oracle_lib, is3d, queues):
    """Two steps (Adam t = 1, 2; dropout steps 0, 1) of two replicas, 2-D and 3-D (the Winograd slabs, the stream lists and
    the bucketed exchange at 74^3), each step against the oracle at the single-replica bars.  queues=8: the five-list
    schedule with the exchange inside -- the discriminators' bucket leaves before the generators' kernel-gradient tail is
    enqueued on the same stream."""
    res = rank_launcher([sys.executable, os.path.join(ROOT, "tests", "tools", "dp_rank.py"), str(tmp_path), "steps=2"] +
                        (["3d"] if is3d else []), ranks=2, env={"GPU_MAX_HW_QUEUES": str(queues)} if queues else {},
                        timeout=900)
    assert res["rc"] == [0, 0], "\n".join(res["tail"])
    r0, r1 = (np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2))
    assert int(r0["nlists"]) == int(r1["nlists"]) == (4 if queues == 8 else _inherited_lists())
    # construction: different seeds -> different weights; the broadcast made them rank 0's (tested again below
    # through the loaded start state); replicas draw different dropout streams
    assert not np.array_equal(r0["init"][:1000], np.zeros(1000)) and np.array_equal(r0["init"], r1["init"])
    assert int(r0["seed"]) == 42 and int(r1["seed"]) == 43
    assert int(r0["step"][0]) == 2 and int(r1["step"][0]) == 2
    # the exchange: both replicas hold the same summed gradient and bit-identical parameters / moments
    assert np.array_equal(r0["grad_all"], r1["grad_all"])
    for key in NETS:
        for which in ("theta", "m", "v"):
            assert np.array_equal(r0[f"{key}.{which}"], r1[f"{key}.{which}"]), (key, which)
    # rank-0-only checkpoint (cgan.py:105-107 under data parallelism)
    assert str(r0["ckpt"]).endswith("ckpt-1.pt") and os.path.isfile(str(r0["ckpt"])) and str(r1["ckpt"]) == ""
    assert not os.path.exists(os.path.join(tmp_path, "ckpt1", "train_dp"))
    # against the oracle: local losses and outputs per replica, mean gradient, moments and parameters, step by step
    for k in range(2):
        _step_matches_oracle((r0, r1), k, is3d)


def test_two_rank_graph_step_equals_eager(tmp_path, rank_launcher):
    """use_graph under data parallelism: the gradient computation and the update as two HIP graphs with the all-reduce
    between them.  Three steps (eager, capture and replay, replay) of two 3-D replicas: losses, grad_all, parameters and
    moments of both ranks bit-identical to the eager job's."""
    recs = {}
    for tag in ("eager", "graph"):
        d = tmp_path / tag
        d.mkdir()
        res = rank_launcher([sys.executable, os.path.join(ROOT, "tests", "tools", "dp_rank.py"), str(d), "3d", "steps=3"] +
                            (["graph"] if tag == "graph" else []), ranks=2, timeout=900)
        assert res["rc"] == [0, 0], "\n".join(res["tail"])
        recs[tag] = [np.load(os.path.join(d, f"rank{r}.npz")) for r in range(2)]
    for r in range(2):
        a, b = recs["eager"][r], recs["graph"][r]
        assert int(a["graphs"]) == 0 and int(b["graphs"]) == 2 and int(b["step"][0]) == 3
        for k in range(3):
            keys = [f"s{k}.losses", f"s{k}.grad_all"] + [f"s{k}.post.{net}.{w}" for net in NETS for w in ("theta", "m", "v")]
            for key in keys:
                assert np.array_equal(a[key], b[key]), (r, key)
    assert not np.array_equal(recs["graph"][0]["s0.losses"], recs["graph"][1]["s0.losses"])     # two replicas, two batches


def test_one_rank_rccl_exchange_is_identity(tmp_path, rank_launcher):
    """RCCL itself (backend "nccl") on the one card of the box: a process group of ONE rank that still issues the
    parameter broadcast and both gradient buckets' all-reduce on the step's streams (TEM_DP_FORCE_EXCHANGE=1).  A sum
    over one replica is the identity and grad_scale is 1, so parameters, moments and losses must equal, bit for bit,
    those of the same two steps without any exchange."""
    outs = []
    for tag, env in (("rccl", {"TEM_DIST_BACKEND": "nccl", "TEM_DP_FORCE_EXCHANGE": "1"}),
                     ("plain", {"TEM_DIST_BACKEND": "gloo"})):
        d = tmp_path / tag
        d.mkdir()
        res = rank_launcher([sys.executable, os.path.join(ROOT, "tests", "tools", "dp_rank.py"), str(d), "3d"],
                            ranks=1, env=env, timeout=600)
        assert res["rc"] == [0], "\n".join(res["tail"])
        outs.append(np.load(os.path.join(d, "rank0.npz")))
    a, b = outs
    assert int(a["step"][0]) == 2
    for k in a.files:
        if k != "ckpt":
            assert np.array_equal(a[k], b[k]), k
