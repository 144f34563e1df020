"""Every stream schedule of the train step against the flat launch order (tests/test_gpu_schedules.py).

    step_schedules.py OUTDIR n=74 dim=3 batch=1 precision=fp32 variants=flat,five,... [lin=five,tail1,...] [teeth]

Started as a fresh process with GPU_MAX_HW_QUEUES=8 in its environment, so that HIP has the hardware queues for the five
streams of the product's schedule before it initialises.  TEM_SIDE_SPLIT and TEM_BWW_TAIL are read when a _CompiledStep is
built: one process builds the variants in turn.

    tag          two_streams  use_graph  TEM_SIDE_SPLIT  TEM_BWW_TAIL   lists  kernel-gradient tails
    flat         False        False      -               -              (not run from the lists)
    five         True         False      unset           unset (2)      4      all six sweeps
    tail1        True         False      unset           1              4      the last sweeps g1, f1
    tail0        True         False      unset           0              4      none
    three        True         False      0               -              3      none
    graph        True         True       unset           -              3      none
    graph_split  True         True       1               unset          4      none

Per variant: the schedule that was built is asserted first (a silent fall-back would make the comparison vacuous), then
the structural checks of its lists (no timing involved), then 3 steps from the same start state (util.scaled_params, seeds
10..13) on the same standardized uint8 inputs; losses, grad_all and theta / m / v of the four networks after every step go
to OUTDIR/<tag>.npz.

lin=<tags>: one step under EVERY priority permutation of the variant's lists (util.linearise over lists_fused, run on one
stream between the input copies and the losses' read-back as train_step does) -> OUTDIR/lin_<tag>.npz.  These are the
extremal orders the declared events allow, not all orders.  Before each measured step one step runs on swapped inputs from
the state the previous one left, so that a launch that overtakes its producer reads data of ANOTHER step, not its own.

teeth: the control.  On a copy of `five`'s lists the one wait in front of the first kernel-gradient launch of tail g1 is
dropped and the order that ranks that list first is run -> OUTDIR/teeth.npz.  Every buffer is preallocated: the launch
reads valid memory that holds the previous step's gradient.

A failed check ends the process with status 2 and the offending item on stderr.
"""
import itertools
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

NETS = ("g", "f", "dx", "dy")
SWEEPS = ("g3", "g2", "g1", "f3", "f2", "f1")
#            two_streams, use_graph, TEM_SIDE_SPLIT, TEM_BWW_TAIL, lists, sweeps whose kernel gradients are in a tail
VARIANTS = dict(flat=(False, False, None, None, None, None),
                five=(True, False, None, None, 4, set(SWEEPS)),
                tail1=(True, False, None, "1", 4, {"g1", "f1"}),
                tail0=(True, False, None, "0", 4, set()),
                three=(True, False, "0", None, 3, set()),
                graph=(True, True, None, None, 3, set()),
                graph_split=(True, True, "1", None, 4, set()))


def fail(msg):
    print("step_schedules: " + msg, file=sys.stderr, flush=True)
    sys.exit(2)


def _is(item, kind):
    return isinstance(item, tuple) and item[0] == kind


def _name(item):
    return repr(item) if isinstance(item, tuple) else item.name


def check_lists(tag, which, lists, launches, bwd):
    """The structural checks of one list set; returns {sweep: kernel-gradient launches of it that sit in a tail}.
    Launch objects are compared by identity."""
    want = {id(l): l for l in launches}
    if len(want) != len(launches):
        fail(f"{tag}.{which}: the flat order holds a launch twice")
    seen = {}
    for li, lst in enumerate(lists):
        for pos, item in enumerate(lst):
            if isinstance(item, tuple):
                if item[0] not in ("wait", "record", "allreduce"):
                    fail(f"{tag}.{which}[{li}][{pos}]: unknown item {item!r}")
                continue
            if id(item) not in want:
                fail(f"{tag}.{which}[{li}][{pos}]: launch {item.name} is not in the flat order")
            if id(item) in seen:
                fail(f"{tag}.{which}[{li}][{pos}]: launch {item.name} occurs twice (first in list {seen[id(item)][0]})")
            seen[id(item)] = (li, pos)
    for k, l in want.items():
        if k not in seen:
            fail(f"{tag}.{which}: launch {l.name} of the flat order is in no list")
    records = {}
    for li, lst in enumerate(lists):
        for pos, item in enumerate(lst):
            if _is(item, "record"):
                if item[1] in records or item[1] == "inputs":
                    fail(f"{tag}.{which}[{li}][{pos}]: event {item[1]} is recorded twice")
                records[item[1]] = (li, pos)
    for li, lst in enumerate(lists):
        for pos, item in enumerate(lst):
            if _is(item, "wait") and item[1] != "inputs" and item[1] not in records:      # "inputs": _run_streams records it
                fail(f"{tag}.{which}[{li}][{pos}]: wait for {item[1]}, which no list records")
    # kernel gradients in a tail: a '.bww.' launch in another list than its sweep's input-gradient launches
    tails = {}
    for sweep in SWEEPS:
        plan = bwd[sweep].launches
        chain = {seen[id(l)][0] for l in plan if ".bww." not in l.name}
        if len(chain) != 1:
            fail(f"{tag}.{which}: the input-gradient launches of sweep {sweep} are spread over lists {sorted(chain)}")
        chain = chain.pop()
        for j, l in enumerate(plan):
            li, pos = seen[id(l)]
            if ".bww." not in l.name or li == chain:
                continue
            tails.setdefault(sweep, []).append(l)
            before = lists[li][pos - 1] if pos else None
            if not _is(before, "wait"):
                fail(f"{tag}.{which}[{li}][{pos}]: tail launch {sweep}:{l.name} is not directly preceded by a wait "
                     f"(but by {_name(before) if before is not None else 'nothing'})")
            ev = before[1]
            if records[ev][0] != chain:
                fail(f"{tag}.{which}[{li}][{pos}]: {sweep}:{l.name} waits for {ev}, recorded in list {records[ev][0]}, "
                     f"not in the sweep's chain (list {chain})")
            rec = records[ev][1]
            prev = next((p for p in reversed(plan[:j]) if ".bww." not in p.name), None)
            nxt = next((p for p in plan[j + 1:] if ".bww." not in p.name), None)
            if prev is not None and not seen[id(prev)][1] < rec:
                fail(f"{tag}.{which}[{li}][{pos}]: {sweep}:{l.name} waits for {ev}, recorded BEFORE {prev.name}, the launch "
                     f"that writes its gradient")
            if nxt is not None and not rec < seen[id(nxt)][1]:
                fail(f"{tag}.{which}[{li}][{pos}]: {sweep}:{l.name} waits for {ev}, recorded after the later launch {nxt.name}")
            if prev is None and nxt is not None:
                # the sweep's first kernel gradient reads the sweep's incoming gradient: the event is the last thing in
                # front of the sweep's first launch, behind everything the chain did (and waited for) before
                between = [it for it in lists[chain][rec + 1:seen[id(nxt)][1]] if not isinstance(it, tuple)]
                if between:
                    fail(f"{tag}.{which}[{li}][{pos}]: {sweep}:{l.name} waits for {ev}, recorded before {between[0].name}")
    return tails


def build(tag, n, is3d, batch, precision, outdir):
    """(model, compiled step) of one variant, its schedule asserted and its lists checked."""
    from transfer_em_amd.cgan import EM2EM
    two, graph_mode, split, tail, nlists, tail_sweeps = VARIANTS[tag]
    for key, val in (("TEM_SIDE_SPLIT", split), ("TEM_BWW_TAIL", tail)):
        os.environ.pop(key, None)
        if val is not None:
            os.environ[key] = val
    model = EM2EM(n, f"sched_{tag}", is3d=is3d, seed=42, checkpoint_root=os.path.join(outdir, "ckpt"), two_streams=two,
                  use_graph=graph_mode, precision=precision)
    cs = model._compiled(batch)
    os.environ.pop("TEM_SIDE_SPLIT", None)
    os.environ.pop("TEM_BWW_TAIL", None)
    tails = check_lists(tag, "lists", cs.lists, cs.compute, cs.bwd)
    tails_f = check_lists(tag, "lists_fused", cs.lists_fused, cs.compute + cs.update, cs.bwd)
    if {k: [id(l) for l in v] for k, v in tails.items()} != {k: [id(l) for l in v] for k, v in tails_f.items()}:
        fail(f"{tag}: lists and lists_fused place different kernel gradients in the tails")
    ntail = sum(len(v) for v in tails.values())
    print(f"variant {tag}: {len(cs.lists)} lists, {ntail} tail launches (sweeps {sorted(tails)}), "
          f"{sum(1 for l in cs.lists for it in l if _is(it, 'wait'))} waits", flush=True)
    if nlists is not None:
        if len(cs.lists) != nlists or len(cs.lists_fused) != nlists:
            fail(f"{tag}: {len(cs.lists)} lists built, {nlists} expected")
        if set(tails) != tail_sweeps:
            fail(f"{tag}: kernel-gradient tails of sweeps {sorted(tails)}, expected {sorted(tail_sweeps)}")
        for sweep, ls in tails.items():
            nb = sum(1 for l in cs.bwd[sweep].launches if ".bww." in l.name)
            if len(ls) != nb:
                fail(f"{tag}: sweep {sweep} has {len(ls)} of its {nb} kernel gradients in the tail")
    return model, cs


def snapshot(model):
    out = {"grad_all": model.grad_all.cpu().numpy()}
    for key, net in zip(NETS, model._nets):
        for which in ("theta", "m", "v"):
            out[f"{key}.{which}"] = getattr(net.params, which).cpu().numpy()
    return out


def run_serial(cs, order, rx, ry):
    """One step in the serial `order` on the current stream, with what train_step does around the lists."""
    from transfer_em_amd import hip_ops as H
    cs.real_x.copy_(rx, non_blocking=True)
    cs.real_y.copy_(ry, non_blocking=True)
    cs.losses.zero_()
    s = H.current_stream()
    for item in order:
        if not isinstance(item, tuple):           # ("allreduce", key): one replica, nothing to exchange
            item(s)
    return cs.losses[:7].to(torch.float32).cpu().numpy()


def main():
    t_start = time.time()
    outdir = sys.argv[1]
    opt = dict(a.split("=", 1) for a in sys.argv[2:] if "=" in a)
    n, is3d, batch = int(opt.get("n", 74)), opt.get("dim", "3") == "3", int(opt.get("batch", 1))
    precision = opt.get("precision", "fp32")
    variants = [v for v in opt.get("variants", "").split(",") if v]
    lin = [v for v in opt.get("lin", "").split(",") if v]
    teeth = "teeth" in sys.argv[2:]
    if os.environ.get("GPU_MAX_HW_QUEUES") != "8":
        fail(f"GPU_MAX_HW_QUEUES is {os.environ.get('GPU_MAX_HW_QUEUES')!r}: the variants' schedules are those of 8 queues")
    torch.cuda.set_device(0)
    from oracle import graph
    from test_gpu_step import _load, _state
    from util import _inputs, linearise
    shape = (batch, n if is3d else 1, n, n, 1)
    rx, ry = torch.from_numpy(_inputs(shape, 1234)).cuda(), torch.from_numpy(_inputs(shape, 5678)).cuda()
    st = _state(graph, is3d, True)

    for tag in variants:
        t0 = time.time()
        model, cs = build(tag, n, is3d, batch, precision, outdir)
        _load(model, st)
        steps = []
        for k in range(3):                       # graph variants: eager, capture + replay, replay
            losses = model.train_step(rx, ry).cpu().numpy()
            steps.append(dict(snapshot(model), losses=losses))
        if VARIANTS[tag][1] and cs.graphs is None:
            fail(f"{tag}: use_graph, but no graph was captured")
        if not VARIANTS[tag][1] and cs.graphs is not None:
            fail(f"{tag}: a graph was captured without use_graph")
        out = {k: np.stack([s[k] for s in steps]) for k in steps[0]}
        out["counts"] = np.asarray([net.params.count for net in model._nets], np.int64)
        out["nlists"] = np.int64(len(cs.lists))
        np.savez(os.path.join(outdir, f"{tag}.npz"), **out)
        print(f"variant {tag}: 3 steps, {time.time() - t0:.1f} s", flush=True)
        del model, cs
        torch.cuda.empty_cache()

    built = {}
    for tag in dict.fromkeys(lin + (["five"] if teeth else [])):
        built[tag] = build(tag, n, is3d, batch, precision, outdir)

    def measured(model, cs, order):
        model.train_step(ry, rx)                 # another step's data in every buffer (swapped inputs, drifted state)
        _load(model, st)
        model.step_dev.zero_()
        losses = run_serial(cs, order, rx, ry)
        return dict(snapshot(model), losses=losses)

    for tag in lin:
        t0 = time.time()
        model, cs = built[tag]
        _load(model, st)
        model.train_step(rx, ry)                 # lazy one-time setup of every kernel, on the variant's own schedule
        out = {}
        for perm in itertools.permutations(range(len(cs.lists_fused))):
            order = linearise(cs.lists_fused, perm)
            if len(order) != len(cs.compute) + len(cs.update) + 1:        # + ("allreduce", "d")
                fail(f"{tag}: order {perm} has {len(order)} items")
            for k, v in measured(model, cs, order).items():
                out["".join(map(str, perm)) + "/" + k] = v
        np.savez(os.path.join(outdir, f"lin_{tag}.npz"), **out)
        print(f"linearisations {tag}: {len(out) // 14} orders, {time.time() - t0:.1f} s", flush=True)

    if teeth:
        model, cs = built["five"]
        lists = [list(l) for l in cs.lists_fused]
        first = next(l for l in cs.bwd["g1"].launches if ".bww." in l.name)
        li, pos = next((i, p) for i, lst in enumerate(lists) for p, it in enumerate(lst) if it is first)
        if li != 1 or not _is(lists[li][pos - 1], "wait"):
            fail(f"teeth: the first kernel gradient of g1 is at [{li}][{pos}] behind {_name(lists[li][pos - 1])}")
        dropped = lists[li].pop(pos - 1)
        # that list first; of the six such orders the first in which the launch does overtake the one that completes its
        # gradient (the tail sits behind the discriminators' update, which waits for the other discriminator's list: with
        # that list ranked last the generator chain gets there first even without the wait)
        add_y = next(l for l in cs.compute if l.name == "dfake_y+=adv")
        for perm in itertools.permutations(range(len(lists))):
            order = linearise(lists, perm)
            at = {id(it): i for i, it in enumerate(order) if not isinstance(it, tuple)}
            if perm[0] == li and at[id(first)] < at[id(add_y)]:
                break
        else:
            fail("teeth: without its wait the kernel gradient still runs behind the launch that completes its gradient")
        print(f"teeth: priority order {perm}", flush=True)
        _load(model, st)
        model.train_step(rx, ry)
        np.savez(os.path.join(outdir, "teeth.npz"), **measured(model, cs, order))
        print(f"teeth: dropped {dropped!r} in front of {first.name}: it runs {at[id(add_y)] - at[id(first)]} launches ahead of "
              f"{add_y.name}", flush=True)
    torch.cuda.synchronize()
    print(f"step_schedules: done in {time.time() - t_start:.1f} s", flush=True)


if __name__ == "__main__":
    main()
