"""Cost of the self-ensemble's spread map (utils.predict_cube(..., ensemble="flips", spread=S)): the 132 model over a
resident uint8 cube, timed with and without `spread=` in the same process, the two alternating within every repetition;
the per-batch device-event times of the fused accumulate beside the plain one and of the spread scatter beside the
prediction's, on one 27-tile batch (output edge 96); and, with --parent DIR (a built tree of the parent commit), the
default path (ensemble=None) of this tree and of that one, each run a fresh child process of
predict_ensemble_time.py --configs none --kernels 0, alternating, best of --reps.  Prints one JSON line.  Run under a
time limit on the GPU box:
    timeout -k 10 900 python tests/tools/predict_spread_time.py [--side 768] [--reps 3] [--parent DIR] [--kernels 1]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MS_X, MS_Y = (0.02, 0.58), (-0.1, 0.4)
IDENT = ((0, 1, 2), (0, 0, 0))
MOVEX = ((0, 2, 1), (0, 0, 0))                  # y <-> x: the LDS-staged kernel


def _events(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    return {"us_min": round(min(t), 1), "us_median": round(sorted(t)[len(t) // 2], 1)}


def kernel_times(ntile=27, yedge=96, tpad=0):
    """Device-event times (us) of the accumulates and the scatters on one batch, and the bytes each moves."""
    from transfer_em_amd import _lib as L
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    y = torch.randn((ntile, yedge, yedge, yedge), dtype=torch.float32, device="cuda")
    acc, ref, s1, s2 = (torch.zeros_like(y) for _ in range(4))
    od = yedge - 2 * tpad
    out = torch.zeros((3 * od,) * 3, dtype=torch.uint8, device="cuda")
    idx = torch.tensor([(a * od, b * od, c * od) for a in range(3) for b in range(3) for c in range(3)][:ntile],
                       dtype=torch.int32).cuda()
    vox = ntile * yedge ** 3
    res = {"ntile": ntile, "yedge": yedge, "accum_add_bytes": 12 * vox, "accum_spread_add_bytes": 32 * vox,
           "scatter_bytes": 5 * vox, "spread_scatter_bytes": 9 * vox}

    def accum(s, first, div):
        return lambda: L.check(lib.tem_f32_tiles_sym_accum(y.data_ptr(), ntile, yedge, *s[0], *s[1], acc.data_ptr(),
                                                           first, div, stream), "accum")

    def accum_spread(s, first, div):
        return lambda: L.check(lib.tem_f32_tiles_sym_accum_spread(
            y.data_ptr(), ntile, yedge, *s[0], *s[1], acc.data_ptr(), first, div, ref.data_ptr(), s1.data_ptr(),
            s2.data_ptr(), stream), "accum_spread")

    def scatter():
        L.check(lib.tem_f32_tiles_unstd_to_u8(acc.data_ptr(), ntile, yedge, tpad, idx.data_ptr(), out.data_ptr(),
                                              *out.shape, *MS_Y, stream), "scatter")

    def spread_scatter():
        L.check(lib.tem_f32_tiles_spread_to_u8(s1.data_ptr(), s2.data_ptr(), ntile, yedge, tpad, idx.data_ptr(),
                                               out.data_ptr(), *out.shape, 8, MS_Y[1], 8.0, stream), "spread_scatter")
    for name, s in (("flip_zyx", ((0, 1, 2), (1, 1, 1))), ("swap_yx", MOVEX)):
        for kind, fn in (("accum", accum), ("accum_spread", accum_spread)):
            res[f"{kind}_first_{name}"] = _events(fn(s, 1, 1))
            res[f"{kind}_add_{name}"] = _events(fn(s, 0, 1))
            res[f"{kind}_add_div8_{name}"] = _events(fn(s, 0, 8))
    res["scatter"] = _events(scatter)
    res["spread_scatter"] = _events(spread_scatter)
    return res


def default_path(tree, side):
    """Best wall time (s) of one predict_cube(ensemble=None) in a fresh child process running the tool of `tree`."""
    tool = os.path.join(tree, "tests", "tools", "predict_ensemble_time.py")
    out = subprocess.run([sys.executable, tool, "--configs", "none", "--kernels", "0", "--side", str(side), "--reps", "2"],
                         check=True, capture_output=True, text=True, cwd=tree, timeout=400).stdout
    return json.loads(out.strip().splitlines()[-1])["configs"]["none"]["s_min"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=768)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--kernels", type=int, default=1)
    a = ap.parse_args()
    res = {}
    if a.parent:                                                             # ahead of this process's own GPU work
        runs = {"this": [], "parent": []}
        for _ in range(a.reps):
            runs["this"].append(default_path(ROOT, a.side))
            runs["parent"].append(default_path(os.path.abspath(a.parent), a.side))
        res["default_path"] = {k: {"s_min": min(v), "all_runs_s": v} for k, v in runs.items()}
    from transfer_em_amd.cgan import EM2EM
    from transfer_em_amd.utils import predict_cube, tile_plan
    vol = np.random.default_rng(0).integers(0, 256, (a.side,) * 3, dtype=np.uint8)
    start, size = (0, 0, 0), (a.side,) * 3
    S = np.zeros((a.side,) * 3, np.uint8)
    configs = {"flips": {"ensemble": "flips"}, "flips+spread": {"ensemble": "flips", "spread": S}}
    with tempfile.TemporaryDirectory() as tmp:
        model = EM2EM(132, "spreadtime", checkpoint_root=tmp)
        res.update({"roi_xyz": list(size), "tiles": len(tile_plan(start, size, model.outdimsize, model.buffer)[3]),
                    "configs": {}})
        runs = {n: [] for n in configs}
        for rep in range(a.reps + 1):                                        # repetition 0 warms plans and kernels
            for n, kw in configs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                predict_cube(vol, start, size, model, MS_X, MS_Y, **kw)      # ends in a device -> host copy
                torch.cuda.synchronize()
                if rep:
                    runs[n].append(time.perf_counter() - t0)
        for n in configs:
            res["configs"][n] = {"s_min": round(min(runs[n]), 4), "all_runs_s": [round(t, 4) for t in runs[n]]}
        res["spread_over_flips"] = round(min(runs["flips+spread"]) / min(runs["flips"]), 4)
        res["map_distinct_values"] = int(len(np.unique(S)))
        if a.kernels:
            model.generator_g.clear_plans()
            res["kernels"] = kernel_times()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
