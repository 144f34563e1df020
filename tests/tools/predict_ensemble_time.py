"""Cost of the self-ensemble of tiled inference (utils.predict_cube(..., ensemble=...)): the 132 model over a resident
uint8 cube, timed with ensemble None, [identity], "flips" and one member that moves x, the configurations alternating
within every repetition; plus the two new kernels' own times from device events on one 27-tile batch (edge 132, output
edge 96), beside the existing gather's.  "none" is called without the keyword, so `--configs none --kernels 0` also
runs on a commit that has no `ensemble` yet, for a before / after figure of the default path.  Prints one JSON line:
per configuration the best and all wall times, k, and (t_k - k t_None) / k per member.  Run under a time limit on the
GPU box:
    timeout -k 10 500 python tests/tools/predict_ensemble_time.py [--side 384] [--reps 3]
        [--configs none,identity,flips,movex] [--kernels 1]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

MS_X, MS_Y = (0.02, 0.58), (-0.1, 0.4)
IDENT = ((0, 1, 2), (0, 0, 0))
MOVEX = ((0, 2, 1), (0, 0, 0))                  # y <-> x: the LDS-staged kernels, stride E without them
MOVEXZ = ((2, 1, 0), (1, 0, 1))                 # z <-> x with flips: stride E^2 without them


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


def kernel_times(vol, ntile=27, edge=132, yedge=96):
    """Device-event times (us) of the gathers and the accumulate on one batch, and the bytes each moves."""
    from transfer_em_amd import _lib as L
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    dv = torch.from_numpy(vol).cuda()
    side = vol.shape[0]
    rng = np.random.default_rng(0)
    org = torch.from_numpy(rng.integers(-20, side - edge + 20, (ntile, 3)).astype(np.int32)).cuda()
    x = torch.empty((ntile, edge, edge, edge), dtype=torch.float32, device="cuda")
    y = torch.randn((ntile, yedge, yedge, yedge), dtype=torch.float32, device="cuda")
    acc = torch.zeros_like(y)
    res = {"ntile": ntile, "edge": edge, "yedge": yedge,
           "gather_bytes": int(ntile * edge ** 3 * 5), "accum_bytes_add": int(ntile * yedge ** 3 * 12)}

    def gather0():
        L.check(lib.tem_u8_tiles_to_f32_std(dv.data_ptr(), *vol.shape, org.data_ptr(), ntile, edge, x.data_ptr(), *MS_X,
                                            stream), "gather")

    def gather_sym(s, mode):
        return lambda: L.check(lib.tem_u8_tiles_to_f32_std_sym(
            dv.data_ptr(), *vol.shape, 0, 0, 0, *vol.shape, mode, org.data_ptr(), ntile, edge, *s[0], *s[1], x.data_ptr(),
            *MS_X, stream), "gather_sym")

    def accum(s, first, div):
        return lambda: L.check(lib.tem_f32_tiles_sym_accum(y.data_ptr(), ntile, yedge, *s[0], *s[1], acc.data_ptr(),
                                                           first, div, stream), "accum")
    res["gather_existing_zeros"] = _events(gather0)
    for name, s in (("identity", IDENT), ("flip_zyx", ((0, 1, 2), (1, 1, 1))), ("swap_yx", MOVEX), ("swap_zx_flips", MOVEXZ)):
        res[f"gather_sym_zeros_{name}"] = _events(gather_sym(s, 0))
        res[f"gather_sym_reflect_{name}"] = _events(gather_sym(s, L.TEM_BOUNDARY_REFLECT))
        res[f"accum_first_{name}"] = _events(accum(s, 1, 1))
        res[f"accum_add_{name}"] = _events(accum(s, 0, 1))
        res[f"accum_add_div8_{name}"] = _events(accum(s, 0, 8))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="none,identity,flips,movex")
    ap.add_argument("--kernels", type=int, default=1)
    a = ap.parse_args()
    from transfer_em_amd.cgan import EM2EM
    from transfer_em_amd.utils import predict_cube, tile_plan
    configs = {"none": {}, "identity": {"ensemble": [IDENT]}, "flips": {"ensemble": "flips"},
               "movex": {"ensemble": [MOVEX]}, "identity+movex": {"ensemble": [IDENT, MOVEX]}}
    ks = {"none": 1, "identity": 1, "flips": 8, "movex": 1, "identity+movex": 2}
    names = a.configs.split(",")
    vol = np.random.default_rng(0).integers(0, 256, (a.side,) * 3, dtype=np.uint8)
    start, size = (0, 0, 0), (a.side,) * 3
    with tempfile.TemporaryDirectory() as tmp:
        model = EM2EM(132, "enstime", checkpoint_root=tmp)
        res = {"roi_xyz": list(size), "tiles": len(tile_plan(start, size, model.outdimsize, model.buffer)[3]),
               "configs": {}}
        runs = {n: [] for n in names}
        for rep in range(a.reps + 1):                                        # repetition 0 warms plans and kernels
            for n in names:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                predict_cube(vol, start, size, model, MS_X, MS_Y, **configs[n])   # ends in a device -> host copy
                torch.cuda.synchronize()
                if rep:
                    runs[n].append(time.perf_counter() - t0)
        for n in names:
            res["configs"][n] = {"k": ks[n], "s_min": round(min(runs[n]), 4), "all_runs_s": [round(t, 4) for t in runs[n]]}
        if "none" in runs:
            t1 = min(runs["none"])
            for n in names:
                r = res["configs"][n]
                r["extra_s_per_member"] = round((r["s_min"] - r["k"] * t1) / r["k"], 4)
        if a.kernels:
            model.generator_g.clear_plans()
            res["kernels"] = kernel_times(vol)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
