"""Cost of aligning the sections on the way into a streamed prediction (predict_volume(..., warp=)), on a 1024x1024x512
EM-like uint8 np.memmap written to a second memmap with the 132 model.  Every section is turned by up to +-0.5 degrees
about the centre and moved by up to a pixel, and bent by a smooth field of up to a pixel on a lattice of --spacing.

--configs, alternating within every repetition, in this process:
    none      predict_volume without the keyword on the raw stack: the pass's own floor
    warp      predict_volume(warp=Warp(maps, fields, spacing)): per chunk the raw box that holds the footprint's taps is
              read and one tem_u8_warp_box launch makes the footprint on the device
    two_pass  the route without the keyword: volume_warp_field memmap -> memmap, then predict_volume on the aligned copy
`warp` is checked against `two_pass`: the two outputs must be equal.  The read amplification is warp_read_voxels /
footprint_voxels of the run's stats, next to the footprints' own voxels over the volume's.
--parent DIR: before anything touches the GPU here, the default path (`--configs none`) is timed in processes of their
own, this checkout and the one at DIR alternating, --procs times each; DIR needs no `warp` keyword.
--root DIR imports transfer_em_amd from DIR (what --parent's processes are given).
Every figure comes with all its runs: the run-to-run spread is what a difference has to exceed.
Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 900 python tests/tools/predict_warp_time.py [--x 1024 --y 1024 --z 512] [--spacing 128] [--reps 3]
        [--configs none,warp,two_pass] [--parent DIR --procs 3] [--root DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

_TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MS_X, MS_Y = (0.02, 0.58), (-0.1, 0.4)


def _rigid(theta, t, centre):
    c, s = np.cos(theta), np.sin(theta)
    L = np.array([[c, -s], [s, c]])
    return np.concatenate([L, (centre - L @ centre + t)[:, None]], axis=1)


def _wave(shape, ny, nx, spacing, amp, phase):
    """float64 [ny, nx, 2]: u_y = amp sin(pi x / (X - 1) + phase), u_x = -amp sin(pi y / (Y - 1) + phase) at the nodes."""
    Y, X = shape[-2:]
    y, x = np.meshgrid(np.arange(ny) * float(spacing), np.arange(nx) * float(spacing), indexing="ij")
    return np.stack([amp * np.sin(np.pi * x / (X - 1) + phase), -amp * np.sin(np.pi * y / (Y - 1) + phase)], axis=-1)


def default_path_in_processes(a):
    """`--configs none` in fresh processes, this checkout and --parent alternating: {name: [each process's runs]}."""
    roots = {"this": os.path.dirname(_TESTS), "parent": os.path.abspath(a.parent)}
    runs = {n: [] for n in roots}
    for _ in range(a.procs):
        for n, root in roots.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--x", str(a.x), "--y", str(a.y), "--z", str(a.z), "--reps",
                   str(a.reps), "--configs", "none", "--root", root]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
            runs[n].append(json.loads(out.strip().splitlines()[-1])["configs"]["none"]["all_runs_s"])
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--spacing", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="none,warp,two_pass")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, built: the default path, process by process")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--root", default=os.path.dirname(_TESTS), help="the checkout to import transfer_em_amd from")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    res = {"volume_xyz": [a.x, a.y, a.z], "spacing": a.spacing, "root": root}
    if a.parent:                                            # first: this process has not touched the GPU yet
        res["default_path_processes"] = default_path_in_processes(a)
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import torch
    from transfer_em_amd import utils
    shape, start, size = (a.z, a.y, a.x), (0, 0, 0), (a.x, a.y, a.z)
    nbytes = a.x * a.y * a.z
    names = a.configs.split(",")
    with tempfile.TemporaryDirectory() as tmp:
        def new(name):
            return np.lib.format.open_memmap(os.path.join(tmp, name + ".npy"), mode="w+", dtype=np.uint8, shape=shape)
        vol = new("vol")
        rng = np.random.default_rng(0)
        blk = np.clip(rng.normal(120, 9, (min(64, a.z),) + shape[1:]), 0, 240).astype(np.uint8)
        for z in range(0, a.z, 64):                         # EM-like: a few dozen bins around 120, drifting with z
            vol[z:z + 64] = blk[:min(64, a.z - z)] + np.uint8(z // 64 % 16)
        vol.flush()
        del vol
        vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")
        W = None
        if "warp" in names or "two_pass" in names:
            centre = np.array([(a.y - 1) / 2, (a.x - 1) / 2])
            M = utils.quantize_maps(np.stack([_rigid(t, s, centre) for t, s in
                                              zip(rng.uniform(-1, 1, a.z) * np.deg2rad(0.5), rng.uniform(-1, 1, (a.z, 2)))]))
            ny, nx = utils.field_grid(shape, a.spacing)
            U = utils.quantize_field(np.stack([_wave(shape, ny, nx, a.spacing, amp, ph) for amp, ph in
                                               zip(rng.uniform(-1, 1, a.z), rng.uniform(0, np.pi, a.z))]), a.spacing)
            W = utils.Warp(M, U, a.spacing)
            aligned = new("aligned")

        from transfer_em_amd.cgan import EM2EM
        from transfer_em_amd.models.generator import generator_param_shapes
        from util import scaled_params                      # tests/util.py: outputs spread over the uint8 range
        model = EM2EM(132, "warptime", checkpoint_root=tmp)
        Pm = scaled_params(generator_param_shapes(True), 4)
        Pm["f2"] = Pm["f2"] * 20
        model.generator_g.params.load_dict(Pm)
        outs = {n: new("pred_" + n) for n in names}

        def run(n, st):
            if n == "none":
                utils.predict_volume(vol, start, size, model, MS_X, MS_Y, out=outs[n], stats=st)
            elif n == "warp":
                utils.predict_volume(vol, start, size, model, MS_X, MS_Y, out=outs[n], stats=st, warp=W)
            else:
                t0 = time.perf_counter()
                utils.volume_warp_field(vol, W.maps, W.fields, a.spacing, out=aligned)
                st["align_s"] = time.perf_counter() - t0
                utils.predict_volume(aligned, start, size, model, MS_X, MS_Y, out=outs[n], stats=st)
        runs = {n: [] for n in names}
        for rep in range(a.reps + 1):                       # repetition 0 warms plans, buffers, page cache
            for n in names:
                st = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(n, st)
                torch.cuda.synchronize()
                if rep:
                    runs[n].append((time.perf_counter() - t0, st))
        res["configs"] = {}
        for n in names:
            wall, st = min(runs[n], key=lambda r: r[0])
            r = res["configs"][n] = {"end_to_end_s": round(wall, 4), "all_runs_s": [round(v[0], 4) for v in runs[n]],
                                     "gvox_per_s": round(nbytes / wall / 1e9, 3), "host_read_s": round(st["read_s"], 4),
                                     "host_write_s": round(st["write_s"], 4), "chunks": st["chunks"]}
            if "align_s" in st:
                r["align_s"] = round(st["align_s"], 4)
            if "warp_read_voxels" in st:
                r.update(warp_read_voxels=int(st["warp_read_voxels"]), footprint_voxels=int(st["footprint_voxels"]),
                         read_amplification=round(st["warp_read_voxels"] / st["footprint_voxels"], 4),
                         footprints_over_volume=round(st["footprint_voxels"] / nbytes, 4))
        if "warp" in names and "two_pass" in names:
            res["warp_equals_two_pass"] = bool(all(np.array_equal(outs["warp"][z], outs["two_pass"][z]) for z in range(a.z)))
            res["differs_from_none"] = bool("none" in names and not np.array_equal(outs["warp"][a.z // 2], outs["none"][a.z // 2]))
        model.generator_g.clear_plans()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
