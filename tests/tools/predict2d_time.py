"""Throughput of the 2-D tiled inference (utils.predict_volume with a 2-D model) with the 132 model over a seeded
4096x4096x64 uint8 image stack in an np.memmap, written into an np.memmap output, against the generator alone on the
same tile batches (the sum of the plan.run() spans, timed with events).  Prints one JSON line.  Run under a time limit
on the GPU box:
    timeout -k 10 600 python tests/tools/predict2d_time.py [--x 4096 --y 4096 --z 64] [--reps 2]
The gather / scatter kernel times and the generator's per-kernel table come from a separate kernel-trace run of the
same command (rocprofv3 --kernel-trace --stats -d <dir> -- python tests/tools/predict2d_time.py --reps 1).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=4096)
    ap.add_argument("--y", type=int, default=4096)
    ap.add_argument("--z", type=int, default=64)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    from transfer_em_amd.cgan import EM2EM
    from transfer_em_amd.utils import _chunk_plan, default_tile_batch, predict_volume
    ms_x, ms_y = (0.02, 0.58), (-0.1, 0.4)
    with tempfile.TemporaryDirectory() as tmp:
        model = EM2EM(132, "p2dtime", is3d=False, checkpoint_root=tmp)
        shape = (a.z, a.y, a.x)
        vol = np.lib.format.open_memmap(os.path.join(tmp, "vol.npy"), mode="w+", dtype=np.uint8, shape=shape)
        rng = np.random.default_rng(0)
        for z in range(a.z):
            vol[z] = rng.integers(0, 256, shape[1:], dtype=np.uint8)
        vol.flush()
        del vol
        vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")
        out = np.lib.format.open_memmap(os.path.join(tmp, "out.npy"), mode="w+", dtype=np.uint8, shape=shape)
        start, size = (0, 0, 0), (a.x, a.y, a.z)
        predict_volume(vol, start, size, model, ms_x, ms_y, out=out)          # warm: plans, pinned buffers, page cache
        torch.cuda.synchronize()
        runs = []
        for _ in range(a.reps):
            torch.cuda.reset_peak_memory_stats()
            st = {}
            t0 = time.perf_counter()
            predict_volume(vol, start, size, model, ms_x, ms_y, out=out, stats=st)
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0, st, torch.cuda.max_memory_allocated()))
        # host planning alone (tile_plan_2d + chunk_plan, part of every predict_volume call)
        t0 = time.perf_counter()
        od, buf, _, chunks = _chunk_plan(start, size, model.outdimsize, model.buffer, shape, None, is3d=False)
        plan_s = time.perf_counter() - t0
        # generator alone on the same batches: sum of the plan.run() spans
        edge = od + 2 * buf
        nb = default_tile_batch(edge, False)
        gen_ms, batches = 0.0, 0
        for c in chunks:
            for b0 in range(0, len(c.tiles), nb):
                plan = model.generator_g.plan((min(nb, len(c.tiles) - b0), 1, edge, edge, 1))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                plan.run()
                e1.record()
                e1.synchronize()
                gen_ms += e0.elapsed_time(e1)
                batches += 1
        wall, st, peak = min(runs, key=lambda r: r[0])
        vox = a.x * a.y * a.z
        print(json.dumps({
            "roi_xyz": list(size), "chunks": st["chunks"], "tiles": sum(len(c.tiles) for c in chunks),
            "tile_batch": nb, "generator_batches": batches, "batch_shapes": len({len(c.tiles) for c in chunks}),
            "host_planning_s": round(plan_s, 4),
            "end_to_end_s": round(wall, 4), "gvox_per_s": round(vox / wall / 1e9, 3),
            "generator_only_s": round(gen_ms / 1e3, 4), "generator_only_gvox_per_s": round(vox / gen_ms / 1e6, 3),
            "end_to_end_over_generator": round(wall / (gen_ms / 1e3), 3),
            "host_read_s": round(st["read_s"], 4), "host_write_s": round(st["write_s"], 4),
            "peak_device_bytes": int(peak), "all_runs_s": [round(r[0], 4) for r in runs]}))


if __name__ == "__main__":
    main()
