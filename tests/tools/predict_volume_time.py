"""Throughput of the out-of-core prediction (utils.predict_volume) with the 132 model over a ~1024x1024x512 uint8
np.memmap, written into an np.memmap output, against the generator alone on the same tiles (the sum of the
plan.run() spans, timed with events).  Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 300 python tests/tools/predict_volume_time.py [--x 1024 --y 1024 --z 512] [--reps 2]
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
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    from transfer_em_amd.cgan import EM2EM
    from transfer_em_amd.utils import _chunk_plan, predict_volume, TILE_BATCH
    ms_x, ms_y = (0.02, 0.58), (-0.1, 0.4)
    with tempfile.TemporaryDirectory() as tmp:
        model = EM2EM(132, "pvtime", checkpoint_root=tmp)
        shape = (a.z, a.y, a.x)
        vol = np.lib.format.open_memmap(os.path.join(tmp, "vol.npy"), mode="w+", dtype=np.uint8, shape=shape)
        rng = np.random.default_rng(0)
        for z in range(0, a.z, 64):
            vol[z:z + 64] = rng.integers(0, 256, (min(64, a.z - z),) + shape[1:], dtype=np.uint8)
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
        # generator alone on the same batches: sum of the plan.run() spans
        od, buf, _, chunks = _chunk_plan(start, size, model.outdimsize, model.buffer, shape, None)
        edge = od + 2 * buf
        gen_ms = 0.0
        for c in chunks:
            for b0 in range(0, len(c.tiles), TILE_BATCH):
                plan = model.generator_g.plan((min(TILE_BATCH, len(c.tiles) - b0), edge, edge, edge, 1))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                plan.run()
                e1.record()
                e1.synchronize()
                gen_ms += e0.elapsed_time(e1)
        wall, st, peak = min(runs, key=lambda r: r[0])
        vox = a.x * a.y * a.z
        print(json.dumps({
            "roi_xyz": list(size), "chunks": st["chunks"], "tiles": sum(len(c.tiles) for c in chunks),
            "end_to_end_s": round(wall, 4), "gvox_per_s": round(vox / wall / 1e9, 3),
            "generator_only_s": round(gen_ms / 1e3, 4), "generator_only_gvox_per_s": round(vox / gen_ms / 1e6, 3),
            "end_to_end_over_generator": round(wall / (gen_ms / 1e3), 3),
            "host_read_s": round(st["read_s"], 4), "host_write_s": round(st["write_s"], 4),
            "peak_device_bytes": int(peak), "all_runs_s": [round(r[0], 4) for r in runs]}))


if __name__ == "__main__":
    main()
