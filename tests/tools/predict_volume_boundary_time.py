"""Cost of the boundary modes of the out-of-core prediction (utils.predict_volume): the 132 model over a
~1024x1024x512 uint8 np.memmap, written into an np.memmap output, under boundary "zeros", "reflect" and "edge" in turn
(the memmap -> memmap run of predict_volume_time.py, once per mode).  "zeros" is called without the keyword, so the
script also runs on a commit that has no `boundary` yet (--modes zeros) for a before / after figure of the default
path.  Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 400 python tests/tools/predict_volume_boundary_time.py [--x 1024 --y 1024 --z 512] [--reps 2]
        [--modes zeros,reflect,edge]
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
    ap.add_argument("--modes", default="zeros,reflect,edge")
    a = ap.parse_args()
    from transfer_em_amd.cgan import EM2EM
    from transfer_em_amd.utils import chunk_plan, predict_volume
    ms_x, ms_y = (0.02, 0.58), (-0.1, 0.4)
    with tempfile.TemporaryDirectory() as tmp:
        model = EM2EM(132, "pvbtime", checkpoint_root=tmp)
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
        res = {"roi_xyz": list(size), "modes": {}}
        for mode in a.modes.split(","):
            kw = {} if mode == "zeros" else {"boundary": mode}
            predict_volume(vol, start, size, model, ms_x, ms_y, out=out, **kw)   # warm: plans, pinned buffers, page cache
            torch.cuda.synchronize()
            runs = []
            for _ in range(a.reps):
                st = {}
                t0 = time.perf_counter()
                predict_volume(vol, start, size, model, ms_x, ms_y, out=out, stats=st, **kw)
                torch.cuda.synchronize()
                runs.append((time.perf_counter() - t0, st))
            wall, st = min(runs, key=lambda r: r[0])
            chunks = chunk_plan(start, size, model.outdimsize, model.buffer, shape, None, **kw)
            res["modes"][mode] = {
                "end_to_end_s": round(wall, 4), "gvox_per_s": round(a.x * a.y * a.z / wall / 1e9, 3),
                "all_runs_s": [round(r[0], 4) for r in runs], "host_read_s": round(st["read_s"], 4),
                "host_write_s": round(st["write_s"], 4), "chunks": st["chunks"],
                "tiles": sum(len(c.tiles) for c in chunks), "voxels_read": sum(int(np.prod(c.block)) for c in chunks)}
        if "zeros" in res["modes"]:
            z = res["modes"]["zeros"]["end_to_end_s"]
            for mode, r in res["modes"].items():
                r["over_zeros"] = round(r["end_to_end_s"] / z, 4)
        print(json.dumps(res))


if __name__ == "__main__":
    main()
