"""Cost of CLAHE around tiled inference, on a 1024x1024x512 uint8 np.memmap with tile 128 and the 132 model.

--passes 1 (default): the two out-of-core passes and their floors, alternating within every repetition:
    histograms  utils.clahe_histograms (read thread -> pinned -> H2D -> tem_u8_hist_tiles, one read-back)
    read        the bare chunked read of the same slabs into one buffer: the floor, the pass is read-bound
    volume      utils.clahe_volume, memmap -> memmap (read -> H2D -> tem_u8_clahe -> D2H -> write)
  and once: the numpy reference (tests/clahe_ref.py: np.bincount per tile, the tables, the interpolated remap) over
  --ref-sections sections, scaled to the volume; its output must equal clahe_volume's on those sections.
--predict 1 (default): utils.predict_volume, memmap -> memmap, in the configurations of --configs that alternate
  within every repetition:
    none   called without the keyword, so `--configs none --passes 0 --kernels 0 --root <checkout>` also runs on a
           commit that has no `clahe` yet, for a before / after figure of the default path, each in its own process
    clahe  clahe = the tables of the volume (one tem_u8_clahe launch per chunk)
--kernels 1 adds the two kernels' own times from device events over 20 launches on one default chunk's footprint
(326^3 bytes at an origin off the tile grid; EM-like bytes, uniformly random bytes and a constant).
Every figure comes with all its runs: the run-to-run spread is what a difference has to exceed.
Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 500 python tests/tools/predict_clahe_time.py [--x 1024 --y 1024 --z 512] [--tile 128] [--reps 3]
        [--configs none,clahe] [--passes 1] [--predict 1] [--kernels 1] [--root DIR]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

_TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MS_X, MS_Y = (0.02, 0.58), (-0.1, 0.4)


def kernel_times(tile):
    from transfer_em_amd import _lib
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    n, org = 326, (77, 301)                                   # a chunk's footprint, off the tile grid
    gy, gx = -(-(org[0] + n) // tile), -(-(org[1] + n) // tile)
    res = {}
    counts = torch.zeros((n, gy, gx, 256), dtype=torch.int32, device="cuda")
    tables = torch.randint(0, 256, (n, gy, gx, 256), dtype=torch.uint8, device="cuda").sort(dim=-1).values
    for fill in ("em_like", "random", "constant"):
        if fill == "random":
            buf = torch.randint(0, 256, (n, n, n), dtype=torch.uint8, device="cuda")
        elif fill == "em_like":
            buf = (torch.randn((n, n, n), device="cuda") * 9 + 120).clamp(0, 255).to(torch.uint8)
        else:
            buf = torch.full((n, n, n), 120, dtype=torch.uint8, device="cuda")
        src = buf.clone()

        def hist():
            _lib.check(lib.tem_u8_hist_tiles(buf.data_ptr(), n, n, n, *org, tile, tile, gy, gx, counts.data_ptr(), stream),
                       "tem_u8_hist_tiles")

        def remap():                                          # in place: every launch starts from the same bytes
            _lib.check(lib.tem_u8_clahe(buf.data_ptr(), n, n, n, 0, *org, tables.data_ptr(), gy, gx, tile, tile, stream),
                       "tem_u8_clahe")
        for name, fn, nbytes in (("hist_tiles", hist, n ** 3), ("clahe", remap, 2 * n ** 3)):
            t = []
            for _ in range(23):
                buf.copy_(src)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                t.append(a.elapsed_time(b) * 1e3)
            t = t[3:]
            res[f"{name}_326_{fill}"] = {"us_min": round(min(t), 1), "us_median": round(sorted(t)[len(t) // 2], 1),
                                         "bytes": nbytes, "tb_per_s": round(nbytes / (min(t) * 1e-6) / 1e12, 3)}
        counts.zero_()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--tile", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="none,clahe")
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--predict", type=int, default=1)
    ap.add_argument("--kernels", type=int, default=1)
    ap.add_argument("--ref-sections", type=int, default=2)
    ap.add_argument("--root", default=os.path.dirname(_TESTS), help="the checkout to import transfer_em_amd from")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path[:0] = [root, os.path.join(root, "tests")]
    from transfer_em_amd import utils
    shape, start, size = (a.z, a.y, a.x), (0, 0, 0), (a.x, a.y, a.z)
    nbytes = a.x * a.y * a.z
    res = {"roi_xyz": list(size), "tile": a.tile, "root": root}
    names = a.configs.split(",")
    with tempfile.TemporaryDirectory() as tmp:
        def new(name):
            return np.lib.format.open_memmap(os.path.join(tmp, name + ".npy"), mode="w+", dtype=np.uint8, shape=shape)
        vol = new("vol")
        rng = np.random.default_rng(0)
        ramp = (24 * np.linspace(-1, 1, a.y)[:, None] + 16 * np.linspace(-1, 1, a.x)[None, :])[None]
        blk = np.clip(rng.normal(120, 9, (min(64, a.z),) + shape[1:]) + ramp, 0, 240).astype(np.uint8)
        for z in range(0, a.z, 64):                     # EM-like: a few dozen bins, drifting in the plane and with z
            vol[z:z + 64] = blk[:min(64, a.z - z)] + np.uint8(z // 64 % 16)
        vol.flush()
        del vol
        vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")
        c = None
        if a.passes or "clahe" in names:
            c = utils.clahe_fit(vol, a.tile)
            res["tables_bytes"] = int(c.tables.nbytes)

        if a.passes:
            slabs = utils.hist_chunks(utils.hist_box(shape))
            stage = np.empty(max((b[0][1] - b[0][0]) for b in slabs) * a.y * a.x, np.uint8)
            eq = new("eq")

            def histograms(st):
                return utils.clahe_histograms(vol, a.tile, stats=st)

            def read(st):
                for (z0, z1), _, _ in slabs:
                    stage[:(z1 - z0) * a.y * a.x].reshape(z1 - z0, a.y, a.x)[...] = vol[z0:z1]

            def volume(st):
                return utils.clahe_volume(vol, c, out=eq, stats=st)
            fns = (("histograms", histograms), ("read", read), ("volume", volume))
            runs = {n: [] for n, _ in fns}
            for rep in range(a.reps + 1):               # repetition 0 warms buffers and the page cache
                for n, fn in fns:
                    st = {}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(st)
                    torch.cuda.synchronize()
                    if rep:
                        runs[n].append((time.perf_counter() - t0, st))
            res["passes"] = {"slabs": len(slabs)}
            for n, r in runs.items():
                wall, st = min(r, key=lambda v: v[0])
                res["passes"][n] = {"s": round(wall, 4), "all_runs_s": [round(v[0], 4) for v in r],
                                    "gb_per_s": round(nbytes / wall / 1e9, 2)}
                for k in ("read_s", "write_s"):
                    if k in st:
                        res["passes"][n]["host_" + k] = round(st[k], 4)
            from clahe_ref import ref_remap, ref_tile_hist
            k = min(a.ref_sections, a.z)
            sec = np.asarray(vol[:k])
            t0 = time.perf_counter()
            h = ref_tile_hist(sec, a.tile, a.tile)
            t1 = time.perf_counter()
            T = utils.clahe_tables(h)
            t2 = time.perf_counter()
            ref = ref_remap(sec, T, a.tile, a.tile)
            t3 = time.perf_counter()
            res["numpy_reference"] = {"sections": k, "histograms_s": round(t1 - t0, 4), "tables_s": round(t2 - t1, 4),
                                      "remap_s": round(t3 - t2, 4),
                                      "scaled_to_volume_s": round((t3 - t0) * a.z / k, 2),
                                      "equals_clahe_volume": bool(np.array_equal(ref, np.asarray(eq[:k])))}

        if a.predict:
            from transfer_em_amd.cgan import EM2EM
            from transfer_em_amd.models.generator import generator_param_shapes
            from util import scaled_params                  # tests/util.py: outputs spread over the uint8 range
            model = EM2EM(132, "clahetime", checkpoint_root=tmp)
            Pm = scaled_params(generator_param_shapes(True), 4)
            Pm["f2"] = Pm["f2"] * 20
            model.generator_g.params.load_dict(Pm)
            out = new("out")

            def run(n, st):
                kw = {} if n == "none" else {"clahe": c}
                utils.predict_volume(vol, start, size, model, MS_X, MS_Y, out=out, stats=st, **kw)
            runs = {n: [] for n in names}
            res["configs"] = {}
            for rep in range(a.reps + 1):                   # repetition 0 warms plans, buffers, page cache
                for n in names:
                    st = {}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(n, st)
                    torch.cuda.synchronize()
                    if rep:
                        runs[n].append((time.perf_counter() - t0, st))
            for n in names:
                wall, st = min(runs[n], key=lambda r: r[0])
                res["configs"][n] = {"end_to_end_s": round(wall, 4), "all_runs_s": [round(r[0], 4) for r in runs[n]],
                                     "gvox_per_s": round(nbytes / wall / 1e9, 3), "host_read_s": round(st["read_s"], 4),
                                     "host_write_s": round(st["write_s"], 4), "chunks": st["chunks"]}
            model.generator_g.clear_plans()
        if a.kernels:
            res["kernels"] = kernel_times(a.tile)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
