"""Cost of the intensity histograms and lookup tables of tiled inference, on a 1024x1024x512 uint8 np.memmap.

--hist 1 (default): the out-of-core histogram pass, three ways over the same memmap, alternating within every
repetition:
    device    utils.volume_histogram (read thread -> pinned -> H2D -> tem_u8_hist, one read-back)
    bincount  np.bincount of the same slabs on the host, summed
    read      the bare chunked read of the same slabs into one buffer: the floor, the pass is read-bound
`device` and `bincount` must give the same counts.  Times and GB/s of the volume's bytes.

--predict 1 (default): utils.predict_volume, memmap -> memmap with the 132 model, in the configurations of --configs
that alternate within every repetition:
    none   called without the new keywords, so `--configs none --hist 0` also runs on a commit that has no `lut` yet,
           for a before / after figure of the default path
    lut    lut = a [256] table (one tem_u8_lut launch per chunk)
    hist   histogram=True (one tem_u8_hist launch per chunk, one read-back); checked against np.bincount of the output
--kernels 1 adds the two kernels' own times from device events over 20 launches on one default chunk's blocks (input
footprint 326^3, output 288^3 bytes of random data, and of a constant for the histogram's contention case).
Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 500 python tests/tools/volume_histogram_time.py [--x 1024 --y 1024 --z 512] [--reps 3]
        [--configs none,lut,hist] [--hist 1] [--predict 1] [--kernels 1]
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
sys.path[:0] = [os.path.dirname(_TESTS), _TESTS]

MS_X, MS_Y = (0.02, 0.58), (-0.1, 0.4)


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


def kernel_times():
    from transfer_em_amd import _lib
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    res = {}
    counts = torch.zeros(256, dtype=torch.int64, device="cuda")
    table = torch.arange(255, -1, -1, dtype=torch.uint8, device="cuda")
    for name, n, fill in (("hist_288_random", 288, None), ("hist_288_em_like", 288, "em"), ("hist_288_constant", 288, 0),
                          ("lut_326_random", 326, None)):
        if fill is None:
            buf = torch.randint(0, 256, (n, n, n), dtype=torch.uint8, device="cuda")
        elif fill == "em":
            buf = (torch.randn((n, n, n), device="cuda") * 9 + 120).clamp(0, 255).to(torch.uint8)
        else:
            buf = torch.full((n, n, n), fill, dtype=torch.uint8, device="cuda")
        if name.startswith("hist"):
            fn = lambda: _lib.check(lib.tem_u8_hist(buf.data_ptr(), n, n, n, 0, n, 0, n, 0, n, counts.data_ptr(), 0,
                                                    stream), "tem_u8_hist")
            nbytes = n ** 3
        else:
            fn = lambda: _lib.check(lib.tem_u8_lut(buf.data_ptr(), n, n, n, table.data_ptr(), 0, 0, stream), "tem_u8_lut")
            nbytes = 2 * n ** 3
        r = _events(fn)
        r["bytes"], r["tb_per_s"] = nbytes, round(nbytes / (r["us_min"] * 1e-6) / 1e12, 3)
        res[name] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="none,lut,hist")
    ap.add_argument("--hist", type=int, default=1)
    ap.add_argument("--predict", type=int, default=1)
    ap.add_argument("--kernels", type=int, default=1)
    a = ap.parse_args()
    from transfer_em_amd import utils
    shape, start, size = (a.z, a.y, a.x), (0, 0, 0), (a.x, a.y, a.z)
    nbytes = a.x * a.y * a.z
    res = {"roi_xyz": list(size)}
    with tempfile.TemporaryDirectory() as tmp:
        def new(name):
            return np.lib.format.open_memmap(os.path.join(tmp, name + ".npy"), mode="w+", dtype=np.uint8, shape=shape)
        vol = new("vol")
        rng = np.random.default_rng(0)
        blk = np.clip(rng.normal(120, 9, (min(64, a.z),) + shape[1:]), 0, 240).astype(np.uint8)
        for z in range(0, a.z, 64):                     # EM-like: a few dozen bins around 120, drifting with z
            vol[z:z + 64] = blk[:min(64, a.z - z)] + np.uint8(z // 64 % 16)
        vol.flush()
        del vol
        vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")

        if a.hist:
            slabs = utils.hist_chunks(utils.hist_box(shape))
            stage = np.empty(max((b[0][1] - b[0][0]) for b in slabs) * a.y * a.x, np.uint8)

            def device(st):
                return utils.volume_histogram(vol, stats=st)

            def bincount(st):
                h = np.zeros(256, np.int64)
                for (z0, z1), _, _ in slabs:
                    h += np.bincount(np.asarray(vol[z0:z1]).reshape(-1), minlength=256)
                return h

            def read(st):
                for (z0, z1), _, _ in slabs:
                    stage[:(z1 - z0) * a.y * a.x].reshape(z1 - z0, a.y, a.x)[...] = vol[z0:z1]
            runs, last = {"device": [], "bincount": [], "read": []}, {}
            for rep in range(a.reps + 1):               # repetition 0 warms buffers and the page cache
                for n, fn in (("device", device), ("bincount", bincount), ("read", read)):
                    st = {}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[n] = fn(st)
                    torch.cuda.synchronize()
                    if rep:
                        runs[n].append((time.perf_counter() - t0, st))
            res["histogram"] = {"slabs": len(slabs), "device_equals_bincount": bool(np.array_equal(last["device"], last["bincount"])),
                                "occupied_bins": int(np.count_nonzero(last["device"]))}
            for n, r in runs.items():
                wall, st = min(r, key=lambda v: v[0])
                res["histogram"][n] = {"s": round(wall, 4), "all_runs_s": [round(v[0], 4) for v in r],
                                       "gb_per_s": round(nbytes / wall / 1e9, 2)}
                if "read_s" in st:
                    res["histogram"][n]["host_read_s"] = round(st["read_s"], 4)

        if a.predict:
            from transfer_em_amd.cgan import EM2EM
            from transfer_em_amd.models.generator import generator_param_shapes
            from util import scaled_params                  # tests/util.py: outputs spread over the uint8 range
            names = a.configs.split(",")
            model = EM2EM(132, "histtime", checkpoint_root=tmp)
            Pm = scaled_params(generator_param_shapes(True), 4)
            Pm["f2"] = Pm["f2"] * 20
            model.generator_g.params.load_dict(Pm)
            out = new("out")
            table = (255 - np.arange(256)).astype(np.uint8)

            def run(n, st):
                if n == "none":
                    utils.predict_volume(vol, start, size, model, MS_X, MS_Y, out=out, stats=st)
                elif n == "lut":
                    utils.predict_volume(vol, start, size, model, MS_X, MS_Y, out=out, stats=st, lut=table)
                else:
                    utils.predict_volume(vol, start, size, model, MS_X, MS_Y, out=out, stats=st, histogram=True)
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
                    if n == "hist" and rep == a.reps:
                        want = np.zeros(256, np.int64)
                        for z in range(0, a.z, 64):
                            want += np.bincount(np.asarray(out[z:z + 64]).reshape(-1), minlength=256)
                        res["histogram_equals_bincount_of_out"] = bool(np.array_equal(st["histogram"], want))
            for n in names:
                wall, st = min(runs[n], key=lambda r: r[0])
                res["configs"][n] = {"end_to_end_s": round(wall, 4), "all_runs_s": [round(r[0], 4) for r in runs[n]],
                                     "gvox_per_s": round(nbytes / wall / 1e9, 3), "host_read_s": round(st["read_s"], 4),
                                     "host_write_s": round(st["write_s"], 4), "chunks": st["chunks"]}
            model.generator_g.clear_plans()
        if a.kernels:
            res["kernels"] = kernel_times()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
