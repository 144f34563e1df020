"""Cost of repairing damaged sections and voxels along z on the device, on a 1024x1024x512 EM-like uint8 np.memmap.

--volume 1 (default): utils.volume_repair, memmap -> memmap, max_gap 8, in two cases that alternate with their floor
  within every repetition:
    sections  a handful of bad sections (--sections, default 5 singles and one run of 3)
    mask      the same plus a mask memmap with 1 % of the voxels bad, in runs of 1...12 along z
    io        the bare chunked read of the same read slabs (once more for the mask) into a buffer plus the bare write of
              the same core slabs from a buffer, in this process on one thread: the pass's own floor
  and once: the numpy reference (tests/repair_ref.py) on a --numpy-box^3 corner with the corner's share of the defects,
  scaled to the volume; volume_repair's output must equal it there.
--kernels 1 (default): tem_u8_repair_z alone on a 326^3 block (a default chunk's footprint of the 132 model; the core is
  the block), device events, 20 launches, min -- on defect-free data (section flags, none set; and a mask of zeros: two
  bytes read per voxel), with 1 % of the voxels masked, and with every other run of 1...12 voxels bad (half-bad: the
  back-fill's worst case) -- beside tem_u8_lut on the same block in the same process.  The block is restored before
  every launch.
--predict 1 (default): utils.predict_volume with the 132 model, memmap -> memmap, in the configurations of --configs
  that alternate within every repetition:
    none    called without the keyword, so `--configs none --volume 0 --kernels 0 --root <checkout>` also runs on a
            commit that has no `repair` yet, for a before / after figure of the default path, each in its own process
    repair  repair = the bad sections (one tem_u8_repair_z launch per chunk, footprints read with max_gap more sections)
Every figure comes with all its runs: the run-to-run spread is what a difference has to exceed.
Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 900 python tests/tools/volume_repair_time.py [--x 1024 --y 1024 --z 512] [--reps 3] [--volume 1]
        [--kernels 1] [--predict 1] [--configs none,repair] [--numpy-box 64] [--root DIR]
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
GAP = 8


def _dims(box):
    return tuple(hi - lo for lo, hi in box)


def run_mask(shape, fraction, rng):
    """A uint8 mask with about `fraction` of the voxels bad, in runs of 1...12 along z at random columns."""
    Z, Y, X = shape
    m = np.zeros(shape, np.uint8)
    n = int(fraction * Z * Y * X / 6.5)
    z, y, x, ln = rng.integers(0, Z, n), rng.integers(0, Y, n), rng.integers(0, X, n), rng.integers(1, 13, n)
    for d in range(12):
        keep = (ln > d) & (z + d < Z)
        m[z[keep] + d, y[keep], x[keep]] = 1
    return m


def kernel_times():
    from transfer_em_amd import _lib
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    n = 326
    rng = np.random.default_rng(1)
    src = (torch.randn((n, n, n), device="cuda") * 9 + 120).clamp(0, 255).to(torch.uint8)
    buf = src.clone()
    flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
    lut = torch.arange(255, -1, -1, dtype=torch.uint8, device="cuda")
    zeros = torch.zeros((n, n, n), dtype=torch.uint8, device="cuda")
    one = torch.from_numpy(run_mask((n, n, n), 0.01, rng)).cuda()
    half = np.zeros((n, n * n), np.uint8)                                  # per column: runs of 1...12, every other one bad
    ln = rng.integers(1, 13, (n, n * n))
    ends = np.cumsum(ln, axis=0)
    for k in range(1, n, 2):
        lo, hi = ends[k - 1], ends[k]
        for d in range(12):
            z = lo + d
            keep = (z < hi) & (z < n)
            half[z[keep], np.flatnonzero(keep)] = 1
    half = torch.from_numpy(half.reshape(n, n, n)).cuda()
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")

    def repair(mask, sections, cnt=None):
        return lambda: _lib.check(lib.tem_u8_repair_z(buf.data_ptr(), n, n, n, 0, 0, n, mask, sections, -1, GAP, cnt,
                                                      stream), "tem_u8_repair_z")
    cases = [("lut", lambda: _lib.check(lib.tem_u8_lut(buf.data_ptr(), n, n, n, lut.data_ptr(), 0, 0, stream),
                                        "tem_u8_lut"), 2 * n ** 3),
             ("repair_defect_free_flags", repair(None, flags.data_ptr()), n ** 3),
             ("repair_defect_free_mask", repair(zeros.data_ptr(), None), 2 * n ** 3),
             ("repair_mask_1pct", repair(one.data_ptr(), None), 2 * n ** 3),
             ("repair_mask_1pct_counts", repair(one.data_ptr(), None, counts.data_ptr()), 2 * n ** 3),
             ("repair_half_bad", repair(half.data_ptr(), None), 2 * n ** 3)]
    res = {"bad_fraction_1pct": round(float(one.float().mean()), 4), "bad_fraction_half": round(float(half.float().mean()), 4)}
    for name, fn, nbytes in cases:
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
        res[name] = {"us_min": round(min(t), 1), "us_median": round(sorted(t)[len(t) // 2], 1), "bytes_read": nbytes if
                     name != "lut" else n ** 3, "tb_per_s": round(nbytes / (min(t) * 1e-6) / 1e12, 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--volume", type=int, default=1)
    ap.add_argument("--kernels", type=int, default=1)
    ap.add_argument("--predict", type=int, default=1)
    ap.add_argument("--configs", default="none,repair")
    ap.add_argument("--numpy-box", type=int, default=64)
    ap.add_argument("--root", default=os.path.dirname(_TESTS), help="the checkout to import transfer_em_amd from")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path[:0] = [root, os.path.join(root, "tests")]
    from transfer_em_amd import utils
    shape, start, size = (a.z, a.y, a.x), (0, 0, 0), (a.x, a.y, a.z)
    nbytes = a.x * a.y * a.z
    res = {"volume_xyz": list(size), "max_gap": GAP, "root": root}
    names = a.configs.split(",")
    sections = sorted({z for z in (3, 40, 41, 42, a.z // 3, a.z // 2, 2 * a.z // 3, a.z - 1) if 0 <= z < a.z})
    res["sections"] = sections
    with tempfile.TemporaryDirectory() as tmp:
        def new(name):
            return np.lib.format.open_memmap(os.path.join(tmp, name + ".npy"), mode="w+", dtype=np.uint8, shape=shape)
        vol = new("vol")
        rng = np.random.default_rng(0)
        blk = np.clip(rng.normal(120, 9, (min(64, a.z),) + shape[1:]), 0, 240).astype(np.uint8)
        for z in range(0, a.z, 64):                         # EM-like: a few dozen bins around 120, drifting with z
            vol[z:z + 64] = blk[:min(64, a.z - z)] + np.uint8(z // 64 % 16)
        for z in sections:
            vol[z] = 0                                      # lost sections: black
        vol.flush()
        del vol
        vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")

        if a.volume:
            import repair_ref as RR
            msk = new("mask")
            mblk = run_mask((min(64, a.z),) + shape[1:], 0.01, rng)
            for z in range(0, a.z, 64):
                msk[z:z + 64] = mblk[:min(64, a.z - z)]
            msk.flush()
            del msk
            msk = np.load(os.path.join(tmp, "mask.npy"), mmap_mode="r")
            out = new("out")
            chunks = utils.repair_chunks(utils.hist_box(shape), shape, GAP)
            stage = [np.empty(max(int(np.prod(_dims(b))) for b in side), np.uint8) for side in zip(*chunks)]
            cases = {"sections": utils.Repair(sections=sections, max_gap=GAP),
                     "mask": utils.Repair(sections=sections, mask=msk, max_gap=GAP)}

            def io(srcs):
                def fn(st):
                    for core, rd in chunks:
                        (z0, z1), (y0, y1), (x0, x1) = rd
                        for s in srcs:
                            stage[1][:int(np.prod(_dims(rd)))].reshape(_dims(rd))[...] = s[z0:z1, y0:y1, x0:x1]
                        (z0, z1), (y0, y1), (x0, x1) = core
                        out[z0:z1, y0:y1, x0:x1] = stage[0][:int(np.prod(_dims(core)))].reshape(_dims(core))
                return fn
            fns = [("sections", lambda st: utils.volume_repair(vol, cases["sections"], out=out, stats=st)),
                   ("io_sections", io([vol])),
                   ("mask", lambda st: utils.volume_repair(vol, cases["mask"], out=out, stats=st)),
                   ("io_mask", io([vol, msk]))]
            runs = {n: [] for n, _ in fns}
            for rep in range(a.reps + 1):                   # repetition 0 warms buffers and the page cache
                for n, fn in fns:
                    st = {}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(st)
                    torch.cuda.synchronize()
                    if rep:
                        runs[n].append((time.perf_counter() - t0, st))
            r = res["volume_repair"] = {"slabs": len(chunks), "bytes_read": sum(int(np.prod(_dims(rd))) for _, rd in chunks),
                                        "bytes_written": nbytes}
            for n, rr in runs.items():
                wall, st = min(rr, key=lambda v: v[0])
                r[n] = {"s": round(wall, 4), "all_runs_s": [round(v[0], 4) for v in rr],
                        "gb_per_s_of_volume": round(nbytes / wall / 1e9, 3)}
                for key in ("read_s", "write_s", "repaired", "unrepaired"):
                    if key in st:
                        r[n][("host_" if key.endswith("_s") else "") + key] = round(st[key], 4) if key.endswith("_s") else st[key]
            nb = min(a.numpy_box, a.z, a.y, a.x)
            utils.volume_repair(vol, cases["mask"], out=out)            # `io` wrote its buffer over the result
            corner, cmask = np.asarray(vol[:, :nb, :nb]), np.asarray(msk[:, :nb, :nb])
            t0 = time.perf_counter()
            want = RR.repair(corner, sections, cmask, None, GAP)
            t1 = time.perf_counter()
            r["numpy_reference"] = {"corner_zyx": list(corner.shape), "s": round(t1 - t0, 4),
                                    "scaled_to_volume_s": round((t1 - t0) * nbytes / corner.size, 2),
                                    "equals_volume_repair": bool(np.array_equal(want, np.asarray(out[:, :nb, :nb])))}
            del out, msk
            os.remove(os.path.join(tmp, "out.npy"))
            os.remove(os.path.join(tmp, "mask.npy"))

        if a.predict:
            from transfer_em_amd.cgan import EM2EM
            from transfer_em_amd.models.generator import generator_param_shapes
            from util import scaled_params                  # tests/util.py: outputs spread over the uint8 range
            model = EM2EM(132, "repairtime", checkpoint_root=tmp)
            Pm = scaled_params(generator_param_shapes(True), 4)
            Pm["f2"] = Pm["f2"] * 20
            model.generator_g.params.load_dict(Pm)
            out = new("pred")

            def run(n, st):
                kw = {} if n == "none" else {"repair": utils.Repair(sections=sections, max_gap=GAP)}
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
            res["kernels"] = kernel_times()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
