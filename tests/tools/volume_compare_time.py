"""Cost of comparing two uint8 volumes on the device, on a pair of 1024x1024x512 uint8 np.memmaps (an EM-like volume
and the same volume plus noise in [-6, 6]: a band around the diagonal of the joint histogram).

--joint 1 (default): the out-of-core joint histogram, three ways over the same memmaps, alternating within every
repetition:
    device    utils.volume_joint_histogram (read thread -> pinned -> H2D -> tem_u8_hist2, one read-back)
    read      the bare chunked read of the same slabs of both files into two buffers: the floor, the pass is read-bound
    numpy     np.bincount(256 a + b) on --numpy-sections sections, scaled to the volume
`device` is checked against np.bincount on those sections.  Times and GB/s of the two volumes' bytes.

--predict 1 (default): utils.predict_volume, memmap -> memmap with the 132 model, in the configurations of --configs
that alternate within every repetition:
    none      called without the keyword, so `--configs none --joint 0 --kernels 0` also runs on a commit that has no
              `compare` yet, for a before / after figure of the default path
    compare   compare = the second memmap (one more read and one tem_u8_hist2 launch per chunk, one read-back);
              checked against np.bincount of (ground truth, output) on the first sections
--kernels 1 adds tem_u8_hist2's own time from device events over 20 launches on one default chunk's output block
(288^3) for three kinds of pair -- EM-like, uniformly random, constant -- next to tem_u8_hist on the same block.
Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 500 python tests/tools/volume_compare_time.py [--x 1024 --y 1024 --z 512] [--reps 3]
        [--configs none,compare] [--joint 1] [--predict 1] [--kernels 1] [--numpy-sections 8]
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


def _joint(a, b):
    return np.bincount(a.ravel().astype(np.int64) * 256 + b.ravel(), minlength=65536).reshape(256, 256)


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


def kernel_times(n=288):
    from transfer_em_amd import _lib
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    res = {}
    joint = torch.zeros((256, 256), dtype=torch.int64, device="cuda")
    counts = torch.zeros(256, dtype=torch.int64, device="cuda")
    for name in ("em_like", "random", "constant"):
        if name == "em_like":
            a = (torch.randn((n, n, n), device="cuda") * 9 + 120).clamp(0, 255).to(torch.uint8)
            b = (a.to(torch.int16) + torch.randint(-6, 7, (n, n, n), device="cuda", dtype=torch.int16)).clamp(0, 255) \
                .to(torch.uint8)
        elif name == "random":
            a = torch.randint(0, 256, (n, n, n), dtype=torch.uint8, device="cuda")
            b = torch.randint(0, 256, (n, n, n), dtype=torch.uint8, device="cuda")
        else:
            a = torch.full((n, n, n), 120, dtype=torch.uint8, device="cuda")
            b = torch.full((n, n, n), 121, dtype=torch.uint8, device="cuda")
        joint.zero_()
        one = lambda: _lib.check(lib.tem_u8_hist2(a.data_ptr(), n, n, n, 0, 0, 0, b.data_ptr(), n, n, n, 0, 0, 0, n, n, n,
                                                  joint.data_ptr(), stream), "tem_u8_hist2")
        one()
        occupied = int(torch.count_nonzero(joint).item())
        r = _events(one)
        r.update(voxels=n ** 3, occupied_bins=occupied, gvox_per_s=round(n ** 3 / (r["us_min"] * 1e-6) / 1e9, 1))
        res[f"hist2_{n}_{name}"] = r
        r = _events(lambda: _lib.check(lib.tem_u8_hist(b.data_ptr(), n, n, n, 0, n, 0, n, 0, n, counts.data_ptr(), 0,
                                                       stream), "tem_u8_hist"))
        r.update(voxels=n ** 3, gvox_per_s=round(n ** 3 / (r["us_min"] * 1e-6) / 1e9, 1))
        res[f"hist_{n}_{name}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="none,compare")
    ap.add_argument("--joint", type=int, default=1)
    ap.add_argument("--predict", type=int, default=1)
    ap.add_argument("--kernels", type=int, default=1)
    ap.add_argument("--numpy-sections", type=int, default=8)
    a = ap.parse_args()
    from transfer_em_amd import utils
    shape, start, size = (a.z, a.y, a.x), (0, 0, 0), (a.x, a.y, a.z)
    nbytes = a.x * a.y * a.z
    res = {"roi_xyz": list(size)}
    names = a.configs.split(",")
    need_gt = a.joint or "compare" in names
    with tempfile.TemporaryDirectory() as tmp:
        def new(name):
            return np.lib.format.open_memmap(os.path.join(tmp, name + ".npy"), mode="w+", dtype=np.uint8, shape=shape)
        vol, gt = new("vol"), new("gt") if need_gt else None
        rng = np.random.default_rng(0)
        zb = min(64, a.z)
        blk = np.clip(rng.normal(120, 9, (zb,) + shape[1:]), 0, 240).astype(np.uint8)
        noise = rng.integers(-6, 7, blk.shape, dtype=np.int16) if need_gt else None
        for z in range(0, a.z, 64):                     # EM-like: a few dozen bins around 120, drifting with z
            sec = blk[:min(64, a.z - z)] + np.uint8(z // 64 % 16)
            vol[z:z + 64] = sec
            if need_gt:
                gt[z:z + 64] = np.clip(sec.astype(np.int16) + noise[:len(sec)], 0, 255).astype(np.uint8)
        vol.flush()
        del vol
        vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")
        if need_gt:
            gt.flush()
            del gt
            gt = np.load(os.path.join(tmp, "gt.npy"), mmap_mode="r")
        ns = min(a.numpy_sections, a.z)

        if a.joint:
            slabs = utils.hist_chunks(utils.hist_box(shape))
            stage = [np.empty(max((b[0][1] - b[0][0]) for b in slabs) * a.y * a.x, np.uint8) for _ in range(2)]

            def device(st):
                return utils.volume_joint_histogram(vol, gt, stats=st)

            def read(st):
                for (z0, z1), _, _ in slabs:
                    for buf, v in zip(stage, (vol, gt)):
                        buf[:(z1 - z0) * a.y * a.x].reshape(z1 - z0, a.y, a.x)[...] = v[z0:z1]

            def numpy_ref(st):
                return _joint(np.asarray(vol[:ns]), np.asarray(gt[:ns]))
            runs, last = {"device": [], "read": [], "numpy": []}, {}
            for rep in range(a.reps + 1):               # repetition 0 warms buffers and the page cache
                for n, fn in (("device", device), ("read", read), ("numpy", numpy_ref)):
                    st = {}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[n] = fn(st)
                    torch.cuda.synchronize()
                    if rep:
                        runs[n].append((time.perf_counter() - t0, st))
            head = utils.volume_joint_histogram(vol, gt, size=(a.x, a.y, ns))
            m = utils.compare_from_joint(last["device"])
            res["joint"] = {"slabs": len(slabs), "device_equals_numpy_on_sections": bool(np.array_equal(head, last["numpy"])),
                            "sections_checked": ns, "occupied_bins": int(np.count_nonzero(last["device"])),
                            "n": m["n"], "rmse": round(m["rmse"], 4), "pearson": round(m["pearson"], 6),
                            "mutual_information_bits": round(m["mutual_information"], 4)}
            for n, r in runs.items():
                wall, st = min(r, key=lambda v: v[0])
                scale = a.z / ns if n == "numpy" else 1.0
                res["joint"][n] = {"s": round(wall * scale, 4), "all_runs_s": [round(v[0] * scale, 4) for v in r],
                                   "gb_per_s": round(2 * nbytes / (wall * scale) / 1e9, 2)}
                if n == "numpy":
                    res["joint"][n]["scaled_from_sections"] = ns
                if "read_s" in st:
                    res["joint"][n]["host_read_s"] = round(st["read_s"], 4)

        if a.predict:
            from transfer_em_amd.cgan import EM2EM
            from transfer_em_amd.models.generator import generator_param_shapes
            from util import scaled_params                  # tests/util.py: outputs spread over the uint8 range
            model = EM2EM(132, "comparetime", checkpoint_root=tmp)
            Pm = scaled_params(generator_param_shapes(True), 4)
            Pm["f2"] = Pm["f2"] * 20
            model.generator_g.params.load_dict(Pm)
            out = new("out")

            def run(n, st):
                if n == "none":
                    utils.predict_volume(vol, start, size, model, MS_X, MS_Y, out=out, stats=st)
                else:
                    utils.predict_volume(vol, start, size, model, MS_X, MS_Y, out=out, stats=st, compare=gt)
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
                    if n == "compare" and rep == a.reps:
                        J = st["joint_histogram"]
                        res["joint_counts_every_voxel"] = bool(J.sum() == nbytes)
                        part = utils.volume_joint_histogram(gt, out, size=(a.x, a.y, ns))
                        res["compare_equals_numpy_on_sections"] = bool(
                            np.array_equal(part, _joint(np.asarray(gt[:ns]), np.asarray(out[:ns]))) and
                            np.array_equal(J, utils.volume_joint_histogram(gt, out)))
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
