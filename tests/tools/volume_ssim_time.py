"""Cost of the windowed SSIM of two uint8 volumes on the device, on a pair of 1024x1024x512 uint8 np.memmaps (an
EM-like volume and the same volume plus noise in [-6, 6]).

--volume 1 (default): the out-of-core pass over the same memmaps, alternating within every repetition:
    win7      utils.volume_ssim, 7 x 7 x 7 windows (read thread -> pinned -> H2D -> tem_u8_ssim, one read-back)
    flat7     ... 1 x 7 x 7 windows, section by section
    win11     ... 11 x 11 x 11 windows
    map7      win7 with map_out = a third memmap (+ D2H -> host write of the map)
    read7     the bare chunked read of win7's read slabs of both files into two buffers: the pass's own floor
    numpy     the numpy reference (tests/ssim_ref.py) at win 7 on a --numpy-box^3 corner, scaled to the volume's windows
`win7` is checked against the numpy reference on that corner.  Times and GB/s of the two volumes' bytes.
--kernels 1 adds tem_u8_ssim's own time from device events over 20 launches on one 64 MiB slab pair (64 x 1024 x 1024)
for three kinds of pair -- EM-like, uniformly random, constant -- at win 7, flat 7 and win 11, with and without the map.
Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 500 python tests/tools/volume_ssim_time.py [--x 1024 --y 1024 --z 512] [--reps 3] [--volume 1]
        [--kernels 1] [--numpy-box 96]
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


def kernel_times(d=(64, 1024, 1024)):
    from transfer_em_amd import _lib
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    res = {}
    sums = torch.zeros((d[0], 3), dtype=torch.int64, device="cuda")
    smap = torch.empty(d[0] * d[1] * d[2], dtype=torch.uint8, device="cuda")
    for name in ("em_like", "random", "constant"):
        if name == "em_like":
            a = (torch.randn(d, device="cuda") * 9 + 120).clamp(0, 255).to(torch.uint8)
            b = (a.to(torch.int16) + torch.randint(-6, 7, d, device="cuda", dtype=torch.int16)).clamp(0, 255).to(torch.uint8)
        elif name == "random":
            a = torch.randint(0, 256, d, dtype=torch.uint8, device="cuda")
            b = torch.randint(0, 256, d, dtype=torch.uint8, device="cuda")
        else:
            a = torch.full(d, 120, dtype=torch.uint8, device="cuda")
            b = torch.full(d, 121, dtype=torch.uint8, device="cuda")
        for win, flat, with_map in ((7, 0, 0), (7, 0, 1), (7, 1, 0), (11, 0, 0)):
            r = _events(lambda: _lib.check(lib.tem_u8_ssim(a.data_ptr(), *d, 0, 0, 0, b.data_ptr(), *d, 0, 0, 0, *d, win, flat,
                                                           sums.data_ptr(), smap.data_ptr() if with_map else None, stream),
                                           "tem_u8_ssim"))
            windows = (d[0] - (0 if flat else win - 1)) * (d[1] - win + 1) * (d[2] - win + 1)
            r.update(windows=windows, gwin_per_s=round(windows / (r["us_min"] * 1e-6) / 1e9, 2))
            res[f"{'flat' if flat else 'win'}{win}{'_map' if with_map else ''}_{name}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--volume", type=int, default=1)
    ap.add_argument("--kernels", type=int, default=1)
    ap.add_argument("--numpy-box", type=int, default=96)
    a = ap.parse_args()
    from transfer_em_amd import utils
    import ssim_ref as R
    shape = (a.z, a.y, a.x)
    nbytes = a.x * a.y * a.z
    res = {"roi_xyz": [a.x, a.y, a.z]}
    if a.volume:
        with tempfile.TemporaryDirectory() as tmp:
            def new(name, shp):
                return np.lib.format.open_memmap(os.path.join(tmp, name + ".npy"), mode="w+", dtype=np.uint8, shape=shp)
            vol, gt = new("vol", shape), new("gt", shape)
            rng = np.random.default_rng(0)
            zb = min(64, a.z)
            blk = np.clip(rng.normal(120, 9, (zb,) + shape[1:]), 0, 240).astype(np.uint8)
            noise = rng.integers(-6, 7, blk.shape, dtype=np.int16)
            for z in range(0, a.z, 64):                     # EM-like: a few dozen bins around 120, drifting with z
                sec = blk[:min(64, a.z - z)] + np.uint8(z // 64 % 16)
                vol[z:z + 64] = sec
                gt[z:z + 64] = np.clip(sec.astype(np.int16) + noise[:len(sec)], 0, 255).astype(np.uint8)
            vol.flush(), gt.flush()
            del vol, gt
            vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")
            gt = np.load(os.path.join(tmp, "gt.npy"), mmap_mode="r")
            smap = new("map", tuple(n - 6 for n in shape))
            nb = min(a.numpy_box, a.z, a.y, a.x)
            reads = [r for _, r in utils.ssim_chunks(utils.hist_box(shape), 7, False)]
            stage = [np.empty(max(int(np.prod([hi - lo for lo, hi in r])) for r in reads), np.uint8) for _ in range(2)]

            def read7(st):
                for (z0, z1), (y0, y1), (x0, x1) in reads:
                    for buf, v in zip(stage, (vol, gt)):
                        d = (z1 - z0, y1 - y0, x1 - x0)
                        buf[:int(np.prod(d))].reshape(d)[...] = v[z0:z1, y0:y1, x0:x1]

            def numpy_ref(st):
                return R.reference(np.asarray(vol[:nb, :nb, :nb]), np.asarray(gt[:nb, :nb, :nb]), 7, False)[0]
            fns = (("win7", lambda st: utils.volume_ssim(vol, gt, stats=st)),
                   ("flat7", lambda st: utils.volume_ssim(vol, gt, flat=True, stats=st)),
                   ("win11", lambda st: utils.volume_ssim(vol, gt, win=11, stats=st)),
                   ("map7", lambda st: utils.volume_ssim(vol, gt, map_out=smap, stats=st)),
                   ("read7", read7), ("numpy", numpy_ref))
            runs, last = {n: [] for n, _ in fns}, {}
            for rep in range(a.reps + 1):                   # repetition 0 warms buffers and the page cache
                for n, fn in fns:
                    st = {}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[n] = fn(st)
                    torch.cuda.synchronize()
                    if rep:
                        runs[n].append((time.perf_counter() - t0, st))
            head = utils.volume_ssim(vol, gt, size=(nb, nb, nb))
            m = utils.ssim_from_sums(last["win7"])
            res["volume"] = {"slabs": len(reads), "read_bytes_over_volume_bytes": round(
                sum(int(np.prod([hi - lo for lo, hi in r])) for r in reads) / nbytes, 4),
                "device_equals_numpy_on_box": bool(np.array_equal(head.sums, last["numpy"])), "box_checked": nb,
                "map_sums_equal": bool(np.array_equal(last["map7"].sums, last["win7"].sums)),
                "n": m["n"], "ssim": round(m["ssim"], 6), "luminance": round(m["luminance"], 6),
                "contrast_structure": round(m["contrast_structure"], 6)}
            windows = m["n"]
            for n, r in runs.items():
                wall, st = min(r, key=lambda v: v[0])
                scale = windows / (nb - 6) ** 3 if n == "numpy" else 1.0
                res["volume"][n] = {"s": round(wall * scale, 4), "all_runs_s": [round(v[0] * scale, 4) for v in r],
                                    "gb_per_s": round(2 * nbytes / (wall * scale) / 1e9, 2)}
                if n == "numpy":
                    res["volume"][n]["scaled_from_box"] = nb
                for key in ("read_s", "write_s"):
                    if key in st:
                        res["volume"][n]["host_" + key] = round(st[key], 4)
            del smap
    if a.kernels:
        res["kernels"] = kernel_times()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
