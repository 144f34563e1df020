"""Cost of the 16-bit ingest, on a 1024x1024x512 EM-like uint16 np.memmap (page cache warm).

--passes 1 (default): the out-of-core passes over the same memmap, alternating within every repetition:
    hist           utils.volume_histogram16 (read thread -> pinned -> H2D -> tem_u16_hist, one read-back)
    hist_sections  the same with per_section=True (512 KiB of counters per section)
    read           the bare chunked read of the same slabs into one buffer: the floor of both
    to_u8          utils.volume_to_u8, memmap -> memmap, one table (with the host thread's read_s / write_s)
    read_write     the bare read of the same slabs plus the bare write of as many uint8 slabs: the floor of to_u8
    bincount       np.bincount of a corner of --corner sections on the host, scaled to the volume
`hist` must equal `hist_sections` summed, and the corner's rows np.bincount; `to_u8` is checked on the corner.
--kernels 1 (default): the kernels alone on one 64 x 1024 x 1024 slab from device events (min of 20 launches) on
EM-like, uniformly random and constant data: tem_u16_hist (plain and per_section) next to tem_u8_hist2 on the same voxel
count, tem_u16_lut_u8 and tem_u16_lut_u8_direct next to tem_u8_lut on the same voxel count.
Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 500 python tests/tools/volume_u16_time.py [--x 1024 --y 1024 --z 512] [--reps 3] [--corner 16]
        [--passes 1] [--kernels 1]
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


def _bits16(v):
    """The int32 values 0...65535 as the 16-bit patterns of a uint16 block (held in an int16 tensor)."""
    return ((v ^ 0x8000) - 0x8000).to(torch.int16)


def _em_like(shape, dev):
    """A bell of a few thousand occupied bins around 30,000, as a 16-bit detector gives (int32 values)."""
    return (torch.randn(shape, device=dev) * 2500 + 30000).clamp(0, 65535).to(torch.int32)


def kernel_times(D=64, H=1024, W=1024):
    from transfer_em_amd import _lib
    from transfer_em_amd import hip_ops as Hh
    lib, stream = Hh.require_gpu(), Hh.current_stream()
    n = D * H * W
    res = {"slab": [D, H, W]}
    counts = torch.zeros((D, 65536), dtype=torch.int64, device="cuda")
    joint = torch.zeros(65536, dtype=torch.int64, device="cuda")
    table16 = (torch.arange(65536, device="cuda") >> 8).to(torch.uint8)
    table8 = torch.arange(255, -1, -1, dtype=torch.uint8, device="cuda")
    dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    for kind in ("em_like", "random", "constant"):
        if kind == "em_like":
            v = _em_like((D, H, W), "cuda")
        elif kind == "random":
            v = torch.randint(0, 65536, (D, H, W), dtype=torch.int32, device="cuda")
        else:
            v = torch.full((D, H, W), 30000, dtype=torch.int32, device="cuda")
        src = _bits16(v)
        a8, b8 = (v >> 8).to(torch.uint8), (v & 255).to(torch.uint8)    # the same voxel count as bytes, for the 8-bit kernels
        del v
        sp, ap, bp = src.data_ptr(), a8.data_ptr(), b8.data_ptr()
        cases = {
            "u16_hist": (lambda: lib.tem_u16_hist(sp, D, H, W, 0, D, 0, H, 0, W, counts.data_ptr(), 0, 0, stream), 2 * n),
            "u16_hist_per_section": (lambda: lib.tem_u16_hist(sp, D, H, W, 0, D, 0, H, 0, W, counts.data_ptr(), 1, 0,
                                                              stream), 2 * n),
            "u8_hist2": (lambda: lib.tem_u8_hist2(ap, D, H, W, 0, 0, 0, bp, D, H, W, 0, 0, 0, D, H, W, joint.data_ptr(),
                                                  stream), 2 * n),
            "u16_lut_u8": (lambda: lib.tem_u16_lut_u8(sp, D, H, W, dst.data_ptr(), table16.data_ptr(), 0, 0, 0, stream),
                           3 * n),
            "u16_lut_u8_direct": (lambda: lib.tem_u16_lut_u8_direct(sp, D, H, W, dst.data_ptr(), table16.data_ptr(), 0, 0,
                                                                    0, stream), 3 * n),
            "u8_lut": (lambda: lib.tem_u8_lut(ap, D, H, W, table8.data_ptr(), 0, 0, stream), 2 * n),
        }
        res[kind] = {}
        for name, (call, nbytes) in cases.items():
            r = _events(lambda: _lib.check(call(), name))
            r["bytes"], r["gb_per_s"] = nbytes, round(nbytes / (r["us_min"] * 1e-6) / 1e9, 1)
            res[kind][name] = r
        del src, a8, b8
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--corner", type=int, default=16)
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--kernels", type=int, default=1)
    a = ap.parse_args()
    from transfer_em_amd import utils
    shape = (a.z, a.y, a.x)
    nbytes = 2 * a.x * a.y * a.z
    res = {"shape_zyx": list(shape), "bytes": nbytes}
    if a.passes:
        with tempfile.TemporaryDirectory() as tmp:
            vol = np.lib.format.open_memmap(os.path.join(tmp, "vol.npy"), mode="w+", dtype=np.uint16, shape=shape)
            rng = np.random.default_rng(0)
            nb = min(32, a.z)
            blk = np.clip(rng.normal(30000, 2500, (nb,) + shape[1:]), 0, 60000).astype(np.uint16)
            for z in range(0, a.z, nb):                     # EM-like, the level drifting with z
                vol[z:z + nb] = blk[:min(nb, a.z - z)] + np.uint16(37 * (z // nb % 16))
            vol.flush()
            del vol, blk
            vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")
            out = np.lib.format.open_memmap(os.path.join(tmp, "out.npy"), mode="w+", dtype=np.uint8, shape=shape)
            slabs = utils.hist_chunks(utils.hist_box(shape), itemsize=2)
            kz = max(b[0][1] - b[0][0] for b in slabs)
            stage, stage8 = np.empty((kz, a.y, a.x), np.uint16), np.zeros((kz, a.y, a.x), np.uint8)
            corner = min(a.corner, a.z)
            table = utils.window_lut16(22000, 38000)

            def hist(st):
                return utils.volume_histogram16(vol, stats=st)

            def hist_sections(st):
                return utils.volume_histogram16(vol, per_section=True, stats=st)

            def read(st):
                for (z0, z1), _, _ in slabs:
                    stage[:z1 - z0] = vol[z0:z1]

            def to_u8(st):
                return utils.volume_to_u8(vol, table, out=out, stats=st)

            def read_write(st):
                for (z0, z1), _, _ in slabs:
                    stage[:z1 - z0] = vol[z0:z1]
                    out[z0:z1] = stage8[:z1 - z0]

            def bincount(st):
                return np.stack([np.bincount(np.asarray(vol[z]).reshape(-1), minlength=65536) for z in range(corner)])
            fns = (("hist", hist), ("hist_sections", hist_sections), ("read", read), ("to_u8", to_u8),
                   ("read_write", read_write), ("bincount", bincount))
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
                    if n == "to_u8" and rep == a.reps:      # before read_write overwrites `out`
                        res["to_u8_equals_numpy_on_the_corner"] = bool(np.array_equal(out[:corner], table[vol[:corner]]))
            res["slabs"] = len(slabs)
            res["hist_equals_sections_summed"] = bool(np.array_equal(last["hist"], last["hist_sections"].sum(axis=0)))
            res["sections_equal_bincount_on_the_corner"] = bool(np.array_equal(last["hist_sections"][:corner],
                                                                               last["bincount"]))
            res["occupied_bins"] = int(np.count_nonzero(last["hist"]))
            res["passes"] = {}
            for n, r in runs.items():
                wall, st = min(r, key=lambda v: v[0])
                scale = a.z / corner if n == "bincount" else 1.0
                e = {"s": round(wall * scale, 4), "all_runs_s": [round(v[0] * scale, 4) for v in r],
                     "gb_per_s": round(nbytes / (wall * scale) / 1e9, 2)}
                for k in ("read_s", "write_s"):
                    if k in st:
                        e["host_" + k] = round(st[k], 4)
                if n == "bincount":
                    e["scaled_from_sections"] = corner
                res["passes"][n] = e
    if a.kernels:
        res["kernels"] = kernel_times()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
