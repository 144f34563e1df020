"""Cost of the centred shift search and of the coarse-to-fine measurement built on it (utils.section_shift_sums_at,
utils.section_shifts_coarse_to_fine), modelled on volume_shifts_time.py.

--kernels 1 (default): on one default slab (64 x 1024 x 1024 bytes, the core its first 63 planes), device events, 20
  launches after 3 warm ones, min and median, per radius (--radii 4,8) in the same process:
    zshift_tiles          tem_u8_zshift_tiles, the sibling
    zshift_tiles_at_zero  tem_u8_zshift_tiles_at with a table of zeros
    zshift_tiles_at_far   tem_u8_zshift_tiles_at with a centre per tile and plane, uniform in [-40, 40]^2
  and `slab_read`: the bare read of such a slab from a page-cache-warm np.memmap into a buffer on one thread, which is
  what the kernel has to stay below to keep the pass bound by its read.
--volume 1 (default): on a 1024x1024x512 uint8 np.memmap of one multi-scale texture displaced from section to section by
  steps of up to +-20 pixels per axis plus noise, tile 128, radius 4, three cases that alternate within every repetition
  (repetition 0 warms buffers and the cache):
    coarse_to_fine  utils.section_shifts_coarse_to_fine(levels=3): three volume_rescale passes, four searches
    shift_sums      one utils.section_shift_sums at the same radius
    io              the bare chunked read of shift_sums' read slabs
  and how many pairs coarse_to_fine measured exactly.
Every figure comes with all its runs.  Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 900 python tests/tools/volume_shifts_at_time.py [--x 1024 --y 1024 --z 512] [--tile 128] [--radii 4,8]
        [--levels 3] [--reps 3] [--volume 1] [--kernels 1]
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


def _dims(box):
    return tuple(hi - lo for lo, hi in box)


def texture(y, x, rng):
    """One section with structure at 4, 16 and 64 pixels, so that every level of a pyramid has something to match."""
    a = np.zeros((y, x))
    for s in (4, 16, 64):
        coarse = rng.normal(0, 1, (-(-y // s), -(-x // s)))
        a += np.repeat(np.repeat(coarse, s, axis=0), s, axis=1)[:y, :x]
    return a


def kernel_times(y, x, tile, radii, slab_read):
    from transfer_em_amd import _lib, utils
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    D = max(2, min(64, utils.HIST_CHUNK_BYTES // (y * x)))
    gy, gx = utils.clahe_grid((D, y, x), tile)
    rng = np.random.default_rng(1)
    src = torch.from_numpy(np.clip(rng.normal(120, 9, (D, y, x)), 0, 240).astype(np.uint8)).cuda()
    far = rng.integers(-40, 41, (D, gy, gx, 2))
    tables = {"zero": torch.zeros((D, gy, gx, 2), dtype=torch.int32, device="cuda"),
              "far": torch.from_numpy(far.astype(np.int32)).cuda()}
    bounds = {"zero": (0, 0, 0), "far": (int(far[..., 0].min()), int(far[..., 0].max()), int(np.abs(far[..., 1]).max()))}
    R = 2 * max(radii) + 1
    sums = torch.zeros((D, gy, gx, R * R * 5), dtype=torch.int64, device="cuda")
    res = {"block_zyx": [D, y, x], "tile": tile, "bytes": D * y * x, "slab_read": slab_read}
    fns = {}
    for r in radii:
        fns[f"zshift_tiles_r{r}"] = lambda r=r: _lib.check(
            lib.tem_u8_zshift_tiles(src.data_ptr(), D, y, x, 0, D - 1, 0, y, 0, y, tile, tile, gy, gx, r, sums.data_ptr(),
                                    stream), "tem_u8_zshift_tiles")
        for name, table in tables.items():
            fns[f"zshift_tiles_at_{name}_r{r}"] = lambda r=r, name=name, table=table: _lib.check(
                lib.tem_u8_zshift_tiles_at(src.data_ptr(), D, y, x, 0, D - 1, 0, y, 0, y, tile, tile, gy, gx, r,
                                           table.data_ptr(), *bounds[name], sums.data_ptr(), stream),
                "tem_u8_zshift_tiles_at")
    for kname, fn in fns.items():
        t = []
        for _ in range(23):
            sums.zero_()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b) * 1e3)
        t = t[3:]
        res[kname] = {"us_min": round(min(t), 1), "us_median": round(sorted(t)[len(t) // 2], 1),
                      "gvoxel_per_s": round((D - 1) * y * x / (min(t) * 1e-6) / 1e9, 2)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--tile", type=int, default=128)
    ap.add_argument("--radii", type=str, default="4,8")
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--volume", type=int, default=1)
    ap.add_argument("--kernels", type=int, default=1)
    a = ap.parse_args()
    root = os.path.dirname(_TESTS)
    sys.path[:0] = [root, _TESTS]
    from transfer_em_amd import utils
    radii = [int(v) for v in a.radii.split(",")]
    shape = (a.z, a.y, a.x)
    nbytes = a.x * a.y * a.z
    res = {"volume_xyz": [a.x, a.y, a.z], "tile": a.tile, "radii": radii, "levels": a.levels}
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.default_rng(0)
        vol = np.lib.format.open_memmap(os.path.join(tmp, "vol.npy"), mode="w+", dtype=np.uint8, shape=shape)
        base = texture(a.y, a.x, rng)
        base = 120.0 + 25.0 * base / base.std()
        pairs = rng.integers(-20, 21, (a.z - 1, 2))
        P = np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(pairs, axis=0)])
        for z in range(a.z):                                    # section z + 1 shows at (y + dy, x + dx) what z shows at (y, x)
            sec = np.roll(base, (int(P[z, 0]), int(P[z, 1])), axis=(0, 1)) + rng.integers(-6, 7, (a.y, a.x))
            vol[z] = np.clip(np.rint(sec), 0, 255).astype(np.uint8)
        vol.flush()
        del vol
        vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")
        D = max(2, min(64, utils.HIST_CHUNK_BYTES // (a.y * a.x), a.z))
        stage = np.empty((D, a.y, a.x), np.uint8)
        t = []
        for _ in range(6):
            t0 = time.perf_counter()
            stage[...] = vol[:D]
            t.append(time.perf_counter() - t0)
        slab_read = {"ms_min": round(min(t[1:]) * 1e3, 3), "all_runs_ms": [round(v * 1e3, 3) for v in t[1:]]}
        if a.volume:
            r = radii[0]
            chunks = utils.zshift_chunks(shape, r)
            stage = np.empty(max(int(np.prod(_dims(rd))) for _, rd in chunks), np.uint8)
            kept = {}

            def io(st):
                for _, rd in chunks:
                    (z0, z1), (y0, y1), (x0, x1) = rd
                    stage[:int(np.prod(_dims(rd)))].reshape(_dims(rd))[...] = vol[z0:z1, y0:y1, x0:x1]

            def c2f(st):
                kept["c"] = utils.section_shifts_coarse_to_fine(vol, a.tile, r, a.levels, stats=st)
            fns = [("coarse_to_fine", c2f), ("shift_sums", lambda st: utils.section_shift_sums(vol, a.tile, r, stats=st)),
                   ("io", io)]
            runs = {n: [] for n, _ in fns}
            for rep in range(a.reps + 1):                       # repetition 0 warms buffers and the page cache
                for n, fn in fns:
                    st = {}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(st)
                    torch.cuda.synchronize()
                    if rep:
                        runs[n].append((time.perf_counter() - t0, st))
            rr = res["volume"] = {"radius": r, "slabs": len(chunks)}
            for n, v in runs.items():
                wall, st = min(v, key=lambda w: w[0])
                rr[n] = {"s": round(wall, 4), "all_runs_s": [round(w[0], 4) for w in v],
                         "gb_per_s_of_volume": round(nbytes / wall / 1e9, 3)}
                if "read_s" in st:
                    rr[n]["host_read_s"], rr[n]["chunks"] = round(st["read_s"], 4), st["chunks"]
            s = kept["c"].shifts
            rr["pairs"] = a.z - 1
            rr["pairs_exact"] = int((s.pairs == pairs).all(axis=1).sum())
            rr["pairs_unresolved"] = len(s.unresolved)
            rr["tiles_decided"] = round(float(s.decided.mean()), 4)
            rr["largest_center"] = int(np.abs(kept["c"].centers).max())
            # where coarse_to_fine's time goes: its level-0 legs alone, min of the repetitions
            c = kept["c"]
            parts = {"rescale_level0": lambda: utils.volume_rescale(vol, (2, 2, 1)),
                     "shift_sums_at_level0": lambda: utils.section_shift_sums_at(vol, c.centers, a.tile, r),
                     "counts_and_shifts_level0": lambda: utils.section_shifts_at(
                         c.q, utils.shift_counts_at(shape, a.tile, r, c.centers), c.centers)}
            rr["parts"] = {}
            for n, fn in parts.items():
                t = []
                for _ in range(a.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    t.append(time.perf_counter() - t0)
                rr["parts"][n] = {"s": round(min(t), 4), "all_runs_s": [round(v, 4) for v in t]}
        del vol
    if a.kernels:
        res["kernels"] = kernel_times(a.y, a.x, a.tile, radii, slab_read)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
