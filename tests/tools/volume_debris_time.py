"""Cost of finding damaged voxels below the tile on the device (utils.section_outlier_sums and utils.volume_outliers, the
two passes behind find_debris), on a 1024x1024x512 EM-like uint8 np.memmap, tile 128, window 9, the page cache warm.

--volume 1 (default): six cases that alternate within every repetition (repetition 0 warms buffers and the cache):
    outlier_sums  utils.section_outlier_sums over the default 64 MiB read slabs (outlier_chunks, radius 0)
    io_sums       the bare chunked read of the same read slabs into a buffer, in this process on one thread: the pass's
                  own floor
    outliers      utils.volume_outliers, memmap -> memmap, with outlier_thresholds of the sums
    io_mask       the bare read of its read slabs plus the bare write of its mask slabs, on one thread
    section_sums  utils.section_sums on the same volume: the sibling sums pass
    repair        utils.volume_repair on the same volume with the mask found and one bad section: the sibling write pass
--kernels 1 (default): tem_u8_zdev_tiles and tem_u8_zdev_mask (radius 1, 4, 7) alone on one default slab (64 x 1024 x 1024
  bytes, the core its planes 1...62), device events, 20 launches after 3 warm ones, min -- on EM-like, uniformly random
  and constant bytes -- beside tem_u8_zcorr_tiles and tem_u8_ssim (flat, win 7) on the same block in the same process,
  and the time one host thread takes to read the slab from a warm memmap: what each kernel is a share of.
Every figure comes with all its runs: the run-to-run spread is what a difference has to exceed.
Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 900 python tests/tools/volume_debris_time.py [--x 1024 --y 1024 --z 512] [--tile 128] [--window 9]
        [--reps 3] [--volume 1] [--kernels 1]
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


def _size(box):
    return int(np.prod(_dims(box)))


def em_like(shape, rng):
    """A few dozen grey levels around 120."""
    return np.clip(rng.normal(120, 9, shape), 0, 240).astype(np.uint8)


def _events(fn, clear):
    t = []
    for _ in range(23):
        clear()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    t = t[3:]
    return {"us_min": round(min(t), 1), "us_median": round(sorted(t)[len(t) // 2], 1)}


def kernel_times(y, x, tile, tmp):
    from transfer_em_amd import _lib, utils
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    D = max(3, min(64, utils.HIST_CHUNK_BYTES // (y * x)))
    gy, gx = utils.clahe_grid((D, y, x), tile)
    rng = np.random.default_rng(1)
    host = em_like((D, y, x), rng)
    data = {"em_like": torch.from_numpy(host).cuda(),
            "random": torch.randint(0, 256, (D, y, x), dtype=torch.uint8, device="cuda"),
            "constant": torch.full((D, y, x), 120, dtype=torch.uint8, device="cuda")}
    slab = np.lib.format.open_memmap(os.path.join(tmp, "slab.npy"), mode="w+", dtype=np.uint8, shape=(D, y, x))
    slab[...] = host
    slab.flush()
    slab = np.load(os.path.join(tmp, "slab.npy"), mmap_mode="r")
    stage, reads = np.empty((D, y, x), np.uint8), []
    for _ in range(4):
        t0 = time.perf_counter()
        stage[...] = slab
        reads.append(time.perf_counter() - t0)
    read_us = min(reads[1:]) * 1e6
    nbr = utils.section_neighbours(D)
    nbr_dev = torch.from_numpy(nbr).cuda()
    thr = np.full((gy, gx), 4096, np.int32)
    thr_dev = torch.from_numpy(thr).cuda()
    sums2 = torch.zeros((D, gy, gx, 2), dtype=torch.int64, device="cuda")
    sums4 = torch.zeros((D, gy, gx, 4), dtype=torch.int64, device="cuda")
    ssum = torch.zeros((D, 3), dtype=torch.int64, device="cuda")
    mask = torch.zeros((D, y, x), dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    res = {"block_zyx": [D, y, x], "tile": tile, "bytes": D * y * x, "slab_read_us": round(read_us, 1),
           "slab_read_all_us": [round(v * 1e6, 1) for v in reads[1:]]}

    def clear():
        sums2.zero_(), sums4.zero_(), ssum.zero_(), count.zero_()
    for name, src in data.items():
        other = src.roll(1, 0).contiguous()
        fns = {"zdev_tiles": lambda: _lib.check(lib.tem_u8_zdev_tiles(
                   src.data_ptr(), D, y, x, 0, D, 1, D - 1, 0, 0, tile, tile, gy, gx, nbr.ctypes.data, nbr_dev.data_ptr(),
                   sums2.data_ptr(), stream), "tem_u8_zdev_tiles"),
               "zcorr_tiles": lambda: _lib.check(lib.tem_u8_zcorr_tiles(
                   src.data_ptr(), D, y, x, 0, D - 1, 0, 0, tile, tile, gy, gx, sums4.data_ptr(), stream), "tem_u8_zcorr_tiles"),
               "ssim_flat_7": lambda: _lib.check(lib.tem_u8_ssim(
                   src.data_ptr(), D, y, x, 0, 0, 0, other.data_ptr(), D, y, x, 0, 0, 0, D, y, x, 7, 1, ssum.data_ptr(),
                   None, stream), "tem_u8_ssim")}
        for r in (1, 4, 7):
            fns[f"zdev_mask_r{r}"] = lambda r=r: _lib.check(lib.tem_u8_zdev_mask(
                src.data_ptr(), D, y, x, 0, D, y, 0, 1, D - 1, 0, y, 0, x, tile, tile, gy, gx, r, nbr.ctypes.data,
                nbr_dev.data_ptr(), thr.ctypes.data, thr_dev.data_ptr(), None, mask.data_ptr(), count.data_ptr(), stream),
                "tem_u8_zdev_mask")
        res[name] = {}
        for kname, fn in fns.items():
            e = _events(fn, clear)
            e["share_of_slab_read"] = round(e["us_min"] / read_us, 4)
            e["tb_per_s_of_block"] = round(D * y * x / (e["us_min"] * 1e-6) / 1e12, 3)
            res[name][kname] = e
        res[name]["flagged_r7"] = int(count.cpu()[0])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--tile", type=int, default=128)
    ap.add_argument("--window", type=int, default=9)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--volume", type=int, default=1)
    ap.add_argument("--kernels", type=int, default=1)
    a = ap.parse_args()
    root = os.path.dirname(_TESTS)
    sys.path[:0] = [root, _TESTS]
    from transfer_em_amd import utils
    shape = (a.z, a.y, a.x)
    nbytes = a.x * a.y * a.z
    res = {"volume_xyz": [a.x, a.y, a.z], "tile": a.tile, "window": a.window}
    with tempfile.TemporaryDirectory() as tmp:
        if a.volume:
            vol = np.lib.format.open_memmap(os.path.join(tmp, "vol.npy"), mode="w+", dtype=np.uint8, shape=shape)
            blk = em_like((min(64, a.z),) + shape[1:], np.random.default_rng(0))
            for z in range(0, a.z, 64):                         # EM-like: a few dozen bins around 120, drifting with z
                vol[z:z + 64] = blk[:min(64, a.z - z)] + np.uint8(z // 64 % 16)
            vol.flush()
            del vol
            vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")
            mask = np.lib.format.open_memmap(os.path.join(tmp, "mask.npy"), mode="w+", dtype=np.uint8, shape=shape)
            fixed = np.lib.format.open_memmap(os.path.join(tmp, "fixed.npy"), mode="w+", dtype=np.uint8, shape=shape)
            whole, nbr = utils.hist_box(shape), utils.section_neighbours(a.z)
            sum_chunks = utils.outlier_chunks(whole, shape, nbr, 0)
            mask_chunks = utils.outlier_chunks(whole, shape, nbr, a.window // 2)
            stage = np.empty(max(_size(rd) for _, rd in sum_chunks + mask_chunks), np.uint8)
            ones = np.ones(max(_size(c) for c, _ in mask_chunks), np.uint8)
            kept = {"thr": np.full(utils.clahe_grid(shape, a.tile), 4096, np.int32)}
            rep = utils.Repair([a.z // 2], mask, None, 8)

            def read(rd):
                (z0, z1), (y0, y1), (x0, x1) = rd
                stage[:_size(rd)].reshape(_dims(rd))[...] = vol[z0:z1, y0:y1, x0:x1]

            def io_sums(st):
                for _, rd in sum_chunks:
                    read(rd)

            def io_mask(st):
                for c, rd in mask_chunks:
                    read(rd)
                    (z0, z1), (y0, y1), (x0, x1) = c
                    mask[z0:z1, y0:y1, x0:x1] = ones[:_size(c)].reshape(_dims(c))

            def sums(st):
                kept["s"] = utils.section_outlier_sums(vol, a.tile, stats=st)
                kept["thr"] = utils.outlier_thresholds(kept["s"]).thr

            def outliers(st):                                   # last in a repetition: `mask` holds the real mask after it
                utils.volume_outliers(vol, kept["thr"], a.tile, a.window, out=mask, stats=st)
                kept["flagged"] = st["flagged"]
            fns = [("outlier_sums", sums), ("io_sums", io_sums), ("io_mask", io_mask), ("outliers", outliers),
                   ("section_sums", lambda st: utils.section_sums(vol, a.tile, stats=st)),
                   ("repair", lambda st: utils.volume_repair(vol, rep, out=fixed, stats=st))]
            runs = {n: [] for n, _ in fns}
            for r in range(a.reps + 1):                         # repetition 0 warms buffers and the page cache
                for n, fn in fns:
                    st = {}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(st)
                    torch.cuda.synchronize()
                    if r:
                        runs[n].append((time.perf_counter() - t0, st))
            rv = res["volume"] = {"sum_slabs": len(sum_chunks), "mask_slabs": len(mask_chunks),
                                  "sum_bytes_read": sum(_size(rd) for _, rd in sum_chunks),
                                  "mask_bytes_read": sum(_size(rd) for _, rd in mask_chunks), "flagged": kept["flagged"],
                                  "thr": [int(kept["thr"].min()), int(kept["thr"].max())]}
            for n, rr in runs.items():
                wall, st = min(rr, key=lambda v: v[0])
                rv[n] = {"s": round(wall, 4), "all_runs_s": [round(v[0], 4) for v in rr],
                         "gb_per_s_of_volume": round(nbytes / wall / 1e9, 3)}
                for key in ("read_s", "write_s"):
                    if key in st:
                        rv[n]["host_" + key] = round(st[key], 4)
                if "chunks" in st:
                    rv[n]["chunks"] = st["chunks"]
            del vol, mask, fixed
        if a.kernels:
            res["kernels"] = kernel_times(a.y, a.x, a.tile, tmp)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
