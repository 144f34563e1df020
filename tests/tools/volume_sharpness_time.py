"""Cost of measuring the in-plane sharpness on the device (utils.section_plane_sums), on 1024x1024 EM-like uint8
sections, tile 128, the page cache warm.

--kernels 1 (default), device events, 20 launches after 3 warm ones, min, on one 64 x 1024 x 1024 block of EM-like,
random and constant bytes:
    tem_u8_zplane_lags at nlag 1, 4 and 8 (the core: every plane and row; the block holds the section's last rows)
      alternating, launch by launch in one process, with tem_u8_zcorr_lags at the same nlag on the same block (the
      core: all but the last nlag planes), with zplane's launch plan (workgroups, rows per run, rows loaded per row
      counted)
    the block's read from a warm np.memmap into a buffer, on one thread: what the pass has to hide the kernel behind.
      THE CONDITION: the kernel's time is below the block's read at every nlag and on every kind of bytes
      ("kernel_below_read").
--volume 1 (default): cases that alternate within every repetition (repetition 0 warms buffers and the cache):
    plane_sums_L   utils.section_plane_sums at max_lag L = 1, 4, 8 over the default slabs (plane_lag_chunks)
    io             the bare chunked read of the same slabs into a buffer, on one thread: the pass's own floor
    section_sums   utils.section_sums, the sibling pass
Every figure comes with all its runs: the run-to-run spread is what a difference has to exceed.
Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 600 python tests/tools/volume_sharpness_time.py [--x 1024 --y 1024 --z 512] [--tile 128] [--reps 3]
        [--volume 1] [--kernels 1]
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


def _stats(t):
    return {"us_min": round(min(t), 1), "us_median": round(sorted(t)[len(t) // 2], 1)}


def _timed_pair(fns, clear):
    """The launches of `fns` alternating, 23 rounds, the first 3 dropped: one list of microseconds per function."""
    t = [[] for _ in fns]
    for _ in range(23):
        for i, fn in enumerate(fns):
            clear()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t[i].append(a.elapsed_time(b) * 1e3)
    return [_stats(v[3:]) for v in t]


def _plane_plan(D, y, x, tile, nlag):
    """csrc/zplane_u8.hip's plan of a whole block on the grid: (workgroups, rows per run, lanes busy of 64)."""
    rows, width = min(tile, y), min(tile, x)
    SC = (min(width, 1024) + 15) // 16
    NR = 64 // SC
    R = min(16, -(-rows // NR))
    units = -(-y // tile) * -(-x // tile) * -(-rows // (NR * R)) * -(-width // 1024)
    return units * -(-D // 4), R, NR * SC


def kernel_times(y, x, tile, tmp):
    from transfer_em_amd import _lib, utils
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    D = max(10, min(64, utils.HIST_CHUNK_BYTES // (y * x)))
    gy, gx = utils.clahe_grid((D, y, x), tile)
    rng = np.random.default_rng(1)
    blocks = {"em_like": em_like((D, y, x), rng), "random": rng.integers(0, 256, (D, y, x), dtype=np.uint8),
              "constant": np.full((D, y, x), 120, np.uint8)}
    res = {"block_zyx": [D, y, x], "tile": tile, "bytes": D * y * x}
    # the block's read from a warm memmap, as the pass reads it: one thread, into a buffer
    m = np.lib.format.open_memmap(os.path.join(tmp, "block.npy"), mode="w+", dtype=np.uint8, shape=(D, y, x))
    m[...] = blocks["em_like"]
    m.flush()
    del m
    m = np.load(os.path.join(tmp, "block.npy"), mmap_mode="r")
    stage = np.empty((D, y, x), np.uint8)
    reads = []
    for _ in range(8):
        t0 = time.perf_counter()
        stage[...] = m[0:D, 0:y, 0:x]
        reads.append((time.perf_counter() - t0) * 1e6)
    del m
    res["read"] = _stats(reads[2:])
    res["read"]["all_us"] = [round(v, 1) for v in reads]
    sums = torch.zeros((D, gy, gx, 19), dtype=torch.int64, device="cuda")
    below = True
    for kind, block in blocks.items():
        src = torch.from_numpy(block).cuda()
        res[kind] = {}
        for nlag in (1, 4, 8):
            plane, lags = _timed_pair(
                [lambda: _lib.check(lib.tem_u8_zplane_lags(src.data_ptr(), D, y, x, 0, D, 0, y, 0, y, tile, tile, gy, gx,
                                                           nlag, sums.data_ptr(), stream), "tem_u8_zplane_lags"),
                 lambda: _lib.check(lib.tem_u8_zcorr_lags(src.data_ptr(), D, y, x, 0, D - nlag, 0, 0, tile, tile, gy, gx,
                                                          nlag, sums.data_ptr(), stream), "tem_u8_zcorr_lags")],
                sums.zero_)
            wgs, R, lanes = _plane_plan(D, y, x, tile, nlag)
            plane.update(tb_per_s=round(D * y * x / (plane["us_min"] * 1e-6) / 1e12, 3), workgroups=wgs, rows_per_run=R,
                         lanes_busy=lanes, loaded_per_counted=round((R + nlag) / R, 2),
                         of_the_read=round(plane["us_min"] / res["read"]["us_min"], 4),
                         of_zcorr_lags=round(plane["us_min"] / lags["us_min"], 3))
            below = below and plane["us_min"] < res["read"]["us_min"]
            res[kind][f"zplane_lags_{nlag}"], res[kind][f"zcorr_lags_{nlag}"] = plane, lags
        del src
    res["kernel_below_read"] = bool(below)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--tile", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--volume", type=int, default=1)
    ap.add_argument("--kernels", type=int, default=1)
    a = ap.parse_args()
    root = os.path.dirname(_TESTS)
    sys.path[:0] = [root, _TESTS]
    from transfer_em_amd import utils
    shape = (a.z, a.y, a.x)
    nbytes = a.x * a.y * a.z
    res = {"volume_xyz": [a.x, a.y, a.z], "tile": a.tile}
    with tempfile.TemporaryDirectory() as tmp:
        if a.volume:
            vol = np.lib.format.open_memmap(os.path.join(tmp, "vol.npy"), mode="w+", dtype=np.uint8, shape=shape)
            blk = em_like((min(64, a.z),) + shape[1:], np.random.default_rng(0))
            for z in range(0, a.z, 64):                         # EM-like: a few dozen bins around 120, drifting with z
                vol[z:z + 64] = blk[:min(64, a.z - z)] + np.uint8(z // 64 % 16)
            vol.flush()
            del vol
            vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")
            chunks = utils.plane_lag_chunks(shape, 8)
            stage = np.empty(utils.HIST_CHUNK_BYTES, np.uint8)

            def read(box):
                (z0, z1), (y0, y1), (x0, x1) = box
                stage[:_size(box)].reshape(_dims(box))[...] = vol[z0:z1, y0:y1, x0:x1]

            fns = [(f"plane_sums_{L}", lambda st, L=L: utils.section_plane_sums(vol, a.tile, L, stats=st)) for L in (1, 4, 8)]
            fns += [("io", lambda st: [read(rd) for _, rd in chunks]),
                    ("section_sums", lambda st: utils.section_sums(vol, a.tile, stats=st))]
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
            r = res["volume"] = {"slabs": len(chunks), "bytes_read": sum(_size(rd) for _, rd in chunks)}
            for n, rr in runs.items():
                wall, st = min(rr, key=lambda v: v[0])
                r[n] = {"s": round(wall, 4), "all_runs_s": [round(v[0], 4) for v in rr],
                        "gb_per_s_of_volume": round(nbytes / wall / 1e9, 3)}
                if "read_s" in st:
                    r[n]["host_read_s"], r[n]["chunks"] = round(st["read_s"], 4), st["chunks"]
            del vol
        if a.kernels:
            res["kernels"] = kernel_times(a.y, a.x, a.tile, tmp)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
