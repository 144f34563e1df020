"""Cost of measuring the sections' spacing along z and of resampling to an even grid on the device
(utils.section_lag_sums and utils.volume_resample_z), on a 1024x1024xZ EM-like uint8 np.memmap, tile 128, the page
cache warm.

--kernels 1 (default), device events, 20 launches after 3 warm ones, min, on one 64 x 1024 x 1024 block:
    tem_u8_zcorr_lags at nlag 1, 4 and 8 (the core: all but the last nlag planes) beside tem_u8_zcorr_tiles (the core:
      all but the last plane) on the same block, with the launch plan (workgroups, planes per run, planes loaded per
      plane counted)
    tem_u8_resample_z of 64 output planes from the same block (a table of uneven spacings around 1; blended and
      nearest) beside tem_u8_lut on the same block: both read and write every byte of a 64 MiB block about once
--volume 1 (default): cases that alternate within every repetition (repetition 0 warms buffers and the cache):
    lag_sums_L     utils.section_lag_sums at max_lag L = 1, 4, 8 over the default read slabs (zlag_chunks)
    io_L           the bare chunked read of the same read slabs into a buffer, on one thread: the pass's own floor
    resample_z     utils.volume_resample_z into a memmap of the same shape
    io_rw          the bare chunked read of its read slabs plus the write of its output slabs
Every figure comes with all its runs: the run-to-run spread is what a difference has to exceed.
Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 600 python tests/tools/volume_zspace_time.py [--x 1024 --y 1024 --z 256] [--tile 128] [--reps 3]
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


def _positions(Z, rng):
    """Uneven spacings in [0.6, 1.5], scaled to run from 0 to Z - 1."""
    p = np.concatenate([[0.0], np.cumsum(rng.uniform(0.6, 1.5, Z - 1))])
    return p * ((Z - 1) / p[-1])


def _timed(fn, clear):
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


def _lag_plan(D, y, x, tile, ncore, nlag):
    """csrc/zlags_u8.hip's plan of a block on the grid: (workgroups, planes per run)."""
    items = 1024 if nlag <= 4 else 512
    S = (min(tile, x) + 15) // 16
    units = -(-y // tile) * -(-x // tile) * -(-min(tile, y) // (items // S))
    zr = ncore * units // 1024
    if zr < 2 * nlag:
        zr = max(zr, min(ncore * units // 512, 2 * nlag))
    zr = min(24 + 8 * nlag, max(1, zr))
    return units * -(-ncore // zr), zr


def kernel_times(y, x, tile):
    from transfer_em_amd import _lib, utils
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    D = max(10, min(64, utils.HIST_CHUNK_BYTES // (y * x)))
    gy, gx = utils.clahe_grid((D, y, x), tile)
    rng = np.random.default_rng(1)
    src = torch.from_numpy(em_like((D, y, x), rng)).cuda()
    res = {"block_zyx": [D, y, x], "tile": tile, "bytes": D * y * x, "lags": {}, "resample": {}}
    sums = torch.zeros((D, gy, gx, 11), dtype=torch.int64, device="cuda")
    r = _timed(lambda: _lib.check(lib.tem_u8_zcorr_tiles(src.data_ptr(), D, y, x, 0, D - 1, 0, 0, tile, tile, gy, gx,
                                                         sums.data_ptr(), stream), "tem_u8_zcorr_tiles"), sums.zero_)
    r["tb_per_s"] = round(D * y * x / (r["us_min"] * 1e-6) / 1e12, 3)
    res["lags"]["zcorr_tiles"] = r
    for nlag in (1, 4, 8):
        r = _timed(lambda: _lib.check(lib.tem_u8_zcorr_lags(src.data_ptr(), D, y, x, 0, D - nlag, 0, 0, tile, tile, gy,
                                                            gx, nlag, sums.data_ptr(), stream), "tem_u8_zcorr_lags"),
                   sums.zero_)
        wgs, zr = _lag_plan(D, y, x, tile, D - nlag, nlag)
        r.update(tb_per_s=round(D * y * x / (r["us_min"] * 1e-6) / 1e12, 3), workgroups=wgs, planes_per_run=zr,
                 loaded_per_counted=round((zr + nlag) / zr, 2))
        res["lags"][f"zcorr_lags_{nlag}"] = r
    del sums
    table = np.ascontiguousarray(utils.resample_z_taps(utils.quantize_positions(_positions(D, rng))))
    tdev = torch.from_numpy(table).cuda()
    dst = torch.empty((table.shape[0], y, x), dtype=torch.uint8, device="cuda")
    moved = (D + table.shape[0]) * y * x
    for name, nearest in (("blend", 0), ("nearest", 1)):
        r = _timed(lambda: _lib.check(lib.tem_u8_resample_z(src.data_ptr(), D, y, x, 0, D, dst.data_ptr(), table.shape[0],
                                                            0, table.shape[0], table.ctypes.data, tdev.data_ptr(),
                                                            nearest, stream), "tem_u8_resample_z"), lambda: None)
        r["tb_per_s_read_plus_written"] = round(moved / (r["us_min"] * 1e-6) / 1e12, 3)
        res["resample"][name] = r
    lut = torch.arange(255, -1, -1, dtype=torch.uint8, device="cuda")
    buf = src.clone()
    r = _timed(lambda: _lib.check(lib.tem_u8_lut(buf.data_ptr(), D, y, x, lut.data_ptr(), 0, 0, stream), "tem_u8_lut"),
               lambda: None)
    r["tb_per_s_read_plus_written"] = round(2 * D * y * x / (r["us_min"] * 1e-6) / 1e12, 3)
    res["resample"]["lut"] = r
    res["resample"]["output_planes"] = int(table.shape[0])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=256)
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
    if a.volume:
        with tempfile.TemporaryDirectory() as tmp:
            vol = np.lib.format.open_memmap(os.path.join(tmp, "vol.npy"), mode="w+", dtype=np.uint8, shape=shape)
            blk = em_like((min(64, a.z),) + shape[1:], np.random.default_rng(0))
            for z in range(0, a.z, 64):                         # EM-like: a few dozen bins around 120, drifting with z
                vol[z:z + 64] = blk[:min(64, a.z - z)] + np.uint8(z // 64 % 16)
            vol.flush()
            del vol
            vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")
            out = np.lib.format.open_memmap(os.path.join(tmp, "out.npy"), mode="w+", dtype=np.uint8, shape=shape)
            P = _positions(a.z, np.random.default_rng(2))
            table = utils.resample_z_taps(utils.quantize_positions(P))
            rchunks = utils.resample_z_chunks(((0, a.z), (0, a.y), (0, a.x)), shape, table)
            lchunks = {L: utils.zlag_chunks(shape, L) for L in (1, 4, 8)}
            stage = np.empty(utils.HIST_CHUNK_BYTES, np.uint8)

            def read(box):
                (z0, z1), (y0, y1), (x0, x1) = box
                stage[:_size(box)].reshape(_dims(box))[...] = vol[z0:z1, y0:y1, x0:x1]

            def io_rw(st):
                for (oz, oy, ox), rd in rchunks:
                    read(rd)
                    out[oz[0]:oz[1], oy[0]:oy[1], ox[0]:ox[1]] = stage[:_size((oz, oy, ox))].reshape(_dims((oz, oy, ox)))

            fns = []
            for L in (1, 4, 8):
                fns.append((f"lag_sums_{L}", lambda st, L=L: utils.section_lag_sums(vol, a.tile, L, stats=st)))
                fns.append((f"io_{L}", lambda st, L=L: [read(rd) for _, rd in lchunks[L]]))
            fns += [("resample_z", lambda st: utils.volume_resample_z(vol, P, out=out, stats=st)), ("io_rw", io_rw)]
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
            r = res["volume"] = {"lag_slabs": {L: len(c) for L, c in lchunks.items()},
                                 "lag_bytes_read": {L: sum(_size(rd) for _, rd in c) for L, c in lchunks.items()},
                                 "resample_slabs": len(rchunks),
                                 "resample_bytes_read": sum(_size(rd) for _, rd in rchunks)}
            for n, rr in runs.items():
                wall, st = min(rr, key=lambda v: v[0])
                r[n] = {"s": round(wall, 4), "all_runs_s": [round(v[0], 4) for v in rr],
                        "gb_per_s_of_volume": round(nbytes / wall / 1e9, 3)}
                if "read_s" in st:
                    r[n]["host_read_s"], r[n]["chunks"] = round(st["read_s"], 4), st["chunks"]
                if "write_s" in st:
                    r[n]["host_write_s"] = round(st["write_s"], 4)
            del vol, out
    if a.kernels:
        res["kernels"] = kernel_times(a.y, a.x, a.tile)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
