"""Cost of measuring how far every section sits from the next one on the device (utils.section_shift_sums, the pass
behind section_shifts), on a 1024x1024x512 EM-like uint8 np.memmap, tile 128, the page cache warm.

--volume 1 (default): per radius (--radii 4,8) three cases that alternate within every repetition (repetition 0 warms
  buffers and the cache):
    shift_sums    utils.section_shift_sums over the default 64 MiB read slabs (zshift_chunks: 63 core sections + 1)
    io            the bare chunked read of the same read slabs into a buffer, in this process on one thread: the
                  pass's own floor
    section_sums  utils.section_sums on the same volume: the sibling pass (one offset instead of (2 r + 1)^2)
  and once per radius: shift_counts + section_shifts + shift_positions on the sums (host only), and the numpy
  reference (tests/zshift_ref.py: volume_sums) on a corner of 2 sections x 256 x 256, scaled to the volume by voxels.
--kernels 1 (default): tem_u8_zshift_tiles alone on one default slab (64 x 1024 x 1024 bytes, the core its first 63
  planes), device events, 20 launches after 3 warm ones, min -- on EM-like, uniformly random and constant bytes --
  beside tem_u8_zcorr_tiles on the same block in the same process.
Every figure comes with all its runs: the run-to-run spread is what a difference has to exceed.
Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 600 python tests/tools/volume_shifts_time.py [--x 1024 --y 1024 --z 512] [--tile 128] [--radii 4,8]
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


def em_like(shape, rng):
    """A few dozen grey levels around 120."""
    return np.clip(rng.normal(120, 9, shape), 0, 240).astype(np.uint8)


def kernel_times(y, x, tile, radii):
    from transfer_em_amd import _lib, utils
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    D = max(2, min(64, utils.HIST_CHUNK_BYTES // (y * x)))
    gy, gx = utils.clahe_grid((D, y, x), tile)
    rng = np.random.default_rng(1)
    data = {"em_like": torch.from_numpy(em_like((D, y, x), rng)).cuda(),
            "random": torch.randint(0, 256, (D, y, x), dtype=torch.uint8, device="cuda"),
            "constant": torch.full((D, y, x), 120, dtype=torch.uint8, device="cuda")}
    R = 2 * max(radii) + 1
    sums = torch.zeros((D, gy, gx, R * R * 5), dtype=torch.int64, device="cuda")
    res = {"block_zyx": [D, y, x], "tile": tile, "bytes": D * y * x}
    for name, src in data.items():
        fns = {"zcorr_tiles": lambda: _lib.check(lib.tem_u8_zcorr_tiles(src.data_ptr(), D, y, x, 0, D - 1, 0, 0, tile,
                                                                         tile, gy, gx, sums.data_ptr(), stream),
                                                 "tem_u8_zcorr_tiles")}
        for r in radii:
            fns[f"zshift_tiles_r{r}"] = lambda r=r: _lib.check(
                lib.tem_u8_zshift_tiles(src.data_ptr(), D, y, x, 0, D - 1, 0, y, 0, y, tile, tile, gy, gx, r,
                                        sums.data_ptr(), stream), "tem_u8_zshift_tiles")
        res[name] = {}
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
            res[name][kname] = {"us_min": round(min(t), 1), "us_median": round(sorted(t)[len(t) // 2], 1),
                                "gvoxel_per_s": round((D - 1) * y * x / (min(t) * 1e-6) / 1e9, 2)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--tile", type=int, default=128)
    ap.add_argument("--radii", type=str, default="4,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--volume", type=int, default=1)
    ap.add_argument("--kernels", type=int, default=1)
    a = ap.parse_args()
    root = os.path.dirname(_TESTS)
    sys.path[:0] = [root, _TESTS]
    from transfer_em_amd import utils
    import zshift_ref
    radii = [int(v) for v in a.radii.split(",")]
    shape = (a.z, a.y, a.x)
    nbytes = a.x * a.y * a.z
    res = {"volume_xyz": [a.x, a.y, a.z], "tile": a.tile, "radii": radii}
    if a.volume:
        with tempfile.TemporaryDirectory() as tmp:
            vol = np.lib.format.open_memmap(os.path.join(tmp, "vol.npy"), mode="w+", dtype=np.uint8, shape=shape)
            blk = em_like((min(64, a.z),) + shape[1:], np.random.default_rng(0))
            for z in range(0, a.z, 64):                         # EM-like: a few dozen bins around 120, drifting with z
                vol[z:z + 64] = blk[:min(64, a.z - z)] + np.uint8(z // 64 % 16)
            vol.flush()
            del vol
            vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")
            res["volume"] = {}
            for r in radii:
                chunks = utils.zshift_chunks(shape, r)
                stage = np.empty(max(int(np.prod(_dims(rd))) for _, rd in chunks), np.uint8)
                kept = {}

                def io(st):
                    for _, rd in chunks:
                        (z0, z1), (y0, y1), (x0, x1) = rd
                        stage[:int(np.prod(_dims(rd)))].reshape(_dims(rd))[...] = vol[z0:z1, y0:y1, x0:x1]

                def sums(st):
                    kept["q"] = utils.section_shift_sums(vol, a.tile, r, stats=st)
                fns = [("shift_sums", sums), ("io", io),
                       ("section_sums", lambda st: utils.section_sums(vol, a.tile, stats=st))]
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
                rr = res["volume"][f"r{r}"] = {"slabs": len(chunks), "sums_bytes": int(kept["q"].nbytes),
                                               "bytes_read": sum(int(np.prod(_dims(rd))) for _, rd in chunks)}
                for n, v in runs.items():
                    wall, st = min(v, key=lambda w: w[0])
                    rr[n] = {"s": round(wall, 4), "all_runs_s": [round(w[0], 4) for w in v],
                             "gb_per_s_of_volume": round(nbytes / wall / 1e9, 3)}
                    if "read_s" in st:
                        rr[n]["host_read_s"], rr[n]["chunks"] = round(st["read_s"], 4), st["chunks"]
                t0 = time.perf_counter()
                s = utils.section_shifts(kept["q"], utils.shift_counts(shape, a.tile, r))
                utils.shift_positions(s.pairs)
                rr["counts_shifts_positions_s"] = round(time.perf_counter() - t0, 4)
                rr["pairs_unresolved"], rr["tiles_decided"] = len(s.unresolved), int(s.decided.sum())
                corner = np.ascontiguousarray(vol[:2, :min(256, a.y), :min(256, a.x)])
                t0 = time.perf_counter()
                ref = zshift_ref.volume_sums(corner, (a.tile, a.tile), r)
                t = time.perf_counter() - t0
                gy, gx = ref.shape[1:3]
                assert np.array_equal(ref[0, :gy - 1, :gx - 1, r, r], kept["q"][0, :gy - 1, :gx - 1, r, r])   # no offset: no face
                rr["numpy_reference"] = {"corner_zyx": list(corner.shape), "s": round(t, 4),
                                         "scaled_to_volume_s": round(t * (a.z - 1) * a.y * a.x / (corner[0].size), 1)}
                del kept
            del vol
    if a.kernels:
        res["kernels"] = kernel_times(a.y, a.x, a.tile, radii)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
