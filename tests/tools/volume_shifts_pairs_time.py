"""Cost of the shift sums over a list of section pairs and of the bridged measurement built on them
(utils.section_shift_sums_pairs, utils.section_shifts_bridged), modelled on volume_shifts_at_time.py.

--kernels 1 (default): on one default slab (64 x 1024 x 1024 bytes), device events, 20 launches after 3 warm ones,
  min, median and spread (max - min) of each, per radius (--radii 4,8); the cases ALTERNATE launch by launch in the same
  process, on the same block and the same centres per tile, uniform in [-40, 40]^2:
    at          tem_u8_zshift_tiles_at over the core planes [0, 63)
    pairs_lag1  tem_u8_zshift_tiles_pairs with the table (d, d + 1), d < 63: the same sums
    pairs_lag2  tem_u8_zshift_tiles_pairs with the table (d, d + 2), d < 62
  and whether pairs_lag1's sums equal at's, byte for byte.
--volume 1 (default): on a 1024x1024x512 uint8 np.memmap of one multi-scale texture displaced from section to section by
  a drift plus steps of up to +-6 pixels per axis plus noise, with a few bad sections (--bad: black), tile 128, radius 4,
  cases that alternate within every repetition (repetition 0 warms buffers and the cache):
    coarse_to_fine  utils.section_shifts_coarse_to_fine(levels=3) on the same volume
    bridged_chain   utils.section_shifts_bridged over section_pairs(Z, bad).pairs, the whole chain
    bridged_only    utils.section_shifts_bridged over the bridges alone
    io              the bare chunked read of the chain's read slabs (utils.zshift_chunks_pairs)
  and how many pairs each measured exactly.
Every figure comes with all its runs.  Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 900 python tests/tools/volume_shifts_pairs_time.py [--x 1024 --y 1024 --z 512] [--tile 128]
        [--radii 4,8] [--levels 3] [--reps 3] [--bad 100,101,300] [--volume 1] [--kernels 1]
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


def kernel_times(y, x, tile, radii):
    from transfer_em_amd import _lib, utils
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    D = max(3, min(64, utils.HIST_CHUNK_BYTES // (y * x)))
    gy, gx = utils.clahe_grid((D, y, x), tile)
    rng = np.random.default_rng(1)
    src = torch.from_numpy(np.clip(rng.normal(120, 9, (D, y, x)), 0, 240).astype(np.uint8)).cuda()
    far = rng.integers(-40, 41, (D, gy, gx, 2))
    table = torch.from_numpy(far.astype(np.int32)).cuda()
    bounds = (int(far[..., 0].min()), int(far[..., 0].max()), int(np.abs(far[..., 1]).max()))
    lag = {k: torch.tensor([(d, d + k) for d in range(D - k)], dtype=torch.int32, device="cuda") for k in (1, 2)}
    res = {"block_zyx": [D, y, x], "tile": tile, "bytes": D * y * x}
    for r in radii:
        R = 2 * r + 1
        sums = torch.zeros((D, gy, gx, R * R * 5), dtype=torch.int64, device="cuda")
        fns = {"at": lambda: _lib.check(
            lib.tem_u8_zshift_tiles_at(src.data_ptr(), D, y, x, 0, D - 1, 0, y, 0, y, tile, tile, gy, gx, r,
                                       table.data_ptr(), *bounds, sums.data_ptr(), stream), "tem_u8_zshift_tiles_at")}
        for k in (1, 2):
            fns[f"pairs_lag{k}"] = lambda k=k: _lib.check(
                lib.tem_u8_zshift_tiles_pairs(src.data_ptr(), D, y, x, 0, D - k, lag[k].data_ptr(), 0, y, 0, y, tile, tile,
                                              gy, gx, r, table.data_ptr(), *bounds, sums.data_ptr(), stream),
                "tem_u8_zshift_tiles_pairs")
        t, kept = {n: [] for n in fns}, {}
        for _ in range(23):                                      # the cases alternate launch by launch
            for n, fn in fns.items():
                sums.zero_()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                t[n].append(a.elapsed_time(b) * 1e3)
                if n != "pairs_lag2":
                    kept[n] = sums[:D - 1].clone()
        rr = res[f"r{r}"] = {"pairs_lag1_equals_at": bool(torch.equal(kept["at"], kept["pairs_lag1"]))}
        for n, v in t.items():
            v = v[3:]
            planes = D - 2 if n == "pairs_lag2" else D - 1
            rr[n] = {"us_min": round(min(v), 1), "us_median": round(sorted(v)[len(v) // 2], 1),
                     "us_spread": round(max(v) - min(v), 1), "pairs": planes,
                     "gvoxel_per_s": round(planes * y * x / (min(v) * 1e-6) / 1e9, 2)}
        del sums
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
    ap.add_argument("--bad", type=str, default="100,101,300,411")
    ap.add_argument("--volume", type=int, default=1)
    ap.add_argument("--kernels", type=int, default=1)
    a = ap.parse_args()
    root = os.path.dirname(_TESTS)
    sys.path[:0] = [root, _TESTS, os.path.join(_TESTS, "tools")]
    from transfer_em_amd import utils
    from volume_shifts_at_time import texture
    radii = [int(v) for v in a.radii.split(",")]
    shape = (a.z, a.y, a.x)
    nbytes = a.x * a.y * a.z
    bad = sorted(int(v) for v in a.bad.split(",") if v and 0 < int(v) < a.z - 1)
    res = {"volume_xyz": [a.x, a.y, a.z], "tile": a.tile, "radii": radii, "levels": a.levels, "bad": bad}
    if a.volume:
        with tempfile.TemporaryDirectory() as tmp:
            rng = np.random.default_rng(0)
            vol = np.lib.format.open_memmap(os.path.join(tmp, "vol.npy"), mode="w+", dtype=np.uint8, shape=shape)
            base = texture(a.y, a.x, rng)
            base = 120.0 + 25.0 * base / base.std()
            steps = rng.integers(-6, 7, (a.z - 1, 2)) + np.array([3, -2])
            P = np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(steps, axis=0)])
            for z in range(a.z):                                # section z + 1 shows at (y + dy, x + dx) what z shows at (y, x)
                sec = np.roll(base, (int(P[z, 0]), int(P[z, 1])), axis=(0, 1)) + rng.integers(-6, 7, (a.y, a.x))
                vol[z] = 0 if z in bad else np.clip(np.rint(sec), 0, 255).astype(np.uint8)
            vol.flush()
            del vol
            vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")
            r = radii[0]
            plan = utils.section_pairs(a.z, bad, max_lag=utils.SHIFT_MAX_LAG)
            chain = plan.pairs
            bridges = chain[chain[:, 1] - chain[:, 0] > 1]
            chunks = utils.zshift_chunks_pairs(shape, chain, r)
            stage = np.empty(max(int(np.prod(_dims(rd))) for _, _, rd in chunks), np.uint8)
            kept = {}

            def io(st):
                for _, _, rd in chunks:
                    (z0, z1), (y0, y1), (x0, x1) = rd
                    stage[:int(np.prod(_dims(rd)))].reshape(_dims(rd))[...] = vol[z0:z1, y0:y1, x0:x1]

            def c2f(st):
                kept["coarse_to_fine"] = utils.section_shifts_coarse_to_fine(vol, a.tile, r, a.levels, stats=st)

            def bridged(name, pairs):
                def run(st):
                    kept[name] = utils.section_shifts_bridged(vol, pairs, a.tile, r, a.levels, stats=st)
                return run
            fns = [("coarse_to_fine", c2f), ("bridged_chain", bridged("bridged_chain", chain)),
                   ("bridged_only", bridged("bridged_only", bridges)), ("io", io)]
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
            rr = res["volume"] = {"radius": r, "chunks_of_the_chain": len(chunks), "pairs_of_the_chain": len(chain),
                                  "bridges": bridges.tolist(), "broken": plan.broken}
            for n, v in runs.items():
                wall, st = min(v, key=lambda w: w[0])
                rr[n] = {"s": round(wall, 4), "all_runs_s": [round(w[0], 4) for w in v],
                         "gb_per_s_of_volume": round(nbytes / wall / 1e9, 3)}
                if "read_s" in st:
                    rr[n]["host_read_s"], rr[n]["chunks"] = round(st["read_s"], 4), st["chunks"]
            s = kept["coarse_to_fine"].shifts
            rr["coarse_to_fine"].update(pairs=a.z - 1, pairs_exact=int((s.pairs == steps).all(axis=1).sum()),
                                        pairs_unresolved=len(s.unresolved),
                                        suspects=utils.suspect_sections(s.unresolved, a.z))
            for n in ("bridged_chain", "bridged_only"):
                b = kept[n]
                true = np.array([P[q] - P[p] for p, q in b.pairs.tolist()]).reshape(-1, 2)
                rr[n].update(pairs=len(b.pairs), pairs_exact=int((b.shifts.pairs == true).all(axis=1).sum()),
                             pairs_unresolved=len(b.shifts.unresolved))
            del vol
    if a.kernels:
        res["kernels"] = kernel_times(a.y, a.x, a.tile, radii)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
