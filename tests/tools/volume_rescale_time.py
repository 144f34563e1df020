"""Cost of bringing a uint8 volume onto another voxel grid on the device, on a 1024x1024x512 EM-like uint8 np.memmap
written to a second memmap, for three steps ((x, y, z)): 2/1 on all axes, 3/2 on all axes, and the anisotropic
(2/1, 2/1, 1/5) of a 4 x 4 x 40 nm stack going to 8 nm isotropic.

--volume 1 (default), per step, alternating within every repetition:
    rescale   utils.volume_rescale (read thread -> pinned -> H2D -> tem_u8_rescale -> D2H -> host write)
    io        the bare chunked read of the same read slabs into a buffer plus the bare write of the same output slabs
              from a buffer, in this process on one thread: the pass's own floor
    numpy     the numpy reference (tests/rescale_ref.py) on a --numpy-box^3 corner of the source, scaled to the volume
    zoom      scipy.ndimage.zoom(order=1, mode="nearest", grid_mode=True) on the same corner, where scipy is installed
              (linear everywhere: the same rule only where an axis grows), scaled likewise
`rescale` is checked against the numpy reference on that corner.  Times, and GB/s of source plus output bytes.
--kernels 1 adds tem_u8_rescale's own time per slab from device events, min of 20 launches, on the volume's middle
slab of each step, beside (source + output bytes) / time and the slab's own read time on the host.
Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 500 python tests/tools/volume_rescale_time.py [--x 1024 --y 1024 --z 512] [--reps 3] [--volume 1]
        [--kernels 1] [--numpy-box 48]
"""
import argparse
import json
import os
import sys
import tempfile
import time
from fractions import Fraction

import numpy as np
import torch

_TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(_TESTS), _TESTS]

STEPS = {"2_1": (2, 2, 2), "3_2": (Fraction(3, 2),) * 3, "aniso_2_2_1over5": (2, 2, Fraction(1, 5))}       # (x, y, z)


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


def _dims(box):
    return tuple(hi - lo for lo, hi in box)


def kernel_time(vol, step, chunks):
    """tem_u8_rescale on the middle slab: device events, and the slab's own read on the host."""
    from transfer_em_amd import _lib
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    out, read = chunks[len(chunks) // 2]
    (z0, z1), (y0, y1), (x0, x1) = read
    host = np.empty(_dims(read), np.uint8)
    reads = []
    for _ in range(3):
        t0 = time.perf_counter()
        host[...] = vol[z0:z1, y0:y1, x0:x1]
        reads.append(time.perf_counter() - t0)
    src = torch.from_numpy(host).cuda()
    dst = torch.empty(_dims(out), dtype=torch.uint8, device="cuda")
    pq = [v for f in reversed(step) for v in (Fraction(f).numerator, Fraction(f).denominator)]
    r = _events(lambda: _lib.check(lib.tem_u8_rescale(src.data_ptr(), *_dims(read), z0, y0, x0, *vol.shape, *pq,
                                                      dst.data_ptr(), *_dims(out), *(lo for lo, _ in out), stream),
                                   "tem_u8_rescale"))
    nbytes = src.numel() + dst.numel()
    r.update(src_dims=list(_dims(read)), out_dims=list(_dims(out)), bytes=nbytes,
             gb_per_s=round(nbytes / (r["us_min"] * 1e-6) / 1e9, 1), slab_read_us=round(min(reads) * 1e6, 1),
             kernel_over_read=round(r["us_min"] * 1e-6 / min(reads), 4))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--volume", type=int, default=1)
    ap.add_argument("--kernels", type=int, default=1)
    ap.add_argument("--numpy-box", type=int, default=48)
    a = ap.parse_args()
    from transfer_em_amd import utils
    import rescale_ref as R
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    shape = (a.z, a.y, a.x)
    res = {"volume_xyz": [a.x, a.y, a.z]}
    with tempfile.TemporaryDirectory() as tmp:
        def new(name, shp):
            return np.lib.format.open_memmap(os.path.join(tmp, name + ".npy"), mode="w+", dtype=np.uint8, shape=shp)
        vol = new("vol", shape)
        rng = np.random.default_rng(0)
        blk = np.clip(rng.normal(120, 9, (min(64, a.z),) + shape[1:]), 0, 240).astype(np.uint8)
        for z in range(0, a.z, 64):                         # EM-like: a few dozen bins around 120, drifting with z
            vol[z:z + 64] = blk[:min(64, a.z - z)] + np.uint8(z // 64 % 16)
        vol.flush()
        del vol
        vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")
        nb = min(a.numpy_box, a.z, a.y, a.x)
        corner = np.asarray(vol[:nb, :nb, :nb])
        for name, step in STEPS.items():
            grid = utils.rescale_shape(shape, step)
            chunks = utils.rescale_chunks(utils.hist_box(grid), shape, step)
            nbytes = int(np.prod(shape)) + int(np.prod(grid))
            r = res[name] = {"grid_zyx": list(grid), "slabs": len(chunks), "bytes": nbytes}
            if a.volume:
                out = new("out_" + name, grid)
                stage = [np.empty(max(int(np.prod(_dims(b))) for b in side), np.uint8) for side in zip(*chunks)]
                pairs = tuple((Fraction(f).numerator, Fraction(f).denominator) for f in reversed(step))

                def io(st):
                    for o, rd in chunks:
                        (z0, z1), (y0, y1), (x0, x1) = rd
                        stage[1][:int(np.prod(_dims(rd)))].reshape(_dims(rd))[...] = vol[z0:z1, y0:y1, x0:x1]
                        (z0, z1), (y0, y1), (x0, x1) = o
                        out[z0:z1, y0:y1, x0:x1] = stage[0][:int(np.prod(_dims(o)))].reshape(_dims(o))

                fns = [("rescale", lambda st: utils.volume_rescale(vol, step, out=out, stats=st)), ("io", io),
                       ("numpy", lambda st: R.reference(corner, pairs))]
                if ndimage is not None:
                    zf = [float(1 / Fraction(f)) for f in reversed(step)]
                    fns.append(("zoom", lambda st: ndimage.zoom(corner, zf, order=1, mode="nearest", grid_mode=True)))
                runs, last = {n: [] for n, _ in fns}, {}
                for rep in range(a.reps + 1):               # repetition 0 warms buffers and the page cache
                    for n, fn in fns:
                        st = {}
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        last[n] = fn(st)
                        torch.cuda.synchronize()
                        if rep:
                            runs[n].append((time.perf_counter() - t0, st))
                utils.volume_rescale(vol, step, out=out)    # `io` wrote its buffer over the result
                want = last["numpy"]
                inner = tuple(slice(0, max(1, n - 8)) for n in want.shape)     # the corner's far face is not the volume's
                r["device_equals_numpy_on_box"] = bool(np.array_equal(np.asarray(out[inner]), want[inner]))
                r["box_checked"] = nb
                for n, rr in runs.items():
                    wall, st = min(rr, key=lambda v: v[0])
                    scale = float(np.prod(shape)) / nb ** 3 if n in ("numpy", "zoom") else 1.0
                    r[n] = {"s": round(wall * scale, 4), "all_runs_s": [round(v[0] * scale, 4) for v in rr],
                            "gb_per_s": round(nbytes / (wall * scale) / 1e9, 3)}
                    if scale != 1.0:
                        r[n]["scaled_from_box"] = nb
                    for key in ("read_s", "write_s"):
                        if key in st:
                            r[n]["host_" + key] = round(st[key], 4)
                del out
                os.remove(os.path.join(tmp, "out_" + name + ".npy"))
            if a.kernels:
                r["kernel"] = kernel_time(vol, step, chunks)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
