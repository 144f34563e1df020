"""Cost of the mip pyramid of the out-of-core prediction (utils.predict_volume(..., mips=L)): the 132 model over a
1024x1024x512 uint8 np.memmap written into np.memmap outputs (the memmap -> memmap run of predict_volume_time.py), in
three configurations that alternate within every repetition:
    none     mips=None -- called without the keyword, so `--configs none --kernels 0` also runs on a commit that has no
             `mips` yet, for a before / after figure of the default path
    device   mips=L: the pyramid pooled on the device, every level written to its own memmap
    host     mips=None, then the same pyramid pooled with numpy on the host from the finished `out` (uint16 sums of the
             strided children, slab by slab, the rule of tem_u8_pool2) into the same memmaps
The levels of the last `device` and `host` runs are compared: they must be the same bytes.  --side N runs a resident
N^3 ndarray -> ndarray instead of the memmaps.  --kernels 1 adds the pooling kernel's own times from device events over
20 launches on one default chunk's output block (27 tiles of 96^3: 288^3 bytes): the level-1 launch with the bytes it
moves (read D H W, write 1/8) as TB/s, the whole cascade of L launches, and the existing scatter of the same chunk
(reads 27 x 100^3 floats, writes 288^3 bytes) beside them.  Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 500 python tests/tools/predict_mips_time.py [--x 1024 --y 1024 --z 512 | --side 768] [--reps 3]
        [--mips 5] [--configs none,device,host] [--kernels 1]
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


def host_pool(a, out, fz=2, slab=64):
    """out = a pooled by (fz, 2, 2): the mean of the children that exist, (sum + (cnt >> 1)) >> log2(cnt).  uint16 sums
    of the strided children, `slab` sections at a time."""
    def counts(n, f):
        return np.minimum(f, n - f * np.arange(-(-n // f))).astype(np.uint16)
    Z, Y, X = a.shape
    cy, cx = counts(Y, 2), counts(X, 2)
    for z0 in range(0, Z, slab):
        blk = np.asarray(a[z0:z0 + slab])
        oz = -(-blk.shape[0] // fz)
        s = np.zeros((oz, len(cy), len(cx)), np.uint16)
        for dz in range(fz):
            for dy in range(2):
                for dx in range(2):
                    v = blk[dz::fz, dy::2, dx::2]
                    s[:v.shape[0], :v.shape[1], :v.shape[2]] += v
        cnt = counts(blk.shape[0], fz)[:, None, None] * cy[None, :, None] * cx[None, None, :]
        sh = (cnt >= 2).astype(np.uint16) + (cnt >= 4) + (cnt >= 8)
        out[z0 // fz:z0 // fz + oz] = ((s + (cnt >> 1)) >> sh).astype(np.uint8)


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


def kernel_times(L, k=3, od=96, tpad=2):
    """Device-event times (us) of the pooling launches on one chunk's output block (k^3 tiles of od^3), and of the
    scatter that fills it."""
    from transfer_em_amd import _lib
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    n, ntile, yedge = k * od, k ** 3, od + 2 * tpad
    dims = [(n >> l,) * 3 for l in range(L + 1)]
    lv = [torch.randint(0, 256, d, dtype=torch.uint8, device="cuda") for d in dims]
    y = torch.randn((ntile, yedge, yedge, yedge), dtype=torch.float32, device="cuda")
    idx = torch.tensor([[a * od, b * od, c * od] for a in range(k) for b in range(k) for c in range(k)],
                       dtype=torch.int32).cuda()

    def pool(l):
        _lib.check(lib.tem_u8_pool2(lv[l].data_ptr(), *dims[l], *dims[l], 2, lv[l + 1].data_ptr(), stream), "tem_u8_pool2")

    def cascade():
        for l in range(L):
            pool(l)

    def scatter():
        _lib.check(lib.tem_f32_tiles_unstd_to_u8(y.data_ptr(), ntile, yedge, tpad, idx.data_ptr(), lv[0].data_ptr(), n, n,
                                                 n, *MS_Y, stream), "scatter")
    res = {"block": [n] * 3, "levels": L}
    for name, fn, nbytes in (("pool_level1", lambda: pool(0), n ** 3 + (n // 2) ** 3), ("pool_cascade", cascade, None),
                             ("scatter", scatter, 4 * ntile * od ** 3 + n ** 3)):
        r = _events(fn)
        if nbytes:
            r["bytes"], r["tb_per_s"] = nbytes, round(nbytes / (r["us_min"] * 1e-6) / 1e12, 3)
        res[name] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--side", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mips", type=int, default=5)
    ap.add_argument("--configs", default="none,device,host")
    ap.add_argument("--kernels", type=int, default=1)
    a = ap.parse_args()
    from transfer_em_amd import utils
    from transfer_em_amd.cgan import EM2EM
    from transfer_em_amd.models.generator import generator_param_shapes
    if a.side:
        a.x = a.y = a.z = a.side
    shape, start, size, L = (a.z, a.y, a.x), (0, 0, 0), (a.x, a.y, a.z), a.mips
    names = a.configs.split(",")
    with tempfile.TemporaryDirectory() as tmp:
        model = EM2EM(132, "mipstime", checkpoint_root=tmp)
        from util import scaled_params                     # tests/util.py: outputs spread over the uint8 range, so that
        Pm = scaled_params(generator_param_shapes(True), 4)    # the comparison of the two pyramids is one of real means
        Pm["f2"] = Pm["f2"] * 20
        model.generator_g.params.load_dict(Pm)
        shapes = [shape]
        for _ in range(L):
            shapes.append(tuple(-(-n // 2) for n in shapes[-1]))

        def new(name, shp):
            if a.side:
                return np.zeros(shp, np.uint8)
            return np.lib.format.open_memmap(os.path.join(tmp, name + ".npy"), mode="w+", dtype=np.uint8, shape=shp)
        vol = new("vol", shape)
        rng = np.random.default_rng(0)
        for z in range(0, a.z, 64):
            vol[z:z + 64] = rng.integers(0, 256, (min(64, a.z - z),) + shape[1:], dtype=np.uint8)
        if not a.side:
            vol.flush()
            del vol
            vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")
        outs = {n: [new(f"{n}{l}", s) for l, s in enumerate(shapes)] for n in names if n != "none"}
        outs["none"] = [outs["host"][0] if "host" in outs else new("none0", shape)]

        def run(n, st):
            if n == "none":
                utils.predict_volume(vol, start, size, model, MS_X, MS_Y, out=outs[n][0], stats=st)
            elif n == "device":
                utils.predict_volume(vol, start, size, model, MS_X, MS_Y, out=outs[n], stats=st, mips=L)
            else:
                utils.predict_volume(vol, start, size, model, MS_X, MS_Y, out=outs[n][0], stats=st)
                t0 = time.perf_counter()
                for l in range(L):
                    host_pool(outs[n][l], outs[n][l + 1])
                st["host_pool_s"] = time.perf_counter() - t0
        res = {"roi_xyz": list(size), "mips": L, "resident": bool(a.side), "configs": {}}
        runs = {n: [] for n in names}
        for rep in range(a.reps + 1):                                        # repetition 0 warms plans, buffers, page cache
            for n in names:
                st = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(n, st)
                torch.cuda.synchronize()
                if rep:
                    runs[n].append((time.perf_counter() - t0, st))
        for n in names:
            wall, st = min(runs[n], key=lambda r: r[0])
            res["configs"][n] = {"end_to_end_s": round(wall, 4), "all_runs_s": [round(r[0], 4) for r in runs[n]],
                                 "gvox_per_s": round(a.x * a.y * a.z / wall / 1e9, 3),
                                 "host_read_s": round(st["read_s"], 4), "host_write_s": round(st["write_s"], 4),
                                 "chunks": st["chunks"]}
            if "host_pool_s" in st:
                res["configs"][n]["host_pool_s"] = round(st["host_pool_s"], 4)
        if "device" in outs and "host" in outs:
            res["device_equals_host"] = all(np.array_equal(d, h) for d, h in zip(outs["device"], outs["host"]))
            res["level0_std"] = round(float(np.asarray(outs["device"][0][:64]).std()), 2)
        if a.kernels:
            model.generator_g.clear_plans()
            res["kernels"] = kernel_times(L)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
