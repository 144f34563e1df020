"""Cost of warping every section of a uint8 volume through "affine map + displacement field" on the device, on a
1024x1024x512 EM-like uint8 np.memmap written to a second memmap, lattice spacing 128.  The maps of the pass are
volume_warp_time.py's (every section turned by up to +-0.5 degrees and moved by a fraction of a pixel), the fields
smooth waves of up to a pixel.

--volume 1 (default), alternating within every repetition:
    field     utils.volume_warp_field (read thread -> pinned -> H2D -> tem_u8_warp_field -> D2H -> host write)
    warp      utils.volume_warp on the same maps, the same volume and the same output
    io        the bare chunked read of the same read slabs into a buffer plus the bare write of the same output slabs
              from a buffer, in this process on one thread: the pass's own floor
`field` is checked against the numpy reference (tests/field_ref.py) on a --numpy-box^3 corner.
--kernels 1 adds the kernels' own times on one default slab (64 sections) from device events, min of 20 launches:
tem_u8_warp_field and its baseline without LDS, tem_u8_warp_field_direct, for a zero field, a field of a pixel and
field and matrix at their limits; tem_u8_warp_affine on the same block and maps; the slab's own read time on the host.
Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 500 python tests/tools/volume_field_time.py [--x 1024 --y 1024 --z 512] [--spacing 128] [--reps 3]
        [--volume 1] [--kernels 1] [--numpy-box 48]
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

from volume_warp_time import _dims, _events  # noqa: E402  (the sibling tool, in this directory)


def _wave(shape, spacing, amp, phase):
    """float64 [ny, nx, 2]: u_y = amp sin(pi x / (X - 1) + phase), u_x = -amp sin(pi y / (Y - 1) + phase) at the nodes."""
    import field_ref as FR
    nodes = FR.nodes(shape, spacing)
    Y, X = shape[-2:]
    return np.stack([amp * np.sin(np.pi * nodes[..., 1] / (X - 1) + phase), -amp * np.sin(np.pi * nodes[..., 0] / (Y - 1) + phase)],
                    axis=-1)


def kernel_times(vol, spacing):
    """The three kernels on the volume's middle slab of up to 64 whole sections; the slab's own read on the host."""
    import field_ref as FR
    import warp_ref as WR
    from transfer_em_amd import _lib, utils
    from transfer_em_amd import hip_ops as H
    lib, stream = H.require_gpu(), H.current_stream()
    Z, Y, X = vol.shape
    D = min(64, Z)
    z0 = (Z - D) // 2
    host = np.empty((D, Y, X), np.uint8)
    reads = []
    for _ in range(3):
        t0 = time.perf_counter()
        host[...] = vol[z0:z0 + D]
        reads.append(time.perf_counter() - t0)
    src = torch.from_numpy(host).cuda()
    dst = torch.empty_like(src)
    c = np.array([(Y - 1) / 2, (X - 1) / 2])
    L = np.array([[1.125, -0.125], [0.125, 0.875]])
    ky, kx = FR.log2s(spacing)
    ny, nx = utils.field_grid((Y, X), spacing)
    near = WR._rigid(np.deg2rad(0.5), np.array([0.37, -1.21]), c)
    cases = {"zero_field": (near, np.zeros((ny, nx, 2), np.int32)),
             "one_px_field": (near, utils.quantize_field(_wave((Y, X), spacing, 1.0, 0.0)[None], spacing)[0]),
             "limits": (np.concatenate([L, (c - L @ c)[:, None]], axis=1), FR.walk((Y, X), spacing, 11))}
    nbytes = 2 * src.numel()
    res = {"block": [D, Y, X], "bytes": nbytes, "spacing": spacing, "slab_read_us": round(min(reads) * 1e6, 1)}
    for name, (m, u) in cases.items():
        mh = utils.quantize_maps(np.tile(m, (D, 1, 1)))
        uh = np.ascontiguousarray(np.tile(u, (D, 1, 1, 1)))
        md, ud = torch.from_numpy(mh).cuda(), torch.from_numpy(uh).cuda()
        want = FR.warp_section(host[0], mh[0], uh[0], spacing)
        res[name] = {}
        for fn in ("tem_u8_warp_field", "tem_u8_warp_field_direct"):
            call = getattr(lib, fn)
            r = _events(lambda: _lib.check(call(src.data_ptr(), D, Y, X, 0, Y, dst.data_ptr(), D, Y, X, 0, 0, mh.ctypes.data,
                                                md.data_ptr(), uh.ctypes.data, ud.data_ptr(), ny, nx, ky, kx, 0, 0, stream), fn))
            r.update(gb_per_s=round(nbytes / (r["us_min"] * 1e-6) / 1e9, 1),
                     kernel_over_read=round(r["us_min"] * 1e-6 / min(reads), 4),
                     equals_numpy_on_section_0=bool(np.array_equal(dst[0].cpu().numpy(), want)))
            res[name][fn] = r
        r = _events(lambda: _lib.check(lib.tem_u8_warp_affine(src.data_ptr(), D, Y, X, 0, Y, dst.data_ptr(), D, Y, X, 0, 0,
                                                              mh.ctypes.data, md.data_ptr(), 0, 0, stream), "tem_u8_warp_affine"))
        res[name]["tem_u8_warp_affine_same_maps"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=1024)
    ap.add_argument("--y", type=int, default=1024)
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--spacing", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--volume", type=int, default=1)
    ap.add_argument("--kernels", type=int, default=1)
    ap.add_argument("--numpy-box", type=int, default=48)
    a = ap.parse_args()
    from transfer_em_amd import utils
    import field_ref as FR
    import warp_ref as WR
    shape = (a.z, a.y, a.x)
    res = {"volume_xyz": [a.x, a.y, a.z], "spacing": a.spacing}
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
        centre = np.array([(a.y - 1) / 2, (a.x - 1) / 2])
        M = utils.quantize_maps(np.stack([WR._rigid(t, s, centre) for t, s in
                                          zip(rng.uniform(-1, 1, a.z) * np.deg2rad(0.5), rng.uniform(-1, 1, (a.z, 2)))]))
        U = utils.quantize_field(np.stack([_wave(shape, a.spacing, amp, ph) for amp, ph in
                                           zip(rng.uniform(-1, 1, a.z), rng.uniform(0, np.pi, a.z))]), a.spacing)
        chunks = utils.field_chunks(utils.hist_box(shape), shape, M, U, a.spacing)
        nbytes = 2 * int(np.prod(shape))
        r = res["pass"] = {"slabs": len(chunks), "bytes": nbytes, "warp_slabs": len(utils.warp_chunks(utils.hist_box(shape), shape, M)),
                           "read_bytes": sum(int(np.prod(_dims(rd))) for _, rd in chunks)}
        if a.volume:
            out = new("out", shape)
            stage = [np.empty(max(int(np.prod(_dims(b))) for b in side), np.uint8) for side in zip(*chunks)]
            nb = min(a.numpy_box, a.z, a.y, a.x)

            def io(st):
                for o, rd in chunks:
                    (z0, z1), (y0, y1), (x0, x1) = rd
                    stage[1][:int(np.prod(_dims(rd)))].reshape(_dims(rd))[...] = vol[z0:z1, y0:y1, x0:x1]
                    (z0, z1), (y0, y1), (x0, x1) = o
                    out[z0:z1, y0:y1, x0:x1] = stage[0][:int(np.prod(_dims(o)))].reshape(_dims(o))

            fns = [("field", lambda st: utils.volume_warp_field(vol, M, U, a.spacing, out=out, stats=st)),
                   ("warp", lambda st: utils.volume_warp(vol, M, out=out, stats=st)), ("io", io)]
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
            utils.volume_warp_field(vol, M, U, a.spacing, out=out)      # `io` wrote its buffer over the result
            want = np.stack([FR.warp_section(vol[z], M[z], U[z], a.spacing, ((0, nb), (0, nb))) for z in range(nb)])
            r["device_equals_numpy_on_box"] = bool(np.array_equal(np.asarray(out[:nb, :nb, :nb]), want))
            r["box_checked"] = nb
            for n, rr in runs.items():
                wall, st = min(rr, key=lambda v: v[0])
                r[n] = {"s": round(wall, 4), "all_runs_s": [round(v[0], 4) for v in rr], "gb_per_s": round(nbytes / wall / 1e9, 3)}
                for key in ("read_s", "write_s"):
                    if key in st:
                        r[n]["host_" + key] = round(st[key], 4)
            del out
        if a.kernels:
            res["kernel"] = kernel_times(vol, a.spacing)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
