"""Input-pipeline throughput of generator-fed 3-D training over a seeded uint8 np.memmap volume: host path
(create_dataset_from_generator, numpy) against the device path (device_volume: tem_crop_batch), samples/s at 132^3
with and without debug.warp_tensor; then 64 EM2EM(132) steps fed by two device datasets (X warped when --warp) against
64 steps on prebuilt device batches.  Prints one JSON line.  Run under a time limit on the GPU box:
    timeout -k 10 900 python tests/tools/volume_dataset_time.py [--host-samples 8] [--steps 64]
The crop kernel's time comes from a separate kernel-trace run of the same command
(rocprofv3 --kernel-trace --stats -d <dir> -- python tests/tools/volume_dataset_time.py --steps 8); at 132^3 one
sample reads 2.3 MB of uint8 and writes 9.2 MB of float32.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def _rate(ds, n_batches, sync):
    t0 = time.perf_counter()
    k = 0
    it = iter(ds)
    for _ in range(n_batches):
        next(it)
        k += 1
    sync()
    return k, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=132)
    ap.add_argument("--shape", type=int, nargs=3, default=(512, 1024, 1024))
    ap.add_argument("--host-samples", type=int, default=8)
    ap.add_argument("--device-samples", type=int, default=256)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--resident-bytes", type=int, default=None)
    a = ap.parse_args()
    from transfer_em_amd import debug
    from transfer_em_amd.cgan import EM2EM
    from transfer_em_amd.datasets import datasets as D, generators as G
    s = a.size
    res = {"size": s, "volume": list(a.shape)}
    sync = torch.cuda.synchronize
    ms = (np.float32(0.01), np.float32(0.57))
    with tempfile.TemporaryDirectory() as tmp:
        vol = np.lib.format.open_memmap(os.path.join(tmp, "vol.npy"), mode="w+", dtype=np.uint8, shape=tuple(a.shape))
        rng = np.random.default_rng(0)
        for z in range(a.shape[0]):
            vol[z] = rng.integers(0, 256, a.shape[1:], dtype=np.uint8)
        vol.flush()
        del vol
        vol = np.load(os.path.join(tmp, "vol.npy"), mmap_mode="r")
        bbox = ((0, 0, 0), (a.shape[2] - s + 1, a.shape[1] - s + 1, a.shape[0] - s + 1))
        mk = lambda seed: G.volume3d_ng(vol, bbox, s, seed=seed)
        for warp in (False, True):
            cm = debug.warp_tensor if warp else None
            tag = "warp" if warp else "plain"
            host, _ = D.create_dataset_from_generator(mk(1), custom_map=cm, batch_size=1, epoch_size=10 ** 6,
                                                      meanstd=ms, enable_augmentation=True)
            k, t = _rate(host, a.host_samples, lambda: None)
            res[f"host_{tag}_samples_per_s"] = k / t
            for mode, rb in (("resident", None), ("streamed", 0)):
                dev, _ = D.create_dataset_from_generator(mk(1), custom_map=cm, batch_size=1, epoch_size=10 ** 6,
                                                         meanstd=ms, enable_augmentation=True, device="cuda",
                                                         resident_bytes=rb)
                _rate(dev, 4, sync)                                  # warm-up
                k, t = _rate(dev, a.device_samples, sync)
                res[f"device_{tag}_{mode}_samples_per_s"] = k / t
        # train steps: fed by device datasets vs prebuilt batches
        model = EM2EM(s, "voltime", checkpoint_root=tmp)
        for warp in (False, True):
            tag = "warp" if warp else "plain"
            kw = dict(batch_size=1, epoch_size=a.steps, meanstd=ms, enable_augmentation=True, device="cuda",
                      resident_bytes=a.resident_bytes)
            dx, _ = D.create_dataset_from_generator(mk(2), custom_map=debug.warp_tensor if warp else None, **kw)
            dy, _ = D.create_dataset_from_generator(mk(3), **kw)
            pre = [(x.clone(), y.clone()) for x, y in zip(dx, dy)]
            for x, y in pre[:4]:
                model.train_step(x, y)
            sync()
            t0 = time.perf_counter()
            for x, y in pre:
                model.train_step(x, y)
            sync()
            t_pre = time.perf_counter() - t0
            t0 = time.perf_counter()
            for x, y in zip(dx, dy):
                model.train_step(x, y)
            sync()
            t_fed = time.perf_counter() - t0
            res[f"steps_{tag}"] = len(pre)
            res[f"prebuilt_{tag}_s"] = t_pre
            res[f"fed_{tag}_s"] = t_fed
            res[f"overhead_{tag}_pct"] = 100.0 * (t_fed / t_pre - 1.0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
