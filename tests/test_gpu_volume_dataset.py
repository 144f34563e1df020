"""The generator dataset over a local volume on the GPU (datasets/device_volume.py, tem_crop_batch,
tem_sample_sums_f32) against the host path: the same batches bit for bit, the warp for the same hole seeds, the
statistics pass, the kernel's 48 axis orders, bounded memory and a short training run."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from transfer_em_amd import debug
from transfer_em_amd.datasets import datasets as D
from transfer_em_amd.datasets import generators as G
from transfer_em_amd.datasets import device_volume as V

pytestmark = pytest.mark.gpu


def _vol(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _epochs(ds, n=2):
    return [np.asarray(b.cpu().numpy() if torch.is_tensor(b) else b) for _ in range(n) for b in ds]


CASES = {   # name: (is3d, size, batch, epoch, augment, padding, explicit meanstd, resident_bytes)
    "3d132_b1_aug": (True, 132, 1, 3, True, None, False, None),
    "3d132_b2_streamed": (True, 132, 2, 4, False, None, False, 0),
    "3d13_b3_reflect": (True, 13, 3, 7, False, [[2, 1], [0, 3], [1, 1]], False, None),
    "3d13_b3_reflect_aug_streamed": (True, 13, 3, 9, True, [[2, 2]] * 3, False, 0),
    "3d21_b2_meanstd": (True, 21, 2, 6, True, None, True, None),
    "2d132_b64_aug": (False, 132, 64, 128, True, None, False, None),
    "2d30_b5_reflect_streamed": (False, 30, 5, 10, True, [[3, 3], [3, 3]], False, 0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_batches_equal_host(name):
    is3d, size, B, epoch, aug, pad, explicit, rb = CASES[name]
    vol = _vol((size + 9, size + 17, size + 12) if is3d else (7, size + 30, size + 21), seed=len(name))
    hi = (12, 17, 9) if is3d else (21, 30, 7)
    mk = lambda: (G.volume3d_ng if is3d else G.image2d_ng)(vol, ((0, 0, 0), hi), size, seed=11)
    ms = (np.float32(0.03), np.float32(0.55)) if explicit else None
    kw = dict(batch_size=B, epoch_size=epoch, padding=pad, enable_augmentation=aug, seed=5, meanstd=ms)
    host, hms = D.create_dataset_from_generator(mk(), **kw)
    dev, dms = D.create_dataset_from_generator(mk(), device="cuda", resident_bytes=rb, **kw)
    assert isinstance(dev, V.DeviceVolumeDataset) and dev.resident == (rb is None)
    if explicit:
        assert dms == ms
    else:
        assert abs(dms[0] - hms[0]) <= 2e-6 * abs(hms[0]) + 1e-7 and abs(dms[1] - hms[1]) <= 2e-6 * hms[1]
        dev.meanstd = hms                                # bit-exact batches need the same statistics
    hb, db = _epochs(host), []
    for _ in range(2):
        for b in dev:
            assert b.is_cuda and b.dtype == torch.float32
            db.append(b.cpu().numpy())
    assert len(hb) == len(db) == 2 * (epoch // B)
    for i, (h, d) in enumerate(zip(hb, db)):
        assert h.shape == d.shape, (i, h.shape, d.shape)
        assert np.array_equal(h.view(np.int32), d.view(np.int32)), (name, i)


def test_device_statistics_match_host():
    vol = _vol((150, 160, 170), 3)
    mk = lambda: G.volume3d_ng(vol, ((0, 0, 0), (30, 20, 10)), 132, seed=2)
    _, hms = D.create_dataset_from_generator(mk(), epoch_size=8, batch_size=2)
    _, dms = D.create_dataset_from_generator(mk(), epoch_size=8, batch_size=2, device="cuda")
    assert abs(dms[0] - hms[0]) <= 2e-6 * abs(hms[0]) and abs(dms[1] - hms[1]) <= 2e-6 * hms[1], (hms, dms)


def _ref_sample(t, pad, ms, rng, aug, seeds=None):
    t = np.pad(t, pad, "reflect") if pad is not None else t
    t = D.scale_tensor(t)
    if seeds is not None:
        class Fixed:
            def uniform(self, lo, hi, shape): return np.where(seeds, 0.0, 1.0)
        t = debug.warp_tensor(t, Fixed())
    t = D.standardize_population(t, ms)
    return D.augment(t, rng) if aug else t


@pytest.mark.parametrize("is3d", [True, False])
def test_warp_path_matches_host_warp_for_the_same_holes(is3d):
    size = 40 if is3d else 132
    vol = _vol((size + 5, size + 6, size + 7) if is3d else (4, size + 6, size + 7), 7)
    hi = (7, 6, 5) if is3d else (7, 6, 4)
    mk = lambda: (G.volume3d_ng if is3d else G.image2d_ng)(vol, ((0, 0, 0), hi), size, seed=1)
    pad = [[1, 1]] * (3 if is3d else 2)
    dev, ms = D.create_dataset_from_generator(mk(), custom_map=debug.warp_tensor, batch_size=3, epoch_size=6,
                                              padding=pad, enable_augmentation=True, seed=4, device="cuda")
    origins = mk().next_origins(12)
    rng = np.random.default_rng([4, 0])
    k = 0
    for _ in range(2):
        for batch, seeds in dev.batches(return_seeds=True):
            b, s = batch.cpu().numpy(), seeds.cpu().numpy().astype(bool)
            for i in range(b.shape[0]):
                z, y, x = origins[k]
                crop = vol[z:z + size, y:y + size, x:x + size] if is3d else vol[z, y:y + size, x:x + size]
                hs = s[i] if is3d else s[i, 0]
                ref = _ref_sample(crop, pad, ms, rng, True, hs)
                assert np.abs(b[i] - ref).max() < 1e-6, k
                k += 1
    assert k == 12 and 0 < s.sum()


def _launch(src, vol_shape, n, pad_lo, pad_hi, table, ext, mean, std, standardize=1, augment=1):
    from transfer_em_amd import _lib, hip_ops as H
    lib = H.require_gpu()
    a = _lib.tem_crop_args()
    Z, Y, X = vol_shape
    a.src, a.src_f32, a.B = src.data_ptr(), 0, len(table)
    a.sB, a.sZ, a.sY, a.sX = 0, Y * X, X, 1
    a.vol[:] = [Z, Y, X]
    a.n[:], a.pad_lo[:], a.pad_hi[:] = n, pad_lo, pad_hi
    a.standardize, a.augment, a.mean, a.std = standardize, augment, mean, std
    params = torch.from_numpy(np.asarray(table, np.int32)).cuda()
    out = torch.full((len(table), int(np.prod(ext))), -7.0, dtype=torch.float32, device="cuda")
    a.params, a.dst = params.data_ptr(), out.data_ptr()
    _lib.check(lib.tem_crop_batch(C.byref(a), H.current_stream()), "tem_crop_batch")
    return out.cpu().numpy()


@pytest.mark.parametrize("n,pads", [((7, 9, 11), ((1, 2), (0, 1), (2, 0))), ((33, 70, 68), ((0, 0), (3, 1), (0, 0)))])
def test_kernel_all_axis_orders_and_flips_against_numpy(n, pads):
    """6 permutations x 8 flip sets in one launch over a non-cubic crop of a non-cubic volume."""
    from itertools import permutations, product
    vol = _vol((n[0] + 5, n[1] + 4, n[2] + 6), 9)
    src = torch.from_numpy(vol).cuda()
    ext = tuple(k + a + b for k, (a, b) in zip(n, pads))
    mean, std = np.float32(0.0123), np.float32(0.577)
    rng = np.random.default_rng(0)
    table, refs = [], []
    for perm, flips in product(permutations(range(3)), product((0, 1), repeat=3)):
        o = [int(rng.integers(0, v - k + 1)) for v, k in zip(vol.shape, n)]
        var_adj, mean_adj = np.float32(rng.uniform(1, 1.05)), np.float32(rng.uniform(-.05, .05))
        table.append(o + list(perm) + list(flips) + [int(var_adj.view(np.int32)), int(mean_adj.view(np.int32)), 0])
        t = vol[o[0]:o[0] + n[0], o[1]:o[1] + n[1], o[2]:o[2] + n[2]]
        t = D.standardize_population(D.scale_tensor(np.pad(t, pads, "reflect"))[..., 0], (mean, std))
        t = np.transpose(t, perm)
        for d in range(3):
            if flips[d]:
                t = np.flip(t, d)
        refs.append((t * var_adj + mean_adj).astype(np.float32))
    out = _launch(src, vol.shape, n, [p[0] for p in pads], [p[1] for p in pads], table, ext, mean, std)
    for i, ref in enumerate(refs):
        assert np.array_equal(out[i].reshape(ref.shape).view(np.int32), np.ascontiguousarray(ref).view(np.int32)), i


def test_crop_outside_volume_reads_nan_not_memory():
    vol = _vol((10, 10, 10))
    out = _launch(torch.from_numpy(vol).cuda(), vol.shape, (4, 4, 4), [0] * 3, [0] * 3,
                  [[7, 0, 0, 0, 1, 2, 0, 0, 0, int(np.float32(1).view(np.int32)), 0, 0]], (4, 4, 4), 0.0, 1.0)
    assert np.isnan(out).all()


def test_device_path_does_no_host_float_work(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("host float work on the device path")
    monkeypatch.setattr(D, "_prepare_one", boom)
    monkeypatch.setattr(D, "scale_tensor", boom)
    monkeypatch.setattr(D, "standardize_population", boom)
    monkeypatch.setattr(D, "augment", boom)
    monkeypatch.setattr(debug, "warp_tensor_device", boom)
    vol = _vol((60, 60, 60))
    for cm in (None, debug.warp_tensor):
        for rb in (None, 0):
            ds, ms = D.create_dataset_from_generator(G.volume3d_ng(vol, ((0, 0, 0), (20, 20, 20)), 32, seed=0),
                                                     custom_map=cm, batch_size=2, epoch_size=4,
                                                     enable_augmentation=True, device="cuda", resident_bytes=rb)
            assert len([b for b in ds]) == 2 and np.isfinite(ms).all()


def test_streamed_device_memory_is_bounded():
    vol = _vol((200, 200, 200))
    mk = lambda: G.volume3d_ng(vol, ((0, 0, 0), (68, 68, 68)), 132, seed=0)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ds, _ = D.create_dataset_from_generator(mk(), batch_size=2, epoch_size=16, enable_augmentation=True,
                                            device="cuda", resident_bytes=0)
    assert not ds.resident
    for _ in range(2):
        for b in ds:
            del b
    torch.cuda.synchronize()
    batch_bytes = 2 * 132 ** 3 * 4
    assert torch.cuda.max_memory_allocated() - base <= 3 * batch_bytes, (torch.cuda.max_memory_allocated() - base)
    assert torch.cuda.memory_allocated() - base < batch_bytes // 2


def test_train_fed_by_device_datasets_matches_host_batches(tmp_path):
    from transfer_em_amd.cgan import EM2EM
    vx, vy = _vol((90, 95, 100), 1), _vol((90, 95, 100), 2)
    mk = lambda v, s: G.volume3d_ng(v, ((0, 0, 0), (20, 15, 10)), 74, seed=s)
    kw = dict(batch_size=1, epoch_size=2, enable_augmentation=True)
    dx, msx = D.create_dataset_from_generator(mk(vx, 1), device="cuda", seed=1, **kw)
    dy, msy = D.create_dataset_from_generator(mk(vy, 2), device="cuda", seed=2, **kw)
    # the host path's batches over the same crops, standardized with the device statistics
    hx, _ = D.create_dataset_from_generator(mk(vx, 1), seed=1, meanstd=msx, **kw)
    hy, _ = D.create_dataset_from_generator(mk(vy, 2), seed=2, meanstd=msy, **kw)
    runs = []
    for tag, (a, b) in (("dev", (dx, dy)), ("host", (hx, hy))):
        model = EM2EM(74, tag, checkpoint_root=str(tmp_path))
        losses = []
        step = model.train_step
        model.train_step = lambda x, y: losses.append(step(torch.as_tensor(x), torch.as_tensor(y))) or losses[-1]
        model.train(a, b, epochs=2)
        runs.append((np.stack([l.cpu().numpy() for l in losses]), [n.params.theta.cpu().numpy() for n in model._nets]))
        assert len(losses) == 4 and np.isfinite(runs[-1][0]).all()
        assert any(os.scandir(tmp_path)), "no checkpoint written"
    (la, wa), (lb, wb) = runs
    assert np.abs(la - lb).max() <= 1e-6 * max(1.0, np.abs(lb).max())
    for a, b in zip(wa, wb):
        assert np.abs(a - b).max() <= 1e-6 * max(1.0, np.abs(b).max())
