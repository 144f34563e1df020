"""The generator dataset over a local volume, cut on the GPU (create_dataset_from_generator(sampler, device=...)).

The host path prepares every sample in numpy (pad, scale, custom map, standardize, augment).  Here the host only draws
numbers -- crop origins from the sampler's stream, augmentation parameters from the dataset's stream, in the host path's
order -- and each batch is one tem_crop_batch launch straight from uint8 data into the standardized, augmented float32
batch, so the batches equal the host path's bit for bit.  With custom_map=debug.warp_tensor the batch is cut unscaled
first, warped per sample (tem_warp_f32, Philox hole seeds drawn from the dataset's warp stream), and cut again from the
float block.

Crops come either from a resident copy of the region all crops can touch (uploaded once) or, when that region is larger
than `resident_bytes`, from a host thread that cuts the batch's uint8 crops into double-buffered pinned staging, copied
to the device on a copy stream; events order the reuse of every buffer.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import datasets as D

WARP_RATE = 4.0 / (128 * 128)            # debug.warp_tensor's hole rate
RESIDENT_BYTES = 4 << 30


def reflect_index(i, n):
    """np.pad(..., mode="reflect") as an index map (what the kernel computes): padded index i - pad_before -> [0, n)."""
    if n == 1:
        return 0
    per = 2 * (n - 1)
    j = i % per
    return per - j if j >= n else j


def pad_pairs(padding, nd):
    """np.pad's pad_width forms (int, (before, after), per-axis pairs) as nd (before, after) pairs."""
    if padding is None:
        return [(0, 0)] * nd
    p = np.broadcast_to(np.asarray(padding, dtype=np.int64), (nd, 2))
    if (p < 0).any():
        raise ValueError(f"negative padding {padding}")
    return [(int(a), int(b)) for a, b in p]


class DeviceVolumeDataset:
    """Re-iterable batch source of a VolumeSampler on the GPU: (B, [D,] H, W, 1) float32 tensors on `device`, enqueued
    on the current stream.  Same epoch length, rank split and drop-remainder rule as datasets.GeneratorDataset."""

    def __init__(self, sampler, batch_size, epoch_size, padding=None, warp=False, meanstd=None, global_adjust=True,
                 enable_augmentation=False, seed=0, device="cuda", rank=0, world_size=1, resident_bytes=RESIDENT_BYTES):
        from .. import hip_ops as H
        self.lib = H.require_gpu()
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.sampler, self.batch_size, self.epoch_size = sampler, int(batch_size), int(epoch_size)
        self.rank, self.world_size = int(rank), int(world_size)
        self.enable_augmentation, self.warp = bool(enable_augmentation), bool(warp)
        self.rng = np.random.default_rng([seed, rank])                  # augmentation: the host Dataset's stream
        self.warp_rng = np.random.default_rng([seed, rank, 0xD0])       # warp hole seeds (a stream of its own)
        self.nd = 3 if sampler.is3d else 2
        pads = pad_pairs(padding, self.nd)
        if not sampler.is3d:
            pads = [(0, 0)] + pads
        self.n = (sampler.size,) * 3 if sampler.is3d else (1, sampler.size, sampler.size)
        self.pad_lo, self.pad_hi = [p[0] for p in pads], [p[1] for p in pads]
        self.ext = tuple(n + a + b for n, a, b in zip(self.n, self.pad_lo, self.pad_hi))
        for n, a, b in zip(self.n, self.pad_lo, self.pad_hi):
            if n == 1 and (a or b):
                raise ValueError("cannot REFLECT-pad an axis of extent 1")
        if self.enable_augmentation and len(set(self.ext[3 - self.nd:])) != 1:
            raise ValueError(f"augmentation permutes axes: the padded sample {self.ext[3 - self.nd:]} must be a cube")
        self.voxels = int(np.prod(self.ext))
        self.standardize = bool(global_adjust)
        self.meanstd = meanstd
        self._head = []                           # (origin, warp seed) of the statistics samples: head of epoch 1
        # where the crops come from
        lo, hi = sampler.hull()
        region = int(np.prod([max(h - l, 0) for l, h in zip(lo, hi)]))
        self.resident = region <= int(resident_bytes)
        if self.resident:
            vol = sampler.location[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
            self.vol = torch.from_numpy(np.array(vol, dtype=np.uint8)).to(self.device)     # one host copy
            self.lo = lo
        else:
            self.vol, self.lo = None, None
        self.last_seeds = None

    def __len__(self):
        return (self.epoch_size // self.world_size) // self.batch_size

    # ------------------------------------------------------------------ launches
    def _params(self, origins, augment):
        """The per-sample table of tem_crop_batch: origin, permutation, flips, var_adj, mean_adj (int32 bits)."""
        tab = np.zeros((len(origins), 12), np.int32)
        tab[:, :3] = origins
        tab[:, 3:6] = (0, 1, 2)
        tab[:, 9] = np.float32(1).view(np.int32)
        if augment:
            off = 3 - self.nd
            for i in range(len(origins)):
                perm, flips, mean_adj, var_adj = D._augment_params(self.nd, self.rng)
                tab[i, 3 + off:6] = [q + off for q in perm]
                tab[i, 6 + off:9] = flips
                tab[i, 9] = np.float32(var_adj).view(np.int32)
                tab[i, 10] = np.float32(mean_adj).view(np.int32)
        return torch.from_numpy(tab).pin_memory().to(self.device, non_blocking=True)

    def _crop(self, src, origins, standardize, augment, stream):
        """One tem_crop_batch launch.  src: ("u8", resident region [Z, Y, X]), ("u8_staged", [B, *crop] block) or
        ("f32", [B, *ext] block); origins relative to it."""
        B = len(origins)
        kind, t = src
        a = _crop_args(t, kind, B, self)
        if kind == "f32":
            a.n[:] = list(self.ext)
            a.pad_lo[:] = [0, 0, 0]
            a.pad_hi[:] = [0, 0, 0]
        params = self._params(origins, augment)
        out = torch.empty((B,) + self.ext, dtype=torch.float32, device=self.device)
        a.standardize = int(standardize)
        a.augment = int(augment)
        if standardize:
            a.mean, a.std = float(self.meanstd[0]), float(self.meanstd[1])
        a.params, a.dst = params.data_ptr(), out.data_ptr()
        from .. import _lib
        _lib.check(self.lib.tem_crop_batch(C.byref(a), stream), "tem_crop_batch")
        return out, params

    def _warp(self, x, seeds, stream):
        """tem_warp_f32 per sample of x [B, *ext]; returns the warped block and the hole seeds."""
        from .. import _lib
        out = torch.empty_like(x)
        holes = torch.empty(x.shape, dtype=torch.uint8, device=self.device)
        sums = torch.empty(x.shape[0], dtype=torch.float64, device=self.device)
        Dz, Hy, Wx = self.ext
        for i, s in enumerate(seeds):
            _lib.check(self.lib.tem_warp_f32(x[i].data_ptr(), Dz, Hy, Wx, WARP_RATE, int(s), out[i].data_ptr(),
                                             holes[i].data_ptr(), sums[i:].data_ptr(), stream), "tem_warp_f32")
        return out, holes

    def _batch(self, src, origins, seeds, standardize, augment, stream):
        """The float32 (B, *ext) block of these crops, not yet shaped as a batch.  Every launch is on `stream`, so the
        temporaries returned in `keep` may be freed as soon as the caller drops them."""
        if not self.warp:
            out, params = self._crop(src, origins, standardize, augment, stream)
            keep = (params,)
        else:
            pre, p0 = self._crop(src, origins, False, False, stream)
            warped, holes = self._warp(pre, seeds, stream)
            self.last_seeds = holes
            out, p1 = self._crop(("f32", warped), [(0, 0, 0)] * len(origins), standardize, augment, stream)
            keep = (pre, p0, warped, p1)
        return out, keep

    def _shape(self, out):
        B = out.shape[0]
        sp = tuple(out.shape[1:]) if self.nd == 3 else tuple(out.shape[2:])
        return out.view((B,) + sp + (1,))

    # ------------------------------------------------------------------ statistics pass
    def compute_meanstd(self, limit, replicas=True):
        """Population statistics of the first `limit` samples of the stream (datasets.get_meanstd on the device): the
        crops are cut and warped as the training samples are, summed per sample in float64 (tem_sample_sums_f32) and
        combined as get_meanstd does.  Their origins and warp seeds become the head of epoch 1."""
        from .. import _lib
        origins = self.sampler.next_origins(limit)
        seeds = [int(self.warp_rng.integers(0, 2 ** 63)) for _ in origins] if self.warp else [0] * len(origins)
        self._head = list(zip(origins, seeds))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        nblk = 32
        means, varis = [], []
        for c0 in range(0, len(origins), self.batch_size):
            org, sd = origins[c0:c0 + self.batch_size], seeds[c0:c0 + self.batch_size]
            with self._sources(iter([list(zip(org, sd))])) as srcs:
                src, rel, _ = next(srcs)
                x, keep = self._batch(src, rel, sd, False, False, stream)
            part = torch.empty((len(org), nblk, 2), dtype=torch.float64, device=self.device)
            _lib.check(self.lib.tem_sample_sums_f32(x.data_ptr(), len(org), self.voxels, nblk, part.data_ptr(), stream),
                       "tem_sample_sums_f32")
            s = part.sum(1)
            m = s[:, 0] / self.voxels
            v = s[:, 1] / self.voxels - m * m
            means.append(m.float().double())         # get_meanstd: float32 per-sample moments, summed in float64
            varis.append(v.float().double())
        mean = float(torch.cat(means).sum()) if means else 0.0
        var = float(torch.cat(varis).sum()) if varis else 0.0
        self.meanstd = D._combine_meanstd(mean, var, len(origins), replicas)
        return self.meanstd

    # ------------------------------------------------------------------ sources
    def _sources(self, batches):
        """Context manager over an iterator of batches (lists of (origin, warp seed)) yielding (src, origins relative
        to src, the batch) in order."""
        return _Sources(self, batches)

    def _plan(self):
        """The batches of one epoch, drawn as they are needed: lists of (origin, warp seed), head first; a short tail
        (a listed stream that runs out) is dropped."""
        B, need = self.batch_size, len(self) * self.batch_size
        head = self._head[:need]
        self._head = self._head[need:]
        for b0 in range(0, need, B):
            items = head[b0:b0 + B]
            fresh = self.sampler.next_origins(B - len(items))
            items += [(o, int(self.warp_rng.integers(0, 2 ** 63)) if self.warp else 0) for o in fresh]
            if len(items) < B:
                return
            yield items

    def batches(self, return_seeds=False):
        """One epoch of batches; with return_seeds, (batch, hole seeds [B, *ext] uint8) -- the warp's seeds, None
        without a warp."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        with self._sources(self._plan()) as srcs:
            for src, rel, b in srcs:
                out, _ = self._batch(src, rel, [s for _, s in b], self.standardize, self.enable_augmentation, stream)
                batch = self._shape(out)
                yield (batch, self.last_seeds if self.warp else None) if return_seeds else batch

    def __iter__(self):
        return self.batches()


class _Sources:
    """Resident: the uploaded region, origins made relative to it.  Streamed: a host thread cuts each batch's crops into
    one of two pinned buffers, an H2D copy on a copy stream moves it to one of two device buffers; the kernel reads the
    staged [B, *crop] block with origin 0.  Events order the reuse of both buffer pairs."""

    def __init__(self, ds, batches):
        self.ds, self.batches = ds, batches

    def __enter__(self):
        ds = self.ds
        if ds.resident:
            return ((("u8", ds.vol), [tuple(o - l for o, l in zip(org, ds.lo)) for org, _ in b], b)
                    for b in self.batches)
        self.pool = ThreadPoolExecutor(max_workers=1)
        return self._streamed()

    def _streamed(self):
        ds = self.ds
        shape = (ds.batch_size,) + tuple(ds.n)
        compute = torch.cuda.current_stream(ds.device)
        h2d = torch.cuda.Stream(ds.device)
        pin = [torch.empty(shape, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        dev = [torch.empty(shape, dtype=torch.uint8, device=ds.device) for _ in range(2)]
        h2d_done, used = {}, {}

        def cut(k, b):                                # host thread: crops of batch k -> pin[k % 2]
            if k >= 2:
                h2d_done.pop(k - 2).synchronize()     # the buffer's previous H2D has finished
            dst = pin[k % 2].numpy()
            for i, (o, _) in enumerate(b):
                ds.sampler.crop(o, out=dst[i] if ds.sampler.is3d else dst[i, 0])

        ahead = []                                    # the next (at most 2) batches: drawn, being cut
        for k in range(2):
            b = next(self.batches, None)
            if b is not None:
                ahead.append((b, self.pool.submit(cut, k, b)))
        k = 0
        while ahead:
            s = k % 2
            b, fut = ahead.pop(0)
            fut.result()
            if k >= 2:
                h2d.wait_event(used.pop(k - 2))        # dev[s]: batch k-2 has been cut from it
            with torch.cuda.stream(h2d):
                dev[s].copy_(pin[s], non_blocking=True)
            h2d_done[k] = h2d.record_event()
            compute.wait_event(h2d_done[k])
            yield ("u8_staged", dev[s]), [(0, 0, 0)] * len(b), b
            used[k] = compute.record_event()
            nxt = next(self.batches, None)
            if nxt is not None:
                ahead.append((nxt, self.pool.submit(cut, k + 2, nxt)))
            k += 1

    def __exit__(self, *exc):
        if not self.ds.resident:
            self.pool.shutdown(wait=True, cancel_futures=True)
            torch.cuda.current_stream(self.ds.device).synchronize()    # nothing in flight on buffers about to be freed
        return False


def _crop_args(t, kind, B, ds):
    from .. import _lib
    a = _lib.tem_crop_args()
    a.src, a.B = t.data_ptr(), B
    if kind == "f32":
        a.src_f32 = 1
        Dz, Hy, Wx = ds.ext
        a.sB, a.sZ, a.sY, a.sX = Dz * Hy * Wx, Hy * Wx, Wx, 1
        a.vol[:] = list(ds.ext)
    elif kind == "u8":                                # resident region [Z, Y, X], shared by every sample
        a.src_f32 = 0
        Z, Y, X = t.shape
        a.sB, a.sZ, a.sY, a.sX = 0, Y * X, X, 1
        a.vol[:] = [Z, Y, X]
    else:                                             # staged [B, *crop] block, origin 0
        a.src_f32 = 0
        Dz, Hy, Wx = ds.n
        a.sB, a.sZ, a.sY, a.sX = Dz * Hy * Wx, Hy * Wx, Wx, 1
        a.vol[:] = list(ds.n)
    a.n[:] = list(ds.n)
    a.pad_lo[:] = ds.pad_lo
    a.pad_hi[:] = ds.pad_hi
    return a
