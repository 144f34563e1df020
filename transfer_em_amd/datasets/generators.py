"""Random-ROI sample streams over a local uint8 volume (mirror of reference transfer_em/datasets/generators.py).

The reference draws crop origins in a bounding box and fetches each crop from a network store (DVID, neuroglancer
precomputed through tensorstore or a cloud-run service).  Here the volume is local: `location` is the uint8 array itself,
indexed [z, y, x] -- an np.ndarray, an np.memmap, or any object with `.shape` and numpy basic slicing (h5py, zarr), the
convention `utils.predict_ng_cube` uses.  Only the crop boxes are ever sliced out of it.

A sampler is an iterator of host uint8 crops, so `datasets.create_dataset_from_generator(sampler, ...)` works as with any
generator.  Given `device=`, that function instead draws the same origins and cuts the crops on the GPU
(`datasets.device_volume`).
"""
import numpy as np

from ..utils import _local_volume


def _box(b):
    (x0, y0, z0), (x1, y1, z1) = b
    return (int(x0), int(y0), int(z0)), (int(x1), int(y1), int(z1))


class VolumeSampler:
    """Stream of crops of a uint8 volume `location` [z, y, x] (see volume3d_ng / image2d_ng).

    Iterating yields contiguous uint8 crops: [size, size, size] cubes (is3d) or [size, size] sections.  `next_origins(n)`
    draws the next n crop origins (z, y, x) from the same stream, in the order iteration would use them, and `crop(o)`
    cuts the crop at an origin; `hull()` bounds every crop the stream can yield."""

    def __init__(self, location, bbox, size=132, seed=None, array=None, sample_array=False, sample_class=False,
                 is3d=True, rank=None):
        self.location = _local_volume(location)
        self.bbox, self.size, self.seed, self.array = bbox, int(size), seed, array
        self.sample_array, self.sample_class, self.is3d = bool(sample_array), bool(sample_class), bool(is3d)
        if len(self.location.shape) != 3:
            raise ValueError(f"location must be a [z, y, x] volume, got shape {tuple(self.location.shape)}")
        if self.size < 1:
            raise ValueError(f"size must be positive, got {size}")
        self._listed = array is not None and not self.sample_array
        if self._listed:
            self._starts = [tuple(int(v) for v in s) for s in array]
            for s in self._starts:
                self._check_box(s, s)
        else:
            if array is not None:
                classes = array if self.sample_class else [array]
                self._classes = [[_box(b) for b in c] for c in classes]
                if not self._classes or any(len(c) == 0 for c in self._classes):
                    raise ValueError("sample_array needs a non-empty list of boxes (per class with sample_class)")
            else:
                if bbox is None:
                    raise ValueError("bbox is required unless `array` lists the starts")
                self._classes = [[_box(bbox)]]
            for c in self._classes:
                for lo, hi in c:
                    if any(h <= l for l, h in zip(lo, hi)):
                        raise ValueError(f"empty box {(lo, hi)}: starts are drawn in [lo, hi) per axis")
                    self._check_box(lo, tuple(h - 1 for h in hi))
        # seed None: fresh entropy, drawn once so that the per-rank streams still share it
        self._key = int(seed) if seed is not None else np.random.SeedSequence().entropy
        self.rank = rank
        self.rng = np.random.default_rng(self._key if rank is None else [self._key, int(rank)])
        self._pos = 0

    def _check_box(self, lo, hi_start):
        """Every start in [lo, hi_start] (x, y, z) gives a crop inside the volume."""
        Z, Y, X = (int(v) for v in self.location.shape)
        ext = (self.size, self.size, self.size if self.is3d else 1)       # crop extent per (x, y, z)
        for a, (l, h, e, n) in enumerate(zip(lo, hi_start, ext, (X, Y, Z))):
            if l < 0 or h + e > n:
                raise ValueError(f"crops from starts {lo}..{hi_start} (x, y, z) with size {self.size} leave the volume "
                                 f"of shape {(Z, Y, X)} (z, y, x) along {'xyz'[a]}")

    def for_rank(self, rank):
        """The sampler of data-parallel rank `rank`: same volume and boxes, stream default_rng([seed, rank])."""
        s = VolumeSampler(self.location, self.bbox, self.size, self._key, self.array, self.sample_array,
                          self.sample_class, self.is3d, rank=rank)
        s.seed = self.seed
        return s

    @property
    def crop_shape(self):
        return (self.size,) * (3 if self.is3d else 2)

    def _draw(self):
        rng = self.rng
        if self._listed:
            if self._pos >= len(self._starts):
                return None
            x, y, z = self._starts[self._pos]
            self._pos += 1
            return z, y, x
        boxes = self._classes[int(rng.integers(0, len(self._classes)))] if self.sample_class else self._classes[0]
        lo, hi = boxes[int(rng.integers(0, len(boxes)))] if self.array is not None else boxes[0]
        x, y, z = (int(rng.integers(l, h)) for l, h in zip(lo, hi))       # tf.random.uniform order: x, y, z
        return z, y, x

    def next_origins(self, n):
        """The next n crop origins (z, y, x); fewer when a listed stream runs out."""
        out = []
        for _ in range(int(n)):
            o = self._draw()
            if o is None:
                break
            out.append(o)
        return out

    def crop(self, origin, out=None):
        z, y, x = origin
        s = self.size
        box = self.location[z:z + s, y:y + s, x:x + s] if self.is3d else self.location[z, y:y + s, x:x + s]
        if out is None:
            return np.ascontiguousarray(box, dtype=np.uint8)
        out[...] = box
        return out

    def hull(self):
        """((z0, y0, x0), (z1, y1, x1)): the box of the volume every crop of this stream lies in."""
        if self._listed:
            if not self._starts:
                return (0, 0, 0), (0, 0, 0)
            lo = np.min(self._starts, axis=0)
            hi = np.max(self._starts, axis=0) + 1
        else:
            boxes = [b for c in self._classes for b in c]
            lo = np.min([b[0] for b in boxes], axis=0)
            hi = np.max([b[1] for b in boxes], axis=0)
        ext = (self.size, self.size, self.size if self.is3d else 1)
        (x0, y0, z0), (x1, y1, z1) = lo, [h - 1 + e for h, e in zip(hi, ext)]
        return (int(z0), int(y0), int(x0)), (int(z1), int(y1), int(x1))

    def __iter__(self):
        return self

    def __next__(self):
        o = self._draw()
        if o is None:
            raise StopIteration
        return self.crop(o)


def volume3d_ng(location, bbox, size=132, seed=None, array=None, cloudrun=None, sample_array=False, sample_class=False):
    """Infinite stream of random 3-D crops (reference generators.py:59-118) of a local uint8 volume.

    Args:
        location: the uint8 volume, indexed [z, y, x] (array, memmap, h5py / zarr dataset).  A path raises
            NotImplementedError: network stores are out of scope.
        bbox: ((x, y, z), (x2, y2, z2)); each start is uniform over [lo, hi) per axis, as tf.random.uniform.
        size: crop edge.
        seed: seed of np.random.default_rng (the same seed gives the same crops; TensorFlow's stream is not reproduced).
        array: without sample_array, a list of (x, y, z) starts yielded in order, then the stream ends; with
            sample_array, a list of bboxes (one is drawn, then a start inside it); with sample_class as well, a list of
            classes, each a list of bboxes (a class is drawn, then a bbox of it, then a start).
        cloudrun: accepted and ignored.
    Returns a VolumeSampler.  Each sample is location[z:z+size, y:y+size, x:x+size] as a contiguous uint8 [z, y, x]
    cube; the reference yields tensorstore's (x, y, z) layout instead.  A crop that could leave the volume raises
    ValueError here."""
    return VolumeSampler(location, bbox, size, seed, array, sample_array, sample_class, is3d=True)


def image2d_ng(location, bbox, size=132, seed=None, array=None, cloudrun=None, sample_array=False, sample_class=False):
    """volume3d_ng for 2-D models (no reference counterpart): a sample is location[z, y:y+size, x:x+size], a [size, size]
    crop of one section of the [z, y, x] stack.  bbox and starts are still (x, y, z); the z start is the section."""
    return VolumeSampler(location, bbox, size, seed, array, sample_array, sample_class, is3d=False)


def volume3d_dvid(dvid_server, uuid, instance, bbox, size=132, seed=None, array=None):
    """Reference generators.py:12-57 fetches crops from a DVID server; network stores are out of scope."""
    raise NotImplementedError("DVID volumes are not supported: load the volume locally (np.memmap, h5py, zarr) and use "
                              "generators.volume3d_ng(array, bbox, ...) over it")
