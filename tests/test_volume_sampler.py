"""Host checks of the local-volume sample streams (datasets/generators.py, reference generators.py:59-118) and of the
index maps the device dataset mirrors: no GPU needed."""
import numpy as np
import pytest

from transfer_em_amd.datasets import datasets as D
from transfer_em_amd.datasets import generators as G
from transfer_em_amd.datasets import device_volume as V


def _vol(shape=(40, 50, 60), seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def test_reference_import_line():
    from transfer_em.datasets import datasets, generators      # the reference notebooks' first line
    assert generators.volume3d_ng is G.volume3d_ng and datasets is D


def test_bbox_xyz_maps_to_zyx_slices_and_starts_in_range():
    vol = _vol()
    bbox = ((3, 5, 7), (20, 30, 25))                             # (x, y, z)
    s = G.volume3d_ng(vol, bbox, size=8, seed=1)
    origins = s.next_origins(400)
    o = np.array(origins)                                        # (z, y, x)
    for a, (lo, hi) in enumerate(zip(bbox[0][::-1], bbox[1][::-1])):
        assert o[:, a].min() == lo and o[:, a].max() == hi - 1  # uniform over [lo, hi)
    s2 = G.volume3d_ng(vol, bbox, size=8, seed=1)
    for (z, y, x) in origins[:5]:
        c = next(s2)
        assert c.dtype == np.uint8 and c.flags.c_contiguous and c.shape == (8, 8, 8)
        assert np.array_equal(c, vol[z:z + 8, y:y + 8, x:x + 8])


def test_same_seed_same_crops_other_seed_differs():
    vol = _vol()
    a = [next(G.volume3d_ng(vol, ((0, 0, 0), (30, 30, 20)), 10, seed=4)) for _ in range(1)]
    s1, s2, s3 = (G.volume3d_ng(vol, ((0, 0, 0), (30, 30, 20)), 10, seed=k) for k in (4, 4, 5))
    c1, c2, c3 = [next(s1) for _ in range(4)], [next(s2) for _ in range(4)], [next(s3) for _ in range(4)]
    assert all(np.array_equal(x, y) for x, y in zip(c1, c2)) and np.array_equal(a[0], c1[0])
    assert not all(np.array_equal(x, y) for x, y in zip(c1, c3))


def test_array_mode_is_finite_and_in_order():
    vol = _vol()
    starts = [(1, 2, 3), (10, 0, 5), (0, 0, 0)]                  # (x, y, z)
    s = G.volume3d_ng(vol, None, size=6, array=starts)
    out = list(s)
    assert len(out) == 3
    for (x, y, z), c in zip(starts, out):
        assert np.array_equal(c, vol[z:z + 6, y:y + 6, x:x + 6])
    assert s.next_origins(2) == []


def test_sample_array_and_sample_class():
    vol = _vol()
    boxes = [((0, 0, 0), (2, 2, 2)), ((30, 30, 20), (32, 32, 22))]
    o = np.array(G.volume3d_ng(vol, None, 8, seed=3, array=boxes, sample_array=True).next_origins(300))
    first = (o < 2).all(1)
    second = (o[:, 0] >= 20) & (o[:, 0] < 22) & (o[:, 1] >= 30) & (o[:, 1] < 32) & (o[:, 2] >= 30) & (o[:, 2] < 32)
    assert (first | second).all() and first.any() and second.any()
    classes = [[boxes[0]], [boxes[1], ((10, 10, 10), (11, 11, 11))]]
    o = np.array(G.volume3d_ng(vol, None, 8, seed=3, array=classes, sample_array=True, sample_class=True)
                 .next_origins(400))
    c0 = (o < 2).all(1)
    c2 = (o == 10).all(1)
    assert c0.any() and c2.any() and (c0.mean() > 0.35) and (c2.mean() < 0.4)   # class drawn first, then a box


def test_out_of_range_raises_and_path_not_implemented():
    vol = _vol((20, 20, 20))
    with pytest.raises(ValueError):
        G.volume3d_ng(vol, ((0, 0, 0), (12, 5, 5)), size=10)        # x start 11 + 10 > 20
    G.volume3d_ng(vol, ((0, 0, 0), (11, 11, 11)), size=10)          # the largest start 10 fits exactly
    with pytest.raises(ValueError):
        G.volume3d_ng(vol, None, size=10, array=[(0, 0, 0), (0, 11, 0)])
    with pytest.raises(ValueError):
        G.volume3d_ng(vol, None, size=10, array=[((0, 0, 0), (2, 2, 2)), ((5, 5, 5), (12, 6, 6))], sample_array=True)
    with pytest.raises(ValueError):
        G.image2d_ng(vol, ((0, 0, 0), (5, 5, 21)), size=10)          # section 20 does not exist
    with pytest.raises(NotImplementedError):
        G.volume3d_ng("gs://bucket/volume", ((0, 0, 0), (1, 1, 1)))
    with pytest.raises(NotImplementedError):
        G.volume3d_dvid("http://server", "uuid", "grayscale", ((0, 0, 0), (1, 1, 1)))


def test_image2d_sections():
    vol = _vol((5, 40, 30))
    s = G.image2d_ng(vol, ((0, 0, 0), (10, 20, 5)), size=16, seed=2)
    origins = s.next_origins(50)
    assert {o[0] for o in origins} <= set(range(5)) and len({o[0] for o in origins}) > 1
    s2 = G.image2d_ng(vol, ((0, 0, 0), (10, 20, 5)), size=16, seed=2)
    for z, y, x in origins[:4]:
        c = next(s2)
        assert c.shape == (16, 16) and np.array_equal(c, vol[z, y:y + 16, x:x + 16])
    assert s.hull() == ((0, 0, 0), (5, 35, 25))


class _Sliced:
    """h5py-like: only .shape and basic slicing; records every box asked for."""

    def __init__(self, a):
        self.a, self.shape, self.boxes = a, a.shape, []

    def __getitem__(self, key):
        self.boxes.append(tuple((k.start, k.stop) if isinstance(k, slice) else k for k in key))
        return self.a[key]


def test_duck_typed_volume_only_sliced_at_crop_boxes():
    vol = _Sliced(_vol())
    s = G.volume3d_ng(vol, ((0, 0, 0), (40, 30, 20)), size=12, seed=9)
    crops = [next(s) for _ in range(5)]
    ref = G.volume3d_ng(vol.a, ((0, 0, 0), (40, 30, 20)), size=12, seed=9).next_origins(5)
    assert vol.boxes == [((z, z + 12), (y, y + 12), (x, x + 12)) for z, y, x in ref]
    assert all(np.array_equal(c, vol.a[z:z + 12, y:y + 12, x:x + 12]) for c, (z, y, x) in zip(crops, ref))


def test_rank_streams():
    vol = _vol()
    s = G.volume3d_ng(vol, ((0, 0, 0), (40, 30, 20)), size=12, seed=9)
    r0, r1 = s.for_rank(0).next_origins(20), s.for_rank(1).next_origins(20)
    assert r0 != r1
    rng = np.random.default_rng([9, 1])
    z, y, x = r1[0]
    assert (x, y, z) == tuple(int(rng.integers(0, h)) for h in (40, 30, 20))
    # world_size 1: the dataset uses the sampler's own stream
    ds, _ = D.create_dataset_from_generator(G.volume3d_ng(vol, ((0, 0, 0), (40, 30, 20)), 12, seed=9), batch_size=2,
                                            epoch_size=4, global_adjust=False)
    own = G.volume3d_ng(vol, ((0, 0, 0), (40, 30, 20)), 12, seed=9).next_origins(4)
    got = np.concatenate(list(ds))[..., 0]
    want = np.stack([vol[z:z + 12, y:y + 12, x:x + 12] for z, y, x in own]).astype(np.float32) / np.float32(127.5) - 1
    assert np.array_equal(got, want)
    # world_size 2: rank 1 draws from the per-rank stream
    ds, _ = D.create_dataset_from_generator(G.volume3d_ng(vol, ((0, 0, 0), (40, 30, 20)), 12, seed=9), batch_size=1,
                                            epoch_size=4, global_adjust=False, rank=1, world_size=2)
    o = r1[0]
    first = next(iter(ds))[0, ..., 0]
    assert np.array_equal(first, vol[o[0]:o[0] + 12, o[1]:o[1] + 12, o[2]:o[2] + 12] / np.float32(127.5) - np.float32(1))


@pytest.mark.parametrize("aug", [False, True])
def test_host_dataset_equals_hand_built_batches(aug):
    vol = _vol()
    pad = [[2, 1], [0, 3], [1, 1]]
    mk = lambda: G.volume3d_ng(vol, ((0, 0, 0), (40, 30, 20)), 10, seed=5)
    ds, ms = D.create_dataset_from_generator(mk(), batch_size=2, epoch_size=6, padding=pad,
                                             enable_augmentation=False, seed=3)
    origins = mk().next_origins(200)
    samples = [D.scale_tensor(np.pad(vol[z:z + 10, y:y + 10, x:x + 10], pad, "reflect")) for z, y, x in origins]
    limit = D.meanstd_samples(samples[0].size, 6)
    assert np.allclose(ms, D.get_meanstd(samples[:limit]), rtol=0, atol=0)
    got = [b for _ in range(2) for b in ds]
    want = [np.stack([D.standardize_population(t, ms) for t in samples[2 * i:2 * i + 2]]) for i in range(6)]
    assert len(got) == 6 and all(np.array_equal(g, w) for g, w in zip(got, want))
    if aug:
        ds, _ = D.create_dataset_from_generator(mk(), batch_size=2, epoch_size=4, meanstd=ms, padding=[[1, 1]] * 3,
                                                enable_augmentation=True, seed=3)
        rng = np.random.default_rng([3, 0])
        own = mk().next_origins(4)
        for b, batch in enumerate(ds):
            for i in range(2):
                z, y, x = own[2 * b + i]
                t = D.standardize_population(D.scale_tensor(np.pad(vol[z:z + 10, y:y + 10, x:x + 10], 1, "reflect")), ms)
                assert np.array_equal(batch[i], D.augment(t, rng))


def test_reflect_index_map_matches_np_pad():
    for n in (2, 3, 5, 13):
        for lo, hi in ((0, 0), (1, 2), (n - 1, n - 1), (n + 3, 2 * n + 1)):
            a = np.arange(n)
            want = np.pad(a, (lo, hi), "reflect")
            got = [V.reflect_index(i - lo, n) for i in range(n + lo + hi)]
            assert list(want) == got, (n, lo, hi)
    assert V.pad_pairs(2, 3) == [(2, 2)] * 3 and V.pad_pairs([1, 3], 2) == [(1, 3)] * 2
    assert V.pad_pairs([[0, 1], [2, 3]], 2) == [(0, 1), (2, 3)]
