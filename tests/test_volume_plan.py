"""Host-side chunk planner of the out-of-core prediction (utils.chunk_plan): the chunks regroup tile_plan's tiles
exactly, read the clipped union of their tiles' haloed boxes, and tile the output once."""
import itertools

import numpy as np
import pytest

from transfer_em_amd.utils import TILE_BATCH, chunk_plan, tile_plan

# (outdimsize, buffer) of the 74, 132 and 260 models; 74 and 260 take the "multiple of 6" path with tpad > 0
MODELS = {74: (40, 17), 132: (96, 18), 260: (224, 18)}

CASES = [
    # model, start (x,y,z), size (x,y,z), volume shape (z,y,x)
    (74, (4, 6, 8), (50, 44, 38), (70, 64, 60)),
    (74, (-30, -25, -20), (200, 170, 150), (110, 130, 150)),         # reaches past all six faces
    (74, (0, 0, 0), (72, 108, 36), (36, 108, 72)),                   # multiple of the tile edge
    (74, (500, 0, 0), (40, 40, 40), (50, 50, 50)),                   # wholly outside the volume
    (132, (-10, 5, 3), (300, 260, 200), (180, 250, 320)),
    (132, (0, 0, 0), (1024, 1024, 512), (512, 1024, 1024)),
    (260, (-3, -3, -3), (500, 300, 230), (200, 280, 480)),
]
CHUNKS = [None, (1, 1, 1), (1, 2, 2), (2, 3, 1), (3, 3, 3), (5, 1, 7)]


def _check(model, start, size, vol_shape, chunk_tiles):
    od0, buf0 = MODELS[model]
    od, buf, tpad, rois, index = tile_plan(start, size, od0, buf0)
    edge = od + 2 * buf
    chunks = chunk_plan(start, size, od0, buf0, vol_shape, chunk_tiles)
    seen, boxes = [], []
    for c in chunks:
        assert len(c.tiles) == len(c.origins) == len(c.offsets) > 0
        if chunk_tiles is None:
            assert len(c.tiles) <= TILE_BATCH
        else:
            assert len(c.tiles) <= int(np.prod(chunk_tiles))
        # tiles back in volume / output coordinates are tile_plan's
        for i, o, f in zip(c.tiles, c.origins, c.offsets):
            seen.append(i)
            assert tuple(o[d] + c.read[d][0] for d in range(3)) == (rois[i][2], rois[i][1], rois[i][0])
            assert tuple(f[d] + c.base[d] for d in range(3)) == (index[i][2], index[i][1], index[i][0])
            assert all(0 <= f[d] and f[d] + od <= c.dims[d] for d in range(3))
        # footprint = clipped union of the haloed boxes; every tile's haloed box n volume lies inside it
        org = [(rois[i][2], rois[i][1], rois[i][0]) for i in c.tiles]
        for d in range(3):
            lo = min(max(min(o[d] for o in org), 0), vol_shape[d])
            hi = max(min(max(o[d] for o in org) + edge, vol_shape[d]), lo)
            assert c.read[d] == (lo, hi) and c.block[d] == hi - lo
            for o in org:
                a, b = max(o[d], 0), min(o[d] + edge, vol_shape[d])
                if a < b:
                    assert lo <= a and b <= hi
        # the tiles fill the device output block exactly once
        blk = np.zeros(c.dims, np.int32)
        for f in c.offsets:
            blk[f[0]:f[0] + od, f[1]:f[1] + od, f[2]:f[2] + od] += 1
        assert (blk == 1).all()
        (z0, z1), (y0, y1), (x0, x1) = c.out_box
        assert (z0, y0, x0) == c.base and z1 - z0 <= c.dims[0] and y1 - y0 <= c.dims[1] and x1 - x0 <= c.dims[2]
        boxes.append((z0, z1, y0, y1, x0, x1))
    assert sorted(seen) == list(range(len(rois)))
    # output boxes: inside (size[2], size[1], size[0]), pairwise disjoint, volumes adding up to the whole
    b = np.array(boxes, np.int64)
    assert (b[:, 0::2] >= 0).all() and (b[:, 1::2] <= [size[2], size[1], size[0]]).all()
    assert (b[:, 1::2] - b[:, 0::2]).prod(axis=1).sum() == size[0] * size[1] * size[2]
    lo, hi = b[:, 0::2], b[:, 1::2]
    inter = np.clip(np.minimum(hi[:, None], hi[None]) - np.maximum(lo[:, None], lo[None]), 0, None).prod(axis=2)
    np.fill_diagonal(inter, 0)
    assert not inter.any()
    return chunks


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
@pytest.mark.parametrize("chunk_tiles", CHUNKS, ids=str)
def test_chunks_regroup_tile_plan(case, chunk_tiles):
    _check(*case, chunk_tiles)


def test_tpad_case_is_covered():
    assert tile_plan((0, 0, 0), (10, 10, 10), *MODELS[74])[2] > 0
    assert tile_plan((0, 0, 0), (10, 10, 10), *MODELS[260])[2] > 0


def test_footprint_is_the_halo_union_inside_the_volume():
    # one chunk of 2x2x2 tiles in the middle of a large volume: edge + od per side
    od, buf = MODELS[132]
    (c,) = chunk_plan((100, 100, 100), (192, 192, 192), od, buf, (1000, 1000, 1000), (2, 2, 2))
    assert c.read == ((82, 82 + 192 + 36),) * 3 and c.block == (228, 228, 228)
    # wholly outside: empty footprint, nothing read
    (c,) = chunk_plan((2000, 0, 0), (96, 96, 96), od, buf, (100, 100, 100), (1, 1, 1))
    assert np.prod(c.block) == 0


def test_default_chunk_is_one_generator_batch():
    od, buf = MODELS[132]
    chunks = chunk_plan((0, 0, 0), (1024, 1024, 512), od, buf, (512, 1024, 1024), None)
    assert max(len(c.tiles) for c in chunks) == TILE_BATCH
    assert len(chunks) == 32
    # same-sized chunks come together (one generator plan shape after another)
    sizes = [len(c.tiles) for c in chunks]
    assert sizes == sorted(sizes, reverse=True)


@pytest.mark.parametrize("world_size", [2, 3])
def test_ranks_partition_the_chunks(world_size):
    od, buf = MODELS[74]
    start, size, shape = (-30, -25, -20), (200, 170, 150), (110, 130, 150)
    every = chunk_plan(start, size, od, buf, shape, (1, 2, 2))
    parts = [chunk_plan(start, size, od, buf, shape, (1, 2, 2), rank=r, world_size=world_size)
             for r in range(world_size)]
    assert all(parts)
    got = sorted(c.tiles for c in itertools.chain(*parts))
    assert got == sorted(c.tiles for c in every)
    assert len(got) == len(set(got))
