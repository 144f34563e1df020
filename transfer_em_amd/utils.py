"""General utilities using the predicted network (mirror of reference transfer_em/utils.py).

`predict_cube` is the local-array form of reference `predict_ng_cube` (utils.py:41-130): the same
tiling / halo / "multiple of 6" logic, with the cloud fetch replaced by slicing a uint8 array that
is already in memory.  Per tile: uint8 -> float (fused scale+standardize kernel) -> generator_g
forward (dropout off) -> (unstandardize+1)*127.5 -> round -> uint8 (fused kernel, wraps like
astype(uint8)) -> written into the output block.  Tiles are independent: `rank`/`world_size`
shard them over processes (one per GPU) without any collective.

`predict_volume` is the out-of-core form for volumes that do not fit in memory (np.memmap, h5py, zarr): the same
tiles, grouped into chunks of whole tiles (`chunk_plan`), each read from the volume by its footprint only and
streamed through the same kernels with the I/O of neighbouring chunks overlapped with the GPU work.

Every entry point dispatches on `model.generator_g.is3d`.  A 2-D model predicts a stack of sections [z, y, x] section
by section (`tile_plan_2d`: tile_plan's in-plane tiling in every section, no halo and no rounding along z) through the
2-D tile kernels, or one image [y, x] given 2-element start / size.

`volume_histogram`, `meanstd_from_histogram` and `match_lut` measure a volume's intensities out of core and turn them into
the statistics and lookup tables that `predict_cube` / `predict_volume` take (`lut=`: remapped on the device ahead of the
gather; `histogram=True`: the histogram of the prediction, counted on the device).

`clahe_histograms`, `clahe_tables` (together: `clahe_fit`) and `clahe_volume` are contrast-limited adaptive histogram
equalisation, section by section, the usual preparation of electron-microscopy volumes: tile histograms counted out of
core on the device, the clipped and cumulated tables in exact integers on the host, and the remap -- bilinear
interpolation between the tile centres, in integers -- on the device, written out (`clahe_volume`, for training volumes)
or applied to the uploaded bytes ahead of the gather (`clahe=` of `predict_cube` / `predict_volume`), so that a model
trained on equalised data sees equalised data without an equalised copy of the volume.

`volume_joint_histogram` holds two uint8 volumes against each other out of core: the 256 x 256 joint histogram, counted
on the device, from which `compare_from_joint` derives RMSE, MAE, PSNR, correlation and mutual information and
`regression_lut` the paired intensity map (a table for `lut=`); `compare=gt` of `predict_cube` / `predict_volume` counts
it for a prediction against its ground truth while the prediction is still on the device.

`volume_ssim` is the structural half of that comparison: the windowed structural similarity (SSIM) of two uint8 volumes
out of core, in integers (tem_u8_ssim), as per-section sums that `ssim_from_sums` turns into the index, and optionally
as a uint8 map of where the two volumes differ in structure.

`volume_rescale` brings a uint8 volume onto the voxel grid of the other domain out of core (tem_u8_rescale): one step
p / q per axis, the area average where an axis shrinks and linear interpolation where it grows, in integers with one
rounding per voxel; `rescale_step`, `rescale_shape`, `rescale_taps` and `rescale_chunks` are its host side.

`volume_repair` fills lost sections and bad voxels along z from the nearest good sections below and above, out of core
(tem_u8_repair_z); `Repair` names what is bad, `flat_sections` finds blank sections in a per-section histogram,
`repair_chunks` is its slab plan, and `repair=` of `predict_cube` / `predict_volume` does the same to the uploaded bytes
ahead of `clahe` and `lut`, without a repaired copy of the volume.

`section_sums` measures out of core how much every tile of a section resembles the same tile one section up
(tem_u8_zcorr_tiles: exact integer sums); `section_scores` turns the sums into correlations, `find_defects` into the
sections and regions that resemble neither neighbour, and `defect_mask` / `defects_repair` into the `Repair` that
`volume_repair` and `repair=` take; `zcorr_chunks` is its slab plan.

`section_shift_sums` is the same measurement against the next section displaced by every integer offset within a
radius (tem_u8_zshift_tiles); `shift_counts` and `shift_scores` turn the sums into correlations, `section_shifts` into
the displacement of every section against the one below it, `shift_positions` into a position per section, and
`volume_shift` moves the sections (or a mask) there on the host; `zshift_chunks` is the slab plan.

`section_shifts_coarse_to_fine` measures displacements far beyond a radius: the same search on a pyramid of 2 x reduced
sections (`volume_rescale`), every finer level centred per pair and tile on the coarser level's answer
(tem_u8_zshift_tiles_at).  `shift_centers`, `zshift_chunks_at`, `shift_counts_at`, `section_shift_sums_at`,
`shift_scores_at`, `section_shifts_at` and `shift_subpixel_at` are the centred forms of the functions above.

`section_shifts_bridged` is the same pyramid over an explicit list of section pairs (a, b), so that the good sections
on either side of a bad one are measured against each other (tem_u8_zshift_tiles_pairs): `section_pairs` and
`suspect_sections` make the list, `zshift_chunks_pairs`, `shift_counts_pairs`, `section_shift_sums_pairs`,
`shift_scores_pairs`, `section_shifts_pairs` and `shift_subpixel_pairs` are the per-pair forms, and `chain_pairs` puts
per-pair shifts, maps or fields back onto the stack's consecutive pairs.

`shift_subpixel` refines the same tile offsets below a pixel, `fit_section_maps` fits one affine map (or translation)
per pair of sections to them, `section_maps` composes the pair maps into one map per section, `quantize_maps` brings
them to the 2^-16 fixed point of the device, and `volume_warp` resamples every section through its map out of core
(tem_u8_warp_affine: bilinear or nearest, in integers with one rounding per voxel); `warp_chunks` is the slab plan.

`fit_section_fields` turns what the affine fit leaves over in the tile offsets into one smooth displacement field per
pair on a lattice (`field_grid`), `section_fields` composes the pairs into one map and one field per section,
`quantize_field` brings the fields to the device's fixed point, and `volume_warp_field` resamples every section through
"affine map + field" out of core (tem_u8_warp_field); `field_chunks` is the slab plan.

`section_lag_sums` is `section_sums` at several lags (tem_u8_zcorr_lags); `lag_scores` turns the sums into correlations
per lag and `section_spacing` into the sections' positions along z, from how fast the correlation decays with the lag;
`quantize_positions` brings them to 2^-16 section, `resample_z_taps` to the table of taps, and `volume_resample_z`
resamples the stack (or, nearest, a mask) onto the even grid out of core (tem_u8_resample_z); `zlag_chunks` and
`resample_z_chunks` are the slab plans.

`section_plane_sums` looks INSIDE a section: the sums behind the correlation of every tile with itself displaced by a few
pixels along y and x (tem_u8_zplane_lags; `plane_lag_chunks` is the slab plan, `plane_lag_counts` the number of pairs).
`plane_scores` turns them into correlations, `section_sharpness` and `find_blurred` into the sections and regions that
are out of focus (a Defects; `join_defects` joins it with find_defects'), `plane_curve` and `z_pitch` into the sections'
distance in pixels, and `pitch_step` into the `volume_rescale` step that makes the stack isotropic.
"""
import contextlib
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from . import hip_ops as H


def _plan_outdimsize(outdimsize):
    """tile_plan's outdimsize: the "multiple of 6" quirk applied ("make sure outdimsize is a multiple of 8" -- the code
    uses 6)."""
    return outdimsize - outdimsize % 6 if outdimsize // 6 != 0 else outdimsize


def _tile_plan(start, size, outdimsize, buffer, is3d):
    """tile_plan (is3d) or tile_plan_2d: the same in-plane tiling; along z a step of outdimsize under the halo, or a
    step of one section and no halo."""
    od = _plan_outdimsize(outdimsize)
    tpad = (outdimsize - od) // 2
    buffer += tpad
    zstep, zhalo = (od, buffer) if is3d else (1, 0)
    rois, index = [], []
    for xiter in range(start[0], start[0] + size[0], od):
        for yiter in range(start[1], start[1] + size[1], od):
            for ziter in range(start[2], start[2] + size[2], zstep):
                rois.append((xiter - buffer, yiter - buffer, ziter - zhalo))
                index.append((xiter - start[0], yiter - start[1], ziter - start[2]))
    return od, buffer, tpad, rois, index


def tile_plan(start, size, outdimsize, buffer):
    """Tile origins of utils.py:68-84.  Returns (outdimsize, buffer, tpad, rois, index)."""
    return _tile_plan(start, size, outdimsize, buffer, True)


TILE_BATCH = 27      # tiles per generator launch sequence (27 x 132^3: ~10 GB of activations; 288 GB HBM)


def tile_plan_2d(start, size, outdimsize, buffer):
    """The 2-D counterpart of tile_plan: every section z in [start[2], start[2] + size[2]) is tiled on its own with
    tile_plan's in-plane rules (same "multiple of 6" quirk, tpad, halo, rounding up to whole tiles in y and x); no
    halo and no rounding along z.  Returns (outdimsize, buffer, tpad, rois, index) with (x, y, z) rois / index whose z
    is the section itself (absolute in rois, relative to start[2] in index)."""
    return _tile_plan(start, size, outdimsize, buffer, False)


def plan_bytes_per_tile(edge, is3d=True, wf=8):
    """Bytes one input tile of edge `edge` pins in a generator inference plan (GenForward): the fp32 input and every
    layer's activation."""
    from .models.generator import generator_edges, generator_param_shapes
    shapes = generator_param_shapes(is3d, wf)
    ch = {k: v[-1] for k, v in shapes.items()}
    ch["u2b"], ch["u1b"] = shapes["u2b"][3], shapes["u1b"][3]
    e, d = generator_edges(edge), 3 if is3d else 2
    return 4 * (edge ** d + sum(e[k] ** d * c for k, c in ch.items()))


TILE_BATCH_MAX_2D = 4096     # cap of the 2-D batch (see default_tile_batch)


def default_tile_batch(edge, is3d=True):
    """Tiles per generator launch sequence when the caller gives none.  3-D: TILE_BATCH, or stable_tile_batch where
    that is smaller (the 260 model: 2).  2-D tiles are ~100x smaller, so the batch is sized by bytes instead: as many
    tiles as fit the activations TILE_BATCH tiles of the 132^3 model pin (~8 GB; 2-D 132: ~2,500 tiles), capped at
    TILE_BATCH_MAX_2D.  A prediction runs full batches and one remainder,
    and the generator caches MAX_PLANS = 2 plan shapes; the cap keeps the small models' batch below the size of most
    requests, so that their full-batch plan is reused from request to request instead of every request's size
    becoming a plan of its own."""
    if is3d:
        return min(TILE_BATCH, stable_tile_batch(edge, True))
    budget = TILE_BATCH * plan_bytes_per_tile(132, True)
    return max(1, min(TILE_BATCH_MAX_2D, budget // plan_bytes_per_tile(edge, False)))


def _dry_view(v, ptr, N, dims, C, strides=None):
    """Fill tem_view `v`: N x dims x C at `ptr` (never dereferenced), dense unless `strides` = (sN, sD, sH, sW)."""
    D, H, W = dims
    v.ptr, v.N, v.D, v.H, v.W, v.C = ptr, N, D, H, W, C
    v.sN, v.sD, v.sH, v.sW = strides or (D * H * W * C, H * W * C, W * C, C)


def plan_routes(edge, N, is3d=True, dtype=torch.float32, wf=8):
    """Kernel symbol of each of the 12 convolution launches of the generator's inference plan (GenForward with
    in_pad = 0, out_crop = 0) on a batch of N tiles of edge `edge`, as an OrderedDict layer -> name: what
    Launch.meta["kernel"] of that plan holds (a transposed layer on its direct form, which no query names, is spelled
    as conv_launch spells it).  Asked of the library's dry queries (tem_conv_is_tiled, the bf16 describe
    entry points) on the plan's dense views with made-up pointers, so no device is needed.  The layers, channels and
    geometry come from generator_blocks / generator_edges / skip_crop, the choice between the Winograd-domain and the
    plain kernel copy is conv_launch's."""
    import ctypes as C
    from collections import OrderedDict
    from .models.generator import generator_blocks, generator_edges, skip_crop
    lib = _lib.load()
    bf16 = dtype == torch.bfloat16
    esz = 2 if bf16 else 4
    blocks, e = generator_blocks(is3d, wf), generator_edges(edge)
    dims = lambda n: (n if is3d else 1, n, n)
    src = dict(zip(blocks, ["in"] + list(blocks)[:-1]))                 # each layer reads the one before it ...
    skips = {"mid": "d2a", "f1": "d1a"}                                 # ... and these two a cropped skip tensor as well
    ptr = {k: 0x7f0000000000 + (i << 40) for i, k in enumerate(e)}     # one made-up 16-byte-aligned base per tensor
    ch = {"in": 1}
    routes = OrderedDict()
    for name, spec in blocks.items():
        T = spec.kind != "conv"
        s_in, c1 = src[name], 0
        a = _lib.tem_conv_args()
        _dry_view(a.in0, ptr[s_in], N, dims(e[s_in]), ch[s_in])
        if name in skips:                                               # GenForward.skip0 / skip1: a window of the skip tensor
            sk = skips[name]
            c1, n = ch[sk], e[sk]
            lo, _ = skip_crop(n, e[s_in])
            st = (dims(n)[0] * n * n * c1, n * n * c1, n * c1, c1)
            off = lo * ((st[1] if is3d else 0) + st[2] + st[3])
            _dry_view(a.in1, ptr[sk] + esz * off, N, dims(e[s_in]), c1, st)
        assert spec.in_ch == ch[s_in] + c1, (name, spec)
        ch[name] = spec.out_ch
        _dry_view(a.out0, ptr[name], N, dims(e[name]), spec.out_ch)
        a.w = 0x7e0000000000
        k, s, p = spec.kernel, spec.stride, (1 if T else 0)            # VALID convolutions; ConvTranspose 'same'
        a.kd, a.kh, a.kw = H._k3(k, is3d)
        a.sd, a.sh, a.sw = H._s3(s, is3d)
        a.pd, a.ph, a.pw = H._p3(p, is3d)
        a.ep.slope = 1.0 if spec.activation == "linear" else H.LEAKY
        buf = C.create_string_buffer(96)
        if bf16:
            rc = (lib.tem_conv_transpose_bf16_describe if T else lib.tem_conv_bf16_describe)(C.byref(a), buf, 96)
            routes[name] = buf.value.decode() if rc == 0 else f"rc={rc}"
            continue
        vox = a.out0.D * a.out0.H * a.out0.W
        if not T and is3d and k == 3 and H.wino_channels(spec.in_ch, spec.out_ch) and vox >= H.WINO_MIN_VOXELS:
            a.w_layout = _lib.TEM_W_WINOGRAD
            if lib.tem_conv_is_tiled(C.byref(a), 0, buf, 96) == 1:
                routes[name] = buf.value.decode()
                continue
        a.w_layout = _lib.TEM_W_TAP_CI_CO
        tiled = lib.tem_conv_is_tiled(C.byref(a), int(T), buf, 96) == 1
        co = spec.out_ch
        routes[name] = buf.value.decode() if (tiled or not T) else f"convT_direct_k<{ch[s_in]}, {co}, 0, {8 if co == 32 else co}>"
    return routes


def route_key(kernel):
    """What of a kernel symbol decides the order of an output's sum: the kernel function.  Its template arguments past
    the channel counts (tiles per wave, waves, z-run lengths: conv_lds_k's MTW changes at N = 5 on the 74 model) are
    picked by the planners' cost models from the block count; they deal outputs to waves and leave each output's own
    chain of fused multiply-adds alone."""
    return kernel.split("<", 1)[0]


_STABLE_BATCH = {}
STABLE_BATCH_SEARCH_MAX = 1 << 20     # past any batch a card can hold (2-D 74: 2^20 tiles pin ~0.6 TB)


def stable_tile_batch(edge, is3d=True, dtype=torch.float32):
    """The largest tile batch N for which every launch of the generator's inference plan runs the kernel it runs at
    N = 1 (plan_routes, compared by route_key).  The tiled kernels address their operands with 32-bit offsets; a view past a kernel's span
    limit goes to another kernel, which sums in another order.  Up to this N a full batch, a remainder batch and a
    single tile all run the same kernels, which is what makes the batched pipeline equal the tile-by-tile one bit for
    bit; predict_cube and predict_volume lower a larger `tile_batch` to it.  A view only grows with N, so every limit
    is crossed once and the routes change at most once per limit: the search doubles N until a route changes, then
    bisects.  Host only (dry queries); cached per (edge, is3d, dtype).  STABLE_BATCH_SEARCH_MAX if nothing changes
    below it."""
    key = (int(edge), bool(is3d), dtype)
    if key not in _STABLE_BATCH:
        keys = lambda n: [route_key(k) for k in plan_routes(edge, n, is3d, dtype).values()]
        base = keys(1)
        same = lambda n: keys(n) == base
        lo = 1
        while lo < STABLE_BATCH_SEARCH_MAX and same(min(2 * lo, STABLE_BATCH_SEARCH_MAX)):
            lo = min(2 * lo, STABLE_BATCH_SEARCH_MAX)
        hi = min(2 * lo, STABLE_BATCH_SEARCH_MAX)          # same(lo), and not same(hi) unless lo reached the cap
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if same(mid) else (lo, mid)
        _STABLE_BATCH[key] = lo
    return _STABLE_BATCH[key]


def _effective_batch(requested, edge, is3d, most):
    """Tiles per generator launch sequence: the request (or the default), at most `most` tiles and at most
    stable_tile_batch (fp32: the precision the inference plans run in)."""
    nb = int(requested or default_tile_batch(edge, is3d))
    return max(1, min(nb, stable_tile_batch(edge, is3d, torch.float32), most))


BOUNDARIES = ("zeros", "reflect", "edge")     # what a tile voxel outside the volume reads


def fold(i, n, boundary):
    """Index that coordinate(s) `i` (int or integer array) of an axis of extent `n` read under `boundary`:
    "edge" clamps to [0, n-1]; "reflect" mirrors without repeating the face voxel (period 2(n-1); extent 1 reads
    index 0).  These are numpy.pad's modes of the same names for any pad width, wider than the axis included.  The
    tile gather kernels (tem_u8_tiles*_to_f32_std_bc) fold by the same rule; "zeros" folds nothing and has no index."""
    if boundary not in BOUNDARIES[1:]:
        raise ValueError(f"fold: boundary must be 'reflect' or 'edge', got {boundary!r}")
    if n < 1:
        raise ValueError(f"boundary={boundary!r} needs a non-empty axis, got extent {n}")
    if boundary == "edge":
        return np.clip(i, 0, n - 1) if isinstance(i, np.ndarray) else min(max(i, 0), n - 1)
    if n == 1:
        return np.zeros_like(i) if isinstance(i, np.ndarray) else 0
    m = 2 * (n - 1)
    r = i % m                                       # non-negative for ints and arrays alike
    return np.where(r < n, r, m - r) if isinstance(i, np.ndarray) else (r if r < n else m - r)


def _check_boundary(boundary, vol_shape):
    if boundary not in BOUNDARIES:
        raise ValueError(f"boundary must be one of {BOUNDARIES}, got {boundary!r}")
    if boundary != "zeros" and min(vol_shape) < 1:
        raise ValueError(f"boundary={boundary!r} needs a non-empty volume, got shape {tuple(vol_shape)}")


def symmetries(is3d=True, kind="flips"):
    """The symmetries of the cube (is3d) or the square that the training augmentation draws from (datasets.augment,
    tem_augment_f32), as a list of (perm, flips) over the spatial axes (z, y, x) -- (y, x) for 2-D:
    T(v) = flip(transpose(v, perm), axes a with flips[a]).

    kind="flips": the identity permutation with every flip combination (8 members in 3-D, 4 in 2-D); kind="all": every
    permutation with every flip combination (48 / 8).  The order is fixed -- an ensemble accumulates in fp32 in this
    order: permutations in lexicographic order (itertools.permutations, identity first), and within one permutation
    the flips as itertools.product((False, True), repeat=n), all-False first and the last axis changing fastest.  The
    identity is member 0."""
    import itertools
    n = 3 if is3d else 2
    if kind not in ("flips", "all"):
        raise ValueError(f"symmetries: kind must be 'flips' or 'all', got {kind!r}")
    perms = [tuple(range(n))] if kind == "flips" else list(itertools.permutations(range(n)))
    return [(p, f) for p in perms for f in itertools.product((False, True), repeat=n)]


def _check_ensemble(ensemble, is3d):
    """None, or the members of `ensemble` ("flips", "all" or a non-empty sequence of symmetries) as 3-axis
    ((p0, p1, p2), (f0, f1, f2)) tuples of ints.  A 2-D model takes 2-axis symmetries over (y, x), or 3-axis ones that
    leave the section axis alone (perm[0] == 0, flips[0] false)."""
    if ensemble is None:
        return None
    if isinstance(ensemble, str):
        ensemble = symmetries(is3d, ensemble)           # raises on another string
    try:
        members = list(ensemble)
    except TypeError:
        raise ValueError(f"ensemble must be None, 'flips', 'all' or a sequence of (perm, flips), got {ensemble!r}")
    if not members:
        raise ValueError("ensemble must not be empty (None runs without one)")
    out = []
    for s in members:
        try:
            perm, flips = s
            perm, flips = tuple(int(p) for p in perm), tuple(bool(f) for f in flips)
        except (TypeError, ValueError):
            raise ValueError(f"ensemble member {s!r} is not a (perm, flips) pair")
        n = len(perm)
        if n not in ((3,) if is3d else (2, 3)) or sorted(perm) != list(range(n)):
            raise ValueError(f"ensemble member {s!r}: perm must be a permutation of the {3 if is3d else '2 (or 3)'} "
                             f"spatial axes")
        if len(flips) != n:
            raise ValueError(f"ensemble member {s!r}: flips must have {n} entries, one per axis")
        if n == 2:                                      # (y, x) of a section
            perm, flips = (0, perm[0] + 1, perm[1] + 1), (False,) + flips
        elif not is3d and (perm[0] != 0 or flips[0]):
            raise ValueError(f"ensemble member {s!r} moves z: a 2-D model predicts section by section")
        if (perm, flips) in out:
            raise ValueError(f"ensemble member {s!r} is given twice")
        out.append((perm, flips))
    return [(p, tuple(int(f) for f in fl)) for p, fl in out]


def _check_spread(spread, spread_gain, syms, size, ndarray=False):
    """The `spread` / `spread_gain` keywords of predict_cube (ndarray=True) and predict_volume: None, or the gain as a
    float where `spread` is a writable uint8 array-like of exactly the result's shape -- (size[2], size[1], size[0]), or
    (size[1], size[0]) for a single image -- and there is an ensemble (`syms`: _check_ensemble's members) to take the
    spread of.  The gain is a finite number above 0, as a float32 too."""
    import numbers
    if not isinstance(spread_gain, numbers.Real) or isinstance(spread_gain, (bool, np.bool_)):
        raise ValueError(f"spread_gain must be a finite number above 0, got {spread_gain!r}")
    gain = float(spread_gain)
    with np.errstate(over="ignore"):
        g32 = float(np.float32(gain))                  # what the kernel is given
    if not (np.isfinite(g32) and g32 > 0):
        raise ValueError(f"spread_gain must be a finite float32 above 0, got {spread_gain!r}")
    if spread is None:
        return None
    if syms is None:
        raise ValueError("spread= is the spread of the ensemble's members: it needs ensemble=")
    if ndarray and not isinstance(spread, np.ndarray):
        raise ValueError(f"spread must be a numpy array, got {type(spread).__name__}")
    want = tuple(int(v) for v in reversed(size))
    if not hasattr(spread, "shape") or tuple(int(v) for v in spread.shape) != want:
        raise ValueError(f"spread has shape {tuple(getattr(spread, 'shape', ()))}, expected {want}")
    if getattr(spread, "dtype", None) is None or np.dtype(spread.dtype) != np.uint8:
        raise ValueError(f"spread must be uint8, got dtype {getattr(spread, 'dtype', None)}")
    if isinstance(spread, np.ndarray) and not spread.flags.writeable:
        raise ValueError("spread must be writable")
    return gain


class _TileRunner:
    """The tile loop of predict_cube and predict_volume, made once per call: gather -> generator -> scatter over the
    tiles of a source block, in batches, all enqueued on `stream`.  It owns the choice of the gather entry point and
    its argument order, the ensemble's fp32 accumulator, the generator plan per batch size and the scatter.  With
    `spread_gain` (the members' spread as a second uint8 block, see predict_cube) it also owns the three fp32 moment
    buffers, folds every member through the `_spread` form of the accumulate and scatters the finished map.

    The gather without an ensemble is the zero-mode entry point under "zeros" and its `_bc` sibling under the mirrored
    modes; with one (`syms`: _check_ensemble's members) it is the `_sym` entry point, which under "zeros" gets mode 0
    with the block handed over as the volume -- what the zero-mode entry point sees.  A source block of shape `block`
    holds the volume's box at `lo` (the resident volume: lo = 0, block = vol_shape)."""

    def __init__(self, lib, model, is3d, edge, tpad, outdimsize, boundary, syms, meanstd_x, meanstd_y, vol_shape,
                 stream, spread_gain=None):
        gname, self.sname, self.aname, self.fname = (
            ("tem_u8_tiles_to_f32_std", "tem_f32_tiles_unstd_to_u8", "tem_f32_tiles_sym_accum",
             "tem_f32_tiles_spread_to_u8") if is3d else
            ("tem_u8_tiles2d_to_f32_std", "tem_f32_tiles2d_unstd_to_u8", "tem_f32_tiles2d_sym_accum",
             "tem_f32_tiles2d_spread_to_u8"))
        self.gname = gname + ("_sym" if syms is not None else "" if boundary == "zeros" else "_bc")
        self.spread_gain = spread_gain
        if spread_gain is not None:
            self.aname += "_spread"
        self.gather, self.scatter, self.accum, self.finish = (
            getattr(lib, n) for n in (self.gname, self.sname, self.aname, self.fname))
        self.mode = {"zeros": 0, "reflect": _lib.TEM_BOUNDARY_REFLECT, "edge": _lib.TEM_BOUNDARY_EDGE}[boundary]
        self.model, self.gen = model, getattr(model, "generator_g", None)
        self.shape = ((edge, edge, edge) if is3d else (1, edge, edge)) + (1,)      # (D, H, W, C) of one generator input
        self.edge, self.tpad, self.outdimsize, self.syms, self.vol_shape, self.stream = \
            edge, tpad, outdimsize, syms, vol_shape, stream
        self.ms_x = (float(meanstd_x[0]), float(meanstd_x[1]))
        self.ms_y = (float(meanstd_y[0]), float(meanstd_y[1]))
        self.plan = self.acc = None             # acc: allocated by the first batch, the largest; smaller use its head
        self.moments = None                     # ref, s1, s2 of the spread: [3, *acc.shape], allocated with acc

    def _input(self, m):
        """(x, run) of a batch of m tiles: the generator's input tensor, and run() -> its output (overwritten by the
        next run).  A plan of another batch size is asked for with none held, so that an evicted plan's buffers are
        released first.  A generator without plans goes through model.predict: only predict_cube gets there,
        predict_volume refuses such a generator."""
        if not hasattr(self.gen, "plan"):
            x = torch.empty((m,) + self.shape, dtype=torch.float32, device=self.model.device)
            return x, lambda: self.model.predict(x).contiguous()
        if self.plan is None or self.plan.x.shape[0] != m:
            self.plan = None
            self.plan = self.gen.plan((m,) + self.shape)                        # static launch plan, buffers reused
        return self.plan.x, lambda: self.plan.run(self.stream)

    def run(self, src, block, lo, origins, offsets, n, nb, dst, dims, last_gather=None, spread_dst=None):
        """Run the n tiles of the source block at `src` (shape `block`, at `lo` in the volume) into the destination
        block at `dst` (shape `dims` = (OZ, OY, OX)) in batches of nb.  `origins` / `offsets` point to the tiles' int32
        (z, y, x) haloed origins in the source block and interior offsets in the destination block.  last_gather() is
        called after the last gather of the last batch: nothing enqueued later reads the source block.

        Under an ensemble a batch runs once per member s in order: the gather cuts T_s(tiles), and T_s^-1 of the
        generator's output is folded into the accumulator -- written by the first member, added to by the others,
        divided by the member count by the last -- whose mean is scattered once.  With a spread the same launch also
        folds the member into the moments, and the map finished from them is scattered into the block at `spread_dst`
        (shape `dims`) behind the prediction's scatter."""
        members = self.syms or [None]
        for b0 in range(0, n, nb):
            m = min(nb, n - b0)
            x, run = self._input(m)
            if self.mode:                       # the kernel folds lo + origin + p into the volume
                where = (*block, *lo, *self.vol_shape, self.mode)
            else:
                where = block if self.syms is None else (*block, 0, 0, 0, *block, 0)
            for i, sym in enumerate(members):
                last = i == len(members) - 1
                _lib.check(self.gather(src, *where, origins + 12 * b0, m, self.edge, *(sym[0] + sym[1] if sym else ()),
                                       x.data_ptr(), *self.ms_x, self.stream), self.gname)
                if last and b0 + m == n and last_gather is not None:
                    last_gather()
                y = run()
                if sym is not None:
                    if self.acc is None:
                        self.acc = torch.empty_like(y)
                        if self.spread_gain is not None:
                            self.moments = torch.empty((3,) + tuple(y.shape), dtype=y.dtype, device=y.device)
                    acc = self.acc[:m]
                    mom = () if self.moments is None else tuple(b[:m].data_ptr() for b in self.moments)
                    _lib.check(self.accum(y.data_ptr(), m, y.shape[2], *sym[0], *sym[1], acc.data_ptr(), int(i == 0),
                                          len(members) if last else 1, *mom, self.stream), self.aname)
                    y = acc
            assert y.shape[2] - 2 * self.tpad == self.outdimsize, (y.shape, self.tpad, self.outdimsize)
            _lib.check(self.scatter(y.data_ptr(), m, y.shape[2], self.tpad, offsets + 12 * b0, dst, *dims, *self.ms_y,
                                    self.stream), self.sname)
            if self.spread_gain is not None:
                _lib.check(self.finish(mom[1], mom[2], m, y.shape[2], self.tpad, offsets + 12 * b0, spread_dst, *dims,
                                       len(members), self.ms_y[1], self.spread_gain, self.stream), self.fname)


class _Prepare:
    """What predict_cube and predict_volume do to uploaded bytes ahead of the gather, made once per call: `clahe`
    (_check_clahe's tuple) and `lut` (_check_lut's table), either may be None, are uploaded here, once.  apply() remaps
    a block in place on `stream`: tem_u8_clahe first, then tem_u8_lut on the equalised bytes.  clahe_volume uses the
    first half alone.  `repair` (_check_repair's spec, or None) comes ahead of both: its section flags are uploaded here,
    once, and repair_block() fills a block's core planes in place (tem_u8_repair_z); volume_repair uses that alone."""

    def __init__(self, lib, clahe, lut, dev, stream, repair=None):
        self.lib, self.clahe, self.lut, self.stream, self.rp = lib, clahe, lut, stream, repair
        self.tab_dev = None if clahe is None else torch.from_numpy(clahe[0]).to(dev)    # every section's tables
        self.lut_dev = None if lut is None else torch.from_numpy(lut).to(dev)
        self.flags_dev = None if repair is None or repair.flags is None else torch.from_numpy(repair.flags).to(dev)

    def repair_block(self, ptr, block, zsec0, c0, c1, mask_ptr, counts_ptr=None):
        """Repair the core planes [c0, c1) of the dense uint8 block of shape `block` at `ptr`, whose plane 0 is the
        volume's section zsec0 and which reaches max_gap planes past the core or to the volume's face; `mask_ptr` is the
        mask's same block (None without a mask).  A block with an empty side is not there and nothing is launched."""
        if self.rp is None or min(block) < 1 or c1 <= c0:
            return
        _lib.check(self.lib.tem_u8_repair_z(ptr, *block, zsec0, c0, c1, mask_ptr,
                                            None if self.flags_dev is None else self.flags_dev.data_ptr(),
                                            self.rp.missing, self.rp.max_gap, counts_ptr, self.stream), "tem_u8_repair_z")

    def apply(self, ptr, block, lo):
        """Remap the dense uint8 block of shape `block` at `ptr` that holds the volume's box at `lo`: the tile grid and
        the rows of a [Z, 256] table belong to the volume (the resident volume: lo = 0, block = its shape).  A block
        with an empty side is not there -- an empty volume, or a chunk wholly outside the volume, whose one stand-in
        zero byte has to stay 0 -- and nothing is launched."""
        if min(block) < 1:
            return
        if self.tab_dev is not None:
            _, th, tw, gy, gx = self.clahe
            _lib.check(self.lib.tem_u8_clahe(ptr, *block, *lo, self.tab_dev.data_ptr(), gy, gx, th, tw, self.stream),
                       "tem_u8_clahe")
        if self.lut_dev is not None:
            _lib.check(self.lib.tem_u8_lut(ptr, *block, self.lut_dev.data_ptr(), int(self.lut.ndim == 2), lo[0],
                                           self.stream), "tem_u8_lut")


class _Measure:
    """What is counted on a uint8 result while it is on the device, made once per call: the int64[256] histogram
    (`histogram`), the int64[256, 256] joint histogram against a ground truth (`joint`) and the int64[256] histogram of
    the ensemble's spread map (`spread`), each one device accumulator that add() / add_spread() launches into on `stream`
    and report() reads back once."""

    def __init__(self, lib, histogram, joint, dev, stream, spread=False):
        self.lib, self.stream = lib, stream
        self.counts = torch.zeros(256, dtype=torch.int64, device=dev) if histogram else None
        self.spread = torch.zeros(256, dtype=torch.int64, device=dev) if spread else None
        self.joint = torch.zeros((256, 256), dtype=torch.int64, device=dev) if joint else None

    def add(self, ptr, dims, valid, gt=None):
        """Count the leading `valid` extents of the dense block of shape `dims` at `ptr` (tem_u8_hist) and, with
        gt = (pointer, dims, at), hold its box of gt's dims at offset `at` against the dense ground-truth block
        (tem_u8_hist2: J[u, v] with u from gt).  gt=None where there is no ground truth for the block."""
        if self.counts is not None and min(valid) > 0:
            _lib.check(self.lib.tem_u8_hist(ptr, *dims, 0, valid[0], 0, valid[1], 0, valid[2], self.counts.data_ptr(), 0,
                                            self.stream), "tem_u8_hist")
        if self.joint is not None and gt is not None:
            gt_ptr, n, at = gt
            _lib.check(self.lib.tem_u8_hist2(gt_ptr, *n, 0, 0, 0, ptr, *dims, *at, *n, self.joint.data_ptr(),
                                             self.stream), "tem_u8_hist2")

    def add_spread(self, ptr, dims, valid):
        """Count the leading `valid` extents of the dense spread block of shape `dims` at `ptr` (tem_u8_hist)."""
        if self.spread is not None and min(valid) > 0:
            _lib.check(self.lib.tem_u8_hist(ptr, *dims, 0, valid[0], 0, valid[1], 0, valid[2], self.spread.data_ptr(), 0,
                                            self.stream), "tem_u8_hist")

    def report(self, st):
        """The one read-back of each accumulator, into st["histogram"] / st["joint_histogram"] / st["spread_histogram"]."""
        if self.spread is not None:
            st["spread_histogram"] = self.spread.cpu().numpy()
        if self.counts is not None:
            st["histogram"] = self.counts.cpu().numpy()
        if self.joint is not None:
            st["joint_histogram"] = self.joint.cpu().numpy()


class _OneSection:
    """A [y, x] array-like seen as a one-section stack [1, y, x] (basic slicing only, for predict_volume)."""

    def __init__(self, a):
        self.a, self.shape, self.dtype = a, (1,) + tuple(int(v) for v in a.shape), getattr(a, "dtype", None)

    def _key(self, key):
        z, y, x = key
        if range(1)[z] != range(1):                    # the whole (only) section
            raise IndexError(f"section {z} of a single image")
        return y, x

    def __getitem__(self, key):
        return np.asarray(self.a[self._key(key)])[None]

    def __setitem__(self, key, value):
        self.a[self._key(key)] = value[0]


def _single_image(model, start, size):
    """True for the [y, x] single-image form (2-element start and size), which only 2-D models accept."""
    if len(start) == 2 and len(size) == 2:
        if getattr(getattr(model, "generator_g", None), "is3d", True):
            raise ValueError("a single [y, x] image (2-element start / size) needs a 2-D model")
        return True
    if len(start) != 3 or len(size) != 3:
        raise ValueError(f"start and size must both have 3 elements (x, y, z) or, for one image, 2 (x, y): "
                         f"got {start}, {size}")
    return False


def max_mips(outdimsize):
    """Levels of the mip pyramid that tiles of `outdimsize` voxels allow (the tile plan's outdimsize, i.e. after the
    "multiple of 6" quirk): the largest L with outdimsize % 2^L == 0.  Chunks are boxes of whole tiles and tiles start
    at multiples of outdimsize, so up to this L every level-l voxel has all its level-0 voxels in one chunk and a chunk
    pools on its own.  96 (the 132 model) -> 5, 36 (74) -> 2, 222 (260) -> 1; an odd outdimsize -> 0."""
    od, n = int(outdimsize), 0
    while od >= 2 and od % 2 == 0:
        od, n = od // 2, n + 1
    return n


def _check_mips(mips, outdimsize):
    """The number of pooled levels L >= 0 that `mips` (None or an integer) asks for, checked against
    max_mips(outdimsize) of the tile plan's outdimsize."""
    import operator
    if mips is None:
        return 0
    limit = max_mips(outdimsize)
    try:
        if isinstance(mips, (bool, np.bool_)):
            raise TypeError
        L = operator.index(mips)
    except TypeError:
        raise ValueError(f"mips must be None or an integer in [0, {limit}], got {mips!r}")
    if not 0 <= L <= limit:
        raise ValueError(f"mips={L} is outside [0, {limit}]: tiles of {outdimsize} voxels pool on their own for at most "
                         f"max_mips({outdimsize}) = {limit} levels (outdimsize % 2^mips must be 0)")
    return L


def mip_shapes(size, mips, is3d=True):
    """Shapes (z, y, x) of the mips + 1 levels of the pyramid of a prediction of `size` = (x, y, z): level 0 is
    (size[2], size[1], size[0]) and every further level ceil(n / f) per axis, f = (2, 2, 2) for a 3-D model and
    (1, 2, 2) for a 2-D one (sections are not pooled).  A 2-element `size` (x, y), the single-image form, gives
    (y, x) shapes."""
    if len(size) == 2:
        return [s[1:] for s in mip_shapes(tuple(size) + (1,), mips, False)]
    shape, shapes = (int(size[2]), int(size[1]), int(size[0])), []
    for _ in range(int(mips) + 1):
        shapes.append(shape)
        shape = (-(-shape[0] // 2) if is3d else shape[0], -(-shape[1] // 2), -(-shape[2] // 2))
    return shapes


def mip_box(chunk, level, is3d=True):
    """Where level `level` of a VolumeChunk's pyramid goes: (box, extent) with `box` the (z, y, x) (lo, hi) pairs in
    that level's output array and `extent` = hi - lo, the leading sub-block of the chunk's level block (chunk.dims
    divided by 2^level on the pooled axes) that holds it.  A pooled axis has lo = base >> level, exact for level <=
    max_mips, and extent ceil(out_box extent / 2^level); z of a 2-D model is not pooled."""
    box = []
    for d, (lo, hi) in enumerate(chunk.out_box):
        l = level if (is3d or d > 0) else 0
        b, n = chunk.base[d] >> l, max(hi - lo, 0)
        box.append((b, b + -(-n // (1 << l))))
    return tuple(box), tuple(hi - lo for lo, hi in box)


def _check_mip_outs(out, size, L, is3d=True):
    """predict_volume's `out` under mips = L >= 1: None, or a sequence of L + 1 array-likes of exactly mip_shapes."""
    if out is None:
        return None
    shapes = mip_shapes(size, L, is3d)
    if hasattr(out, "shape") or not hasattr(out, "__len__"):
        raise ValueError(f"with mips={L}, out must be None or a sequence of {L + 1} arrays (one per level), got "
                         f"{type(out).__name__}")
    outs = list(out)
    if len(outs) != L + 1:
        raise ValueError(f"with mips={L}, out must hold {L + 1} levels, got {len(outs)}")
    for l, (o, s) in enumerate(zip(outs, shapes)):
        if not hasattr(o, "shape") or tuple(int(v) for v in o.shape) != s:
            raise ValueError(f"out[{l}] has shape {tuple(getattr(o, 'shape', ()))}, expected {s}")
    return outs


def _pool_levels(lib, src_ptr, dims, valid, L, is3d, dst_ptrs, stream):
    """The L pooling launches of one block: level l + 1 = tem_u8_pool2 of level l, level 0 at `src_ptr` with dense
    `dims` and valid extents `valid`, level l at dst_ptrs[l - 1].  Returns the levels' (dims, valid) from level 1 on."""
    fz, levels = 2 if is3d else 1, []
    half = lambda v: (-(-v[0] // fz), -(-v[1] // 2), -(-v[2] // 2))
    for l in range(L):
        _lib.check(lib.tem_u8_pool2(src_ptr, *dims, *valid, fz, dst_ptrs[l], stream), "tem_u8_pool2")
        src_ptr, dims, valid = dst_ptrs[l], half(dims), half(valid)
        levels.append((dims, valid))
    return levels


HIST_CHUNK_BYTES = 64 << 20      # volume_histogram's default slab: two pinned and two device buffers of this size


def hist_box(vol_shape, start=None, size=None):
    """The (z, y, x) (lo, hi) box of the ROI `start` / `size` ((x, y, z) order; None: the whole volume) of a volume of
    shape (Z, Y, X).  One image: a 2-element shape with 2-element (x, y) start / size, returned as the box of a
    one-section stack.  The ROI must lie inside the volume -- a voxel that does not exist has no intensity --
    ValueError otherwise, as for a negative size or a wrong number of elements."""
    shape = tuple(int(v) for v in vol_shape)
    if len(shape) not in (2, 3):
        raise ValueError(f"volume must be [z, y, x] or one image [y, x], got shape {shape}")
    nd = len(shape)
    start = (0,) * nd if start is None else tuple(int(v) for v in start)
    size = tuple(reversed(shape)) if size is None else tuple(int(v) for v in size)
    if len(start) != nd or len(size) != nd:
        raise ValueError(f"start and size must have {nd} elements for a volume of shape {shape}: got {start}, {size}")
    box = []
    for d in range(nd):                               # d over (x, y[, z]); axis nd - 1 - d of the volume
        lo, n, ext = start[d], size[d], shape[nd - 1 - d]
        if n < 0 or lo < 0 or lo + n > ext:
            raise ValueError(f"the ROI start={start}, size={size} (x, y, z) reaches outside the volume of shape {shape}: "
                             f"voxels that do not exist have no intensity")
        box.append((lo, lo + n))
    box = tuple(reversed(box))
    return box if nd == 3 else ((0, 1),) + box


def hist_chunks(box, chunk_bytes=None, rank=0, world_size=1, itemsize=1):
    """Cut the (z, y, x) (lo, hi) `box` into disjoint slabs of at most `chunk_bytes` bytes (HIST_CHUNK_BYTES when None)
    whose union is the box: runs of whole sections, or, where one section of the box is larger than the budget, runs of
    whole rows of one section (one row at the least: a budget below a row's bytes gives one-row slabs).  x is never
    cut.  A voxel holds `itemsize` bytes (1, or 2 for the 16-bit passes: the budget is bytes, so such a slab holds half
    the voxels).  Slabs are in (z, y) order and go round-robin to the ranks; returns this rank's list of boxes.  Pure
    host function."""
    budget = _budget(chunk_bytes, rank, world_size)
    if itemsize not in (1, 2):
        raise ValueError(f"itemsize must be 1 or 2, got {itemsize!r}")
    return [core for core, _ in _cut_slabs(box, box[:2], budget, rank, world_size, itemsize=itemsize)]


def _budget(chunk_bytes, rank, world_size):
    """A cutter's budget in bytes: `chunk_bytes`, HIST_CHUNK_BYTES when None.  ValueError for a budget below 1 and for a
    rank outside [0, world_size)."""
    budget = HIST_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    if budget < 1:
        raise ValueError(f"chunk_bytes must be positive, got {chunk_bytes}")
    if not 0 <= rank < world_size:
        raise ValueError(f"rank {rank} is outside [0, {world_size})")
    return budget


def _cut_slabs(box, limits, budget, rank, world_size, zreach=(0, 0), yreach=(0, 0), itemsize=1):
    """The one rule behind hist_chunks, zcorr_chunks, zlag_chunks, repair_chunks, plane_lag_chunks and zshift_chunks*:
    this rank's list of (core slab, read slab), (z, y, x) (lo, hi) boxes.  The cores are disjoint and their union is
    `box`: runs of whole sections while a core next to its halo fits `budget` bytes, else runs of whole rows of one
    section, one row at the least; x is never cut; (z, y) order, dealt round-robin to the ranks.  A read slab is its
    core extended by `zreach` = (below, above) sections and `yreach` = (below, above) rows and clipped to `limits`, the
    (lo, hi) of z and of y; the budget counts a core next to both reaches.  A voxel holds `itemsize` bytes."""
    (z0, z1), (y0, y1), (x0, x1) = box
    (za, zb), (ya, yb) = zreach, yreach
    ny, nx = y1 - y0, (x1 - x0) * itemsize                  # nx: a row's bytes
    if z1 <= z0 or ny <= 0 or nx <= 0:
        return []
    if (1 + za + zb) * ny * nx <= budget:
        kz = budget // (ny * nx) - (za + zb)
        cores = [((z, min(z + kz, z1)), (y0, y1)) for z in range(z0, z1, kz)]
    else:
        ky = max(1, budget // ((1 + za + zb) * nx) - (ya + yb))
        cores = [((z, z + 1), (y, min(y + ky, y1))) for z in range(z0, z1) for y in range(y0, y1, ky)]
    (lz, hz), (ly, hy) = limits
    slabs = [((cz, cy, (x0, x1)), ((max(cz[0] - za, lz), min(cz[1] + zb, hz)), (max(cy[0] - ya, ly), min(cy[1] + yb, hy)),
                                   (x0, x1))) for cz, cy in cores]
    return slabs[rank::world_size]


class _InputStream:
    """The double-buffered input side of an out-of-core pass over K blocks of `nbytes[k]` bytes: block k is read on
    the executor's thread into pinned buffer k % 2 by read_into(k, flat uint8 ndarray), copied to device buffer k % 2
    on a copy stream, and waited for by the compute stream (the current stream of `dev`).  The read seconds add up in
    st["read_s"].  Used as a context manager around the pass, it owns the executor's end: on any exception it cancels
    what is queued, waits for the thread, synchronises the device -- nothing is in flight on the buffers about to be
    freed -- and re-raises; otherwise it waits for the queued work.

    The consumer's loop over k: `get(k)`, its kernels on the compute stream, `release(k, event)` once nothing
    enqueued later reads the buffer, `prefetch(k + 2)`.  The executor is the caller's, so that it can queue work of
    its own on the same thread in an order of its choice.  Buffer k % 2 is reused in this order: the read of block k
    waits for the H2D of block k - 2, and the H2D of block k for the release event of block k - 2."""

    def __init__(self, nbytes, read_into, dev, pool, st):
        self.nbytes, self.read_into, self.dev, self.pool, self.st = nbytes, read_into, dev, pool, st
        self.compute, self.h2d = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
        size, n = max(nbytes, default=0), min(2, len(nbytes))
        self.pin = [torch.empty(size, dtype=torch.uint8, pin_memory=True) for _ in range(n)]
        self.buf = [torch.empty(size, dtype=torch.uint8, device=dev) for _ in range(n)]
        self.reads, self.h2d_done, self.released = {}, {}, {}

    def __enter__(self):
        for k in range(len(self.pin)):
            self.prefetch(k)
        return self

    def __exit__(self, exc_type, exc, tb):
        self.pool.shutdown(wait=True, cancel_futures=exc_type is not None)
        if exc_type is not None:
            torch.cuda.synchronize(self.dev)

    def _read(self, k):                     # host thread: block k -> pin[k % 2]
        if k >= 2:
            self.h2d_done.pop(k - 2).synchronize()          # the buffer's previous H2D has finished
        t0 = time.perf_counter()
        self.read_into(k, self.pin[k % 2][:self.nbytes[k]].numpy())
        self.st["read_s"] += time.perf_counter() - t0

    def prefetch(self, k):
        if k < len(self.nbytes):
            self.reads[k] = self.pool.submit(self._read, k)

    def get(self, k):
        """The device buffer that holds block k in its first nbytes[k] bytes, once the compute stream gets there."""
        s, n = k % 2, self.nbytes[k]
        self.reads.pop(k).result()
        if k >= 2:
            self.h2d.wait_event(self.released.pop(k - 2))   # buf[s]: the consumer is done with block k - 2
        with torch.cuda.stream(self.h2d):
            self.buf[s][:n].copy_(self.pin[s][:n], non_blocking=True)
        self.h2d_done[k] = self.h2d.record_event()
        self.compute.wait_event(self.h2d_done[k])
        return self.buf[s]

    def release(self, k, event):
        self.released[k] = event


class _OutputStream:
    """The double-buffered output side of an out-of-core pass over K blocks of `nbytes[k]` bytes, the counterpart of
    _InputStream: block k is copied from the device into pinned buffer k % 2 on a copy stream and handed to
    write_from(k, flat uint8 ndarray) on the executor's thread.  The write seconds add up in st["write_s"].  With
    `own_buffers` it also holds two device buffers for the consumer's kernels to write block k into (`device(k)`);
    without, put() is given the device tensor to copy out of.  Used as a context manager inside the _InputStream's
    (the same executor: one host thread, whose work the consumer queues in the order write(k), read(k + 2)): leaving
    the pass waits for the queued writes, and a failed one raises there; on an exception it does nothing, the
    _InputStream around it owns the executor's end.  A slab pass makes it with _SlabPass.writing and feeds it with
    _SlabPass.put; predict_volume drives one of its own.

    The consumer's loop over k: [`device(k)`,] its kernels on the compute stream (the current stream of `dev`),
    `put(k, event)` with the event behind the last of them.  Buffers k % 2 are reused in this order: the D2H of block
    k waits for that event and, on the host, for the write of block k - 2 to have returned; the write of block k waits
    for that D2H; and the compute stream waits for the D2H of block k - 2 before `device(k)` is written again."""

    def __init__(self, nbytes, write_from, dev, pool, st, own_buffers=False):
        self.nbytes, self.write_from, self.pool, self.st = nbytes, write_from, pool, st
        self.compute, self.d2h = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
        size, n = max(nbytes, default=0), min(2, len(nbytes))
        self.pin = [torch.empty(size, dtype=torch.uint8, pin_memory=True) for _ in range(n)]
        self.buf = [torch.empty(size, dtype=torch.uint8, device=dev) for _ in range(n)] if own_buffers else None
        self.writes, self.copied = {}, [None, None]

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            for k in sorted(self.writes):
                self.writes.pop(k).result()

    def _write(self, k, copied):            # host thread: pin[k % 2] -> wherever write_from puts block k
        copied.synchronize()
        t0 = time.perf_counter()
        self.write_from(k, self.pin[k % 2][:self.nbytes[k]].numpy())
        self.st["write_s"] += time.perf_counter() - t0

    def device(self, k):
        """The own device buffer that block k goes into, once the compute stream gets there."""
        if k >= 2:
            self.compute.wait_event(self.copied[k % 2])         # buf[k % 2]: block k - 2's D2H has read it
        return self.buf[k % 2]

    def put(self, k, ready, src=None):
        """Copy block k out of `src` (default: the own device buffer) once `ready` and queue its write.  Returns the
        D2H's event: `src` is free when it has passed."""
        s, n = k % 2, self.nbytes[k]
        src = self.buf[s] if src is None else src
        if k >= 2:
            self.writes.pop(k - 2).result()                     # pin[s]: block k - 2 has been written
        self.d2h.wait_event(ready)
        with torch.cuda.stream(self.d2h):
            self.pin[s][:n].copy_(src[:n], non_blocking=True)
        self.copied[s] = self.d2h.record_event()
        self.writes[k] = self.pool.submit(self._write, k, self.copied[s])
        return self.copied[s]


class _SlabPass:
    """One out-of-core pass over a box of one or more uint8 array-likes [z, y, x] (one image [y, x]: a one-section
    stack), slab by slab through the input side of predict_volume's pipeline.  Making it is host work and comes ahead
    of any GPU work: the dtype check (ValueError) and this rank's slabs of boxes[0] (hist_chunks, or the list `slabs`
    of boxes inside boxes[0] where the caller cuts them itself: overlapping read slabs, ssim_chunks); the slab of
    volumes[i] is the same box shifted from boxes[0] to boxes[i].  itemsize=2 is the pass over native-endian uint16 /
    int16 volumes: the budget and the buffers stay bytes (a slab holds half the voxels) and the reader writes through a
    16-bit view.  `st` holds the read seconds `read_s` and the slab
    count `chunks`.

    `with p.streaming(stats):` is the pass, on `device` (None: the current one) as the current device: one host thread
    (`p.pool`) reads every volume's slab into an _InputStream of its own, which also ends the thread, on an exception
    as it describes; a pass that ends cleanly leaves `st` in the dict `stats` where one is given.  Inside,
    `for k, slab, dims, buffers in p:` gives slab k's box, its shape and one device buffer per volume that holds it,
    for the caller's launches on `p.compute`; behind them the buffers are released -- on `p.release_on` where an event
    has been set for this slab, else on one recorded there -- and the slabs k + 2 are prefetched.

    `with p.writing(out, box) as outp:`, inside the pass, is its output side: an _OutputStream on the same host thread
    that writes block k into slab k's box of `out`, the array-like of the ROI `box` (_roi_out).  The launches of slab k
    write into `outp.device(k)`, or work in place on the input buffer; `p.put(k)`, or `p.put(k, src)`, behind them hands
    the block over and sets `p.release_on`, so the host thread is given write(k) before read(k + 2)."""

    def __init__(self, volumes, boxes, chunk_bytes, rank, world_size, device, slabs=None, itemsize=1):
        check = _check_u8 if itemsize == 1 else _check_16
        for v in volumes:
            check(v)
        self.slabs = hist_chunks(boxes[0], chunk_bytes, rank, world_size, itemsize) if slabs is None else list(slabs)
        self.dims = [tuple(hi - lo for lo, hi in s) for s in self.slabs]
        self.nbytes = [int(np.prod(d)) * itemsize for d in self.dims]
        self.views = [np.dtype(np.uint8) if itemsize == 1 else np.dtype(v.dtype) for v in volumes]
        self.volumes = [_OneSection(v) if len(v.shape) == 2 else v for v in volumes]
        self.shifts = [tuple(b[0] - a[0] for a, b in zip(boxes[0], box)) for box in boxes]
        self.device, self.st = device, {"read_s": 0.0, "chunks": len(self.slabs)}

    def _reader(self, vol, shift, view=np.dtype(np.uint8)):
        slabs, dims = self.slabs, self.dims         # not `self`: the streams, which the pass holds, must not hold it

        def read_into(k, flat):                     # the buffers are bytes; a 16-bit slab is written through a view
            (z0, z1), (y0, y1), (x0, x1) = (tuple(v + o for v in r) for r, o in zip(slabs[k], shift))
            flat.view(view).reshape(dims[k])[...] = vol[z0:z1, y0:y1, x0:x1]
        return read_into

    @contextlib.contextmanager
    def streaming(self, stats=None):
        dev = self.dev = (torch.device("cuda", torch.cuda.current_device()) if self.device is None else
                          torch.device(self.device))
        self.pool = ThreadPoolExecutor(max_workers=1)            # one reader thread, however many volumes
        with torch.cuda.device(dev), contextlib.ExitStack() as stack:
            self.compute = torch.cuda.current_stream(dev)
            self.inputs = [stack.enter_context(_InputStream(self.nbytes, self._reader(v, o, w), dev, self.pool, self.st))
                           for v, o, w in zip(self.volumes, self.shifts, self.views)]
            yield self
        if stats is not None:                                    # a clean end: the thread is done with `st`
            stats.update(self.st)

    @contextlib.contextmanager
    def writing(self, out, box, out_slabs=None, own_buffers=True):
        """The output side: block k goes into the box out_slabs[k] (default: the pass's own slab k; else the cores or
        output slabs, in the coordinates of `box`) of `out`, whose origin is the ROI `box`'s; one image [y, x] is
        written as a one-section stack.  With `own_buffers` the stream holds the device buffers that the launches write
        into; without, put() copies out of the input buffer.  `st` gains the write seconds `write_s`."""
        slabs = self.slabs if out_slabs is None else list(out_slabs)
        dims = [tuple(hi - lo for lo, hi in s) for s in slabs]
        origin = tuple(lo for lo, _ in box)
        dst = _OneSection(out) if len(out.shape) == 2 else out
        self.st["write_s"] = 0.0

        def write_from(k, flat):                    # host thread; like _reader's closure it does not hold `self`
            (z0, z1), (y0, y1), (x0, x1) = (tuple(v - o for v in r) for r, o in zip(slabs[k], origin))
            dst[z0:z1, y0:y1, x0:x1] = flat.reshape(dims[k])

        with _OutputStream([int(np.prod(d)) for d in dims], write_from, self.dev, self.pool, self.st,
                           own_buffers=own_buffers) as self.outp:        # the reader's thread: write(k), read(k + 2)
            yield self.outp

    def put(self, k, src=None):
        """Behind slab k's launches: queue the D2H and the write of block k, and say when the input buffers are free.
        Out of the stream's own buffer that is behind the kernel; out of `src`, a view of the input buffer that the
        launches worked on in place, once the D2H has read it."""
        ready = self.compute.record_event()
        copied = self.outp.put(k, ready, src)
        self.release_on = ready if src is None else copied

    def __iter__(self):
        for k, (slab, dims) in enumerate(zip(self.slabs, self.dims)):
            self.release_on = None
            yield k, slab, dims, [inp.get(k) for inp in self.inputs]
            done = self.release_on or self.compute.record_event()    # counted
            for inp in self.inputs:
                inp.release(k, done)
            for inp in self.inputs:
                inp.prefetch(k + 2)


class _RowAccumulator:
    """The device accumulator of a pass that sums into `rows` rows of `shape` elements each -- a row per section, per
    section of the ROI, per pair -- of `dtype`: np.int64, or np.uint32, which the kernels add into as int32.  Made inside
    `p.streaming()`.  Where the whole table is at most CLAHE_ACC_BYTES (the module's value at that moment) it lives on
    `dev` and is read back once; else the device holds `most` rows, the most that one slab touches, zeroed ahead of
    every slab, read back behind it and added on the host.  Per slab, whose rows are [r0, r1): the launch adds at
    `ptr(r0, r1)`, and `add(r0, r1)` follows it; `result()` is the table, np `dtype` [rows, *shape]."""

    def __init__(self, dev, rows, shape, most, dtype=np.int64):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.row_bytes = int(np.prod(shape)) * self.dtype.itemsize
        self.whole = rows * self.row_bytes <= CLAHE_ACC_BYTES
        self.out = None if self.whole else np.zeros((rows,) + self.shape, self.dtype)
        self.acc = torch.zeros((rows if self.whole else most, int(np.prod(shape))), device=dev,
                               dtype=torch.int64 if self.dtype == np.int64 else torch.int32)

    def _host(self, rows):
        return rows.cpu().numpy().view(self.dtype).reshape((rows.shape[0],) + self.shape)

    def ptr(self, r0, r1):
        if self.whole:
            return self.acc.data_ptr() + self.row_bytes * r0
        self.acc[:r1 - r0].zero_()
        return self.acc.data_ptr()

    def add(self, r0, r1):
        if not self.whole:                                       # this slab's rows, added on the host
            self.out[r0:r1] += self._host(self.acc[:r1 - r0])

    def result(self):
        return self._host(self.acc) if self.whole else self.out  # the one read-back


def _most_rows(spans):
    """The `most` of a _RowAccumulator: the longest of the row ranges (r0, r1) of this rank's slabs, 1 without any."""
    return max((r1 - r0 for r0, r1 in spans), default=1)


def _roi_out(out, box, one, any_dtype=False):
    """The `out` of a pass that writes the ROI `box`: a writable uint8 array-like of the box's shape -- [y, x] for `one`
    image; with `any_dtype` the shape alone is checked --, allocated when None.  ValueError otherwise."""
    shape = tuple(hi - lo for lo, hi in box)
    want = shape[1:] if one else shape
    if out is None:
        return np.zeros(want, np.uint8)
    dtype = getattr(out, "dtype", None)
    if tuple(out.shape) != want or not (any_dtype or dtype == np.uint8):
        raise ValueError(f"out must be {'' if any_dtype else 'uint8 '}of the ROI's shape {want}, got {dtype} "
                         f"{tuple(out.shape)}")
    return out


def volume_histogram(volume, start=None, size=None, per_section=False, chunk_bytes=None, rank=0, world_size=1,
                     device=None, stats=None):
    """Intensity histogram of the ROI [start, start + size) ((x, y, z) order; default: the whole volume) of a uint8
    array-like `volume` indexed [z, y, x] (ndarray, np.memmap, h5py / zarr dataset: `.shape` and basic slicing are all
    it needs), or of one image [y, x] with 2-element start / size.  Returns np.int64[256], or with per_section
    np.int64[size_z, 256] whose row i counts section start_z + i.  The ROI must lie inside the volume: ValueError
    otherwise, before any GPU work.

    Out of core, through the input side of predict_volume's pipeline: the ROI is cut into slabs of at most
    `chunk_bytes` (hist_chunks); one host thread reads each slab into double-buffered pinned memory -> H2D on a copy
    stream -> tem_u8_hist on the compute stream, adding into ONE device accumulator that is read back once at the end.
    The pass is bound by the read (`stats` receives the read seconds `read_s` and the slab count `chunks`).  Ranks
    (rank / world_size) take slabs round-robin: each returns the counts of its own slabs, the ranks' results add up to
    the whole, and no collective is used."""
    box = hist_box(volume.shape, start, size)
    p = _SlabPass([volume], [box], chunk_bytes, rank, world_size, device)
    lib = H.require_gpu()
    with p.streaming(stats):
        acc = torch.zeros((box[0][1] - box[0][0] if per_section else 1, 256), dtype=torch.int64, device=p.dev)
        for k, slab, d, (src,) in p:
            row = (slab[0][0] - box[0][0]) if per_section else 0
            _lib.check(lib.tem_u8_hist(src.data_ptr(), *d, 0, d[0], 0, d[1], 0, d[2], acc.data_ptr() + 2048 * row,
                                       int(bool(per_section)), p.compute.cuda_stream), "tem_u8_hist")
        out = acc.cpu().numpy()                              # the one read-back
    return out if per_section else out[0]


def volume_joint_histogram(a, b, start=None, size=None, b_start=None, chunk_bytes=None, rank=0, world_size=1,
                           device=None, stats=None):
    """Joint histogram of two uint8 array-likes `a` and `b` indexed [z, y, x] (ndarray, np.memmap, h5py / zarr dataset;
    they may differ in shape), or of two images [y, x] with 2-element arguments: np.int64[256, 256] with J[u, v] the
    number of voxels p of the ROI with a[start + p] == u and b[b_start + p] == v.  The ROI is [start, start + size) of
    `a` ((x, y, z) order; default: all of `a`) against [b_start, b_start + size) of `b` (b_start=None: the same start).
    Both boxes must lie inside their volumes (hist_box's rule): ValueError otherwise, as for a dtype other than uint8,
    before any GPU work.  compare_from_joint turns the table into RMSE, MAE, PSNR, correlation and mutual
    information, regression_lut into the paired intensity map.

    Out of core exactly as volume_histogram: the ROI is cut into slabs of at most `chunk_bytes` per volume
    (hist_chunks on a's box; b's slab is the same box shifted), one host thread reads both slabs of a pair into
    double-buffered pinned memory (two _InputStreams, two pinned and two device buffers each) -> H2D on copy streams ->
    tem_u8_hist2 on the compute stream, adding into ONE device accumulator that is read back once at the end.  `stats`
    receives the read seconds `read_s` and the slab count `chunks`.  Ranks (rank / world_size) take slabs round-robin:
    each returns the counts of its own slabs, the ranks' results add up to the whole, and no collective is used."""
    box = hist_box(a.shape, start, size)
    nd = len(a.shape)
    extent = tuple(hi - lo for lo, hi in reversed(box))[:nd]             # (x, y[, z])
    box_b = hist_box(b.shape, tuple(lo for lo, _ in reversed(box))[:nd] if b_start is None else b_start, extent)
    p = _SlabPass([a, b], [box, box_b], chunk_bytes, rank, world_size, device)
    lib = H.require_gpu()
    with p.streaming(stats):
        measure = _Measure(lib, False, True, p.dev, p.compute.cuda_stream)
        for k, slab, d, (pa, pb) in p:
            measure.add(pb.data_ptr(), d, d, gt=(pa.data_ptr(), d, (0, 0, 0)))
        res = {}
        measure.report(res)                                      # the one read-back
    return res["joint_histogram"]


def _check_joint(J, who):
    J = np.asarray(J)
    if J.shape != (256, 256) or J.dtype.kind not in "iu":
        raise ValueError(f"{who}: a joint histogram is integer counts of shape [256, 256], got {J.dtype} {J.shape}")
    if int(J.min()) < 0:
        raise ValueError(f"{who}: the joint histogram has negative counts")
    if not J.any():
        raise ValueError(f"{who}: the joint histogram is empty")
    return J


def _entropy_bits(counts, n):
    p = counts[counts > 0].astype(np.float64) / n
    return float(-(p * np.log2(p)).sum())


def compare_from_joint(J):
    """What a joint histogram J[u, v] (np integer [256, 256]: volume_joint_histogram(a, b), or stats["joint_histogram"]
    of predict_cube / predict_volume(compare=gt) with u = ground truth, v = prediction) says about the pair, as a dict.
    The sums are exact Python integers; every float is derived from them once, in float64:
        n                                   voxels counted
        sum_abs_diff, sum_sq_diff           sum of |v - u| and of (v - u)^2 (integers)
        mae, rmse, bias                     sum_abs_diff / n, sqrt(sum_sq_diff / n), mean of v - u
        psnr                                20 log10(255 / rmse) in dB; inf when the volumes are equal
        rmse_scaled                         rmse / 127.5: debug.accuracy of the two volumes as scaled tensors
                                            v / 127.5 - 1, the reference's metric
        pearson                             the correlation coefficient; nan when either side is constant
        entropy_a, entropy_b, mutual_information    in bits; H(a) + H(b) - H(a, b), not below 0
        hist_a, hist_b                      the marginals J.sum(1) and J.sum(0) (np.int64[256])
    ValueError for another shape or dtype kind, a negative count or an empty table."""
    import math
    J = _check_joint(J, "compare_from_joint").astype(np.int64)
    hist_a, hist_b = J.sum(axis=1), J.sum(axis=0)
    n = int(hist_a.sum())
    diag = {k: int(np.trace(J, offset=k)) for k in range(-255, 256)}     # voxels with v - u == k
    sum_abs = sum(abs(k) * c for k, c in diag.items())
    sum_sq = sum(k * k * c for k, c in diag.items())
    su = sum(u * int(c) for u, c in enumerate(hist_a))
    sv = sum(v * int(c) for v, c in enumerate(hist_b))
    suu = sum(u * u * int(c) for u, c in enumerate(hist_a))
    svv = sum(v * v * int(c) for v, c in enumerate(hist_b))
    suv = sum(u * int(c) for u, c in enumerate(J @ np.arange(256, dtype=np.int64)))
    var_a, var_b, cov = n * suu - su * su, n * svv - sv * sv, n * suv - su * sv       # each times n^2
    rmse = math.sqrt(sum_sq / n)
    h_a, h_b, h_ab = _entropy_bits(hist_a, n), _entropy_bits(hist_b, n), _entropy_bits(J.ravel(), n)
    return {"n": n, "sum_abs_diff": sum_abs, "sum_sq_diff": sum_sq, "mae": sum_abs / n, "rmse": rmse,
            "bias": (sv - su) / n, "psnr": math.inf if sum_sq == 0 else 20.0 * math.log10(255.0 / rmse),
            "rmse_scaled": rmse / 127.5,
            "pearson": math.nan if var_a == 0 or var_b == 0 else cov / math.sqrt(var_a * var_b),
            "entropy_a": h_a, "entropy_b": h_b, "mutual_information": max(h_a + h_b - h_ab, 0.0),
            "hist_a": hist_a, "hist_b": hist_b}


def regression_lut(J):
    """The paired intensity map of a joint histogram J[u, v] of (a, b) -- volume_joint_histogram(a, b), in that order of
    the arguments -- as a lookup table: np.uint8[256] with t[u] = the mean of b over the voxels where a == u, rounded
    half up in integers, (2 sum_v v J[u, v] + n_u) // (2 n_u).  A value u that never occurs in `a` takes the entry of
    the nearest value that does, the lower one on a tie.  The result is a table for `lut=` of predict_cube /
    predict_volume (and tem_u8_lut): applied to `a` it gives the least-squares estimate of `b` from a's intensities
    alone; to map b towards a, pass the transposed table J.T.  ValueError as compare_from_joint."""
    J = _check_joint(J, "regression_lut").astype(np.int64)
    n_u = [int(c) for c in J.sum(axis=1)]
    s_u = [int(c) for c in J @ np.arange(256, dtype=np.int64)]
    seen = [u for u in range(256) if n_u[u]]
    t = np.zeros(256, np.uint8)
    for u in range(256):
        w = min(seen, key=lambda s: (abs(s - u), s))
        t[u] = (2 * s_u[w] + n_u[w]) // (2 * n_u[w])
    return t


SSIM_Q = 1 << 30                 # tem_u8_ssim's fixed point: q = rint(x * 2^30)


class SsimSums(NamedTuple):
    """volume_ssim's result: `sums` np.int64[Zw, 3] with the sums of q_s, q_l, q_cs (SSIM, luminance, contrast-structure,
    each rint(x * 2^30)) over the windows whose first section is the row's, `windows` the number of windows per
    window-section (Yw * Xw), `win` the window (wz, wy, wx)."""
    sums: np.ndarray
    windows: int
    win: tuple


def _ssim_window(win, flat):
    """(wz, wy, wx) of the in-plane edge `win` (odd, 3...11); ValueError otherwise."""
    import operator
    try:
        if isinstance(win, (bool, np.bool_)):
            raise TypeError
        w = operator.index(win)
    except TypeError:
        raise ValueError(f"win must be an odd integer in 3...11, got {win!r}")
    if w < 3 or w > 11 or w % 2 == 0:
        raise ValueError(f"win must be an odd integer in 3...11, got {win!r}")
    return (1 if flat else w), w, w


def ssim_chunks(box, win=7, flat=False, chunk_bytes=None, rank=0, world_size=1):
    """Cut the windows of the (z, y, x) (lo, hi) voxel `box` into slabs for volume_ssim.  Windows are wz x win x win
    voxels (wz = 1 if flat else win), lie wholly inside the box and are named by their first voxel: the window box is
    the voxel box less (wz - 1, win - 1, win - 1) at the high end.  Returns this rank's list of (window_slab, read_slab),
    both (z, y, x) (lo, hi) boxes in the box's coordinates: the window slabs are disjoint and their union is the window
    box; a read slab is the voxels its windows cover, the window slab extended by (wz - 1, win - 1) at the high end of
    z and y, over the box's full x extent -- x is never cut -- so neighbouring read slabs overlap by the window.  A
    read slab holds at most `chunk_bytes` bytes (HIST_CHUNK_BYTES when None): runs of whole window-sections, or, where
    wz sections of the box are larger than the budget, runs of whole rows of windows of one window-section (one row at
    the least: where wz x win x nx bytes exceed the budget, every slab is one row of windows).  Slabs are in (z, y)
    order and go round-robin to the ranks.  A box in which no window fits gives [].  Pure host function; ValueError as
    hist_chunks, and for a `win` that is not odd or outside 3...11."""
    wz, wy, wx = _ssim_window(win, flat)
    budget = _budget(chunk_bytes, rank, world_size)
    (z0, z1), (y0, y1), (x0, x1) = box
    ny, nx = y1 - y0, x1 - x0
    zw1, yw1, xw1 = z1 - wz + 1, y1 - wy + 1, x1 - wx + 1                # the window box's high ends
    if zw1 <= z0 or yw1 <= y0 or xw1 <= x0:
        return []
    if wz * ny * nx <= budget:
        kz = budget // (ny * nx) - (wz - 1)                              # window-sections per slab
        wins = [((z, min(z + kz, zw1)), (y0, yw1)) for z in range(z0, zw1, kz)]
    else:
        ky = max(1, budget // (wz * nx) - (wy - 1))                      # rows of windows per slab
        wins = [((z, z + 1), (y, min(y + ky, yw1))) for z in range(z0, zw1) for y in range(y0, yw1, ky)]
    slabs = [((wz_, wy_, (x0, xw1)), ((wz_[0], wz_[1] + wz - 1), (wy_[0], wy_[1] + wy - 1), (x0, x1))) for wz_, wy_ in wins]
    return slabs[rank::world_size]


def volume_ssim(a, b, start=None, size=None, b_start=None, win=7, flat=False, map_out=None, chunk_bytes=None, rank=0,
                world_size=1, device=None, stats=None):
    """Windowed structural similarity (SSIM) of two uint8 array-likes `a` and `b` indexed [z, y, x] (ndarray, np.memmap,
    h5py / zarr dataset; they may differ in shape), or of two images [y, x] with 2-element arguments, as an SsimSums;
    ssim_from_sums turns it into the index.  It is the structural companion of volume_joint_histogram, whose measures
    are blind to where a voxel is.  The ROI is volume_joint_histogram's: [start, start + size) of `a` ((x, y, z) order;
    default: all of `a`) against [b_start, b_start + size) of `b` (b_start=None: the same start), both inside their
    volumes.

    Windows are uniform boxes of wz x win x win voxels, `win` odd in 3...11; wz = win, or 1 with flat=True: section by
    section, for 2-D models, anisotropic stacks and images (always flat).  Only windows wholly inside the ROI count --
    the set skimage's structural_similarity averages after cropping its border -- so the window box is
    (Zw, Yw, Xw) = (nz - wz + 1, ny - win + 1, nx - win + 1).  Per window the value is Wang's SSIM with skimage's
    defaults (uniform window, sample covariance, data range 255, K1 = 0.01, K2 = 0.03) from integer window sums, as two
    correctly rounded float64 divisions, and enters as q = rint(x * 2^30) (include/tem_hip.h has the formula): the
    sums are integers and do not depend on slab cuts, launch geometry or ranks.

    Out of core as volume_joint_histogram, over read slabs that overlap by the window (ssim_chunks on a's box; b's slab
    is the same box shifted): one host thread reads both slabs of a pair into double-buffered pinned memory (two
    _InputStreams) -> H2D on copy streams -> tem_u8_ssim on the compute stream, adding into ONE device accumulator that
    is read back once.  `map_out`, a writable uint8 array-like of the window box's shape ([Yw, Xw] for images), receives
    the SSIM map: (255 max(q_s, 0) + 2^29) >> 30 per window, at the window's first voxel; each slab's map goes through
    an _OutputStream with device buffers of its own into the slab's box of map_out, on the reader's thread in
    clahe_volume's order, write(k) then read(k + 2).  Ranks (rank / world_size) take slabs round-robin: each returns the
    sums of its own slabs, the ranks' `sums` add to the whole, no collective is used, and the ranks write disjoint
    boxes of a shared map_out.  `stats` receives `read_s`, `chunks`, and `write_s` when a map is written.

    There is no ssim= keyword on predict_cube / predict_volume: a streamed chunk does not hold its neighbours'
    prediction, which the windows across its faces need.  Call volume_ssim(gt, out) on the finished output.

    ValueError, before any GPU work: a side that is not uint8, an ROI outside either volume, `win` even or outside
    3...11, an ROI in which no window fits, a map_out of another shape or dtype."""
    one = len(a.shape) == 2
    wz, wy, wx = _ssim_window(win, flat or one)
    box = hist_box(a.shape, start, size)
    nd = len(a.shape)
    extent = tuple(hi - lo for lo, hi in reversed(box))[:nd]             # (x, y[, z])
    box_b = hist_box(b.shape, tuple(lo for lo, _ in reversed(box))[:nd] if b_start is None else b_start, extent)
    wshape = tuple(hi - lo - w + 1 for (lo, hi), w in zip(box, (wz, wy, wx)))
    if min(wshape) < 1:
        raise ValueError(f"no {wz} x {wy} x {wx} window fits the ROI of {tuple(hi - lo for lo, hi in box)} voxels (z, y, x)")
    chunks = ssim_chunks(box, wy, wz == 1, chunk_bytes, rank, world_size)
    p = _SlabPass([a, b], [box, box_b], chunk_bytes, rank, world_size, device, slabs=[read for _, read in chunks])
    if map_out is not None:
        want = wshape[1:] if one else wshape
        if tuple(map_out.shape) != want or getattr(map_out, "dtype", None) != np.uint8:
            raise ValueError(f"map_out must be uint8 of the window box's shape {want}, got "
                             f"{getattr(map_out, 'dtype', None)} {tuple(map_out.shape)}")
    lib = H.require_gpu()
    wslabs = [w for w, _ in chunks]
    with p.streaming(stats):
        acc = torch.zeros((wshape[0], 3), dtype=torch.int64, device=p.dev)
        with contextlib.ExitStack() as stack:
            outp = None if map_out is None else stack.enter_context(p.writing(map_out, box, wslabs))
            for k, slab, d, (pa, pb) in p:
                mp = outp.device(k).data_ptr() if outp is not None else None
                _lib.check(lib.tem_u8_ssim(pa.data_ptr(), *d, 0, 0, 0, pb.data_ptr(), *d, 0, 0, 0, *d, wy, int(wz == 1),
                                           acc.data_ptr() + 24 * (wslabs[k][0][0] - box[0][0]), mp,
                                           p.compute.cuda_stream), "tem_u8_ssim")
                if outp is not None:
                    p.put(k)
        sums = acc.cpu().numpy()                                         # the one read-back
    return SsimSums(sums, wshape[1] * wshape[2], (wz, wy, wx))


def ssim_from_sums(s):
    """What an SsimSums (volume_ssim's, or one whose `sums` are the element-wise sum of several ranks') says, as a dict.
    The totals are exact Python integers; every float is derived from them once, in float64:
        n                                   windows counted
        ssim, luminance, contrast_structure the mean over all windows of s, l and cs: total / (n 2^30)
        per_section                         np.float64[Zw, 3]: the same three per window-section, the profile along z
    ValueError for `sums` of another shape or dtype kind, a `windows` below 1, and a row whose magnitude exceeds
    windows * 2^30 (no window's s, l or cs lies outside [-1, 1])."""
    try:
        sums, windows, win = s
        sums = np.asarray(sums)
    except (TypeError, ValueError):
        raise ValueError(f"ssim_from_sums takes an SsimSums (sums, windows, win), got {type(s).__name__}")
    if sums.ndim != 2 or sums.shape[1] != 3 or sums.shape[0] < 1 or sums.dtype.kind not in "iu":
        raise ValueError(f"ssim_from_sums: sums must be integers of shape [Zw, 3], got {sums.dtype} {sums.shape}")
    windows = int(windows)
    if windows < 1:
        raise ValueError(f"ssim_from_sums: windows must be positive, got {windows}")
    rows = [[int(v) for v in row] for row in sums]
    if any(abs(v) > windows * SSIM_Q for row in rows for v in row):
        raise ValueError(f"ssim_from_sums: a sum exceeds windows * 2^30 = {windows * SSIM_Q} in magnitude")
    n = windows * len(rows)
    total = [sum(row[i] for row in rows) / (n * SSIM_Q) for i in range(3)]
    per = np.array([[v / (windows * SSIM_Q) for v in row] for row in rows], np.float64)
    return {"n": n, "ssim": total[0], "luminance": total[1], "contrast_structure": total[2], "per_section": per}


RESCALE_MAX_PQ = 64              # tem_u8_rescale: 1 <= p, q <= 64 and 1/8 <= p / q <= 8 keep 2 S + Den below 2^31
RESCALE_MAX_STEP = 8


def _rescale_fraction(s):
    """One axis' step as a reduced Fraction p / q: an int, a Fraction or a (p, q) pair; ValueError otherwise, and for
    p or q outside 1...RESCALE_MAX_PQ or a step outside [1 / RESCALE_MAX_STEP, RESCALE_MAX_STEP]."""
    try:
        if isinstance(s, (bool, np.bool_, float, np.floating, str, bytes)):
            raise TypeError
        if isinstance(s, (tuple, list)):
            if len(s) != 2 or any(isinstance(v, (bool, float)) for v in s):
                raise TypeError
            f = Fraction(int(s[0]), int(s[1]))
        else:
            f = Fraction(s)
    except (TypeError, ValueError, ZeroDivisionError):
        raise ValueError(f"a step must be an int, a Fraction or a (p, q) pair of positive integers, got {s!r}")
    p, q = f.numerator, f.denominator
    if not (1 <= p <= RESCALE_MAX_PQ and 1 <= q <= RESCALE_MAX_PQ and q <= RESCALE_MAX_STEP * p and
            p <= RESCALE_MAX_STEP * q):
        raise ValueError(f"a step p / q needs 1 <= p, q <= {RESCALE_MAX_PQ} in lowest terms and 1/{RESCALE_MAX_STEP} <= "
                         f"p / q <= {RESCALE_MAX_STEP}, got {s!r}")
    return f


def _rescale_steps(step, nd):
    """`step` as `nd` reduced Fractions in (x, y[, z]) order: one step per axis, or one int or Fraction for all."""
    if isinstance(step, (int, np.integer, Fraction)) and not isinstance(step, (bool, np.bool_)):
        return (_rescale_fraction(step),) * nd
    if not isinstance(step, (tuple, list)) or len(step) != nd:
        raise ValueError(f"step must have {nd} elements in (x, y, z) order, or be one int or Fraction, got {step!r}")
    return tuple(_rescale_fraction(s) for s in step)


def rescale_step(src_size, dst_size):
    """The steps that bring a volume of voxel size `src_size` onto a grid of voxel size `dst_size`, both (x, y, z)
    (or (x, y)) in one unit, e.g. (4, 4, 40) and (8, 8, 8) nm: the tuple of reduced Fractions dst / src, the output
    voxel's edge in source voxels -- (2, 2, 1/5) there.  ValueError for a step volume_rescale does not take."""
    src, dst = tuple(src_size), tuple(dst_size)
    if len(src) != len(dst) or len(src) not in (2, 3):
        raise ValueError(f"voxel sizes must both be (x, y, z) or (x, y), got {src_size!r}, {dst_size!r}")
    try:
        steps = tuple(Fraction(d) / Fraction(s) for s, d in zip(src, dst))
    except (TypeError, ValueError, ZeroDivisionError):
        raise ValueError(f"voxel sizes must be positive integers or Fractions, got {src_size!r}, {dst_size!r}")
    return tuple(_rescale_fraction(f) for f in steps)


def rescale_shape(vol_shape, step):
    """The shape [z, y, x] (or [y, x]) of the output grid of a volume of shape `vol_shape` at `step` ((x, y, z) order,
    each an int, a Fraction or a (p, q) pair): ceil(n q / p) per axis."""
    shape = tuple(int(v) for v in vol_shape)
    if len(shape) not in (2, 3) or min(shape) < 1:
        raise ValueError(f"volume must be a non-empty [z, y, x] or one image [y, x], got shape {shape}")
    steps = _rescale_steps(step, len(shape))
    return tuple(-(-n * f.denominator // f.numerator) for n, f in zip(shape, reversed(steps)))


def _rescale_tap(j, n, p, q):
    """(first tap, weights, W) of output j of an axis of n source voxels at step p / q: the rule of rescale_taps."""
    if p >= q:
        lo, hi = j * p, min((j + 1) * p, n * q)
        first = lo // q
        return first, tuple(min((i + 1) * q, hi) - max(i * q, lo) for i in range(first, (hi - 1) // q + 1)), hi - lo
    C = (2 * j + 1) * p - q
    i0 = C // (2 * q)
    f = C - 2 * q * i0
    a, b = min(max(i0, 0), n - 1), min(max(i0 + 1, 0), n - 1)
    return (a, (2 * q,), 2 * q) if a == b or f == 0 else (a, (2 * q - f, f), 2 * q)


def rescale_taps(n, p, q):
    """The one host copy of tem_u8_rescale's rule for one axis of `n` source voxels at step p / q (reduced): a list
    with, per output voxel j < ceil(n q / p), (first, weights, W) -- the taps are source voxels first, first + 1, ...
    with those integer weights, and W is their sum.
      p >= q, the area average: in units of 1 / q source voxel j covers [j p, (j + 1) p) and voxel i [i q, (i + 1) q);
        a weight is the length of the overlap, over the voxels that exist; W = p, or less at the far face.
      p < q, linear between voxel centres: C = (2 j + 1) p - q, i0 = floor(C / 2 q), f = C - 2 q i0, taps
        (clamp(i0), 2 q - f) and (clamp(i0 + 1), f); W = 2 q.  Taps that clamp onto one voxel are given as one tap of
        weight 2 q, and a tap of weight 0 (f == 0) is dropped: every weight returned is positive.
    The voxel is (2 S + Den) // (2 Den) with S the sum over the tap product of the three axes and Den = Wz Wy Wx."""
    f = _rescale_fraction((p, q))
    if (f.numerator, f.denominator) != (p, q):
        raise ValueError(f"the step {p} / {q} is not in lowest terms")
    if n < 1:
        raise ValueError(f"an axis has at least one voxel, got {n}")
    return [_rescale_tap(j, n, p, q) for j in range(-(-n * q // p))]


def _rescale_hull(lo, hi, n, f):
    """The (lo, hi) source voxels that outputs [lo, hi) of an axis of n voxels at step f read."""
    first = _rescale_tap(lo, n, f.numerator, f.denominator)
    last = _rescale_tap(hi - 1, n, f.numerator, f.denominator)
    return first[0], last[0] + len(last[1])


def rescale_chunks(out_box, vol_shape, step, chunk_bytes=None, rank=0, world_size=1):
    """Cut the (z, y, x) (lo, hi) box `out_box` of the output grid of a volume of shape `vol_shape` [z, y, x] at `step`
    ((x, y, z) order) into slabs for volume_rescale.  Returns this rank's list of (output slab, read slab), (z, y, x)
    (lo, hi) boxes of the output grid and of the volume: the output slabs are disjoint and their union is the box; a
    read slab is the tight hull of its output slab's taps along z and y, over the volume's whole x extent -- x is never
    cut -- so neighbouring read slabs overlap by the taps they share.  Both slabs hold at most `chunk_bytes` bytes
    (HIST_CHUNK_BYTES when None): runs of whole output planes of the box, as many as fit, or, where one output plane or
    its hull is larger than the budget, runs of whole output rows of that plane (one row at the least).  Slabs are in
    (z, y) order and go round-robin to the ranks.  Pure host function; ValueError as hist_chunks, for a bad step and
    for a box outside the grid."""
    budget = _budget(chunk_bytes, rank, world_size)
    vol_shape = tuple(int(v) for v in vol_shape)
    if len(vol_shape) != 3:
        raise ValueError(f"rescale_chunks takes a volume shape [z, y, x], got {vol_shape}")
    grid = rescale_shape(vol_shape, step)
    fx, fy, fz = _rescale_steps(step, 3)
    (z0, z1), (y0, y1), (x0, x1) = out_box
    if any(lo < 0 or hi > n for (lo, hi), n in zip(out_box, grid)):
        raise ValueError(f"the box {tuple(out_box)} reaches outside the output grid of shape {grid}")
    VZ, VY, VX = vol_shape
    ny, nx = y1 - y0, x1 - x0
    if z1 <= z0 or ny <= 0 or nx <= 0:
        return []

    def fits(nz, rz, rows, ry):         # an output slab of nz planes of `rows` rows and its hull of rz planes of ry rows
        return nz * rows * nx <= budget and rz * ry * VX <= budget

    whole_y = _rescale_hull(y0, y1, VY, fy)
    slabs, z = [], z0
    while z < z1:
        lo, hi = _rescale_hull(z, z + 1, VZ, fz)
        if fits(1, hi - lo, ny, whole_y[1] - whole_y[0]):
            k = 1
            while z + k < z1:
                more = _rescale_hull(z, z + k + 1, VZ, fz)[1]
                if not fits(k + 1, more - lo, ny, whole_y[1] - whole_y[0]):
                    break
                k, hi = k + 1, more
            slabs.append((((z, z + k), (y0, y1), (x0, x1)), ((lo, hi), whole_y, (0, VX))))
            z += k
            continue
        y = y0
        while y < y1:
            ylo, yhi = _rescale_hull(y, y + 1, VY, fy)
            k = 1
            while y + k < y1:
                more = _rescale_hull(y, y + k + 1, VY, fy)[1]
                if not fits(1, hi - lo, k + 1, more - ylo):
                    break
                k, yhi = k + 1, more
            slabs.append((((z, z + 1), (y, y + k), (x0, x1)), ((lo, hi), (ylo, yhi), (0, VX))))
            y += k
        z += 1
    return slabs[rank::world_size]


def volume_rescale(volume, step, out=None, start=None, size=None, chunk_bytes=None, rank=0, world_size=1, device=None,
                   stats=None):
    """A uint8 array-like `volume` indexed [z, y, x] (ndarray, np.memmap, h5py / zarr dataset), or one image [y, x] with
    a 2-element step, brought onto a grid of another voxel size: the step between two EM domains that seldom share one
    (4 nm against 8 nm FIB-SEM; 4 x 4 x 40 nm ssTEM against 8 nm isotropic) -- once over a training volume ahead of
    volume3d_ng, over the input ahead of predict_volume, and the inverse step on the way back.  Intensities only: a
    label volume needs nearest or majority, which this is not.

    `step` holds one step per axis in (x, y, z) order, each an int, a Fraction or a (p, q) pair (or is one int or
    Fraction for every axis; rescale_step derives it from two voxel sizes): the output voxel's edge in source voxels,
    p / q in lowest terms with 1 <= p, q <= 64 and 1/8 <= p / q <= 8.  An axis of n voxels gives ceil(n q / p), anchored
    at voxel 0 (rescale_shape).  Where an axis shrinks the output is the area average over the source voxels it covers,
    those that exist (tem_u8_pool2's rule at step 2); where it grows, linear interpolation between voxel centres,
    clamped at the faces (scipy.ndimage.zoom(order=1, mode="nearest", grid_mode=True)).  The three axes' integer
    weights multiply, and the voxel is rounded once, half up: (2 S + Den) // (2 Den) -- rescale_taps has the rule,
    numpy reproduces it bit for bit, and a voxel does not depend on the slab, ROI or rank it was computed in.

    `start` / `size` are an ROI of the OUTPUT grid in (x, y, z) order (default: the whole grid); `out` is a writable
    uint8 array-like of the ROI's shape (allocated when None) and is returned.  Out of core as clahe_volume: the ROI is
    cut into output slabs and the read slabs that hold their taps (rescale_chunks), both at most `chunk_bytes`; host
    thread -> pinned -> H2D -> one tem_u8_rescale launch per slab -> D2H -> host write, on double buffers, in the order
    write(k), read(k + 2) on the one host thread.  Ranks (rank / world_size) take slabs round-robin and write disjoint
    boxes of a shared `out`.  `stats` receives `read_s`, `write_s` and `chunks`.

    There is no rescale= keyword on predict_cube / predict_volume: a rescaled chunk's footprint would need hull logic
    of its own inside chunk_plan.  Rescale, then predict.

    ValueError, before any GPU work: a volume that is not uint8, a bad step, an ROI outside the output grid, an `out` of
    another shape or dtype."""
    _check_u8(volume)
    vshape = tuple(int(v) for v in volume.shape)
    one = len(vshape) == 2
    grid = rescale_shape(vshape, step)
    steps = _rescale_steps(step, len(vshape)) + ((Fraction(1),) if one else ())      # (x, y, z)
    try:
        box = hist_box(grid, start, size)
    except ValueError as e:
        raise ValueError(f"volume_rescale: start / size are an ROI of the output grid of shape {grid}: {e}")
    out = _roi_out(out, box, one)
    vol3 = (1,) + vshape if one else vshape
    chunks = rescale_chunks(box, vol3, steps, chunk_bytes, rank, world_size)
    p = _SlabPass([volume], [hist_box(vshape)], chunk_bytes, rank, world_size, device, slabs=[r for _, r in chunks])
    lib = H.require_gpu()
    oslabs = [o for o, _ in chunks]
    pq = [v for f in reversed(steps) for v in (f.numerator, f.denominator)]          # pz, qz, py, qy, px, qx
    with p.streaming(stats), p.writing(out, box, oslabs) as outp:
        for k, slab, d, (src,) in p:
            _lib.check(lib.tem_u8_rescale(src.data_ptr(), *d, *(lo for lo, _ in slab), *vol3, *pq,
                                          outp.device(k).data_ptr(), *(hi - lo for lo, hi in oslabs[k]),
                                          *(lo for lo, _ in oslabs[k]), p.compute.cuda_stream), "tem_u8_rescale")
            p.put(k)
    return out


REPAIR_MAX_GAP = 32              # tem_u8_repair_z: 1 <= max_gap <= 32


class Repair(NamedTuple):
    """What the `repair=` keyword and volume_repair take: which voxels of a uint8 volume [z, y, x] are bad, and how far
    along z a good voxel may lie to fill them.  A voxel is bad if any source that is given says so:
      sections       an iterable of whole bad sections z (lost, black, folded, charged; flat_sections finds the blank ones)
      mask           a uint8 array-like of the volume's shape: bad where mask[z, y, x] != 0
      missing_value  one grey level in 0...255 that stands for "no data"
    and takes, with R = max_gap (1...32), the nearest good voxel of its own column (y, x) at most R sections below
    (value a, distance d0) and above (b, d1):
      both exist: (2 (a d1 + b d0) + n) // (2 n), n = d0 + d1 -- linear between the two, the nearer one weighted more,
      rounded half up; one exists: that value; neither: the voxel stays as it is.
    Good voxels are never changed and a bad voxel is never a source, so a voxel's result depends only on the sections
    [z - R, z + R] of its own column: not on the slab, chunk, ROI or rank it was computed in.  A run of up to R bad
    voxels between two good ones is interpolated throughout; a run longer than 2 R keeps an untouched middle
    (volume_repair counts those voxels)."""
    sections: object = None
    mask: object = None
    missing_value: object = None
    max_gap: int = 8


class _RepairSpec(NamedTuple):
    """_check_repair's result: `flags` np.uint8[Z] (1: a bad section) or None, `mask` the array-like or None, `missing`
    -1 or the grey level, `max_gap`."""
    flags: object
    mask: object
    missing: int
    max_gap: int


def _index(v, what):
    import operator
    try:
        if isinstance(v, (bool, np.bool_)):
            raise TypeError
        return operator.index(v)
    except TypeError:
        raise ValueError(f"{what} must be an integer, got {v!r}")


def _check_repair(repair, vol_shape):
    """None, or the _RepairSpec of `repair` (a Repair, or any (sections, mask, missing_value, max_gap) tuple) for a
    volume of shape `vol_shape` [z, y, x].  ValueError for: no source at all, max_gap outside 1...32, a section outside
    [0, Z), a mask of another shape or dtype, a missing_value outside 0...255, and a single image [y, x], which has no z
    to repair along."""
    if repair is None:
        return None
    if isinstance(repair, _RepairSpec):
        return repair
    try:
        sections, mask, missing, max_gap = repair
    except (TypeError, ValueError):
        raise ValueError(f"repair must be None or a Repair (sections, mask, missing_value, max_gap), got "
                         f"{type(repair).__name__}")
    shape = tuple(int(v) for v in vol_shape)
    if len(shape) != 3:
        raise ValueError(f"repair fills along z: it needs a volume [z, y, x], got shape {shape}")
    R = _index(max_gap, "max_gap")
    if not 1 <= R <= REPAIR_MAX_GAP:
        raise ValueError(f"max_gap must lie in 1...{REPAIR_MAX_GAP}, got {R}")
    if sections is None and mask is None and missing is None:
        raise ValueError("repair names no bad voxel: give sections, mask or missing_value")
    flags = None
    if sections is not None:
        try:
            zs = [_index(z, "a section") for z in sections]
        except TypeError:
            raise ValueError(f"sections must be an iterable of section indices, got {sections!r}")
        flags = np.zeros(shape[0], np.uint8)
        for z in zs:
            if not 0 <= z < shape[0]:
                raise ValueError(f"section {z} is outside [0, {shape[0]})")
            flags[z] = 1
    if mask is not None:
        mshape, dtype = getattr(mask, "shape", None), getattr(mask, "dtype", None)
        if mshape is None or dtype is None or dtype != np.uint8:
            raise ValueError(f"mask must be a uint8 array-like, got {type(mask).__name__} of dtype {dtype}")
        if tuple(int(v) for v in mshape) != shape:
            raise ValueError(f"mask must have the volume's shape {shape}, got {tuple(mshape)}")
    m = -1
    if missing is not None:
        m = _index(missing, "missing_value")
        if not 0 <= m <= 255:
            raise ValueError(f"missing_value must lie in 0...255, got {m}")
    return _RepairSpec(flags, mask, m, R)


def repair_chunks(box, vol_shape, max_gap, chunk_bytes=None, rank=0, world_size=1):
    """Cut the (z, y, x) (lo, hi) `box` of a volume of shape `vol_shape` [z, y, x] into slabs for volume_repair.  Returns
    this rank's list of (core slab, read slab), both (z, y, x) (lo, hi) boxes of the volume: the cores are disjoint and
    their union is the box (hist_chunks' cuts: runs of whole sections of the box, or runs of whole rows of one section;
    x is never cut); a read slab is its core extended by `max_gap` sections along z on each side and clipped to the
    volume, so neighbouring read slabs overlap.  A read slab holds at most `chunk_bytes` bytes (HIST_CHUNK_BYTES when
    None) wherever one core plane allows it: as many whole sections per core as fit next to the 2 max_gap around them,
    or, where 2 max_gap + 1 sections of the box are larger than the budget, one section's rows, as many as fit (one row
    at the least).  Slabs are in (z, y) order and go round-robin to the ranks.  Pure host function; ValueError as
    hist_chunks, and for a max_gap outside 1...32."""
    budget = _budget(chunk_bytes, rank, world_size)
    R = _index(max_gap, "max_gap")
    if not 1 <= R <= REPAIR_MAX_GAP:
        raise ValueError(f"max_gap must lie in 1...{REPAIR_MAX_GAP}, got {R}")
    return _cut_slabs(box, ((0, int(vol_shape[0])), box[1]), budget, rank, world_size, zreach=(R, R))


def volume_repair(volume, repair, out=None, start=None, size=None, chunk_bytes=None, stats=None, rank=0, world_size=1,
                  device=None):
    """The ROI [start, start + size) ((x, y, z) order; default: the whole volume) of a uint8 array-like `volume` [z, y, x]
    (ndarray, np.memmap, h5py / zarr dataset) with its damaged sections and voxels filled along z from the nearest good
    sections below and above, by the rule of `Repair` (a Repair of the WHOLE volume: its mask has the volume's shape),
    written into `out`: a writable uint8 array-like of the ROI's shape (allocated when None), which is returned.  This
    is how training volumes are prepared, ahead of clahe_fit and volume3d_ng, so that no crop teaches a loss to
    reproduce a defect; predict_*(repair=...) sees the same bytes without the copy.  Everything is integers and numpy
    reproduces it byte for byte; a voxel depends only on the sections [z - max_gap, z + max_gap] of its own column, so
    the result of an ROI is the ROI of the whole result, however it is cut.

    Out of core exactly like clahe_volume, over read slabs that overlap by max_gap sections (repair_chunks): one host
    thread reads each read slab -- and the mask's same box, through a second input stream, when there is a mask --
    into double-buffered pinned memory -> H2D -> one tem_u8_repair_z launch per slab, in place -> D2H of the core
    planes only, one contiguous range of the block -> host write, in the order write(k), read(k + 2) on the one host
    thread.  The section flags are uploaded once.  Ranks take slabs round-robin and write disjoint boxes of a shared
    `out`.  `stats` receives `read_s`, `write_s`, `chunks`, and `repaired` / `unrepaired`: the bad voxels of this
    rank's cores that were filled, and those left as they are because no good voxel lies within max_gap (the middle of
    a run longer than 2 max_gap); cores are disjoint, so the ranks' counts add.
    ValueError, before any GPU work: _check_repair's, an ROI outside the volume, a non-uint8 volume, an `out` of another
    shape or dtype."""
    _check_u8(volume)
    vshape = tuple(int(v) for v in volume.shape)
    rp = _check_repair(repair, vshape)
    if rp is None:
        raise ValueError("volume_repair needs a Repair")
    box = hist_box(vshape, start, size)
    out = _roi_out(out, box, False)
    chunks = repair_chunks(box, vshape, rp.max_gap, chunk_bytes, rank, world_size)
    whole = hist_box(vshape)
    vols = [volume] + ([rp.mask] if rp.mask is not None else [])
    p = _SlabPass(vols, [whole] * len(vols), chunk_bytes, rank, world_size, device, slabs=[r for _, r in chunks])
    lib = H.require_gpu()
    cores = [c for c, _ in chunks]
    with p.streaming(stats):
        prepare = _Prepare(lib, None, None, p.dev, p.compute.cuda_stream, repair=rp)     # the section flags, once
        counts = torch.zeros(2, dtype=torch.int64, device=p.dev)
        with p.writing(out, box, cores, own_buffers=False):
            for k, slab, d, bufs in p:
                c0, c1 = (v - slab[0][0] for v in cores[k][0])
                prepare.repair_block(bufs[0].data_ptr(), d, slab[0][0], c0, c1,
                                     bufs[1].data_ptr() if rp.mask is not None else None, counts.data_ptr())
                p.put(k, bufs[0][c0 * d[1] * d[2]:])     # the core planes: one contiguous range of the block
        p.st["repaired"], p.st["unrepaired"] = (int(v) for v in counts.cpu().numpy())    # the one read-back
    return out


def flat_sections(h, fraction=Fraction(1, 2)):
    """A first detector of lost sections, host only: the sorted list of the sections z of a per-section histogram `h`
    (np integer [Z, 256]: volume_histogram(..., per_section=True)) whose most frequent grey level holds at least
    `fraction` (an int, a Fraction or a (num, den) pair in (0, 1]) of their pixels, decided in integers:
    max(h[z]) den >= num sum(h[z]).  An empty section is not flagged.  Blank and saturated sections are what this
    finds -- the list is what Repair takes as `sections` --; find_defects finds the sections and tile-sized regions that
    resemble neither neighbour, find_debris the particles far smaller than a tile."""
    h = np.asarray(h)
    if h.ndim != 2 or h.shape[1] != 256 or h.dtype.kind not in "iu":
        raise ValueError(f"flat_sections: h must be integer counts of shape [Z, 256], got {h.dtype} {h.shape}")
    if h.size and int(h.min()) < 0:
        raise ValueError("flat_sections: h has negative counts")
    try:
        if isinstance(fraction, (bool, np.bool_, float, np.floating, str, bytes)):
            raise TypeError
        f = Fraction(int(fraction[0]), int(fraction[1])) if isinstance(fraction, (tuple, list)) else Fraction(fraction)
    except (TypeError, ValueError, ZeroDivisionError, IndexError):
        raise ValueError(f"fraction must be an int, a Fraction or a (num, den) pair, got {fraction!r}")
    if not 0 < f <= 1:
        raise ValueError(f"fraction must lie in (0, 1], got {fraction!r}")
    num, den = f.numerator, f.denominator
    out = []
    for z, row in enumerate(h):
        top, total = int(row.max()), sum(int(c) for c in row)
        if total > 0 and top * den >= num * total:
            out.append(z)
    return out


def zcorr_chunks(vol_shape, chunk_bytes=None, rank=0, world_size=1):
    """Cut a volume of shape `vol_shape` [z, y, x] (one image [y, x]: one section) into slabs for section_sums.  Returns
    this rank's list of (core slab, read slab), both (z, y, x) (lo, hi) boxes: the cores are disjoint and their union is
    the volume (hist_chunks' cuts: runs of whole sections, or runs of whole rows of one section; x is never cut); a read
    slab is its core plus the same rows of the next section where the volume has one -- the plane its last core plane
    is correlated with.  A read slab holds at most `chunk_bytes` bytes (HIST_CHUNK_BYTES when None) wherever one row
    allows it: as many whole sections per core as fit next to the one above them, or, where two sections are larger
    than the budget, one section's rows, as many as fit twice (one row at the least).  Slabs are in (z, y) order and go
    round-robin to the ranks.  Pure host function; ValueError as hist_box and hist_chunks."""
    return _zhalo_chunks(vol_shape, 1, chunk_bytes, rank, world_size)


def _zhalo_chunks(vol_shape, reach, chunk_bytes, rank, world_size):
    """zcorr_chunks' cuts with read slabs that reach `reach` sections past their core, where the volume has them."""
    budget = _budget(chunk_bytes, rank, world_size)
    box = hist_box(vol_shape)
    return _cut_slabs(box, box[:2], budget, rank, world_size, zreach=(0, min(reach, box[0][1] - 1)))


def section_sums(volume, tile=128, chunk_bytes=None, rank=0, world_size=1, device=None, stats=None):
    """The sums behind the correlation of every tile of a section with the same tile one section up: np.int64
    [Z, gy, gx, 4] over the WHOLE uint8 `volume` [z, y, x] (ndarray, np.memmap, h5py / zarr dataset; one image [y, x]:
    Z = 1) on clahe_grid's tiles of `tile` pixels (an int or (th, tw) in [1, 2048]).  With v the voxels of tile (i, j) of
    section z and v+ those one section up:
      s[z, i, j] = (sum v, sum v v, sum v v+, the number of voxels);   the last section's sum v v+ is 0.
    Exact integers that numpy reproduces bit for bit, whatever the slabs, ranks and launches.  section_scores turns
    them into correlations, find_defects into the sections and regions that resemble neither neighbour.

    Out of core exactly as clahe_histograms, over read slabs that reach one section past their core (zcorr_chunks): one
    host thread -> pinned -> H2D -> one tem_u8_zcorr_tiles launch per slab, adding into a device accumulator.  The
    accumulator holds the whole volume's Z*gy*gx*32 bytes and is read back once where that is at most CLAHE_ACC_BYTES;
    else it holds one slab's core sections and is read back, and added on the host, per slab.  Ranks take slabs
    round-robin and their results add up to the whole.  `stats` receives `read_s` and `chunks`.  ValueError, before any
    GPU work: a non-uint8 volume, a bad tile, shape, chunk_bytes or rank."""
    _check_u8(volume)
    th, tw = _clahe_tile(tile)
    gy, gx = clahe_grid(volume.shape, (th, tw))
    box = hist_box(volume.shape)
    chunks = zcorr_chunks(volume.shape, chunk_bytes, rank, world_size)
    p = _SlabPass([volume], [box], chunk_bytes, rank, world_size, device, slabs=[r for _, r in chunks])
    lib = H.require_gpu()
    with p.streaming(stats):
        acc = _RowAccumulator(p.dev, box[0][1], (gy, gx, 4), _most_rows(c[0] for c, _ in chunks))
        for k, ((r0, _), (y0, _), (x0, _)), d, (src,) in p:
            z0, z1 = chunks[k][0][0]
            _lib.check(lib.tem_u8_zcorr_tiles(src.data_ptr(), *d, z0 - r0, z1 - r0, y0, x0, th, tw, gy, gx,
                                              acc.ptr(z0, z1), p.compute.cuda_stream), "tem_u8_zcorr_tiles")
            acc.add(z0, z1)
        return acc.result()


def _check_sums(s, who):
    s = np.asarray(s)
    if s.ndim != 4 or s.shape[3] != 4 or s.dtype.kind not in "iu":
        raise ValueError(f"{who}: s must be section_sums' integer array [Z, gy, gx, 4], got {s.dtype} {s.shape}")
    return s.astype(np.int64, copy=False)


def section_scores(s):
    """float64 c[Z - 1, gy, gx]: the Pearson correlation of every tile of section z with the same tile of section z + 1,
    from section_sums' `s`.  Host only.  Per tile, with n = s[..., 3], S1 = s[..., 0], S2 = s[..., 1], S12 = s[..., 2]:
      A = n S2[z] - S1[z]^2,   B = the same at z + 1,   N = n S12[z] - S1[z] S1[z + 1]
    -- exact in int64: a tile holds at most 2^22 voxels of at most 255, so every term stays below 2^61 -- and
    c = N / (sqrt(A) sqrt(B)) where A > 0 and B > 0, else 0.0: a constant tile correlates with nothing."""
    s = _check_sums(s, "section_scores")
    Z = s.shape[0]
    c = np.zeros((max(Z - 1, 0),) + s.shape[1:3], np.float64)
    if Z < 2:
        return c
    n, S1, S2, S12 = (s[..., q] for q in (3, 0, 1, 2))
    var = n * S2 - S1 * S1
    A, B = var[:-1], var[1:]
    N = n[:-1] * S12[:-1] - S1[:-1] * S1[1:]
    ok = (A > 0) & (B > 0)
    c[ok] = N[ok] / (np.sqrt(A[ok].astype(np.float64)) * np.sqrt(B[ok].astype(np.float64)))
    return c


class Defects(NamedTuple):
    """find_defects' verdict: `sections` the sorted list of bad sections, `tiles` bool[Z, gy, gx] the bad tiles of the
    other sections, `undecided` bool[gy, gx] the tile columns without a verdict, `scores` float64[Z, gy, gx] what it was
    decided on."""
    sections: list
    tiles: np.ndarray
    undecided: np.ndarray
    scores: np.ndarray


def _unit(v, what, closed):
    try:
        if isinstance(v, (bool, np.bool_, str, bytes)):
            raise TypeError
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a number, got {v!r}")
    if not (0 < f <= 1 if closed else 0 < f < 1):
        raise ValueError(f"{what} must lie in (0, 1{']' if closed else ')'}, got {v!r}")
    return f


def find_defects(s, ratio=0.5, min_corr=0.1, section_fraction=0.5):
    """The sections and regions of a volume that resemble neither the section below nor the section above -- charging
    noise, a fold or a tear, a section from the wrong place, a blank one -- from section_sums' `s`.  Host only.  With
    c = section_scores(s):
      scores     t[z, i, j] = the larger of c[z - 1, i, j] and c[z, i, j] that exist: a tile is suspect only if it
                 resembles NEITHER neighbour, so a clean cut in the data (two good halves) flags nothing
      med[i, j]  = np.median(c[:, i, j]): what "resembles" means for this column of tiles
      undecided  med <= min_corr: resin, or nothing to correlate -- no verdict for this column
      bad        decided and t < ratio med
      sections   the sorted list of sections whose bad tiles are at least `section_fraction` of the decided tiles
      tiles      bool[Z, gy, gx]: the bad tiles of the other sections
    Z < 2 gives no verdict anywhere (every column undecided).  `ratio` and `section_fraction` lie in (0, 1], `min_corr`
    in (0, 1): ValueError otherwise.  The limit of the rule: a run of two or more bad sections that resemble EACH OTHER
    (a block from the wrong place) is seen only at its two ends, as the two low correlations of section_scores across
    its cuts -- every section of the run, the end ones included, still resembles a neighbour inside the run, so none is
    flagged; that is what a clean cut looks like, too.  Blank or saturated sections in a row are still found, since a
    constant tile correlates with nothing.  defects_repair turns the verdict into a Repair."""
    s = _check_sums(s, "find_defects")
    ratio, frac = _unit(ratio, "ratio", True), _unit(section_fraction, "section_fraction", True)
    min_corr = _unit(min_corr, "min_corr", False)
    Z, grid = s.shape[0], s.shape[1:3]
    t = np.zeros((Z,) + grid, np.float64)
    if Z < 2:
        return Defects([], np.zeros((Z,) + grid, bool), np.ones(grid, bool), t)
    c = section_scores(s)
    t[0], t[-1] = c[0], c[-1]
    t[1:-1] = np.maximum(c[:-1], c[1:])
    med = np.median(c, axis=0)
    undecided = med <= min_corr
    bad = ~undecided[None] & (t < ratio * med[None])
    decided = int((~undecided).sum())
    nbad = bad.reshape(Z, -1).sum(axis=1)
    sections = [z for z in range(Z) if nbad[z] > 0 and nbad[z] >= frac * decided]
    tiles = bad.copy()
    tiles[sections] = False
    return Defects(sections, tiles, undecided, t)


def defect_mask(tiles, tile, vol_shape, out=None):
    """The uint8 mask [Z, Y, X] of a volume of shape `vol_shape` that is 1 in the voxels of the tiles (i, j) of section z
    with tiles[z, i, j] and 0 elsewhere, on clahe_grid's tiles of `tile` pixels: what Repair takes as `mask`.  Written
    into `out` (ndarray, np.memmap, h5py / zarr dataset of the volume's shape, uint8) section by section -- every
    section, so `out` need not be cleared --, or into a new ndarray; returned.  Host only.  ValueError for a shape that
    is not [z, y, x], tiles of another shape than (Z, gy, gx), a bad tile or `out`."""
    th, tw = _clahe_tile(tile)
    shape = tuple(int(v) for v in vol_shape)
    if len(shape) != 3:
        raise ValueError(f"defect_mask needs a volume [z, y, x], got shape {shape}")
    gy, gx = clahe_grid(shape, (th, tw))
    tiles = np.asarray(tiles)
    if tiles.shape != (shape[0], gy, gx):
        raise ValueError(f"tiles must have the shape {(shape[0], gy, gx)} of the volume's tile grid, got {tiles.shape}")
    tiles = tiles != 0
    if out is None:
        out = np.zeros(shape, np.uint8)
    elif tuple(out.shape) != shape or getattr(out, "dtype", None) != np.uint8:
        raise ValueError(f"out must be uint8 of the volume's shape {shape}, got {getattr(out, 'dtype', None)} "
                         f"{tuple(out.shape)}")
    clear = np.zeros(shape[1:], np.uint8)
    for z in range(shape[0]):
        if tiles[z].any():
            out[z] = np.repeat(np.repeat(tiles[z], th, axis=0), tw, axis=1)[:shape[1], :shape[2]].astype(np.uint8)
        else:
            out[z] = clear
    return out


def defects_repair(d, tile, vol_shape, mask_out=None, max_gap=8):
    """The Repair of find_defects' verdict `d` for a volume of shape `vol_shape` [z, y, x] on tiles of `tile` pixels: its
    `sections` are d.sections, its mask defect_mask(d.tiles, ...) -- written into `mask_out` where that is given -- when
    any tile is bad, otherwise it has no mask (and `mask_out` is left as it is).  volume_repair and `repair=` take it
    unchanged; a verdict without any defect gives a Repair that changes nothing."""
    R = _index(max_gap, "max_gap")
    if not 1 <= R <= REPAIR_MAX_GAP:
        raise ValueError(f"max_gap must lie in 1...{REPAIR_MAX_GAP}, got {R}")
    try:
        sections, tiles = [_index(z, "a section") for z in d.sections], np.asarray(d.tiles)
    except (AttributeError, TypeError):
        raise ValueError(f"defects_repair needs find_defects' Defects, got {type(d).__name__}")
    mask = defect_mask(tiles, tile, vol_shape, mask_out) if tiles.any() else None
    return Repair(sections, mask, None, R)


OUTLIER_MAX_RADIUS = 7           # tem_u8_zdev_mask: windows of 3...15 pixels
OUTLIER_MAX_THR = 255 * 256      # a threshold, in 1/256 grey level


def section_neighbours(Z, skip=(), max_lag=4):
    """The nearest good sections below and above every section of a stack of `Z` when the sections `skip` are bad:
    np.int32 nbr[Z, 2] = (lo, hi), the table that tem_u8_zdev_tiles and tem_u8_zdev_mask judge a section against
    (include/tem_hip.h has the definition).  A row is (-1, -1), no verdict, for a skipped section, for the first and the
    last good section, and for a good section whose nearest good neighbour on either side is further than `max_lag`
    (1...SHIFT_MAX_LAG) away; every other row is lo < z < hi.  No `skip` gives (z - 1, z + 1) for 0 < z < Z - 1.  Host
    only; section_pairs' ValueErrors."""
    try:
        skip = list(skip)
    except TypeError:
        raise ValueError(f"skip must be a list of sections, got {skip!r}")
    section_pairs(Z, skip, max_lag)                              # the checks, and their messages
    Z, lag = _index(Z, "Z"), _index(max_lag, "max_lag")
    bad = {_index(z, "a skipped section") for z in skip}
    good = [z for z in range(Z) if z not in bad]
    nbr = np.full((Z, 2), -1, np.int32)
    for lo, z, hi in zip(good[:-2], good[1:-1], good[2:]):
        if z - lo <= lag and hi - z <= lag:
            nbr[z] = (lo, hi)
    return nbr


def _check_neighbours(nbr, Z):
    """int32[Z, 2] of `nbr`: rows (-1, -1) or lo < z < hi in [0, Z) at most SHIFT_MAX_LAG away.  ValueError otherwise."""
    t = np.asarray(nbr)
    if t.shape != (Z, 2) or t.dtype.kind not in "iu":
        raise ValueError(f"nbr must be section_neighbours' integers [{Z}, 2], got {t.dtype} {t.shape}")
    t = t.astype(np.int64)
    z = np.arange(Z)
    lo, hi = t[:, 0], t[:, 1]
    ok = ((lo == -1) & (hi == -1)) | ((lo >= 0) & (lo < z) & (hi > z) & (hi < Z) & (z - lo <= SHIFT_MAX_LAG) &
                                      (hi - z <= SHIFT_MAX_LAG))
    if not ok.all():
        k = int(np.flatnonzero(~ok)[0])
        raise ValueError(f"nbr[{k}] = {tuple(int(v) for v in t[k])} is neither (-1, -1) nor lo < {k} < hi inside [0, {Z}) "
                         f"at most {SHIFT_MAX_LAG} sections away")
    return np.ascontiguousarray(t.astype(np.int32))


def _outlier_radius(radius, least):
    r = _index(radius, "radius")
    if not least <= r <= OUTLIER_MAX_RADIUS:
        raise ValueError(f"radius must lie in {least}...{OUTLIER_MAX_RADIUS}, got {r}")
    return r


def _outlier_window(window):
    """The radius of an odd `window` in 3...15."""
    win = _index(window, "window")
    if not 3 <= win <= 2 * OUTLIER_MAX_RADIUS + 1 or not win & 1:
        raise ValueError(f"window must be odd and lie in 3...{2 * OUTLIER_MAX_RADIUS + 1}, got {win}")
    return win // 2


def _outlier_params(ratio, min_dev):
    try:
        if any(isinstance(v, (bool, np.bool_, str, bytes)) for v in (ratio, min_dev)):
            raise TypeError
        ratio, min_dev = float(ratio), float(min_dev)
    except (TypeError, ValueError):
        raise ValueError(f"ratio and min_dev must be numbers, got {ratio!r}, {min_dev!r}")
    if not ratio > 0 or not np.isfinite(ratio):
        raise ValueError(f"ratio must be positive, got {ratio!r}")
    if not 0 < min_dev <= 255:
        raise ValueError(f"min_dev must lie in (0, 255], got {min_dev!r}")
    return ratio, min_dev


def outlier_chunks(box, vol_shape, nbr, radius, chunk_bytes=None, rank=0, world_size=1):
    """Cut the (z, y, x) (lo, hi) `box` of a volume of shape `vol_shape` [z, y, x] into slabs for volume_outliers and, with
    radius = 0 and the whole volume as the box, for section_outlier_sums.  Returns this rank's list of (core slab, read
    slab), both (z, y, x) (lo, hi) boxes of the volume: the cores are disjoint and their union is the box (hist_chunks'
    kinds of cut: runs of whole sections of the box, or runs of whole rows of one section; x is never cut); a read slab
    is the dense hull along z of its core's sections and their (lo, hi) of `nbr` (section_neighbours' table; a section
    without a verdict asks for itself alone), the core's rows and `radius` (0...7) more on each side, cut to the volume,
    and the volume's whole x extent.  A read slab holds at most `chunk_bytes` bytes (HIST_CHUNK_BYTES when None) wherever
    one row allows it: as many whole sections per core as fit with their hull, or, where one section's hull is larger
    than the budget, that section's rows, as many as fit next to their 2 radius (one row at the least).  Slabs are in
    (z, y) order and go round-robin to the ranks.  Pure host function; ValueError as hist_chunks, for a bad table or
    radius and a box outside the volume."""
    budget = _budget(chunk_bytes, rank, world_size)
    vol_shape = tuple(int(v) for v in vol_shape)
    if len(vol_shape) != 3 or min(vol_shape) < 1:
        raise ValueError(f"outlier_chunks takes a non-empty volume shape [z, y, x], got {vol_shape}")
    Z, Y, X = vol_shape
    t = _check_neighbours(nbr, Z)
    r = _outlier_radius(radius, 0)
    (z0, z1), (y0, y1), (x0, x1) = box
    if any(lo < 0 or hi > n for (lo, hi), n in zip(box, vol_shape)):
        raise ValueError(f"the box {tuple(box)} reaches outside the volume of shape {vol_shape}")
    if z1 <= z0 or y1 <= y0 or x1 <= x0:
        return []
    first = np.where(t[:, 0] < 0, np.arange(Z), t[:, 0])
    last = np.where(t[:, 0] < 0, np.arange(Z), t[:, 1])
    ra, rb = max(y0 - r, 0), min(y1 + r, Y)                      # the rows read for a core of whole sections
    slabs, z = [], z0
    while z < z1:
        lo, hi = int(first[z]), int(last[z]) + 1
        if (hi - lo) * (rb - ra) * X <= budget:
            k = 1
            while z + k < z1:
                more = min(lo, int(first[z + k])), max(hi, int(last[z + k]) + 1)
                if (more[1] - more[0]) * (rb - ra) * X > budget:
                    break
                k, (lo, hi) = k + 1, more
            slabs.append((((z, z + k), (y0, y1), (x0, x1)), ((lo, hi), (ra, rb), (0, X))))
            z += k
            continue
        ky = max(1, budget // ((hi - lo) * X) - 2 * r)
        slabs += [(((z, z + 1), (y, min(y + ky, y1)), (x0, x1)),
                   ((lo, hi), (max(y - r, 0), min(min(y + ky, y1) + r, Y)), (0, X))) for y in range(y0, y1, ky)]
        z += 1
    return slabs[rank::world_size]


def section_outlier_sums(volume, tile=128, skip=(), max_lag=4, chunk_bytes=None, rank=0, world_size=1, device=None,
                         stats=None):
    """How far the voxels of every tile of a section lie outside the range of the voxels below and above them:
    np.int64 [Z, gy, gx, 2] over the WHOLE uint8 `volume` [z, y, x] (ndarray, np.memmap, h5py / zarr dataset; one image
    [y, x]: Z = 1, all zero) on clahe_grid's tiles of `tile` pixels (an int or (th, tw) in [1, 2048]).  With
    (lo, hi) = section_neighbours(Z, skip, max_lag)[z], the nearest good sections around z, and per voxel
    a = volume[lo, y, x], v = volume[z, y, x], b = volume[hi, y, x]:
      e = |v - median(a, v, b)|: 0 where v lies between a and b, else its distance to the nearer one
      s[z, i, j] = (sum e, the number of voxels) over tile (i, j);   (0, 0) for a section without a verdict
    -- the voxel's form of find_defects' rule "resembles NEITHER neighbour", and the three-tap temporal median of film
    restoration.  Exact integers that numpy reproduces bit for bit, whatever the slabs, ranks and launches.
    outlier_thresholds turns them into what is ordinary for each column of tiles, volume_outliers into a mask; find_debris
    runs all three.  The stack must be ALIGNED first (section_shifts ... volume_warp): misaligned sections read as
    outliers everywhere.

    section_sums' pass over outlier_chunks' read slabs (radius 0): one host thread -> pinned -> H2D -> one
    tem_u8_zdev_tiles launch per slab, adding into a device accumulator that holds the whole volume's Z*gy*gx*16 bytes
    and is read back once where that is at most CLAHE_ACC_BYTES, else one slab's core sections, read back and added on
    the host per slab.  The table goes to the device once.  Ranks take slabs round-robin and their results add up to
    the whole.  `stats` receives `read_s` and `chunks`.  ValueError, before any GPU work: as section_sums, and
    section_pairs' for skip and max_lag."""
    _check_u8(volume)
    th, tw = _clahe_tile(tile)
    gy, gx = clahe_grid(volume.shape, (th, tw))
    box = hist_box(volume.shape)
    Z = box[0][1]
    nbr = section_neighbours(Z, skip, max_lag)
    chunks = outlier_chunks(box, tuple(hi for _, hi in box), nbr, 0, chunk_bytes, rank, world_size)
    p = _SlabPass([volume], [box], chunk_bytes, rank, world_size, device, slabs=[r for _, r in chunks])
    lib = H.require_gpu()
    with p.streaming(stats):
        acc = _RowAccumulator(p.dev, Z, (gy, gx, 2), _most_rows(c[0] for c, _ in chunks))
        nbr_dev = torch.from_numpy(nbr).to(p.dev)                # uploaded once
        for k, ((s0, _), (y0, _), (x0, _)), d, (src,) in p:
            z0, z1 = chunks[k][0][0]
            _lib.check(lib.tem_u8_zdev_tiles(src.data_ptr(), *d, s0, Z, z0 - s0, z1 - s0, y0, x0, th, tw, gy, gx,
                                             nbr.ctypes.data, nbr_dev.data_ptr(), acc.ptr(z0, z1),
                                             p.compute.cuda_stream), "tem_u8_zdev_tiles")
            acc.add(z0, z1)
        return acc.result()


class OutlierThresholds(NamedTuple):
    """outlier_thresholds' result: `thr` int32[gy, gx], what volume_outliers compares a window's mean deviation with, in
    1/256 grey level; `scale` float64[gy, gx], the ordinary mean deviation of each column of tiles, in grey levels."""
    thr: np.ndarray
    scale: np.ndarray


def outlier_thresholds(s, ratio=12.0, min_dev=16.0):
    """What is ordinary for each column of tiles, from section_outlier_sums' `s`.  Host only.
      scale[i, j] = np.median over the sections with n > 0 of sum e / n: the ordinary mean deviation of a voxel of the
                    column from its neighbours' range, in grey levels; 0.0 for a column with no such section
      thr[i, j]   = min(ceil(256 max(ratio scale, min_dev)), 65280)
    A window is flagged where its mean deviation exceeds thr / 256 grey levels: `ratio` (> 0) times the ordinary one, and
    at least `min_dev` (in (0, 255]), a floor in grey levels that keeps resin and constant columns from flagging their
    noise.  ValueError for an `s` of another kind and parameters out of range."""
    s = np.asarray(s)
    if s.ndim != 4 or s.shape[3] != 2 or s.dtype.kind not in "iu":
        raise ValueError(f"outlier_thresholds: s must be section_outlier_sums' integer array [Z, gy, gx, 2], got "
                         f"{s.dtype} {s.shape}")
    ratio, min_dev = _outlier_params(ratio, min_dev)
    grid = s.shape[1:3]
    scale = np.zeros(grid, np.float64)
    for i in range(grid[0]):
        for j in range(grid[1]):
            n = s[:, i, j, 1]
            if (n > 0).any():
                scale[i, j] = np.median(s[n > 0, i, j, 0] / n[n > 0])
    thr = np.minimum(np.ceil(256.0 * np.maximum(ratio * scale, min_dev)), OUTLIER_MAX_THR).astype(np.int32)
    return OutlierThresholds(thr, scale)


def volume_outliers(volume, thr, tile=128, window=9, skip=(), max_lag=4, tiles=None, out=None, start=None, size=None,
                    chunk_bytes=None, stats=None, rank=0, world_size=1, device=None):
    """The uint8 mask, 1 or 0, of the voxels of the ROI [start, start + size) ((x, y, z) order; default: the whole
    volume) of a uint8 array-like `volume` [z, y, x] (ndarray, np.memmap, h5py / zarr dataset) that stand out from the
    nearest good sections below and above them -- dust, precipitate, knife debris: damage far smaller than a tile --,
    written into `out`: a writable uint8 array-like of the ROI's shape (ndarray, memmap, h5py, zarr; allocated when
    None), which is returned; Repair takes it as `mask` where the ROI is the whole volume.  With e the deviation of
    section_outlier_sums (neighbours by `skip` and `max_lag`), r = (window - 1) / 2 for an odd `window` in 3...15, Ws the
    sum of e over the window of `window` x `window` pixels around the voxel, cut to the section, and c the number of
    voxels of the cut window:
      mask = 1 iff 256 Ws > thr[i, j] c, (i, j) the voxel's tile of `tile` pixels     (equality does not flag)
    -- the window's mean deviation exceeds thr / 256 grey levels -- with `thr` outlier_thresholds' result or its int
    table [gy, gx] in [1, 65280]; also 1 throughout the tiles named by `tiles` (find_defects' bool [Z, gy, gx]) where
    given.  Summed over the window, a particle stands apart from the ordinary change between sections; the mask reaches
    up to r pixels past it.  A section without a verdict, and one image [y, x], give zeros.  Everything is integers and
    numpy reproduces every byte; a voxel depends on its window and two other sections alone, so the result of an ROI is
    the ROI of the whole result, however it is cut.  The stack must be aligned first, and damage two or more sections
    thick at the same place resembles a neighbour and is NOT flagged: find_defects or a `skip` list is the tool for that.

    volume_repair's pass over outlier_chunks' read slabs: one host thread reads each -- the core, the sections its
    neighbours name, r rows more on each side -- into double-buffered pinned memory -> H2D -> one tem_u8_zdev_mask
    launch per slab -> D2H through the output stream -> host write, in the order write(k), read(k + 2) on the one host
    thread.  The tables are uploaded once.  Ranks take slabs round-robin and write disjoint boxes of a shared `out`.
    `stats` receives `read_s`, `write_s`, `chunks` and `flagged`: the ones written by this rank.
    ValueError, before any GPU work: a non-uint8 volume, an ROI outside it, a bad tile, window, skip or max_lag, a `thr`
    or `tiles` of another shape, dtype or range, an `out` of another shape or dtype."""
    _check_u8(volume)
    th, tw = _clahe_tile(tile)
    gy, gx = clahe_grid(volume.shape, (th, tw))
    box = hist_box(volume.shape, start, size)
    whole = hist_box(volume.shape)
    Z, Y, X = (hi for _, hi in whole)
    r = _outlier_window(window)
    nbr = section_neighbours(Z, skip, max_lag)
    t = np.asarray(thr.thr if isinstance(thr, OutlierThresholds) else thr)
    if t.shape != (gy, gx) or t.dtype.kind not in "iu":
        raise ValueError(f"thr must be outlier_thresholds' integers of the tile grid's shape {(gy, gx)}, got {t.dtype} "
                         f"{t.shape}")
    if int(t.min()) < 1 or int(t.max()) > OUTLIER_MAX_THR:
        raise ValueError(f"thr must lie in [1, {OUTLIER_MAX_THR}], got {int(t.min())}...{int(t.max())}")
    t = np.ascontiguousarray(t.astype(np.int32))
    if tiles is not None:
        tiles = np.asarray(tiles)
        if tiles.shape != (Z, gy, gx) or tiles.dtype.kind not in "biu":
            raise ValueError(f"tiles must be bool or integers of the shape {(Z, gy, gx)} of the volume's tile grid, got "
                             f"{tiles.dtype} {tiles.shape}")
        tiles = np.ascontiguousarray((tiles != 0).astype(np.uint8))
    out = _roi_out(out, box, len(volume.shape) == 2)
    chunks = outlier_chunks(box, (Z, Y, X), nbr, r, chunk_bytes, rank, world_size)
    p = _SlabPass([volume], [whole], chunk_bytes, rank, world_size, device, slabs=[rd for _, rd in chunks])
    lib = H.require_gpu()
    cores = [c for c, _ in chunks]
    with p.streaming(stats):
        nbr_dev, thr_dev = torch.from_numpy(nbr).to(p.dev), torch.from_numpy(t).to(p.dev)   # the tables, once
        tiles_dev = None if tiles is None else torch.from_numpy(tiles).to(p.dev)
        count = torch.zeros(1, dtype=torch.int64, device=p.dev)
        with p.writing(out, box, cores) as outp:
            for k, ((s0, _), (ry, _), _), d, (src,) in p:
                (cz0, cz1), (cy0, cy1), (cx0, cx1) = cores[k]
                _lib.check(lib.tem_u8_zdev_mask(src.data_ptr(), *d, s0, Z, Y, ry, cz0 - s0, cz1 - s0, cy0 - ry, cy1 - ry,
                                                cx0, cx1, th, tw, gy, gx, r, nbr.ctypes.data, nbr_dev.data_ptr(),
                                                t.ctypes.data, thr_dev.data_ptr(),
                                                None if tiles is None else tiles_dev.data_ptr() + cz0 * gy * gx,
                                                outp.device(k).data_ptr(), count.data_ptr(), p.compute.cuda_stream),
                           "tem_u8_zdev_mask")
                p.put(k)
        p.st["flagged"] = int(count.cpu().numpy()[0])                    # the one read-back
    return out


def find_debris(volume, tile=128, window=9, ratio=12.0, min_dev=16.0, skip=(), max_lag=4, defects=None, mask_out=None,
                max_gap=8, **pass_kw):
    """Find the small damage of a uint8 `volume` [z, y, x] -- dust, precipitate, knife debris: particles on ONE section,
    far below what find_defects' tile correlations can see -- and return the Repair that fills it:
    section_outlier_sums -> outlier_thresholds(ratio, min_dev) -> volume_outliers(window) over the whole volume, the
    mask written into `mask_out` where given (a uint8 array-like of the volume's shape; np.memmap for a volume that does
    not fit).  The sections `skip` (black, lost, foreign) are judged by nobody and no section is judged against them:
    their neighbours are bridged up to `max_lag`.  With `defects` (find_defects' Defects) its sections join `skip` and
    its bad tiles are set in the mask whole.  Returns Repair(sorted skipped sections, mask, None, max_gap), which
    volume_repair and predict_*(repair=...) take unchanged.  `pass_kw` (chunk_bytes, device, stats) goes to both passes;
    `stats` is the mask pass's.  For several ranks run the passes themselves: their sums must be added in between.

    The stack must be aligned first: misaligned sections read as outliers everywhere.  The limit of the rule: damage two
    or more sections thick at the same place resembles a neighbour and is not flagged; find_defects or a `skip` list is
    the tool for that."""
    R = _index(max_gap, "max_gap")
    if not 1 <= R <= REPAIR_MAX_GAP:
        raise ValueError(f"max_gap must lie in 1...{REPAIR_MAX_GAP}, got {R}")
    extra = set(pass_kw) - {"chunk_bytes", "device", "stats"}
    if extra:
        raise ValueError(f"find_debris passes chunk_bytes, device and stats on, got {sorted(extra)}")
    if len(volume.shape) != 3:
        raise ValueError(f"find_debris needs a volume [z, y, x], got shape {tuple(volume.shape)}")
    try:
        bad = {_index(z, "a skipped section") for z in skip}
    except TypeError:
        raise ValueError(f"skip must be a list of sections, got {skip!r}")
    tiles = None
    if defects is not None:
        try:
            bad |= {_index(z, "a section") for z in defects.sections}
            tiles = np.asarray(defects.tiles)
        except (AttributeError, TypeError):
            raise ValueError(f"defects must be find_defects' Defects, got {type(defects).__name__}")
    sections = sorted(bad)
    _check_u8(volume)                                            # every ValueError ahead of the first pass
    tile = _clahe_tile(tile)
    _outlier_window(window), _outlier_params(ratio, min_dev)
    vshape = tuple(int(v) for v in volume.shape)
    if mask_out is not None and (tuple(mask_out.shape) != vshape or getattr(mask_out, "dtype", None) != np.uint8):
        raise ValueError(f"mask_out must be uint8 of the volume's shape {vshape}, got {getattr(mask_out, 'dtype', None)} "
                         f"{tuple(mask_out.shape)}")
    if tiles is not None and tiles.shape != (vshape[0],) + clahe_grid(vshape, tile):
        raise ValueError(f"defects.tiles must have the shape {(vshape[0],) + clahe_grid(vshape, tile)} of the volume's "
                         f"tile grid, got {tiles.shape}")
    sums_kw = {k: v for k, v in pass_kw.items() if k != "stats"}
    s = section_outlier_sums(volume, tile, sections, max_lag, **sums_kw)
    t = outlier_thresholds(s, ratio, min_dev)
    mask = volume_outliers(volume, t, tile, window, sections, max_lag, tiles=tiles, out=mask_out, **pass_kw)
    return Repair(sections, mask, None, R)


ZLAG_MAX = 8                     # tem_u8_zcorr_lags: 1 <= nlag <= 8
ZSPACE_MIN, ZSPACE_MAX = Fraction(1, 8), 8       # a section's spacing along z, in sections: volume_rescale's step limits
ZSPACE_UNIT = 1 << 16            # quantize_positions: positions along z in 2^-16 section


def _max_lag(max_lag):
    L = _index(max_lag, "max_lag")
    if not 1 <= L <= ZLAG_MAX:
        raise ValueError(f"max_lag must lie in 1...{ZLAG_MAX}, got {L}")
    return L


def zlag_chunks(vol_shape, max_lag=4, chunk_bytes=None, rank=0, world_size=1):
    """zcorr_chunks for section_lag_sums: the same cores, and read slabs that reach min(max_lag, Z - 1) sections past
    their core where the volume has them -- the planes a core plane is correlated with.  The budget counts a core next to
    that halo.  With max_lag = 1 it is zcorr_chunks.  Pure host function; ValueError as zcorr_chunks and for max_lag
    outside 1...ZLAG_MAX."""
    return _zhalo_chunks(vol_shape, _max_lag(max_lag), chunk_bytes, rank, world_size)


def section_lag_sums(volume, tile=128, max_lag=4, chunk_bytes=None, rank=0, world_size=1, device=None, stats=None):
    """section_sums with L = `max_lag` (1...8) partners instead of one: np.int64 [Z, gy, gx, 3 + L] over the WHOLE uint8
    `volume` [z, y, x] on clahe_grid's tiles of `tile` pixels.  With v the voxels of tile (i, j) of section z and v+k
    those k sections up:
      s[z, i, j] = (sum v, sum v v, the number of voxels, sum v v+1, ..., sum v v+L);   sum v v+k is 0 where z + k >= Z.
    Exact integers that numpy reproduces bit for bit, whatever the slabs, ranks and launches.  lag_scores turns them into
    correlations per lag, section_spacing into the sections' positions along z.

    Out of core exactly as section_sums, over read slabs that reach L sections past their core (zlag_chunks): one
    tem_u8_zcorr_lags launch per slab into a device accumulator, which holds the whole volume's sums and is read back
    once where they are at most CLAHE_ACC_BYTES, else one slab's.  Ranks take slabs round-robin and their results add up
    to the whole.  `stats` receives `read_s` and `chunks`.  ValueError, before any GPU work, as section_sums and for
    max_lag outside 1...8."""
    _check_u8(volume)
    L = _max_lag(max_lag)
    th, tw = _clahe_tile(tile)
    gy, gx = clahe_grid(volume.shape, (th, tw))
    box = hist_box(volume.shape)
    chunks = zlag_chunks(volume.shape, L, chunk_bytes, rank, world_size)
    p = _SlabPass([volume], [box], chunk_bytes, rank, world_size, device, slabs=[r for _, r in chunks])
    lib = H.require_gpu()
    with p.streaming(stats):
        acc = _RowAccumulator(p.dev, box[0][1], (gy, gx, 3 + L), _most_rows(c[0] for c, _ in chunks))
        for k, ((r0, _), (y0, _), (x0, _)), d, (src,) in p:
            z0, z1 = chunks[k][0][0]
            _lib.check(lib.tem_u8_zcorr_lags(src.data_ptr(), *d, z0 - r0, z1 - r0, y0, x0, th, tw, gy, gx, L,
                                             acc.ptr(z0, z1), p.compute.cuda_stream), "tem_u8_zcorr_lags")
            acc.add(z0, z1)
        return acc.result()


def _check_lag_sums(s, who):
    s = np.asarray(s)
    if s.ndim != 4 or not 4 <= s.shape[3] <= 3 + ZLAG_MAX or s.dtype.kind not in "iu":
        raise ValueError(f"{who}: s must be section_lag_sums' integer array [Z, gy, gx, 3 + L], got {s.dtype} {s.shape}")
    return s.astype(np.int64, copy=False)


def lag_scores(s):
    """float64 c[Z, gy, gx, L]: the Pearson correlation of every tile of section z with the same tile of section
    z + k, k = 1...L in c[..., k - 1], from section_lag_sums' `s`.  Host only.  section_scores' formula per lag, with
    n = s[..., 2], S1 = s[..., 0], S2 = s[..., 1], Pk = s[..., 2 + k]:
      A = n S2[z] - S1[z]^2,   B = the same at z + k,   N = n Pk[z] - S1[z] S1[z + k]
    exact in int64, and c = N / (sqrt(A) sqrt(B)) where A > 0 and B > 0, else 0.0 -- as past the last section."""
    s = _check_lag_sums(s, "lag_scores")
    Z, L = s.shape[0], s.shape[3] - 3
    c = np.zeros(s.shape[:3] + (L,), np.float64)
    n, S1, S2 = s[..., 2], s[..., 0], s[..., 1]
    var = n * S2 - S1 * S1
    for k in range(1, min(L, Z - 1) + 1):
        A, B = var[:-k], var[k:]
        N = n[:-k] * s[:-k, :, :, 2 + k] - S1[:-k] * S1[k:]
        ok = (A > 0) & (B > 0)
        c[:-k, :, :, k - 1][ok] = N[ok] / (np.sqrt(A[ok].astype(np.float64)) * np.sqrt(B[ok].astype(np.float64)))
    return c


class Spacing(NamedTuple):
    """section_spacing's estimate: `positions` float64[Z] of the sections along z, in sections, from 0 to Z - 1;
    `curve` float64[L + 1] the correlation at a distance of 0...L sections; `used` bool[Z, L] the pairs (z, z + k) that
    were measured; `clipped` the list of (a, b), consecutive good sections whose spacing was cut to the limits;
    `unresolved` the list of (a, b), consecutive good sections between which nominal spacing was assumed."""
    positions: np.ndarray
    curve: np.ndarray
    used: np.ndarray
    clipped: list
    unresolved: list


def _lower_median(v, axis):
    """The element at index (n - 1) // 2 of the sorted values along `axis`, NaNs last and not counted; NaN for none."""
    v = np.sort(v, axis=axis)                                            # NaNs sort to the end
    n = np.sum(~np.isnan(v), axis=axis, keepdims=True)
    got = np.take_along_axis(v, np.maximum(n - 1, 0) // 2, axis=axis)
    return np.where(n > 0, got, np.nan).squeeze(axis)


def _solve_banded(U, rhs):
    """x of the symmetric positive definite band system whose upper band is U[i, t] = A[i, i + t]: elimination without
    pivoting, O(n L^2), in place."""
    n, B = U.shape
    for i in range(n):
        for t in range(1, min(B, n - i)):
            if U[i, t] != 0.0:
                f = U[i, t] / U[i, 0]
                U[i + t, :B - t] -= f * U[i, t:]
                rhs[i + t] -= f * rhs[i]
    x = np.zeros(n, np.float64)
    for i in range(n - 1, -1, -1):
        m = min(B, n - i)
        x[i] = (rhs[i] - np.dot(U[i, 1:m], x[i + 1:i + m])) / U[i, 0]
    return x


def section_spacing(s, skip=(), min_corr=0.1):
    """Where the sections of a stack sit along z, from how fast their correlation decays with the lag (Hanslovsky et
    al. 2017): Spacing(positions, curve, used, clipped, unresolved) from section_lag_sums' `s` [Z, gy, gx, 3 + L].  Host
    only and deterministic.  Run it after in-plane alignment: misaligned sections read as "far apart".  `skip` lists
    the bad sections (find_defects, suspect_sections, flat_sections); the others are good.  The rule:
      1. a tile column is decided where its median lag-1 score over the pairs of good sections is above `min_corr`;
      2. c[z, k] is the lower median over the decided columns of the score of (z, z + k), both sections good;
      3. curve[k] is the median over z of c[z, k], curve[0] = 1: the correlation at a distance of k sections of median
         spacing.  ValueError where the curve is not strictly decreasing (no decided column, too few sections);
      4. a pair is used where c[z, k] > curve[L]; its distance d is the piecewise-linear inverse of the curve at
         min(c, 1), between 0 and L;
      5. the positions p of the good sections are the weighted least squares of p[z + k] - p[z] = d over the used
         pairs, weight 1 / k, the first section of each connected group at 0: a band system, solved in O(Z L^2);
      6. a group of good sections that no used pair joins to the sections before it starts at nominal spacing -- 1 per
         section spanned -- behind the good section before it, and that pair is listed in `unresolved`;
      7. the spacing of two consecutive good sections is cut to [ZSPACE_MIN, ZSPACE_MAX] x (sections spanned), and the
         pair is listed in `clipped`;
      8. a skipped section is placed linearly between its good neighbours (at spacing 1 before the first good section
         and behind the last);
      9. the positions are normalised to P[0] = 0 and P[Z - 1] = Z - 1.
    ValueError for sums of another shape, a bad skip or min_corr (in (0, 1)), a stack without two good sections."""
    s = _check_lag_sums(s, "section_spacing")
    Z, L = s.shape[0], s.shape[3] - 3
    try:
        bad = {_index(z, "a skipped section") for z in skip}
    except TypeError:
        raise ValueError(f"skip must be a list of sections, got {skip!r}")
    if any(not 0 <= z < Z for z in bad):
        raise ValueError(f"skip names sections outside [0, {Z}): {sorted(z for z in bad if not 0 <= z < Z)}")
    m = _unit(min_corr, "min_corr", closed=False)
    good = np.array([z not in bad for z in range(Z)], bool)
    gidx = np.flatnonzero(good)
    if gidx.size < 2:
        raise ValueError(f"section_spacing needs two good sections at least, got {gidx.size} of {Z}")
    c = lag_scores(s)                                                    # [Z, gy, gx, L]
    both = np.zeros((Z, L), bool)                                        # (z, z + k): both sections good
    for k in range(1, min(L, Z - 1) + 1):
        both[:-k, k - 1] = good[:-k] & good[k:]
    c = np.where(both[:, None, None, :], c, np.nan)
    # 1. the decided columns
    pairs1 = (~np.isnan(c[..., 0])).sum(axis=0)                          # [gy, gx]
    decided = (pairs1 > 0) & (np.nanmedian(np.where(pairs1 > 0, c[..., 0], 0.0), axis=0) > m)
    # 2. the lower median over the decided columns
    cz = _lower_median(c[:, decided, :], axis=1) if decided.any() else np.full((Z, L), np.nan)
    # 3. the curve
    curve = np.ones(L + 1, np.float64)
    for k in range(L):
        v = cz[:, k][~np.isnan(cz[:, k])]
        curve[k + 1] = np.median(v) if v.size else np.nan
    if not np.all(np.diff(curve) < 0):                                   # a NaN fails too
        raise ValueError(f"section_spacing: the correlation does not decrease strictly with the lag: {curve.tolist()}")
    # 4. the used pairs and their distances
    used = ~np.isnan(cz) & (np.nan_to_num(cz, nan=-2.0) > curve[L])
    dist = np.interp(np.minimum(np.nan_to_num(cz, nan=1.0), 1.0), curve[::-1], np.arange(L, -1, -1.0))
    # 5. the band system over the good sections, in their order
    rank_of = np.cumsum(good) - 1
    n = gidx.size
    U, rhs = np.zeros((n, L + 1), np.float64), np.zeros(n, np.float64)
    group = np.arange(n)                                                 # union-find: the connected groups

    def root(a):
        while group[a] != a:
            group[a] = group[group[a]]
            a = group[a]
        return a

    for z, k in np.argwhere(used).tolist():
        a, b, w, d = int(rank_of[z]), int(rank_of[z + k + 1]), 1.0 / (k + 1), dist[z, k]
        U[a, 0] += w
        U[b, 0] += w
        U[a, b - a] -= w
        rhs[a] -= w * d
        rhs[b] += w * d
        ra, rb = root(a), root(b)
        if ra != rb:
            group[max(ra, rb)] = min(ra, rb)                             # a group's root is its first section
    roots = np.array([root(a) for a in range(n)])
    for f in np.flatnonzero(roots == np.arange(n)).tolist():             # p[first of a group] = 0: its row and column go
        for t in range(1, min(L + 1, n - f)):
            U[f, t] = 0.0
        for t in range(1, min(L + 1, f + 1)):
            U[f - t, t] = 0.0
        U[f, 0], rhs[f] = 1.0, 0.0
    p = _solve_banded(U, rhs)
    # 6. the groups, in the order of their first sections
    unresolved, shift = [], np.zeros(n, np.float64)
    for a in range(1, n):
        if roots[a] == a:
            shift[a] = p[a - 1] + shift[roots[a - 1]] + float(gidx[a] - gidx[a - 1])
            unresolved.append((int(gidx[a - 1]), int(gidx[a])))
    p = p + shift[roots]
    # 7. the limits
    span = np.diff(gidx).astype(np.float64)
    raw = np.diff(p)
    step = np.clip(raw, float(ZSPACE_MIN) * span, float(ZSPACE_MAX) * span)
    clipped = [(int(gidx[a]), int(gidx[a + 1])) for a in np.flatnonzero(step != raw).tolist()]
    p = np.concatenate([[0.0], np.cumsum(step)])
    # 8. the skipped sections
    P = np.interp(np.arange(Z), gidx, p)
    P[:gidx[0]] = p[0] - (gidx[0] - np.arange(gidx[0]))
    P[gidx[-1] + 1:] = p[-1] + (np.arange(gidx[-1] + 1, Z) - gidx[-1])
    # 9. the scale
    P = (P - P[0]) * ((Z - 1) / (P[-1] - P[0]))
    P[0], P[-1] = 0.0, float(Z - 1)
    return Spacing(P, curve, used, clipped, unresolved)


def quantize_positions(P):
    """np.int64[Z]: the positions `P` of a stack's sections along z (section_spacing's, or any float or integer
    sequence; integers are taken as quantised already) in units of 2^-16 section, rounded to nearest.  ValueError,
    naming the section: a first position that is not 0, positions that do not increase strictly, a spacing outside
    [ZSPACE_MIN, ZSPACE_MAX] sections."""
    a = np.asarray(P)
    if a.ndim != 1 or a.size < 1 or a.dtype.kind not in "iuf":
        raise ValueError(f"positions must be one number per section, got {a.dtype} {a.shape}")
    if a.dtype.kind == "f":
        if not np.all(np.isfinite(a)) or np.abs(a).max() >= 2.0 ** 40:
            raise ValueError("positions must be finite and below 2^40")
        Q = np.rint(a * ZSPACE_UNIT).astype(np.int64)
    else:
        Q = a.astype(np.int64)
    if Q[0] != 0:
        raise ValueError(f"section 0 must sit at position 0, got {P[0]!r}")
    d = np.diff(Q)
    lo, hi = int(ZSPACE_MIN * ZSPACE_UNIT), int(ZSPACE_MAX * ZSPACE_UNIT)
    for z in np.flatnonzero((d <= 0) | (d < lo) | (d > hi)).tolist():
        if d[z] <= 0:
            raise ValueError(f"positions must increase strictly: section {z + 1} at {Q[z + 1] / ZSPACE_UNIT} does not "
                             f"lie above section {z} at {Q[z] / ZSPACE_UNIT}")
        raise ValueError(f"the spacing of sections {z} and {z + 1}, {d[z] / ZSPACE_UNIT}, is outside "
                         f"[{ZSPACE_MIN}, {ZSPACE_MAX}] sections")
    return Q


def resample_z_taps(Q, nz=None):
    """The one host copy of tem_u8_resample_z's table: np.int32[NZ, 2] = (z0, w) per section j of an even grid of
    spacing 1 over sections at the quantised positions `Q` (quantize_positions), in exact integers.  With t = j 2^16:
      z0 is the largest z with Q[z] <= t, held to Z - 1;   den = Q[z0 + 1] - Q[z0];
      w = (512 (t - Q[z0]) + den) // (2 den), the weight of section z0 + 1 in 1/256, rounded half up;
      w == 256 becomes (z0 + 1, 0), and the last section has w = 0: a tap of weight 0 is no tap.
    `nz` defaults to Q[Z - 1] // 2^16 + 1, the sections up to the last position; a larger one repeats the last
    section.  ValueError for what quantize_positions refuses and nz below 1."""
    Q = quantize_positions(np.asarray(Q))
    Z = Q.size
    NZ = int(Q[-1]) // ZSPACE_UNIT + 1 if nz is None else _index(nz, "nz")
    if NZ < 1:
        raise ValueError(f"nz must be positive, got {NZ}")
    t = np.arange(NZ, dtype=np.int64) * ZSPACE_UNIT
    z0 = np.minimum(np.searchsorted(Q, t, side="right") - 1, Z - 1)
    z1 = np.minimum(z0 + 1, Z - 1)
    den = np.where(z1 > z0, Q[z1] - Q[z0], 1)
    w = np.where(z1 > z0, (512 * (t - Q[z0]) + den) // (2 * den), 0)
    w = np.where(z1 > z0, np.minimum(w, 256), 0)                         # past the last position: the last section
    carry = w == 256
    return np.stack([np.where(carry, z0 + 1, z0), np.where(carry, 0, w)], axis=1).astype(np.int32)


def _check_taps(taps, Z):
    t = np.asarray(taps)
    if t.ndim != 2 or t.shape[1] != 2 or t.shape[0] < 1 or t.dtype.kind not in "iu":
        raise ValueError(f"taps must be resample_z_taps' integers [NZ, 2], got {t.dtype} {t.shape}")
    t = t.astype(np.int64)
    bad = np.flatnonzero((t[:, 0] < 0) | (t[:, 0] > Z - 1) | (t[:, 1] < 0) | (t[:, 1] > 255))
    if bad.size:
        j = int(bad[0])
        raise ValueError(f"taps[{j}] = {tuple(int(v) for v in t[j])} is not 0 <= z0 <= {Z - 1}, 0 <= w <= 255")
    return t


def resample_z_chunks(out_box, vol_shape, taps, chunk_bytes=None, rank=0, world_size=1):
    """Cut the (z, y, x) (lo, hi) box `out_box` of the output [NZ, Y, X] of a volume of shape `vol_shape` [Z, Y, X]
    resampled through `taps` (resample_z_taps) into slabs for volume_resample_z.  Returns this rank's list of (output
    slab, read slab), (z, y, x) (lo, hi) boxes of the output and of the volume with the same y and x: the output slabs
    are disjoint and their union is the box -- runs of whole sections of the box, or runs of whole rows of one section
    --; a read slab is the dense hull along z of its output sections' taps of weight above 0.  The two together hold at
    most `chunk_bytes` bytes (HIST_CHUNK_BYTES when None) wherever one row allows it.  Slabs are in (z, y) order and go
    round-robin to the ranks.  Pure host function; ValueError as hist_chunks, for bad taps and a box outside the
    output."""
    budget = _budget(chunk_bytes, rank, world_size)
    vol_shape = tuple(int(v) for v in vol_shape)
    if len(vol_shape) != 3 or min(vol_shape) < 1:
        raise ValueError(f"resample_z_chunks takes a non-empty volume shape [z, y, x], got {vol_shape}")
    VZ = vol_shape[0]
    t = _check_taps(taps, VZ)
    grid = (t.shape[0],) + vol_shape[1:]
    (z0, z1), (y0, y1), (x0, x1) = out_box
    if any(lo < 0 or hi > n for (lo, hi), n in zip(out_box, grid)):
        raise ValueError(f"the box {tuple(out_box)} reaches outside the output of shape {grid}")
    ny, nx = y1 - y0, x1 - x0
    if z1 <= z0 or ny <= 0 or nx <= 0:
        return []
    first = t[:, 0]
    last = np.where(t[:, 1] > 0, np.minimum(t[:, 0] + 1, VZ - 1), t[:, 0])

    def hull(a, b):                     # the source sections of output sections [a, b)
        return int(first[a:b].min()), int(last[a:b].max()) + 1

    slabs, z = [], z0
    while z < z1:
        lo, hi = hull(z, z + 1)
        if (1 + hi - lo) * ny * nx <= budget:
            k = 1
            while z + k < z1:
                more = hull(z, z + k + 1)
                if (k + 1 + more[1] - more[0]) * ny * nx > budget:
                    break
                k, (lo, hi) = k + 1, more
            slabs.append((((z, z + k), (y0, y1), (x0, x1)), ((lo, hi), (y0, y1), (x0, x1))))
            z += k
            continue
        ky = max(1, budget // ((1 + hi - lo) * nx))
        slabs += [(((z, z + 1), (y, min(y + ky, y1)), (x0, x1)), ((lo, hi), (y, min(y + ky, y1)), (x0, x1)))
                  for y in range(y0, y1, ky)]
        z += 1
    return slabs[rank::world_size]


def volume_resample_z(volume, positions, out=None, start=None, size=None, nz=None, nearest=False, chunk_bytes=None,
                      rank=0, world_size=1, device=None, stats=None):
    """A uint8 array-like `volume` [z, y, x] (ndarray, np.memmap, h5py / zarr dataset) whose sections sit at
    `positions` along z (section_spacing's floats, or quantize_positions' integers), resampled onto the even grid of
    spacing 1: output section j is the linear blend of the two sections around position j, weights in 1/256, rounded
    once, half up (resample_z_taps has the table, include/tem_hip.h the voxel's rule; numpy reproduces it bit for
    bit).  `nearest=True` takes the nearer of the two instead: that moves a mask.  The output has `nz` sections
    (default: up to the last position; with section_spacing's positions that is Z).  Where sections are denser than
    the output, the nearest two are blended and the others are not averaged in.

    `start` / `size` are an ROI of the OUTPUT in (x, y, z) order (default: all of it); `out` is a writable uint8
    array-like of the ROI's shape (allocated when None) and is returned.  volume_rescale's pass: the ROI is cut into
    output slabs and the read slabs that hold their taps (resample_z_chunks), together at most `chunk_bytes`; host
    thread -> pinned -> H2D -> one tem_u8_resample_z launch per slab -> D2H -> host write, on double buffers.  Ranks
    take slabs round-robin and write disjoint boxes of a shared `out`.  `stats` receives `read_s`, `write_s` and
    `chunks`.

    There is no resample_z= keyword on predict_cube / predict_volume: the output's shape changes, as with rescale.

    ValueError, before any GPU work: a volume that is not uint8 [z, y, x], positions that quantize_positions refuses or
    that are not one per section, an ROI outside the output, an `out` of another shape or dtype."""
    _check_u8(volume)
    vshape = tuple(int(v) for v in volume.shape)
    if len(vshape) != 3 or min(vshape) < 1:
        raise ValueError(f"volume_resample_z takes a non-empty volume [z, y, x], got shape {vshape}")
    Q = quantize_positions(positions)
    if Q.size != vshape[0]:
        raise ValueError(f"positions must hold one position per section: {vshape[0]}, got {Q.size}")
    taps = np.ascontiguousarray(resample_z_taps(Q, nz))
    grid = (taps.shape[0],) + vshape[1:]
    try:
        box = hist_box(grid, start, size)
    except ValueError as e:
        raise ValueError(f"volume_resample_z: start / size are an ROI of the output of shape {grid}: {e}")
    out = _roi_out(out, box, False)
    chunks = resample_z_chunks(box, vshape, taps, chunk_bytes, rank, world_size)
    p = _SlabPass([volume], [hist_box(vshape)], chunk_bytes, rank, world_size, device, slabs=[r for _, r in chunks])
    lib = H.require_gpu()
    oslabs = [o for o, _ in chunks]
    with p.streaming(stats):
        taps_dev = torch.from_numpy(taps).to(p.dev)
        with p.writing(out, box, oslabs) as outp:
            for k, slab, d, (src,) in p:
                oz0, oz1 = oslabs[k][0]
                _lib.check(lib.tem_u8_resample_z(src.data_ptr(), *d, slab[0][0], vshape[0], outp.device(k).data_ptr(),
                                                 oz1 - oz0, oz0, grid[0], taps.ctypes.data, taps_dev.data_ptr(),
                                                 int(bool(nearest)), p.compute.cuda_stream), "tem_u8_resample_z")
                p.put(k)
    return out


PLANE_LAG_MAX = 8                # tem_u8_zplane_lags: 1 <= nlag <= 8


def _plane_lag(max_lag):
    L = _index(max_lag, "max_lag")
    if not 1 <= L <= PLANE_LAG_MAX:
        raise ValueError(f"max_lag must lie in 1...{PLANE_LAG_MAX}, got {L}")
    return L


def plane_lag_chunks(vol_shape, max_lag=8, chunk_bytes=None, rank=0, world_size=1):
    """Cut a volume of shape `vol_shape` [z, y, x] (one image [y, x]: one section) into slabs for section_plane_sums.
    Returns this rank's list of (core slab, read slab), both (z, y, x) (lo, hi) boxes: the cores are disjoint and their
    union is the volume (hist_chunks' cuts: runs of whole sections, or runs of whole rows of one section; x is never
    cut).  Nothing is looked at along z, so a run of whole sections is its own read slab; where a section is cut into
    rows, the read slab reaches `max_lag` rows past the core, clipped to the section -- where the y partners of its
    last rows lie.  A read slab holds at most `chunk_bytes` bytes (HIST_CHUNK_BYTES when None) wherever one core row
    allows it: as many whole sections as fit, or, where one section is larger than the budget, as many rows as fit next
    to their max_lag rows of halo (one row at the least).  Slabs are in (z, y) order and go round-robin to the ranks.
    Pure host function; ValueError as hist_box and hist_chunks, and for max_lag outside 1...PLANE_LAG_MAX."""
    L = _plane_lag(max_lag)
    budget = _budget(chunk_bytes, rank, world_size)
    box = hist_box(vol_shape)
    return _cut_slabs(box, box[:2], budget, rank, world_size, yreach=(0, L))


def plane_lag_counts(vol_shape, tile, max_lag=8):
    """np.int64 n[gy, gx, 2, L]: the number of voxels (y, x) of tile (i, j) of a section of a volume of shape
    `vol_shape` ([z, y, x] or [y, x]) whose partner lies inside the section -- n[i, j, 0, k - 1] for the partner
    (y + k, x), n[i, j, 1, k - 1] for (y, x + k): the number of terms of section_plane_sums' s[z, i, j, 2 + k] and
    s[z, i, j, 2 + L + k].  Geometry only, in closed form: rows times columns, the tile's rows (columns) cut to
    [0, extent - k).  Pure host function."""
    L = _plane_lag(max_lag)
    th, tw = _clahe_tile(tile)
    gy, gx = clahe_grid(vol_shape, (th, tw))
    _, (_, Y), (_, X) = hist_box(vol_shape)
    k = np.arange(1, L + 1, dtype=np.int64)

    def along(t, g, n):                                                  # [g, 1 + L]: the whole interval, then cut by k
        lo = (np.arange(g, dtype=np.int64) * t)[:, None]
        cut = np.concatenate([[0], k])[None, :]
        return np.maximum(np.minimum(lo + t, n - cut) - lo, 0)
    ry, rx = along(th, gy, Y), along(tw, gx, X)
    n = np.zeros((gy, gx, 2, L), np.int64)
    n[:, :, 0, :] = ry[:, None, 1:] * rx[None, :, :1]
    n[:, :, 1, :] = ry[:, None, :1] * rx[None, :, 1:]
    return n


def section_plane_sums(volume, tile=128, max_lag=8, chunk_bytes=None, rank=0, world_size=1, device=None, stats=None):
    """The sums behind the correlation of every tile of a section with ITSELF displaced by 1...L = `max_lag` (1...8)
    pixels along y and along x: np.int64 s[Z, gy, gx, 3 + 2 L] over the WHOLE uint8 `volume` [z, y, x] (ndarray,
    np.memmap, h5py / zarr dataset; one image [y, x]: Z = 1) on clahe_grid's tiles of `tile` pixels (an int or (th, tw)
    in [1, 2048]).  Over the voxels v = volume[z, y, x] of tile (i, j), with the partner w = volume[z, y + k, x] for
    the y lag k and w = volume[z, y, x + k] for the x lag k, where it lies inside the section -- it may lie outside the
    tile:
      s[z, i, j] = (sum v, sum v v, the number of voxels, sum (v - w)^2 for y lag 1...L, sum (v - w)^2 for x lag 1...L)
    The number of terms per lag is plane_lag_counts'.  Exact integers that numpy reproduces bit for bit, whatever the
    slabs, ranks and launches.  plane_scores turns them into correlations, section_sharpness and find_blurred into the
    sections and regions that are out of focus, plane_curve and z_pitch into the sections' thickness in pixels.

    Out of core exactly as section_lag_sums, over plane_lag_chunks' read slabs (a core of rows reaches L rows further):
    one host thread -> pinned -> H2D -> one tem_u8_zplane_lags launch per slab, adding into a device accumulator.  The
    accumulator holds the whole volume's sums and is read back once where they are at most CLAHE_ACC_BYTES; else it
    holds one slab's core sections and is read back, and added on the host, per slab.  Ranks take slabs round-robin and
    their results add up to the whole.  `stats` receives `read_s` and `chunks`.  ValueError, before any GPU work: a
    non-uint8 volume, a bad tile, max_lag, shape, chunk_bytes or rank."""
    _check_u8(volume)
    L = _plane_lag(max_lag)
    th, tw = _clahe_tile(tile)
    gy, gx = clahe_grid(volume.shape, (th, tw))
    box = hist_box(volume.shape)
    chunks = plane_lag_chunks(volume.shape, L, chunk_bytes, rank, world_size)
    p = _SlabPass([volume], [box], chunk_bytes, rank, world_size, device, slabs=[r for _, r in chunks])
    lib = H.require_gpu()
    Z, Y = box[0][1], box[1][1]
    with p.streaming(stats):
        acc = _RowAccumulator(p.dev, Z, (gy, gx, 3 + 2 * L), _most_rows(c[0] for c, _ in chunks))
        for k, ((s0, _), (y0, _), _), d, (src,) in p:
            (z0, z1), (c0, c1), _ = chunks[k][0]
            _lib.check(lib.tem_u8_zplane_lags(src.data_ptr(), *d, z0 - s0, z1 - s0, c0 - y0, c1 - y0, y0, Y, th, tw, gy,
                                              gx, L, acc.ptr(z0, z1), p.compute.cuda_stream), "tem_u8_zplane_lags")
            acc.add(z0, z1)
        return acc.result()


def _check_plane_sums(s, n, who):
    s, n = np.asarray(s), np.asarray(n)
    if s.ndim != 4 or s.shape[3] < 5 or (s.shape[3] - 3) % 2 or s.shape[3] > 3 + 2 * PLANE_LAG_MAX or \
            s.dtype.kind not in "iu":
        raise ValueError(f"{who}: s must be section_plane_sums' integer array [Z, gy, gx, 3 + 2 L], got {s.dtype} "
                         f"{s.shape}")
    L = (s.shape[3] - 3) // 2
    if n.shape != s.shape[1:3] + (2, L) or n.dtype.kind not in "iu":
        raise ValueError(f"{who}: n must be plane_lag_counts' integer array {s.shape[1:3] + (2, L)}, got {n.dtype} "
                         f"{n.shape}")
    return s.astype(np.int64, copy=False), n.astype(np.int64, copy=False), L


def plane_scores(s, n):
    """float64 r[Z, gy, gx, 2, L]: the correlation of every tile of a section with itself displaced by k = 1...L pixels
    along y (r[..., 0, k - 1]) and along x (r[..., 1, k - 1]), from section_plane_sums' `s` and plane_lag_counts' `n`.
    Host only.  It is the variogram's form, r = 1 - (D / n) / (2 var): with N = s[..., 2], S1 = s[..., 0],
    S2 = s[..., 1] and D the lag's sum of squared differences,
      A = N S2 - S1^2          exact in int64: the tile's variance is A / N^2
      r = 1.0 - (float(D) * float(N * N)) / ((2.0 * float(n)) * float(A))      in this order, in float64
    and 0.0 where A <= 0 (a constant tile correlates with nothing) or n = 0 (no pair)."""
    s, n, L = _check_plane_sums(s, n, "plane_scores")
    N, S1, S2 = s[..., 2], s[..., 0], s[..., 1]
    A = (N * S2 - S1 * S1)[..., None, None]
    D = s[..., 3:].reshape(s.shape[:3] + (2, L))
    ok = (A > 0) & (n[None] > 0)
    r = np.zeros(D.shape, np.float64)
    num = D.astype(np.float64) * (N * N).astype(np.float64)[..., None, None]
    den = (2.0 * n.astype(np.float64))[None] * A.astype(np.float64)
    np.divide(num, den, out=r, where=ok)
    return np.where(ok, 1.0 - r, 0.0)


def _plane_mean_scores(s, n, who, least):
    r = plane_scores(s, n)
    if r.shape[4] < least:
        raise ValueError(f"{who} needs sums of {least} lags at least, got {r.shape[4]}")
    return (r[..., 0, :] + r[..., 1, :]) * 0.5                          # [Z, gy, gx, L]


def section_sharpness(s, n):
    """float64 g[Z, gy, gx]: how fast every tile's correlation with itself decays from a displacement of one pixel to
    two -- with r_k the mean of plane_scores' y and x score at lag k ((r_y + r_x) * 0.5), g = 1 - r_2 / r_1 where
    r_1 > 0, else 0.0.  Host only; needs L >= 2 (ValueError).  A section that is out of focus has lost its fine detail:
    its correlation decays slowly, g is small.  The decay, not 1 - r_1: white detector noise lowers every r_k, k >= 1,
    by the same factor, so the ratio does not see it."""
    m = _plane_mean_scores(s, n, "section_sharpness", 2)
    r1, r2 = m[..., 0], m[..., 1]
    g = np.zeros(r1.shape, np.float64)
    np.divide(r2, r1, out=g, where=r1 > 0)
    return np.where(r1 > 0, 1.0 - g, 0.0)


def find_blurred(s, n, ratio=0.65, min_corr=0.1, section_fraction=0.5):
    """The sections and regions of a volume that are softer than the same place in the other sections -- focus drift, a
    section that lifted off the grid, a frame taken while the beam re-tuned -- from section_plane_sums' `s` and
    plane_lag_counts' `n`: a Defects, as find_defects', which passes them all (a soft section still resembles both
    neighbours).  Host only.  With r_1 the mean lag-1 score of plane_scores and g = section_sharpness(s, n):
      undecided  np.median(r_1[:, i, j]) <= min_corr, or np.median(g[:, i, j]) is not positive: resin, no texture
                 -- no verdict for this column of tiles
      bad        decided and g < ratio x the column's median of g
      sections   the sorted list of sections whose bad tiles are at least `section_fraction` of the decided tiles
      tiles      bool[Z, gy, gx]: the bad tiles of the other sections
      scores     g
    One image (Z = 1) is judged against nothing: every column is undecided.  `ratio` and `section_fraction` lie in
    (0, 1], `min_corr` in (0, 1): ValueError otherwise, as for fewer than two lags.  The limits of the rule: a run of
    soft sections longer than half the stack moves the median, and then the SHARP sections are what differs; a column
    that is soft throughout the stack is not flagged.  join_defects and defects_repair turn the verdict, with
    find_defects', into one Repair."""
    m = _plane_mean_scores(s, n, "find_blurred", 2)
    ratio, frac = _unit(ratio, "ratio", True), _unit(section_fraction, "section_fraction", True)
    min_corr = _unit(min_corr, "min_corr", False)
    g = section_sharpness(s, n)
    Z, grid = g.shape[0], g.shape[1:]
    if Z < 2:
        return Defects([], np.zeros((Z,) + grid, bool), np.ones(grid, bool), g)
    med = np.median(g, axis=0)
    undecided = (np.median(m[..., 0], axis=0) <= min_corr) | ~(med > 0)
    bad = ~undecided[None] & (g < ratio * med[None])
    decided = int((~undecided).sum())
    nbad = bad.reshape(Z, -1).sum(axis=1)
    sections = [z for z in range(Z) if nbad[z] > 0 and nbad[z] >= frac * decided]
    tiles = bad.copy()
    tiles[sections] = False
    return Defects(sections, tiles, undecided, g)


def join_defects(*d):
    """One Defects from several verdicts on the same stack and tile grid (find_defects', find_blurred's): `sections`
    the union, `tiles` the OR with the tiles of bad sections cleared, `undecided` the AND -- a column is without a
    verdict only where no rule had one --, `scores` the first verdict's (scores of different rules do not combine).
    defects_repair(join_defects(...), ...) is then one Repair.  ValueError for no verdict, for something that is not a
    Defects, and for verdicts of different shapes."""
    if not d:
        raise ValueError("join_defects needs one verdict at least")
    try:
        sections = sorted({_index(z, "a section") for v in d for z in v.sections})
        tiles = [np.asarray(v.tiles) != 0 for v in d]
        undecided = [np.asarray(v.undecided) != 0 for v in d]
        scores = d[0].scores
    except (AttributeError, TypeError):
        raise ValueError(f"join_defects needs Defects, got {[type(v).__name__ for v in d]}")
    if any(t.ndim != 3 or t.shape != tiles[0].shape or u.shape != t.shape[1:] for t, u in zip(tiles, undecided)):
        raise ValueError(f"join_defects: the verdicts' shapes differ: {[t.shape for t in tiles]}, "
                         f"{[u.shape for u in undecided]}")
    if any(not 0 <= z < tiles[0].shape[0] for z in sections):
        raise ValueError(f"join_defects: sections outside [0, {tiles[0].shape[0]}): {sections}")
    t = np.logical_or.reduce(tiles)
    t[sections] = False
    return Defects(sections, t, np.logical_and.reduce(undecided), scores)


def plane_curve(s, n, skip=(), min_corr=0.1):
    """float64 curve[K + 1]: the correlation of the stack's texture with itself at an in-plane distance of 0...K
    pixels, K <= L -- the ruler, in pixels, for section_spacing's curve along z (z_pitch).  From section_plane_sums' `s`
    and plane_lag_counts' `n`; host only.  `skip` lists the bad sections (find_defects, find_blurred); the others are
    good.  With r_k the mean of plane_scores' y and x score at lag k:
      1. a tile column is decided where the median of r_1 over the good sections is above `min_corr`;
      2. c[z, k] is the lower median over the decided columns of r_k of section z;
      3. curve[0] = 1 and curve[k] is the median of c[z, k] over the good sections;
      4. the curve is cut behind the last lag up to which it decreases strictly: K.
    ValueError if K < 1 (no good section, no decided column, a flat stack), and for a bad skip or min_corr."""
    m = _plane_mean_scores(s, n, "plane_curve", 1)
    Z, L = m.shape[0], m.shape[3]
    try:
        bad = {_index(z, "a skipped section") for z in skip}
    except TypeError:
        raise ValueError(f"skip must be a list of sections, got {skip!r}")
    if any(not 0 <= z < Z for z in bad):
        raise ValueError(f"skip names sections outside [0, {Z}): {sorted(z for z in bad if not 0 <= z < Z)}")
    mc = _unit(min_corr, "min_corr", closed=False)
    good = [z for z in range(Z) if z not in bad]
    curve = [1.0]
    if good:
        m = m[good]
        decided = np.median(m[..., 0], axis=0) > mc
        if decided.any():
            c = _lower_median(m[:, decided, :], axis=1)                  # [good, L]
            for k in range(L):
                v = float(np.median(c[:, k]))
                if not v < curve[-1]:
                    break
                curve.append(v)
    if len(curve) < 2:
        raise ValueError(f"plane_curve: the correlation does not decrease with the distance ({len(good)} good sections)")
    return np.array(curve, np.float64)


class ZPitch(NamedTuple):
    """z_pitch's estimate: `pixels` the distance of two consecutive sections in in-plane pixels (the median of
    `per_lag`'s used entries), `per_lag` float64[Lz] the estimate of z lag k in [k - 1], NaN where the lag is out of
    reach, `used` bool[Lz]."""
    pixels: float
    per_lag: np.ndarray
    used: np.ndarray


def _check_curve(c, what):
    c = np.asarray(c, np.float64)
    if c.ndim != 1 or c.size < 2 or not np.isfinite(c).all() or c[0] != 1.0 or not np.all(np.diff(c) < 0):
        raise ValueError(f"{what} must be a curve that decreases strictly from 1.0, two values at least, got {c!r}")
    return c


def z_pitch(z_curve, p_curve):
    """How far two consecutive sections lie apart, in in-plane pixels: ZPitch(pixels, per_lag, used) from `z_curve`,
    the correlation at 0...Lz sections (section_spacing's Spacing.curve), and `p_curve`, the correlation at 0...K
    pixels (plane_curve).  Host only.  For every z lag k with p_curve[K] < z_curve[k] < 1, the in-plane distance at
    which the texture is as correlated as across k sections is the piecewise-linear inverse of p_curve at z_curve[k]
    (section_spacing's step 4); divided by k it is that lag's estimate, and `pixels` is the median of the estimates.
    pitch_step turns it into volume_rescale's step.  The assumption: the tissue's statistics and the imaging blur are
    isotropic -- a section is thick and the beam's spot is not, so a real stack's pitch comes out a little large.
    ValueError for curves that do not decrease strictly from 1.0, and where no lag is within reach."""
    zc, pc = _check_curve(z_curve, "z_curve"), _check_curve(p_curve, "p_curve")
    K = pc.size - 1
    per_lag = np.full(zc.size - 1, np.nan)
    used = (zc[1:] > pc[K]) & (zc[1:] < 1.0)
    if not used.any():
        raise ValueError(f"z_pitch: no z lag lies within reach of the in-plane curve: z {zc.tolist()}, plane {pc.tolist()}")
    dist = np.interp(zc[1:], pc[::-1], np.arange(K, -1, -1.0))
    per_lag[used] = dist[used] / np.arange(1, zc.size)[used]
    return ZPitch(float(np.median(per_lag[used])), per_lag, used)


def pitch_step(pixels):
    """volume_rescale's step (1, 1, Fraction) in (x, y, z) order that makes a stack isotropic whose sections lie
    `pixels` in-plane pixels apart (z_pitch): along z an output voxel is 1 / pixels sections, brought to the nearest
    p / q with 1 <= p, q <= RESCALE_MAX_PQ (the smallest q on a tie).  ValueError for a pitch that is not a positive
    finite number, and where 1 / pixels lies outside [1 / RESCALE_MAX_STEP, RESCALE_MAX_STEP]."""
    try:
        if isinstance(pixels, (bool, np.bool_, str, bytes)):
            raise TypeError
        x = float(pixels)
    except (TypeError, ValueError):
        raise ValueError(f"pixels must be a number, got {pixels!r}")
    if not (np.isfinite(x) and x > 0) or not 1 / RESCALE_MAX_STEP <= 1 / x <= RESCALE_MAX_STEP:
        raise ValueError(f"a pitch must be positive and 1 / pixels within [1/{RESCALE_MAX_STEP}, {RESCALE_MAX_STEP}], "
                         f"got {pixels!r}")
    best = None
    for q in range(1, RESCALE_MAX_PQ + 1):
        p = min(max(int(np.floor(q / x + 0.5)), 1), RESCALE_MAX_PQ)
        f = Fraction(p, q)
        if RESCALE_MAX_STEP * f >= 1 and f <= RESCALE_MAX_STEP and (best is None or abs(f - 1 / Fraction(x)) < best[0]):
            best = (abs(f - 1 / Fraction(x)), f)
    return (Fraction(1), Fraction(1), best[1])


SHIFT_MAX_RADIUS = 8             # offsets of section_shift_sums: [-r, r]^2, r in 1...8
SHIFT_MAX_CENTER = 1024          # tem_u8_zshift_tiles_at: |cy|, |cx| of a search window's centre, at most
SHIFT_MAX_LEVELS = 6             # section_shifts_coarse_to_fine: the centres stay below (8 - 1) (2^7 - 2) = 882


def _shift_radius(radius):
    r = _index(radius, "radius")
    if not 1 <= r <= SHIFT_MAX_RADIUS:
        raise ValueError(f"radius must lie in 1...{SHIFT_MAX_RADIUS}, got {r}")
    return r


def zshift_chunks(vol_shape, radius, chunk_bytes=None, rank=0, world_size=1):
    """Cut a volume of shape `vol_shape` [z, y, x] (one image [y, x]: one section) into slabs for section_shift_sums.
    Returns this rank's list of (core slab, read slab), both (z, y, x) (lo, hi) boxes: the cores are disjoint and their
    union is the volume (hist_chunks' cuts: runs of whole sections, or runs of whole rows of one section; x is never
    cut); a read slab is its core plus `radius` rows on each side, clipped to the volume, and the same rows of the next
    section where the volume has one -- where the partners of its last core plane lie.  A read slab holds at most
    `chunk_bytes` bytes (HIST_CHUNK_BYTES when None) wherever one core row allows it: as many whole sections per core as
    fit next to the one above them, or, where two sections are larger than the budget, one section's rows, as many as
    fit twice next to their 2 radius rows of halo (one row at the least).  Slabs are in (z, y) order and go round-robin
    to the ranks.  Pure host function; ValueError as zcorr_chunks, and for a radius outside 1...8."""
    return _zshift_chunks(vol_shape, radius, 0, 0, chunk_bytes, rank, world_size)


def _zshift_chunks(vol_shape, radius, lo, hi, chunk_bytes, rank, world_size):
    """zshift_chunks' list for windows centred within [lo, hi] rows of zero, lo <= 0 <= hi: a read slab is its core plus
    radius - lo rows below and radius + hi rows above it."""
    r = _shift_radius(radius)
    budget = _budget(chunk_bytes, rank, world_size)
    box = hist_box(vol_shape)
    return _cut_slabs(box, box[:2], budget, rank, world_size, zreach=(0, min(1, box[0][1] - 1)), yreach=(r - lo, r + hi))


def shift_counts(vol_shape, tile, radius):
    """np.int64 n[gy, gx, R, R], R = 2 radius + 1: the number of voxels (y, x) of tile (i, j) of a section of a volume of
    shape `vol_shape` ([z, y, x] or [y, x]) whose partner (y + dy, x + dx) lies inside the section -- the number of
    terms of section_shift_sums' q[z, i, j, dy + radius, dx + radius].  Geometry only, in closed form: rows times
    columns, each the length of the tile's interval cut to [-d, extent - d).  Pure host function."""
    r = _shift_radius(radius)
    th, tw = _clahe_tile(tile)
    gy, gx = clahe_grid(vol_shape, (th, tw))
    return _shift_counts(vol_shape, (th, tw), r, np.zeros((1, gy, gx, 2), np.int64))[0]


def _shift_counts(vol_shape, tile, r, C):
    """shift_counts for every pair z and tile (i, j) at the total offsets C[z, i, j] + (dy, dx): int64[P, gy, gx, R, R]
    from centres C int64[P, gy, gx, 2]."""
    th, tw = tile
    _, (_, Y), (_, X) = hist_box(vol_shape)
    gy, gx = C.shape[1:3]
    local = np.arange(-r, r + 1, dtype=np.int64)

    def along(t, g, n, c, axis):
        lo = (np.arange(g, dtype=np.int64) * t).reshape((1, g, 1, 1) if axis == 1 else (1, 1, g, 1))
        d = c[..., None] + local
        return np.maximum(np.minimum(np.minimum(lo + t, n), n - d) - np.maximum(lo, -d), 0)
    return along(th, gy, Y, C[..., 0], 1)[..., :, None] * along(tw, gx, X, C[..., 1], 2)[..., None, :]


def section_shift_sums(volume, tile=128, radius=4, chunk_bytes=None, rank=0, world_size=1, device=None, stats=None):
    """The sums behind the correlation of every tile of a section with the next section displaced by every integer
    offset (dy, dx) in [-radius, radius]^2: np.int64 q[Z, gy, gx, R, R, 5], R = 2 radius + 1, over the WHOLE uint8
    `volume` [z, y, x] (ndarray, np.memmap, h5py / zarr dataset; one image [y, x]: Z = 1) on clahe_grid's tiles of `tile`
    pixels (an int or (th, tw) in [1, 2048]).  Over the voxels (y, x) of tile (i, j) whose partner (y + dy, x + dx) lies
    inside the section -- it may lie outside the tile --, with v = volume[z, y, x], w = volume[z + 1, y + dy, x + dx]:
      q[z, i, j, dy + radius, dx + radius] = (sum v, sum v v, sum w, sum w w, sum v w);   the last section's are 0.
    The number of terms is shift_counts'.  Exact integers that numpy reproduces bit for bit, whatever the slabs, ranks
    and launches.  shift_scores turns them into correlations, section_shifts into the displacement of every section
    against the one below it.

    Out of core exactly as section_sums, over read slabs that reach `radius` rows and one section past their core
    (zshift_chunks): one host thread -> pinned -> H2D -> one tem_u8_zshift_tiles launch per slab, adding into a device
    accumulator.  The accumulator holds the whole volume's Z*gy*gx*R*R*40 bytes and is read back once where that is at
    most CLAHE_ACC_BYTES; else it holds one slab's core sections and is read back, and added on the host, per slab.
    Ranks take slabs round-robin and their results add up to the whole.  `stats` receives `read_s` and `chunks`.
    ValueError, before any GPU work: a non-uint8 volume, a bad tile, radius, shape, chunk_bytes or rank."""
    return _shift_sums_pass(volume, None, tile, radius, chunk_bytes, rank, world_size, device, stats)


def _shift_sums_pass(volume, centers, tile, radius, chunk_bytes, rank, world_size, device, stats):
    """section_shift_sums (centers None: tem_u8_zshift_tiles) and section_shift_sums_at (tem_u8_zshift_tiles_at with the
    table of shift_centers) are this one pass."""
    _check_u8(volume)
    th, tw = _clahe_tile(tile)
    r = _shift_radius(radius)
    gy, gx = clahe_grid(volume.shape, (th, tw))
    box = hist_box(volume.shape)
    lo = hi = cx_max = 0
    if centers is not None:
        C = shift_centers(centers, volume.shape, (th, tw))
        if C.size:
            lo, hi = min(int(C[..., 0].min()), 0), max(int(C[..., 0].max()), 0)
            cx_max = int(np.abs(C[..., 1]).max())
    chunks = _zshift_chunks(volume.shape, r, lo, hi, chunk_bytes, rank, world_size)
    p = _SlabPass([volume], [box], chunk_bytes, rank, world_size, device, slabs=[s for _, s in chunks])
    lib = H.require_gpu()
    R = 2 * r + 1
    Z, Y = box[0][1], box[1][1]
    with p.streaming(stats):
        acc = _RowAccumulator(p.dev, Z, (gy, gx, R, R, 5), _most_rows(c[0] for c, _ in chunks))
        if centers is not None:                                  # uploaded once; the last section's row is never read
            table = torch.zeros((Z, gy * gx * 2), dtype=torch.int32, device=p.dev)
            if C.size:
                table[:Z - 1] = torch.from_numpy(C.astype(np.int32).reshape(Z - 1, -1)).to(p.dev)
        for k, ((s0, _), (y0, _), _), d, (src,) in p:
            (z0, z1), (c0, c1), _ = chunks[k][0]
            where = acc.ptr(z0, z1)
            if centers is None:
                _lib.check(lib.tem_u8_zshift_tiles(src.data_ptr(), *d, z0 - s0, z1 - s0, c0 - y0, c1 - y0, y0, Y, th, tw,
                                                   gy, gx, r, where, p.compute.cuda_stream), "tem_u8_zshift_tiles")
            else:
                _lib.check(lib.tem_u8_zshift_tiles_at(src.data_ptr(), *d, z0 - s0, z1 - s0, c0 - y0, c1 - y0, y0, Y, th,
                                                      tw, gy, gx, r, table.data_ptr() + 8 * gy * gx * z0, lo, hi, cx_max,
                                                      where, p.compute.cuda_stream), "tem_u8_zshift_tiles_at")
            acc.add(z0, z1)
        return acc.result()


def _check_shift_sums(q, n, who):
    q, n = np.asarray(q), np.asarray(n)
    if q.ndim != 6 or q.shape[5] != 5 or q.dtype.kind not in "iu" or q.shape[3] != q.shape[4] or \
            q.shape[3] % 2 != 1 or not 3 <= q.shape[3] <= 2 * SHIFT_MAX_RADIUS + 1:
        raise ValueError(f"{who}: q must be section_shift_sums' integer array [Z, gy, gx, R, R, 5], got {q.dtype} "
                         f"{q.shape}")
    if who.endswith("_pairs"):                                   # a row of sums and of counts per pair
        if n.shape != q.shape[:5] or n.dtype.kind not in "iu":
            raise ValueError(f"{who}: n must be shift_counts_pairs' integer array {q.shape[:5]}, got {n.dtype} {n.shape}")
    elif who.endswith("_at"):                                    # the counts carry the pair axis
        if n.shape != (max(q.shape[0] - 1, 0),) + q.shape[1:5] or n.dtype.kind not in "iu":
            raise ValueError(f"{who}: n must be shift_counts_at's integer array "
                             f"{(max(q.shape[0] - 1, 0),) + q.shape[1:5]}, got {n.dtype} {n.shape}")
    elif n.shape != q.shape[1:5] or n.dtype.kind not in "iu":
        raise ValueError(f"{who}: n must be shift_counts' integer array {q.shape[1:5]}, got {n.dtype} {n.shape}")
    return q.astype(np.int64, copy=False), n.astype(np.int64, copy=False)


def shift_scores(q, n):
    """float64 c[Z - 1, gy, gx, R, R]: the Pearson correlation of every tile of section z with section z + 1 displaced
    by (dy, dx), from section_shift_sums' `q` and shift_counts' `n`.  Host only.  Per entry, with
    (S1, S2, T1, T2, P) = q[z, i, j, dy + r, dx + r]:
      A = n S2 - S1^2,   B = n T2 - T1^2,   N = n P - S1 T1
    -- exact in int64: a tile holds at most 2^22 voxels of at most 255, so every term stays below 2^61 -- and
    c = N / (sqrt(A) sqrt(B)) where A > 0 and B > 0, else 0.0: a constant tile correlates with nothing."""
    return _shift_scores(*_check_shift_sums(q, n, "shift_scores"))


def _shift_scores(q, n):
    """shift_scores' formula; `n` is per tile and offset [gy, gx, R, R], or carries the pair axis in front."""
    return _pair_scores(q[:-1], n)


def _pair_scores(q, n):
    """shift_scores' formula on one row of sums per PAIR, q[P, gy, gx, R, R, 5]: float64 c[P, gy, gx, R, R]."""
    c = np.zeros(q.shape[:5], np.float64)
    if not q.shape[0]:
        return c
    S1, S2, T1, T2, P = (q[..., k] for k in range(5))
    A, B, N = n * S2 - S1 * S1, n * T2 - T1 * T1, n * P - S1 * T1
    ok = (A > 0) & (B > 0)
    c[ok] = N[ok] / (np.sqrt(A[ok].astype(np.float64)) * np.sqrt(B[ok].astype(np.float64)))
    return c


class Shifts(NamedTuple):
    """section_shifts' verdict: `pairs` int64[Z - 1, 2] the (dy, dx) by which section z + 1 is displaced against section
    z, `tiles` int64[Z - 1, gy, gx, 2] the offset of every tile's largest score, `peak` float64[Z - 1, gy, gx] that
    score, `decided` bool[Z - 1, gy, gx] the tiles that were counted, `unresolved` the sorted list of the pairs z without
    a decided tile."""
    pairs: np.ndarray
    tiles: np.ndarray
    peak: np.ndarray
    decided: np.ndarray
    unresolved: list


def section_shifts(q, n, min_corr=0.1):
    """How far consecutive sections sit apart, from section_shift_sums' `q` and shift_counts' `n`.  Host only.  With
    c = shift_scores(q, n) and r the radius:
      tiles[z, i, j]  = the offset (dy, dx) of the largest c[z, i, j]; the offsets are searched in the order
                        (dy^2 + dx^2, dy, dx), so ties go to the smaller displacement
      peak[z, i, j]   = the score at that offset
      decided         peak > min_corr, and the offset not on the rim of the search (|dy| < r and |dx| < r): a maximum
                      on the rim says only "at least this far"
      pairs[z]        per axis the lower median, sorted[(k - 1) // 2], of the k decided tiles' offsets: section z + 1
                      shows at (y + dy, x + dx) what section z shows at (y, x)
      unresolved      the pairs without a decided tile; they get (0, 0)
    `min_corr` lies in (0, 1): ValueError otherwise.  shift_positions adds the pairs up into a position per section,
    volume_shift moves the sections there."""
    q, n = _check_shift_sums(q, n, "section_shifts")
    min_corr = _unit(min_corr, "min_corr", False)
    return _section_shifts(_shift_scores(q, n), None, min_corr)[0]


def _section_shifts(c, C, min_corr):
    """section_shifts' rules on the scores `c` of searches centred on C int64[Z - 1, gy, gx, 2] (None: zero): the order
    of the search, the rim and the tie-break are those of the LOCAL offset; `tiles` and `pairs` are TOTAL offsets,
    centre + local; a pair without a decided tile gets the per-axis lower median of its tiles' centres.  Returns the
    Shifts and the local offsets of `tiles`."""
    R = c.shape[3]
    r = R // 2
    order = sorted(((dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)),
                   key=lambda o: (o[0] * o[0] + o[1] * o[1], o[0], o[1]))
    offs = np.array(order, np.int64)                                             # [R R, 2]
    flat = c.reshape(c.shape[:3] + (R * R,))[..., (offs[:, 0] + r) * R + offs[:, 1] + r]
    best = flat.argmax(axis=-1)                                                  # the first of equal maxima
    local = offs[best]
    peak = np.take_along_axis(flat, best[..., None], axis=-1)[..., 0]
    decided = (peak > min_corr) & (np.abs(local) < r).all(axis=-1)
    tiles = local if C is None else C + local
    pairs, unresolved = np.zeros((c.shape[0], 2), np.int64), []
    for z in range(c.shape[0]):
        k = int(decided[z].sum())
        if k == 0:
            unresolved.append(z)
            if C is not None:                                                    # the guess stands
                pairs[z] = np.sort(C[z].reshape(-1, 2), axis=0)[(C[z].size // 2 - 1) // 2]
            continue
        pairs[z] = np.sort(tiles[z][decided[z]], axis=0)[(k - 1) // 2]
    return Shifts(pairs, tiles, peak, decided, unresolved), local


def shift_positions(pairs, window=None):
    """np.int64 P[Z, 2]: the (y, x) position of every section in the frame of section 0, from section_shifts' pairs
    [Z - 1, 2]: P[0] = 0, P[z + 1] = P[z] + pairs[z].  With `window` (an odd int >= 3) the lower median of P over the
    sections [z - window // 2, z + window // 2], clipped to the stack, is subtracted per axis: that removes the jitter
    and keeps a real oblique trend, which a cut through tilted tissue shows.  Integers throughout.  Host only;
    ValueError for pairs of another shape or dtype, or a bad window."""
    pairs = np.asarray(pairs)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
        raise ValueError(f"pairs must be integers of shape [Z - 1, 2], got {pairs.dtype} {pairs.shape}")
    P = np.zeros((pairs.shape[0] + 1, 2), np.int64)
    np.cumsum(pairs.astype(np.int64), axis=0, out=P[1:])
    if window is None:
        return P
    w = _index(window, "window")
    if w < 3 or w % 2 != 1:
        raise ValueError(f"window must be an odd integer >= 3, got {w}")
    h, Z = w // 2, P.shape[0]
    trend = np.empty_like(P)
    for z in range(Z):
        run = np.sort(P[max(z - h, 0):min(z + h + 1, Z)], axis=0)
        trend[z] = run[(run.shape[0] - 1) // 2]
    return P - trend


def volume_shift(volume, positions, out=None, start=None, size=None, fill=0):
    """The ROI [start, start + size) ((x, y, z) order; default: the whole volume) of an array-like `volume` [z, y, x]
    (ndarray, np.memmap, h5py / zarr dataset) with every section moved back by its position:
      out[z, y, x] = volume[z, y + P[z, 0], x + P[z, 1]]   where that voxel exists, else `fill`
    with P = `positions`, integers [Z, 2] (shift_positions'), written into `out`: a writable array-like of the ROI's
    shape and the volume's dtype (allocated when None), which is returned.  The same call moves a mask.
    Host only, section by section like defect_mask: it is a copy, and the out-of-core passes next to it are bound by
    their one host thread's read and write, so a device leg would add two transfers and no speed.  Shifts below a pixel,
    rotation, scale and shear need resampling: that is volume_warp, on the device.  ValueError for a
    volume that is not [z, y, x], positions of another shape or dtype, an ROI outside the volume, an `out` of another
    shape or dtype, a fill that the dtype does not hold."""
    vshape = tuple(int(v) for v in volume.shape)
    if len(vshape) != 3:
        raise ValueError(f"volume_shift needs a volume [z, y, x], got shape {vshape}")
    dtype = np.dtype(getattr(volume, "dtype", np.uint8))
    P = np.asarray(positions)
    if P.shape != (vshape[0], 2) or P.dtype.kind not in "iu":
        raise ValueError(f"positions must be integers of shape {(vshape[0], 2)}, got {P.dtype} {P.shape}")
    try:
        if isinstance(fill, (bool, np.bool_)) and dtype.kind != "b":
            raise TypeError
        f = np.array(fill).astype(dtype)
        if f.ndim or f != fill:
            raise TypeError
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"fill must be one value that {dtype} holds, got {fill!r}")
    (z0, z1), (y0, y1), (x0, x1) = hist_box(vshape, start, size)
    shape = (z1 - z0, y1 - y0, x1 - x0)
    if out is None:
        out = np.zeros(shape, dtype)
    elif tuple(out.shape) != shape or getattr(out, "dtype", None) != dtype:
        raise ValueError(f"out must be {dtype} of the ROI's shape {shape}, got {getattr(out, 'dtype', None)} "
                         f"{tuple(out.shape)}")
    Y, X = vshape[1:]
    sec = np.empty(shape[1:], dtype)
    for z in range(z0, z1):
        dy, dx = int(P[z, 0]), int(P[z, 1])
        ya, yb, xa, xb = max(y0 + dy, 0), min(y1 + dy, Y), max(x0 + dx, 0), min(x1 + dx, X)    # what exists, in the volume
        sec[...] = f
        if ya < yb and xa < xb:
            sec[ya - dy - y0:yb - dy - y0, xa - dx - x0:xb - dx - x0] = volume[z, ya:yb, xa:xb]
        out[z - z0] = sec
    return out


class SubShifts(NamedTuple):
    """shift_subpixel's verdict: `offsets` float64[Z - 1, gy, gx, 2] the (dy, dx) of every tile, refined below a pixel
    where the tile is decided, `decided` and `peak` those of section_shifts, unchanged."""
    offsets: np.ndarray
    decided: np.ndarray
    peak: np.ndarray


def shift_subpixel(q, n, min_corr=0.1):
    """section_shifts' tile offsets refined below a pixel, from section_shift_sums' `q` and shift_counts' `n`.  Host
    only.  It starts from section_shifts' `tiles`, `decided` and `peak`, unchanged.  A decided tile is never on the rim
    of the search, so both neighbours of its peak exist along each axis; per axis, with c0 the peak of shift_scores and
    m, p the scores one offset below and above it along that axis, the vertex of the parabola through the three,
      delta = (m - p) / (2 (m - 2 c0 + p)),   clipped to [-1/2, 1/2],
    is added where the denominator is below 0 (a true maximum).  Undecided tiles keep their integer offset and stay
    undecided.  fit_section_maps turns the offsets into one map per pair."""
    q, n = _check_shift_sums(q, n, "section_shifts")
    min_corr = _unit(min_corr, "min_corr", False)
    return _shift_subpixel(_shift_scores(q, n), None, min_corr)


def _shift_subpixel(c, C, min_corr):
    """shift_subpixel on the scores `c` of searches centred on C (None: zero): the parabola on the local table, added to
    the total offset."""
    s, local = _section_shifts(c, C, min_corr)
    r = c.shape[-1] // 2
    offsets = s.tiles.astype(np.float64)
    for z, i, j in zip(*np.nonzero(s.decided)):
        dy, dx = (int(v) for v in local[z, i, j])
        c0 = c[z, i, j, dy + r, dx + r]
        for axis, (m, p) in enumerate(((c[z, i, j, dy + r - 1, dx + r], c[z, i, j, dy + r + 1, dx + r]),
                                       (c[z, i, j, dy + r, dx + r - 1], c[z, i, j, dy + r, dx + r + 1]))):
            den = m - 2.0 * c0 + p
            if den < 0:
                offsets[z, i, j, axis] += min(max((m - p) / (2.0 * den), -0.5), 0.5)
    return SubShifts(offsets, s.decided, s.peak)


def shift_centers(centers, vol_shape, tile):
    """The centres of the `_at` family's search windows, validated and expanded: np.int64 C[Z - 1, gy, gx, 2] = (cy, cx)
    per pair of sections z (section z against z + 1) and tile (i, j) of clahe_grid's tiles of `tile` pixels over a
    volume of shape `vol_shape`.  `centers` is integers of shape [Z - 1, 2] (one centre per pair, for every tile) or
    [Z - 1, gy, gx, 2]; one image [y, x] has no pairs (Z - 1 = 0).  A centre goes per TILE because a rotation of a
    fraction of a degree already displaces the corners of a large section by tens of pixels against its middle.
    Pure host function; ValueError for another shape, a dtype that is not integer, and a component beyond
    SHIFT_MAX_CENTER = 1024 (the message names the pair and the tile)."""
    th, tw = _clahe_tile(tile)
    gy, gx = clahe_grid(vol_shape, (th, tw))
    return _centers_table(centers, hist_box(vol_shape)[0][1] - 1, gy, gx)


def _centers_table(centers, P, gy, gx):
    """shift_centers for `P` pairs on a grid of gy x gx tiles."""
    C = np.asarray(centers)
    if C.dtype.kind not in "iu" or C.shape not in ((P, 2), (P, gy, gx, 2)):
        raise ValueError(f"centers must be integers of shape {(P, 2)} or {(P, gy, gx, 2)}, got {C.dtype} {C.shape}")
    C = C.astype(np.int64)
    if C.ndim == 2:
        C = np.broadcast_to(C[:, None, None, :], (P, gy, gx, 2)).copy()
    far = np.argwhere(np.abs(C) > SHIFT_MAX_CENTER)
    if far.size:
        z, i, j, _ = (int(v) for v in far[0])
        raise ValueError(f"centers: pair {z}, tile ({i}, {j}) is centred on {tuple(int(v) for v in C[z, i, j])}, beyond "
                         f"+-{SHIFT_MAX_CENTER}")
    return C


def _shift_reach(reach):
    try:
        lo, hi = reach
        lo, hi = _index(lo, "reach"), _index(hi, "reach")
    except TypeError:
        raise ValueError(f"reach must be a pair of integers (lo, hi), got {reach!r}")
    if not -SHIFT_MAX_CENTER <= lo <= 0 <= hi <= SHIFT_MAX_CENTER:
        raise ValueError(f"reach (lo, hi) needs -{SHIFT_MAX_CENTER} <= lo <= 0 <= hi <= {SHIFT_MAX_CENTER}, got {reach!r}")
    return lo, hi


def zshift_chunks_at(vol_shape, radius, reach, chunk_bytes=None, rank=0, world_size=1):
    """zshift_chunks for section_shift_sums_at: `reach` = (lo, hi), lo <= 0 <= hi, are the least and the largest row
    centre cy of the pass (and 0).  The cores are cut as zshift_chunks cuts them; a read slab is its core plus the rows
    [lo - radius, hi + radius] around it, clipped to the volume, and the same rows of the next section -- every partner
    row of the core at every centre within the reach; where rows are cut, as many as fit twice next to their
    2 radius + hi - lo rows of halo (one row at the least).  reach (0, 0) gives zshift_chunks' list.  Pure host
    function; ValueError as zshift_chunks, and for a reach that is no such pair of integers within SHIFT_MAX_CENTER."""
    lo, hi = _shift_reach(reach)
    return _zshift_chunks(vol_shape, radius, lo, hi, chunk_bytes, rank, world_size)


def shift_counts_at(vol_shape, tile, radius, centers):
    """np.int64 n[Z - 1, gy, gx, R, R]: shift_counts for searches centred on `centers` (shift_centers): the number of
    voxels (y, x) of tile (i, j) whose partner (y + cy + dy, x + cx + dx) lies inside the section, (cy, cx) the centre
    of pair z and tile (i, j) -- the number of terms of section_shift_sums_at's q[z, i, j, dy + radius, dx + radius].
    The same closed form with the total offset; 0 where the window has left the section.  Pure host function."""
    r = _shift_radius(radius)
    th, tw = _clahe_tile(tile)
    return _shift_counts(vol_shape, (th, tw), r, shift_centers(centers, vol_shape, (th, tw)))


def section_shift_sums_at(volume, centers, tile=128, radius=4, chunk_bytes=None, rank=0, world_size=1, device=None,
                          stats=None):
    """section_shift_sums with the search of every pair of sections and tile centred on an offset of its own:
    np.int64 q[Z, gy, gx, R, R, 5] over the WHOLE uint8 `volume`, where for the centre (cy, cx) = C[z, i, j] of
    `centers` (shift_centers: [Z - 1, 2] or [Z - 1, gy, gx, 2] integers within SHIFT_MAX_CENTER) and the local offset
    (dy, dx) in [-radius, radius]^2 the sums run over the voxels (y, x) of tile (i, j) whose partner
    (y + cy + dy, x + cx + dx) lies inside the section, v = volume[z, y, x], w = volume[z + 1, y + cy + dy, x + cx + dx]:
      q[z, i, j, dy + radius, dx + radius] = (sum v, sum v v, sum w, sum w w, sum v w);   the last section's are 0.
    The number of terms is shift_counts_at's.  Exact integers that numpy reproduces bit for bit; zero centres give
    section_shift_sums' array.

    The pass is section_shift_sums', over zshift_chunks_at with reach = the least and the largest cy over all centres
    (and 0): the table goes to the device once, as int32; one tem_u8_zshift_tiles_at launch per slab, given the table's
    rows of the slab's first core section; the same accumulator and read-back rule (CLAHE_ACC_BYTES); ranks' results
    add.  `stats` receives `read_s` and `chunks`.  ValueError, before any GPU work: as section_shift_sums, and
    shift_centers' for the centres."""
    if centers is None:
        raise ValueError("centers must be integers of shape [Z - 1, 2] or [Z - 1, gy, gx, 2], got None")
    return _shift_sums_pass(volume, centers, tile, radius, chunk_bytes, rank, world_size, device, stats)


def shift_scores_at(q, n):
    """shift_scores for section_shift_sums_at's `q` and shift_counts_at's `n`, which carries the pair axis:
    float64 c[Z - 1, gy, gx, R, R] indexed by the LOCAL offset.  Host only."""
    return _shift_scores(*_check_shift_sums(q, n, "shift_scores_at"))


def _check_centers_for(q, centers, who):
    C = np.asarray(centers)
    P = q.shape[0] if who.endswith("_pairs") else max(q.shape[0] - 1, 0)
    if C.dtype.kind not in "iu" or C.shape not in ((P, 2), (P,) + q.shape[1:3] + (2,)):
        raise ValueError(f"{who}: centers must be integers of shape {(P, 2)} or {(P,) + q.shape[1:3] + (2,)}, got "
                         f"{C.dtype} {C.shape}")
    C = C.astype(np.int64)
    return np.broadcast_to(C[:, None, None, :], (P,) + q.shape[1:3] + (2,)) if C.ndim == 2 else C


def section_shifts_at(q, n, centers, min_corr=0.1):
    """section_shifts for searches centred on `centers` ([Z - 1, 2] or [Z - 1, gy, gx, 2] integers), from
    section_shift_sums_at's `q` and shift_counts_at's `n`.  Host only.  The rules are section_shifts' on the LOCAL
    offsets -- the search order (dy^2 + dx^2, dy, dx), ties to the smaller local displacement, the rim |dy| = r or
    |dx| = r not trusted --; `tiles` and `pairs` of the Shifts are TOTAL offsets, centre + local.  A pair without a
    decided tile is listed in `unresolved` and gets the per-axis lower median of its tiles' centres: the guess stands.
    Zero centres reproduce section_shifts."""
    q, n = _check_shift_sums(q, n, "section_shifts_at")
    C = _check_centers_for(q, centers, "section_shifts_at")
    min_corr = _unit(min_corr, "min_corr", False)
    return _section_shifts(_shift_scores(q, n), C, min_corr)[0]


def shift_subpixel_at(q, n, centers, min_corr=0.1):
    """shift_subpixel for searches centred on `centers`: SubShifts whose offsets are section_shifts_at's total tile
    offsets plus the vertex of the same parabola on the local table.  fit_section_maps takes it unchanged."""
    q, n = _check_shift_sums(q, n, "section_shifts_at")
    C = _check_centers_for(q, centers, "section_shifts_at")
    min_corr = _unit(min_corr, "min_corr", False)
    return _shift_subpixel(_shift_scores(q, n), C, min_corr)


class CoarseShifts(NamedTuple):
    """section_shifts_coarse_to_fine's verdict, all of the finest level (the volume itself): `shifts` the Shifts in total
    offsets, `q` and `n` the sums and counts of the last search and `centers` int64[Z - 1, gy, gx, 2] where it was
    centred -- what shift_subpixel_at takes."""
    shifts: Shifts
    q: np.ndarray
    n: np.ndarray
    centers: np.ndarray


def section_shifts_coarse_to_fine(volume, tile=128, radius=4, levels=3, min_corr=0.1, min_decided=0.5, coarse=None,
                                  chunk_bytes=None, device=None, stats=None):
    """How far consecutive sections of the uint8 `volume` [z, y, x] sit apart where that is far more than a search
    radius: section_shifts on a pyramid.  V_0 = volume, V_(l+1) = volume_rescale(V_l, (2, 2, 1)) for l < `levels`
    (1...6; sections halved in y and x on the device, z kept).  The coarsest level is searched around zero; every finer
    level l is searched around the doubled answer of level l + 1 (section_shift_sums_at -> section_shifts_at): the
    centre of tile (i, j) of pair z is 2 tiles_(l+1)[z, i // 2, j // 2] where that coarse tile is decided, else
    2 pairs_(l+1)[z].  `tile` and `radius` are the same at every level, in that level's pixels, so one pixel of the
    coarsest search is 2^levels pixels of the volume and a displacement of up to (radius - 1) 2^levels is found there.

    Returns CoarseShifts(shifts, q, n, centers) of level 0.  There a pair with fewer than `min_decided` (a number in
    [0, 1]) of its tiles decided, and every pair section_shifts_at could not resolve, is listed in `unresolved` and gets
    (0, 0): a section is not moved on a guess.  That is also how a displacement beyond the reach of the coarsest level
    shows: its finer searches are centred off the truth and few of their tiles are decided -- chance peaks just above
    `min_corr` can decide some, which is why the fraction, not the peaks, is the test.

    `coarse`: None, or `levels` writable uint8 array-likes for V_1, V_2, ... of rescale_shape's shapes (np.memmap, h5py,
    zarr) where the pyramid does not fit in memory; ndarrays are allocated otherwise.  `chunk_bytes` and `device` go to
    every pass; `stats` receives `read_s` and `chunks` summed over all passes.  ValueError, before any GPU work: a volume
    that is not a uint8 [z, y, x], a bad tile, radius, min_corr, min_decided or chunk_bytes, levels outside 1...6 or so
    many that the coarsest section's shorter side min(Y, X) >> levels falls below 4 radius, a `coarse` of another
    length, shape or dtype."""
    def measure(v, C, tile, r, st):                              # looked up at the call: the tests' stand-ins apply
        return section_shift_sums_at(v, C, tile, r, chunk_bytes=chunk_bytes, device=device, stats=st)
    s, q, n, C = _shifts_pyramid(volume, None, measure, tile, radius, levels, min_corr, min_decided, coarse, chunk_bytes,
                                 device, stats, "section_shifts_coarse_to_fine")
    return CoarseShifts(s, q, n, C)


def _shifts_pyramid(volume, pairs, measure, tile, radius, levels, min_corr, min_decided, coarse, chunk_bytes, device,
                    stats, who):
    """The one coarse-to-fine driver: section_shifts_coarse_to_fine (`pairs` None: section z against z + 1 for every z)
    and section_shifts_bridged (`pairs` int64[P, 2], checked).  `measure(V_l, C, tile, r, st)` returns level l's sums
    with a row per pair in front (further rows are ignored).  The pyramid holds the sections that a pair spans, run by
    run; all of them for the chain of every z.  Returns (Shifts, q, n, C) of level 0."""
    _check_u8(volume)
    vshape = tuple(int(v) for v in volume.shape)
    if len(vshape) != 3 or min(vshape) < 1:
        raise ValueError(f"{who} needs a non-empty volume [z, y, x], got shape {vshape}")
    th, tw = _clahe_tile(tile)
    r = _shift_radius(radius)
    L = _index(levels, "levels")
    # a decided offset is at most r - 1 and is doubled on the way down: the centres of level l are at most
    # (r - 1) (2^(L - l + 1) - 2), so the largest, at level 0, is (r - 1) (2^(L + 1) - 2) <= 7 x 126 = 882 < SHIFT_MAX_CENTER
    if not 1 <= L <= SHIFT_MAX_LEVELS:
        raise ValueError(f"levels must lie in 1...{SHIFT_MAX_LEVELS}, got {L}")
    assert (SHIFT_MAX_RADIUS - 1) * (2 ** (SHIFT_MAX_LEVELS + 1) - 2) <= SHIFT_MAX_CENTER
    if min(vshape[1:]) >> L < 4 * r:
        raise ValueError(f"levels={L} leaves sections of {vshape[1] >> L} x {vshape[2] >> L} pixels at the coarsest level: "
                         f"the shorter side must be at least 4 radius = {4 * r}")
    min_corr = _unit(min_corr, "min_corr", False)
    try:
        if isinstance(min_decided, (bool, np.bool_, str, bytes)):
            raise TypeError
        min_decided = float(min_decided)
        if not 0 <= min_decided <= 1:
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"min_decided must be a number in [0, 1], got {min_decided!r}")
    if chunk_bytes is not None and int(chunk_bytes) < 1:
        raise ValueError(f"chunk_bytes must be positive, got {chunk_bytes}")
    shapes = [vshape]
    for _ in range(L):
        shapes.append(rescale_shape(shapes[-1], (2, 2, 1)))
    if coarse is None:
        coarse = [None] * L
    elif len(coarse) != L or any(tuple(c.shape) != s or getattr(c, "dtype", None) != np.uint8
                                 for c, s in zip(coarse, shapes[1:])):
        raise ValueError(f"coarse must be {L} uint8 array-likes of shapes {shapes[1:]}")
    P = vshape[0] - 1 if pairs is None else pairs.shape[0]
    runs = [(0, vshape[0])] if pairs is None else _pair_runs(pairs)  # the sections the searches read, as z runs
    total = {"read_s": 0.0, "chunks": 0}

    def counted(st):
        total["read_s"] += st.get("read_s", 0.0)
        total["chunks"] += st.get("chunks", 0)
    V = [volume]
    for l in range(L):
        if runs == [(0, vshape[0])]:
            st = {}
            V.append(volume_rescale(V[l], (2, 2, 1), out=coarse[l], chunk_bytes=chunk_bytes, device=device, stats=st))
            counted(st)
            continue
        V.append(np.zeros(shapes[l + 1], np.uint8) if coarse[l] is None else coarse[l])
        for z0, z1 in runs:                                      # z is kept: output section z is source section z
            st = {}
            V[l + 1][z0:z1] = volume_rescale(V[l], (2, 2, 1), start=(0, 0, z0), size=shapes[l + 1][:0:-1] + (z1 - z0,),
                                             chunk_bytes=chunk_bytes, device=device, stats=st)
            counted(st)
    s = None
    for l in range(L, -1, -1):
        gy, gx = clahe_grid(shapes[l], (th, tw))
        C = np.zeros((P, gy, gx, 2), np.int64)
        if s is not None:                                        # ceil(ceil(Y / 2) / th) = ceil(gy / 2): i // 2 exists
            i, j = np.arange(gy)[:, None] // 2, np.arange(gx)[None, :] // 2
            C[...] = 2 * np.where(s.decided[:, i, j, None], s.tiles[:, i, j], s.pairs[:, None, None, :])
        st = {}
        q = measure(V[l], C, (th, tw), r, st)
        counted(st)
        n = _shift_counts(shapes[l], (th, tw), r, C)
        s = _section_shifts(_pair_scores(q[:P], n), C, min_corr)[0]
    few = s.decided.sum(axis=(1, 2)) < min_decided * s.decided.shape[1] * s.decided.shape[2]
    unresolved = sorted(set(s.unresolved) | set(int(z) for z in np.nonzero(few)[0]))
    found = s.pairs.copy()
    found[np.array(unresolved, np.int64)] = 0
    if stats is not None:
        stats.update(total)
    return Shifts(found, s.tiles, s.peak, s.decided, unresolved), q, n, C


SHIFT_MAX_LAG = 8                # b - a of a pair of section_shift_sums_pairs, at most: bounds a chunk's dense read slab


class SectionPairs(NamedTuple):
    """section_pairs' plan: `pairs` int64[P, 2] the pairs (a, b) of good sections to measure, ascending, `broken` the list
    of the gaps (a, b) between consecutive good sections that are longer than max_lag and stay unmeasured."""
    pairs: np.ndarray
    broken: list


def section_pairs(Z, skip=(), max_lag=4):
    """Which sections of a stack of `Z` to measure against each other when the sections `skip` are bad (black, charged,
    folded, foreign: suspect_sections, find_defects or the user's own list): consecutive GOOD sections (g_k, g_(k+1)),
    so a bad section is bridged by its neighbours, lag 2 and more, instead of breaking the chain twice.  Gaps longer
    than `max_lag` (1...SHIFT_MAX_LAG) are listed in `broken` and not measured: sections too far apart in z share too
    little.  No `skip` gives (z, z + 1) for every z.  Host only; ValueError for a Z or an entry of skip that is no
    integer, an entry outside [0, Z), max_lag outside 1...8."""
    Z = _index(Z, "Z")
    if Z < 0:
        raise ValueError(f"Z must not be negative, got {Z}")
    lag = _index(max_lag, "max_lag")
    if not 1 <= lag <= SHIFT_MAX_LAG:
        raise ValueError(f"max_lag must lie in 1...{SHIFT_MAX_LAG}, got {lag}")
    try:
        bad = {_index(z, "a skipped section") for z in skip}
    except TypeError:
        raise ValueError(f"skip must be a list of sections, got {skip!r}")
    if any(not 0 <= z < Z for z in bad):
        raise ValueError(f"skip names sections outside [0, {Z}): {sorted(z for z in bad if not 0 <= z < Z)}")
    good = [z for z in range(Z) if z not in bad]
    steps = list(zip(good[:-1], good[1:]))
    pairs = np.array([p for p in steps if p[1] - p[0] <= lag], np.int64).reshape(-1, 2)
    return SectionPairs(pairs, [p for p in steps if p[1] - p[0] > lag])


def _check_pairs(pairs, Z):
    """int64[P, 2] of `pairs`: integers (a, b) with 0 <= a < b < Z and b - a <= SHIFT_MAX_LAG, sorted lexicographically,
    none twice.  ValueError otherwise."""
    p = np.asarray(pairs)
    if p.ndim != 2 or p.shape[1] != 2 or p.dtype.kind not in "iu":
        raise ValueError(f"pairs must be integers of shape [P, 2], got {p.dtype} {p.shape}")
    p = p.astype(np.int64)
    bad = np.nonzero((p[:, 0] < 0) | (p[:, 0] >= p[:, 1]) | (p[:, 1] >= Z) | (p[:, 1] - p[:, 0] > SHIFT_MAX_LAG))[0]
    if bad.size:
        k = int(bad[0])
        raise ValueError(f"pairs[{k}] = {tuple(int(v) for v in p[k])} is not 0 <= a < b < {Z} with b - a <= {SHIFT_MAX_LAG}")
    d = np.diff(p, axis=0)
    bad = np.nonzero((d[:, 0] < 0) | ((d[:, 0] == 0) & (d[:, 1] <= 0)))[0]
    if bad.size:
        k = int(bad[0]) + 1
        raise ValueError(f"pairs must be sorted by (a, b) without duplicates: pairs[{k}] = {tuple(int(v) for v in p[k])} "
                         f"follows {tuple(int(v) for v in p[k - 1])}")
    return p


def _pair_runs(pairs):
    """The sections that the sorted `pairs` span, as the list of maximal z runs (z0, z1) of the union of [a, b]."""
    runs = []
    for a, b in pairs.tolist():
        if runs and a <= runs[-1][1] - 1:
            runs[-1][1] = max(runs[-1][1], b + 1)
        else:
            runs.append([a, b + 1])
    return [tuple(r) for r in runs]


def zshift_chunks_pairs(vol_shape, pairs, radius, reach=(0, 0), chunk_bytes=None, rank=0, world_size=1):
    """Cut the list `pairs` (_check_pairs' rules: section_pairs' list, or any part of it) over a volume of shape
    `vol_shape` [z, y, x] into chunks for section_shift_sums_pairs.  Returns this rank's list of
    ((k0, k1), (y0, y1), read slab): the list entries [k0, k1), their core rows, and the (z, y, x) (lo, hi) box to read.
    A chunk is a run of consecutive entries, each of which starts inside the sections the run already spans (a <= the
    largest b so far: a chain; a gap in z ends the run, so nothing between two distant bridges is read); its read slab
    is the DENSE box of the sections [a_k0, largest b], all rows -- skipped sections inside it are read and ignored,
    which SHIFT_MAX_LAG bounds -- and holds at most `chunk_bytes` bytes (HIST_CHUNK_BYTES when None): as many entries
    as fit.  Where even one pair's b - a + 1 sections exceed the budget, the pair alone is cut into runs of core rows:
    its b - a + 1 sections of as many rows as fit next to their halo, radius - lo rows below and radius + hi above for
    `reach` = (lo, hi) (zshift_chunks_at's), one core row at the least.  Chunks are in list order and go round-robin to
    the ranks.  With section_pairs(Z).pairs the read slabs are zshift_chunks_at's, less its last one where that holds
    the last section alone.  Pure host function; ValueError as zshift_chunks_at, and _check_pairs'."""
    r = _shift_radius(radius)
    lo, hi = _shift_reach(reach)
    budget = _budget(chunk_bytes, rank, world_size)
    (_, Z), (_, ny), (_, nx) = hist_box(vol_shape)
    p = _check_pairs(pairs, Z).tolist()
    chunks, k = [], 0
    while k < len(p):
        a, top = p[k]
        if (top - a + 1) * ny * nx > budget:                     # one pair in runs of rows
            ky = max(1, budget // ((top - a + 1) * nx) - (2 * r + hi - lo))
            chunks += [((k, k + 1), (y, min(y + ky, ny)), ((a, top + 1), (max(y - r + lo, 0), min(y + ky + r + hi, ny)),
                                                           (0, nx))) for y in range(0, ny, ky)]
            k += 1
            continue
        k1 = k + 1
        while k1 < len(p) and p[k1][0] <= top and (max(top, p[k1][1]) - a + 1) * ny * nx <= budget:
            top = max(top, p[k1][1])
            k1 += 1
        chunks.append(((k, k1), (0, ny), ((a, top + 1), (0, ny), (0, nx))))
        k = k1
    return chunks[rank::world_size]


def shift_counts_pairs(vol_shape, tile, radius, centers):
    """np.int64 n[P, gy, gx, R, R]: shift_counts_at for a list of P pairs: the number of terms of
    section_shift_sums_pairs' q[k, i, j, dy + radius, dx + radius] with `centers` integers [P, 2] or [P, gy, gx, 2]
    within SHIFT_MAX_CENTER -- geometry only, so which sections a pair names does not enter.  Pure host function."""
    r = _shift_radius(radius)
    th, tw = _clahe_tile(tile)
    C = np.asarray(centers)
    return _shift_counts(vol_shape, (th, tw), r, _centers_table(C, C.shape[0] if C.ndim else 0,
                                                                *clahe_grid(vol_shape, (th, tw))))


def section_shift_sums_pairs(volume, pairs, centers=None, tile=128, radius=4, chunk_bytes=None, rank=0, world_size=1,
                             device=None, stats=None):
    """section_shift_sums_at over an explicit list of section pairs: np.int64 q[P, gy, gx, R, R, 5] -- a row per PAIR,
    none for "the last section" -- of the uint8 `volume` [z, y, x], where for pair k = (a, b) of `pairs`, the centre
    (cy, cx) = C[k, i, j] and the local offset (dy, dx) in [-radius, radius]^2 the sums run over the voxels (y, x) of
    tile (i, j) whose partner (y + cy + dy, x + cx + dx) lies inside the section, v = volume[a, y, x],
    w = volume[b, y + cy + dy, x + cx + dx]:
      q[k, i, j, dy + radius, dx + radius] = (sum v, sum v v, sum w, sum w w, sum v w)
    `pairs` is integers [P, 2], sorted by (a, b), none twice, 0 <= a < b < Z and b - a <= SHIFT_MAX_LAG = 8:
    section_pairs' bridges over bad sections, or a few pairs to measure again; only the sections they span are read.
    `centers` is None (zero) or integers [P, 2] or [P, gy, gx, 2] within SHIFT_MAX_CENTER.  The number of terms is
    shift_counts_pairs'.  Exact integers that numpy reproduces bit for bit; the pairs (z, z + 1) give
    section_shift_sums_at's rows.

    The pass is section_shift_sums_at's, over zshift_chunks_pairs with reach = the least and the largest cy (and 0):
    both tables go to the device once, as int32; one tem_u8_zshift_tiles_pairs launch per chunk, given the tables'
    rows of the chunk's first pair; the accumulator holds all P rows and is read back once where P*gy*gx*R*R*40 bytes
    are at most CLAHE_ACC_BYTES, else one chunk's rows, read back and added on the host per chunk; ranks' results add.
    `stats` receives `read_s` and `chunks`.  ValueError, before any GPU work: as section_shift_sums, a volume that is
    not [z, y, x], _check_pairs' and shift_centers' rules."""
    _check_u8(volume)
    th, tw = _clahe_tile(tile)
    r = _shift_radius(radius)
    if len(volume.shape) != 3:
        raise ValueError(f"section_shift_sums_pairs needs a volume [z, y, x], got shape {tuple(volume.shape)}")
    gy, gx = clahe_grid(volume.shape, (th, tw))
    (_, Z), (_, Y), _ = hist_box(volume.shape)
    pr = _check_pairs(pairs, Z)
    P = pr.shape[0]
    C = _centers_table(np.zeros((P, 2), np.int64) if centers is None else centers, P, gy, gx)
    lo = hi = cx_max = 0
    if C.size:
        lo, hi = min(int(C[..., 0].min()), 0), max(int(C[..., 0].max()), 0)
        cx_max = int(np.abs(C[..., 1]).max())
    chunks = zshift_chunks_pairs(volume.shape, pr, r, (lo, hi), chunk_bytes, rank, world_size)
    p = _SlabPass([volume], [hist_box(volume.shape)], chunk_bytes, rank, world_size, device, slabs=[s for _, _, s in chunks])
    R = 2 * r + 1
    shape = (gy, gx, R, R, 5)
    if not chunks:                                               # nothing to read: no GPU is needed
        if stats is not None:
            stats.update(p.st)
        return np.zeros((P,) + shape, np.int64)
    lib = H.require_gpu()
    with p.streaming(stats):
        acc = _RowAccumulator(p.dev, P, shape, _most_rows(c[0] for c in chunks))
        table = torch.from_numpy(pr.astype(np.int32)).to(p.dev)                  # both uploaded once
        ctable = torch.from_numpy(C.astype(np.int32).reshape(P, -1)).to(p.dev)
        for k, ((s0, _), (y0, _), _), d, (src,) in p:
            (k0, k1), (c0, c1), _ = chunks[k]
            _lib.check(lib.tem_u8_zshift_tiles_pairs(src.data_ptr(), *d, s0, k1 - k0, table.data_ptr() + 8 * k0, c0 - y0,
                                                     c1 - y0, y0, Y, th, tw, gy, gx, r,
                                                     ctable.data_ptr() + 8 * gy * gx * k0, lo, hi, cx_max,
                                                     acc.ptr(k0, k1), p.compute.cuda_stream), "tem_u8_zshift_tiles_pairs")
            acc.add(k0, k1)
        return acc.result()


def shift_scores_pairs(q, n):
    """shift_scores for section_shift_sums_pairs' `q` and shift_counts_pairs' `n`, both with a row per pair:
    float64 c[P, gy, gx, R, R] indexed by the LOCAL offset.  Host only."""
    return _pair_scores(*_check_shift_sums(q, n, "shift_scores_pairs"))


def section_shifts_pairs(q, n, centers, min_corr=0.1):
    """section_shifts_at for a list of P pairs, from section_shift_sums_pairs' `q`, shift_counts_pairs' `n` and the
    `centers` ([P, 2] or [P, gy, gx, 2] integers) of that search.  Host only, and the same rules: row k of the Shifts
    speaks of pair k -- `pairs[k]` is the (dy, dx) by which section b shows what section a shows at (y, x) --, and
    `unresolved` lists indices k into the pair list."""
    q, n = _check_shift_sums(q, n, "section_shifts_pairs")
    C = _check_centers_for(q, centers, "section_shifts_pairs")
    min_corr = _unit(min_corr, "min_corr", False)
    return _section_shifts(_pair_scores(q, n), C, min_corr)[0]


def shift_subpixel_pairs(q, n, centers, min_corr=0.1):
    """shift_subpixel_at for a list of P pairs: SubShifts with a row per pair.  fit_section_maps takes it unchanged,
    chain_pairs puts the fitted maps back onto the stack."""
    q, n = _check_shift_sums(q, n, "section_shifts_pairs")
    C = _check_centers_for(q, centers, "section_shifts_pairs")
    min_corr = _unit(min_corr, "min_corr", False)
    return _shift_subpixel(_pair_scores(q, n), C, min_corr)


class BridgedShifts(NamedTuple):
    """section_shifts_bridged's verdict, all of the finest level and with a row per pair of `pairs` int64[P, 2]:
    `shifts` the Shifts in total offsets (`unresolved` holds indices into `pairs`), `q` and `n` the sums and counts of
    the last search and `centers` int64[P, gy, gx, 2] where it was centred -- what shift_subpixel_pairs takes."""
    pairs: np.ndarray
    shifts: Shifts
    q: np.ndarray
    n: np.ndarray
    centers: np.ndarray


def section_shifts_bridged(volume, pairs, tile=128, radius=4, levels=3, min_corr=0.1, min_decided=0.5, coarse=None,
                           chunk_bytes=None, device=None, stats=None):
    """section_shifts_coarse_to_fine over a list of section pairs (section_pairs: the good sections on either side of a
    bad one are measured against each other): the same pyramid and rescales, the same centre rule per pair and tile --
    2 tiles_(l+1)[k, i // 2, j // 2] where that coarse tile is decided, else 2 pairs_(l+1)[k] --, the same
    `min_decided` verdict, with section_shift_sums_pairs as the device pass.  `pairs` follows its rules.  Returns
    BridgedShifts(pairs, shifts, q, n, centers); for section_pairs(Z).pairs these are section_shifts_coarse_to_fine's
    shifts, q[:-1], n and centers exactly.  chain_pairs spreads `shifts.pairs` (or maps or fields fitted per pair) back
    onto the Z - 1 consecutive pairs for shift_positions and its siblings.

    The list may hold only the bridges, to mend an alignment that exists: then only the sections that these pairs span
    are read, rescaled and searched, run by run; every other section of the pyramid, and of `coarse`, is left as it
    is.  `coarse`, `chunk_bytes`, `device`, `stats` and every ValueError are section_shifts_coarse_to_fine's, plus
    section_shift_sums_pairs' rules for the pairs, before any GPU work."""
    _check_u8(volume)
    vshape = tuple(int(v) for v in volume.shape)
    if len(vshape) != 3 or min(vshape) < 1:
        raise ValueError(f"section_shifts_bridged needs a non-empty volume [z, y, x], got shape {vshape}")
    pr = _check_pairs(pairs, vshape[0])

    def measure(v, C, tile, r, st):                              # looked up at the call, as its sibling
        return section_shift_sums_pairs(v, pr, C, tile, r, chunk_bytes=chunk_bytes, device=device, stats=st)
    s, q, n, C = _shifts_pyramid(volume, pr, measure, tile, radius, levels, min_corr, min_decided, coarse, chunk_bytes,
                                 device, stats, "section_shifts_bridged")
    return BridgedShifts(pr, s, q, n, C)


def suspect_sections(unresolved, Z):
    """The sections of a stack of `Z` that no neighbour resembles, from the `unresolved` pairs z (section z against
    z + 1) of section_shifts_coarse_to_fine or section_shifts: those both of whose adjoining pairs, z - 1 and z, are
    unresolved; for sections 0 and Z - 1 their one pair decides.  A sorted list: the `skip` of section_pairs where
    nobody supplies one.  Host only; ValueError for entries that are no integers in [0, Z - 1)."""
    Z = _index(Z, "Z")
    u = {_index(z, "an unresolved pair") for z in unresolved}
    if any(not 0 <= z < Z - 1 for z in u):
        raise ValueError(f"unresolved names pairs outside [0, {max(Z - 1, 0)}): {sorted(z for z in u if not 0 <= z < Z - 1)}")
    return [z for z in range(Z) if Z > 1 and (z == 0 or z - 1 in u) and (z == Z - 1 or z in u)]


def chain_pairs(pairs, values, Z, base=None):
    """Per-pair values of a pair list spread back onto the Z - 1 consecutive pairs (z, z + 1) of the stack, for
    shift_positions, section_maps, section_fields and what follows them, which are used unchanged.  `values` has a row
    per pair of `pairs` ([P, 2], _check_pairs' rules): integer shifts [P, 2], maps [P, 2, 3] or fields [P, ny, nx, 2].
    One rule for all three: start from `base` ([Z - 1, ...]; None: the identity -- zero shifts and fields, the map
    [[1, 0, 0], [0, 1, 0]]); pair (a, b) writes its value at index a and the identity at a + 1 ... b - 1.  So a skipped
    section takes the position of the good section above it, and the sections above a bridge sit where the bridge
    says.  What no pair covers -- section_pairs' `broken` gaps -- keeps the base; to leave an unresolved pair at the
    identity, drop its row or give the identity for it.  Returns a new array of the values' dtype.  Host only;
    ValueError for values of another shape, a base of another shape or dtype."""
    Z = _index(Z, "Z")
    pr = _check_pairs(pairs, Z)
    v = np.asarray(values)
    is_map = v.ndim == 3 and v.shape[1:] == (2, 3)
    if v.shape[:1] != (pr.shape[0],) or v.dtype.kind not in "iuf" or \
            not (is_map or (v.ndim == 2 and v.shape[1] == 2) or (v.ndim == 4 and v.shape[3] == 2)):
        raise ValueError(f"values must be numbers of shape [{pr.shape[0]}, 2], [{pr.shape[0]}, 2, 3] or "
                         f"[{pr.shape[0]}, ny, nx, 2], got {v.dtype} {v.shape}")
    ident = np.zeros(v.shape[1:], v.dtype)
    if is_map:
        ident[0, 0] = ident[1, 1] = 1
    shape = (max(Z - 1, 0),) + v.shape[1:]
    if base is None:
        out = np.broadcast_to(ident, shape).copy()
    else:
        out = np.array(base)
        if out.shape != shape or out.dtype != v.dtype:
            raise ValueError(f"base must be {v.dtype} of shape {shape}, got {out.dtype} {out.shape}")
    for (a, b), val in zip(pr.tolist(), v):
        out[a], out[a + 1:b] = val, ident
    return out


class SectionFits(NamedTuple):
    """fit_section_maps' verdict: `maps` float64[Z - 1, 2, 3] the map T_z of every pair (rows (y, x); columns: from y,
    from x, constant), `kept` bool[Z - 1, gy, gx] the tiles the final fit rests on, `residual` float64[Z - 1] the
    largest max-norm residual among them in pixels, `unresolved` the sorted list of the pairs without a decided tile."""
    maps: np.ndarray
    kept: np.ndarray
    residual: np.ndarray
    unresolved: list


def _fit_map(pts, target, affine):
    """The least-squares map of `pts` [k, 2] onto `target` [k, 2] as [2, 3], and whether it is affine: L = I where
    `affine` is False or the points do not span the plane."""
    mean = pts.mean(axis=0)
    A = np.concatenate([pts - mean, np.ones((pts.shape[0], 1))], axis=1)
    if affine and np.linalg.matrix_rank(A) == 3:
        coef = np.linalg.lstsq(A, target, rcond=None)[0]                 # [3, 2]: target = (p - mean) L^T + c
        L = coef[:2].T
        return np.concatenate([L, (coef[2] - L @ mean)[:, None]], axis=1)
    return np.concatenate([np.eye(2), (target - pts).mean(axis=0)[:, None]], axis=1)


def fit_section_maps(sub, tile, vol_shape, model="affine", max_residual=1.0):
    """One map per pair of sections from the tile offsets of shift_subpixel (or any (offsets, decided, ...) tuple) on
    clahe_grid's tiles of `tile` pixels over a volume of shape `vol_shape`.  Host only.  The pair map is
    T_z(p) = L p + b with p = (y, x) in voxel indices: section z + 1 shows at T_z(p) what section z shows at p.  A
    tile's point is the mean index of its existing voxels, (lo + hi - 1) / 2 per axis; the fit is ordinary least squares
    of point + offset on (point, 1) over the kept tiles, which start as the decided ones.  Robust and deterministic:
    fit; if the worst max-norm residual exceeds `max_residual` pixels, drop that one tile (ties: the lowest index) and
    refit; stop when none exceeds it or half of the decided tiles are gone.  model="translation" fixes L = I;
    "affine" falls back to it for a pair whose kept points do not span the plane.  A pair without a decided tile gets
    the identity and a place in `unresolved`.  section_maps composes the pair maps into one map per section.
    What the maps leave over tile by tile (`residual`) is what fit_section_fields turns into a smooth displacement
    field per pair.  ValueError for offsets or decided of another shape, an unknown model, a
    max_residual that is not a positive number."""
    th, tw = _clahe_tile(tile)
    gy, gx = clahe_grid(vol_shape, (th, tw))
    _, (_, Y), (_, X) = hist_box(vol_shape)
    offsets, decided = np.asarray(sub[0]), np.asarray(sub[1])
    if offsets.ndim != 4 or offsets.shape[1:] != (gy, gx, 2) or offsets.dtype.kind not in "fiu":
        raise ValueError(f"offsets must be numbers of shape [Z - 1, {gy}, {gx}, 2], got {offsets.dtype} {offsets.shape}")
    if decided.shape != offsets.shape[:3] or decided.dtype != np.bool_:
        raise ValueError(f"decided must be bool of shape {offsets.shape[:3]}, got {decided.dtype} {decided.shape}")
    if model not in ("affine", "translation"):
        raise ValueError(f"model must be 'affine' or 'translation', got {model!r}")
    if isinstance(max_residual, (bool, np.bool_)) or not isinstance(max_residual, (int, float, np.integer, np.floating)) \
            or not (max_residual > 0 and np.isfinite(max_residual)):
        raise ValueError(f"max_residual must be a positive number, got {max_residual!r}")
    offsets = offsets.astype(np.float64)
    centre = lambda t, g, n: np.array([(k * t + min((k + 1) * t, n) - 1) / 2 for k in range(g)])
    points = np.stack(np.meshgrid(centre(th, gy, Y), centre(tw, gx, X), indexing="ij"), axis=-1)     # [gy, gx, 2]
    P = offsets.shape[0]
    maps = np.tile(np.concatenate([np.eye(2), np.zeros((2, 1))], axis=1), (P, 1, 1))
    kept, residual, unresolved = decided.copy(), np.zeros(P, np.float64), []
    for z in range(P):
        nd, gone = int(decided[z].sum()), 0
        if nd == 0:
            unresolved.append(z)
            continue
        while True:
            idx = np.flatnonzero(kept[z])
            pts = points.reshape(-1, 2)[idx]
            target = pts + offsets[z].reshape(-1, 2)[idx]
            m = _fit_map(pts, target, model == "affine")
            res = np.abs(pts @ m[:, :2].T + m[:, 2] - target).max(axis=1)
            worst = int(res.argmax())                                    # the first of equal maxima: the lowest index
            if res[worst] <= max_residual or 2 * gone >= nd or idx.size == 1:
                break
            kept[z].reshape(-1)[idx[worst]] = False
            gone += 1
        maps[z], residual[z] = m, res.max()
    return SectionFits(maps, kept, residual, unresolved)


def _map_compose(a, b):
    """a o b of two [2, 3] maps."""
    return np.concatenate([a[:, :2] @ b[:, :2], (a[:, :2] @ b[:, 2] + a[:, 2])[:, None]], axis=1)


def section_maps(pair_maps, window=None):
    """float64 B[Z, 2, 3]: one map per section from fit_section_maps' pair maps [Z - 1, 2, 3]: B_0 = I and
    B_{z + 1} = T_z o B_z, so that out[z](p) = volume[z](B_z p) shows what section 0 shows at p -- what volume_warp
    computes.  With `window` (an odd int >= 3) the trend, the element-wise running lower median of the six coefficients
    over the sections [z - window // 2, z + window // 2], clipped to the stack, is taken out: the result is
    B_z o trend_z^-1, which removes the jitter and keeps a real drift.  For integer translations this equals
    shift_positions(pairs, window) exactly.  Host only; ValueError for maps of another shape or dtype, values that are
    not finite, a bad window."""
    T = np.asarray(pair_maps)
    if T.ndim != 3 or T.shape[1:] != (2, 3) or T.dtype.kind != "f" or not np.isfinite(T).all():
        raise ValueError(f"pair_maps must be finite floats of shape [Z - 1, 2, 3], got {T.dtype} {T.shape}")
    T = T.astype(np.float64)
    B = np.empty((T.shape[0] + 1, 2, 3), np.float64)
    B[0] = [[1, 0, 0], [0, 1, 0]]
    for z in range(T.shape[0]):
        B[z + 1] = _map_compose(T[z], B[z])
    if window is None:
        return B
    w = _index(window, "window")
    if w < 3 or w % 2 != 1:
        raise ValueError(f"window must be an odd integer >= 3, got {w}")
    h, Z = w // 2, B.shape[0]
    out = np.empty_like(B)
    for z in range(Z):
        run = np.sort(B[max(z - h, 0):min(z + h + 1, Z)].reshape(-1, 6), axis=0)
        (a, b, ty), (c, d, tx) = run[(run.shape[0] - 1) // 2].reshape(2, 3)
        det = a * d - b * c
        if det == 0:
            raise ValueError(f"the trend of section {z} cannot be inverted")
        Li = np.array([[d, -b], [-c, a]]) / det
        inv = np.concatenate([Li, (-Li @ np.array([ty, tx]))[:, None]], axis=1)
        out[z] = _map_compose(B[z], inv)
    return out


WARP_UNIT = 1 << 16              # tem_u8_warp_affine: coefficients in 2^-16, a matrix coefficient within 2^13 of I,
WARP_MAX_DEV = 1 << 13           # |b| below 2^47
WARP_MAX_B = 1 << 47


def _check_qmaps(M, what):
    """int64 [Z, 6] `M` inside tem_u8_warp_affine's limits, or ValueError."""
    dev = np.abs(M - np.array([WARP_UNIT, 0, 0, 0, WARP_UNIT, 0], np.int64))
    if (dev[:, [0, 1, 3, 4]] > WARP_MAX_DEV).any() or (dev[:, [2, 5]] >= WARP_MAX_B).any():
        z = int(np.flatnonzero((dev[:, [0, 1, 3, 4]] > WARP_MAX_DEV).any(axis=1) | (dev[:, [2, 5]] >= WARP_MAX_B).any(axis=1))[0])
        raise ValueError(f"{what}: the map of section {z}, {M[z].tolist()} in 2^-16, is outside the limits: a matrix "
                         f"coefficient within 1/8 of the identity's, |b| below 2^31 pixels")
    return M


def quantize_maps(maps):
    """np.int64[Z, 6] = (a_yy, a_yx, b_y, a_xy, a_xx, b_x) in units of 2^-16, rounded with rint, of float maps [Z, 2, 3]
    (section_maps'): what tem_u8_warp_affine and volume_warp compute with.  ValueError for another shape or dtype,
    values that are not finite, and outside the limits |a_yy - 2^16|, |a_yx|, |a_xy|, |a_xx - 2^16| <= 2^13 and
    |b| < 2^47: one eighth -- seven degrees, or 12 % of scale -- which is what bounds the kernel's staging hull."""
    m = np.asarray(maps)
    if m.ndim != 3 or m.shape[1:] != (2, 3) or m.dtype.kind != "f":
        raise ValueError(f"maps must be floats of shape [Z, 2, 3], got {m.dtype} {m.shape}")
    if not np.isfinite(m).all():
        raise ValueError("maps must be finite")
    m = m.astype(np.float64) * WARP_UNIT
    if (np.abs(m) >= 2.0 ** 62).any():
        raise ValueError("maps: a coefficient is outside the limits")
    return _check_qmaps(np.rint(m).astype(np.int64).reshape(-1, 6), "maps")


def _warp_table(maps, Z, one):
    """volume_warp's `maps` as the int64[Z, 6] table: float [Z, 2, 3] is quantised, int64 [Z, 6] is checked; one image
    also takes one map [2, 3] or [6]."""
    m = np.asarray(maps)
    if one and m.ndim == (2 if m.dtype.kind == "f" else 1):
        m = m[None]
    if m.dtype.kind == "f" and m.shape == (Z, 2, 3):
        return quantize_maps(m)
    if m.dtype == np.int64 and m.shape == (Z, 6):
        return _check_qmaps(np.array(m), "maps")                          # a writable copy
    raise ValueError(f"maps must be floats of shape {(Z, 2, 3)} or int64 of shape {(Z, 6)}, got {m.dtype} {m.shape}")


def _warp_rows(M, z0, z1, y0, y1, x0, x1, Y):
    """The rows [lo, hi) of the section that the outputs [y0, y1) x [x0, x1) of sections [z0, z1) can read: [min iy,
    max iy + 2) over the box's corners -- where the affine sy takes its extremes --, unioned over the sections and
    clipped to the section; one row at the least."""
    a, b, c = M[z0:z1, 0], M[z0:z1, 1], M[z0:z1, 2]
    s, ey, ex = a * y0 + b * x0 + c, a * (y1 - 1 - y0), b * (x1 - 1 - x0)
    lo = int(((s + np.minimum(ey, 0) + np.minimum(ex, 0) + 128) >> 16).min())
    hi = int(((s + np.maximum(ey, 0) + np.maximum(ex, 0) + 128) >> 16).max()) + 2
    lo = min(max(lo, 0), Y - 1)
    return lo, max(min(hi, Y), lo + 1)


def warp_chunks(out_box, vol_shape, M, chunk_bytes=None, rank=0, world_size=1):
    """Cut the (z, y, x) (lo, hi) box `out_box` of a volume of shape `vol_shape` [z, y, x] into slabs for volume_warp
    under the maps `M`, quantize_maps' int64[Z, 6].  Returns this rank's list of (output slab, read slab), (z, y, x)
    (lo, hi) boxes of the volume: the output slabs are disjoint and their union is the box -- runs of whole sections of
    the box, as many as fit, or, where one section or its hull is larger than the budget, runs of whole rows of that
    section (one row at the least).  A read slab is the same sections with the rows [min iy, max iy + 2) over its
    output slab's corners, unioned over its sections and clipped to the section (one row at the least, when everything
    is outside), over the volume's whole x extent: x is never cut.  Both slabs hold at most `chunk_bytes` bytes
    (HIST_CHUNK_BYTES when None).  Slabs are in (z, y) order and go round-robin to the ranks.  Pure host function;
    ValueError as rescale_chunks, and for maps of another shape or dtype or outside the limits."""
    budget = _budget(chunk_bytes, rank, world_size)
    vol_shape = tuple(int(v) for v in vol_shape)
    if len(vol_shape) != 3 or min(vol_shape) < 1:
        raise ValueError(f"warp_chunks takes a non-empty volume shape [z, y, x], got {vol_shape}")
    Z, Y, X = vol_shape
    M = np.asarray(M)
    if M.dtype != np.int64 or M.shape != (Z, 6):
        raise ValueError(f"M must be int64 of shape {(Z, 6)}, got {M.dtype} {M.shape}")
    _check_qmaps(M, "M")
    (z0, z1), (y0, y1), (x0, x1) = out_box
    if any(lo < 0 or hi > n for (lo, hi), n in zip(out_box, vol_shape)):
        raise ValueError(f"the box {tuple(out_box)} reaches outside the volume of shape {vol_shape}")
    ny, nx = y1 - y0, x1 - x0
    if z1 <= z0 or ny <= 0 or nx <= 0:
        return []

    rows = lambda za, zb, ya, yb: _warp_rows(M, za, zb, ya, yb, x0, x1, Y)
    return _row_cut_slabs(rows, out_box, X, budget)[rank::world_size]


def _row_cut_slabs(rows, out_box, X, budget):
    """warp_chunks' cut of a non-empty `out_box`: (output slab, read slab) in (z, y) order, where rows(z0, z1, y0, y1)
    gives the rows [lo, hi) that the outputs [y0, y1) of the sections [z0, z1) read, over a volume of X columns."""
    (z0, z1), (y0, y1), (x0, x1) = out_box
    ny, nx = y1 - y0, x1 - x0

    def fits(nz, nrows, ry):            # an output slab of nz sections of `nrows` rows and its read slab of ry rows
        return nz * nrows * nx <= budget and nz * ry * X <= budget

    slabs, z = [], z0
    while z < z1:
        lo, hi = rows(z, z + 1, y0, y1)
        if fits(1, ny, hi - lo):
            k = 1
            while z + k < z1:
                more = rows(z, z + k + 1, y0, y1)
                if not fits(k + 1, ny, more[1] - more[0]):
                    break
                k, (lo, hi) = k + 1, more
            slabs.append((((z, z + k), (y0, y1), (x0, x1)), ((z, z + k), (lo, hi), (0, X))))
            z += k
            continue
        y = y0
        while y < y1:
            rd = rows(z, z + 1, y, y + 1)
            k = 1
            while y + k < y1:
                more = rows(z, z + 1, y, y + k + 1)
                if not fits(1, k + 1, more[1] - more[0]):
                    break
                k, rd = k + 1, more
            slabs.append((((z, z + 1), (y, y + k), (x0, x1)), ((z, z + 1), rd, (0, X))))
            y += k
        z += 1
    return slabs


def volume_warp(volume, maps, out=None, start=None, size=None, fill=0, nearest=False, chunk_bytes=None, rank=0,
                world_size=1, device=None, stats=None):
    """A uint8 array-like `volume` indexed [z, y, x] (ndarray, np.memmap, h5py / zarr dataset), or one image [y, x], with
    every section resampled through its own affine map, on the device: out[z](p) = volume[z](B_z p) with B = `maps`,
    float [Z, 2, 3] (section_maps': rows (y, x); columns from y, from x, constant; quantised inside with
    quantize_maps) or quantize_maps' int64 [Z, 6]; one image takes one map.  This is the sub-pixel, rotating, scaling
    and shearing form of volume_shift -- section_shift_sums -> shift_subpixel -> fit_section_maps -> section_maps ->
    volume_warp aligns a stack -- and with the identity matrix and integer translations it reproduces volume_shift byte
    for byte.

    The position is computed in 64-bit integers in units of 2^-16, rounded half up to 1/256 px; a voxel whose position
    lies outside [0, Y - 1] x [0, X - 1] is `fill` (0...255) -- no tap is ever blended with fill; otherwise it is the
    bilinear blend of the 2 x 2 voxels around it in integers, rounded once, half up (tem_u8_warp_affine; include/
    tem_hip.h has the definition, numpy reproduces it bit for bit), or with `nearest`, for masks, the voxel nearest to
    it.  A voxel depends on its section and its map alone, not on the slab, ROI or rank it was computed in.  A matrix
    coefficient must lie within 1/8 of the identity's (seven degrees, or 12 % of scale).

    The output grid is the volume's own; `start` / `size` are an ROI of it in (x, y, z) order (default: all of it),
    `out` a writable uint8 array-like of the ROI's shape (allocated when None), which is returned.  Out of core as
    volume_rescale: the ROI is cut into output slabs and the read slabs that hold their taps (warp_chunks), both at most
    `chunk_bytes`; host thread -> pinned -> H2D -> one tem_u8_warp_affine launch per slab -> D2H -> host write, on
    double buffers, in the order write(k), read(k + 2) on the one host thread; the table of maps is uploaded once.
    Ranks (rank / world_size) take slabs round-robin and write disjoint boxes of a shared `out`.  `stats` receives
    `read_s`, `write_s` and `chunks`.

    Elastic warps -- the map plus a smooth displacement field -- are volume_warp_field's.  Out of scope: resampling
    along z, and majority resampling of labels (nearest is what masks get).  predict_cube / predict_volume take the
    same maps as warp=Warp(maps) and align on the way in, without the aligned copy.

    ValueError, before any GPU work: a volume that is not uint8 or not [z, y, x] (or one image), maps of a wrong shape
    or dtype or outside the limits, an ROI outside the volume, an `out` of another shape or dtype, a fill outside
    0...255."""
    _check_u8(volume)
    vshape = tuple(int(v) for v in volume.shape)
    if len(vshape) not in (2, 3) or min(vshape) < 1:
        raise ValueError(f"volume_warp needs a non-empty volume [z, y, x] or one image [y, x], got shape {vshape}")
    one = len(vshape) == 2
    vol3 = (1,) + vshape if one else vshape
    M = _warp_table(maps, vol3[0], one)
    fill = _index(fill, "fill")
    if not 0 <= fill <= 255:
        raise ValueError(f"fill must lie in 0...255, got {fill}")
    box = hist_box(vshape, start, size)
    out = _roi_out(out, box, one)
    chunks = warp_chunks(box, vol3, M, chunk_bytes, rank, world_size)
    p = _SlabPass([volume], [hist_box(vshape)], chunk_bytes, rank, world_size, device, slabs=[r for _, r in chunks])
    lib = H.require_gpu()
    oslabs = [o for o, _ in chunks]
    with p.streaming(stats):
        table = torch.from_numpy(M).to(p.dev)                            # the whole table, once
        with p.writing(out, box, oslabs) as outp:
            for k, ((z0, _), (y0, _), _), d, (src,) in p:
                _lib.check(lib.tem_u8_warp_affine(src.data_ptr(), *d, y0, vol3[1], outp.device(k).data_ptr(),
                                                  *(hi - lo for lo, hi in oslabs[k]), oslabs[k][1][0], oslabs[k][2][0],
                                                  M.ctypes.data + 48 * z0, table.data_ptr() + 48 * z0, fill,
                                                  int(bool(nearest)), p.compute.cuda_stream), "tem_u8_warp_affine")
                p.put(k)
    return out


FIELD_MAX = 1 << 21              # tem_u8_warp_field: |U| <= 2^21 (32 px); adjacent nodes differ by at most S 2^13


def _field_spacing(spacing):
    """(ky, kx) of `spacing`, an int or (Sy, Sx): powers of two in 16...1024."""
    try:
        sy, sx = (spacing, spacing) if not hasattr(spacing, "__len__") else spacing
        sy, sx = _index(sy, "spacing"), _index(sx, "spacing")
    except (TypeError, ValueError):
        raise ValueError(f"spacing must be an int or (Sy, Sx), got {spacing!r}")
    for v in (sy, sx):
        if not 16 <= v <= 1024 or v & (v - 1):
            raise ValueError(f"spacing must be a power of two in 16...1024 per axis, got {(sy, sx)}")
    return sy.bit_length() - 1, sx.bit_length() - 1


def field_grid(vol_shape, spacing):
    """(ny, nx) = (((Y - 1) >> ky) + 2, ((X - 1) >> kx) + 2): the nodes of the displacement lattice with the spacings
    (Sy, Sx) = (2^ky, 2^kx) -- `spacing`, an int or (Sy, Sx), powers of two in 16...1024 -- over a section of a volume of
    shape [Z, Y, X] or an image [Y, X].  Node (i, j) sits at pixel (i Sy, j Sx); every pixel of the section lies in a cell
    with four nodes.  Pure host function."""
    ky, kx = _field_spacing(spacing)
    shape = tuple(int(v) for v in vol_shape)
    if len(shape) not in (2, 3) or min(shape) < 1:
        raise ValueError(f"volume must be a non-empty [z, y, x] or one image [y, x], got shape {shape}")
    return ((shape[-2] - 1) >> ky) + 2, ((shape[-1] - 1) >> kx) + 2


def _field_interp(F, ky, kx, p):
    """The lattice function F [ny, nx, c] interpolated bilinearly at the points p [..., 2] = (y, x) in pixels, clamped to
    the lattice."""
    ny, nx = F.shape[:2]
    gy, gx = np.clip(p[..., 0] / (1 << ky), 0, ny - 1), np.clip(p[..., 1] / (1 << kx), 0, nx - 1)
    i, j = np.minimum(np.floor(gy).astype(np.int64), ny - 2), np.minimum(np.floor(gx).astype(np.int64), nx - 2)
    ty, tx = (gy - i)[..., None], (gx - j)[..., None]
    return (1 - ty) * ((1 - tx) * F[i, j] + tx * F[i, j + 1]) + ty * ((1 - tx) * F[i + 1, j] + tx * F[i + 1, j + 1])


def _field_nodes(ny, nx, ky, kx):
    """float64 [ny, nx, 2]: the nodes' pixels (y, x)."""
    return np.stack(np.meshgrid(np.arange(ny, dtype=np.float64) * (1 << ky), np.arange(nx, dtype=np.float64) * (1 << kx),
                                indexing="ij"), axis=-1)


class FieldFits(NamedTuple):
    """fit_section_fields' verdict: `fields` float64[Z - 1, ny, nx, 2] the displacement (u_y, u_x) in pixels of every
    pair at the lattice's nodes, on top of the pair's map; `used` bool[Z - 1, gy, gx] the tiles it rests on; `residual`
    float64[Z - 1] the largest max-norm misfit of a used tile against the field at its point, in pixels."""
    fields: np.ndarray
    used: np.ndarray
    residual: np.ndarray


_BINOMIAL = np.array([[1.0, 2.0, 1.0], [2.0, 4.0, 2.0], [1.0, 2.0, 1.0]])


def fit_section_fields(sub, fits, tile, vol_shape, spacing, smooth=1, max_residual=1.0):
    """One smooth displacement field per pair of sections from what fit_section_maps' maps leave over: `sub` are
    shift_subpixel's tile offsets (or any (offsets, decided, ...) tuple), `fits` fit_section_maps' verdict on them (or
    any (maps, kept, residual, unresolved) tuple), `tile` and `vol_shape` those of the fit, `spacing` the lattice's
    (field_grid).  Host only.  With T_z = fits.maps[z], the pair function becomes F_z(p) = T_z p + r_z(p), r_z the field
    interpolated bilinearly on the lattice.

    Per pair: the residual of a decided tile is e = point + offset - T_z(point) at fit_section_maps' tile points.  A
    tile is dropped when e lies further, in max norm, than `max_residual` pixels from the per-axis lower median of the
    decided tiles of its 3 x 3 neighbourhood (itself included); the rest are `used`.  `smooth` passes (an int >= 0) of a
    3 x 3 binomial average, normalised over the tiles that have a value, smooth the used tiles and fill tiles without a
    value from neighbours that have one; a tile that still has none gets 0.  The node values are the separable linear
    interpolation of the tile values between the tile points (np.interp along y, then along x); outside the outermost
    points the value is held.  A pair in fits.unresolved, or without a decided tile, gets a zero field.  Deterministic:
    the same input gives the same bytes.  section_fields composes the pairs; finer fields than 16 px are out of scope.
    ValueError for offsets, decided or maps of another shape, a bad spacing, a smooth that is not an integer >= 0, a
    max_residual that is not a positive number."""
    th, tw = _clahe_tile(tile)
    gy, gx = clahe_grid(vol_shape, (th, tw))
    ky, kx = _field_spacing(spacing)
    ny, nx = field_grid(vol_shape, spacing)
    _, (_, Y), (_, X) = hist_box(vol_shape)
    offsets, decided = np.asarray(sub[0]), np.asarray(sub[1])
    if offsets.ndim != 4 or offsets.shape[1:] != (gy, gx, 2) or offsets.dtype.kind not in "fiu":
        raise ValueError(f"offsets must be numbers of shape [Z - 1, {gy}, {gx}, 2], got {offsets.dtype} {offsets.shape}")
    if decided.shape != offsets.shape[:3] or decided.dtype != np.bool_:
        raise ValueError(f"decided must be bool of shape {offsets.shape[:3]}, got {decided.dtype} {decided.shape}")
    P = offsets.shape[0]
    maps = np.asarray(fits[0])
    if maps.shape != (P, 2, 3) or maps.dtype.kind != "f" or not np.isfinite(maps).all():
        raise ValueError(f"fits.maps must be finite floats of shape {(P, 2, 3)}, got {maps.dtype} {maps.shape}")
    unresolved = set(int(z) for z in fits[3])
    smooth = _index(smooth, "smooth")
    if smooth < 0:
        raise ValueError(f"smooth must be an integer >= 0, got {smooth}")
    if isinstance(max_residual, (bool, np.bool_)) or not isinstance(max_residual, (int, float, np.integer, np.floating)) \
            or not (max_residual > 0 and np.isfinite(max_residual)):
        raise ValueError(f"max_residual must be a positive number, got {max_residual!r}")
    offsets, maps = offsets.astype(np.float64), maps.astype(np.float64)
    centre = lambda t, g, n: np.array([(k * t + min((k + 1) * t, n) - 1) / 2 for k in range(g)])
    py, px = centre(th, gy, Y), centre(tw, gx, X)
    points = np.stack(np.meshgrid(py, px, indexing="ij"), axis=-1)                                    # [gy, gx, 2]
    node_y, node_x = np.arange(ny, dtype=np.float64) * (1 << ky), np.arange(nx, dtype=np.float64) * (1 << kx)
    fields, used, residual = np.zeros((P, ny, nx, 2), np.float64), np.zeros((P, gy, gx), bool), np.zeros(P, np.float64)
    for z in range(P):
        if z in unresolved or not decided[z].any():
            continue
        e = points + offsets[z] - (points @ maps[z][:, :2].T + maps[z][:, 2])
        for i, j in zip(*np.nonzero(decided[z])):
            hood = (slice(max(i - 1, 0), i + 2), slice(max(j - 1, 0), j + 2))
            near = np.sort(e[hood][decided[z][hood]], axis=0)
            used[z, i, j] = np.abs(e[i, j] - near[(near.shape[0] - 1) // 2]).max() <= max_residual
        val, have = np.where(used[z][..., None], e, 0.0), used[z].copy()
        for _ in range(smooth):
            num, den = np.zeros((gy, gx, 2)), np.zeros((gy, gx))
            v, h = np.pad(val, ((1, 1), (1, 1), (0, 0))), np.pad(have.astype(np.float64), 1)
            for a in range(3):
                for b in range(3):
                    num += _BINOMIAL[a, b] * v[a:a + gy, b:b + gx]
                    den += _BINOMIAL[a, b] * h[a:a + gy, b:b + gx]
            have = den > 0
            val = np.where(have[..., None], num / np.where(have, den, 1.0)[..., None], 0.0)
        along_y = np.stack([[np.interp(node_y, py, val[:, j, c]) for c in range(2)] for j in range(gx)])   # [gx, 2, ny]
        fields[z] = np.stack([[np.interp(node_x, px, along_y[:, c, i]) for c in range(2)] for i in range(ny)]) \
            .transpose(0, 2, 1)                                                                       # [ny, nx, 2]
        if used[z].any():
            residual[z] = np.abs(e - _field_interp(fields[z], ky, kx, points)).max(axis=-1)[used[z]].max()
    return FieldFits(fields, used, residual)


def section_fields(pair_maps, pair_fields, spacing, vol_shape, window=None):
    """(maps float64[Z, 2, 3], fields float64[Z, ny, nx, 2]): one map and one displacement field per section from
    fit_section_maps' pair maps [Z - 1, 2, 3] and fit_section_fields' pair fields [Z - 1, ny, nx, 2] on the lattice of
    `spacing` over `vol_shape` -- what volume_warp_field takes: out[z](p) = volume[z](maps[z] p + fields[z](p)) shows
    what section 0 shows at p.  Host only.

    With the pair function F_z(q) = T_z q + r_z(q), r_z the pair field interpolated bilinearly at q and clamped to the
    lattice, the composition G_0 = id, G_{z + 1}(p) = F_z(G_z(p)) is followed at every node p.  `maps` is
    section_maps(pair_maps, window), unchanged, and with B the composition of the maps without a window the field is
    what the maps do not explain, D_z = G_z - B_z, computed as D_{z + 1}(p) = L_z D_z(p) + r_z(B_z p + D_z(p)) (L_z the
    matrix of T_z), so that zero pair fields give zero fields exactly.  For window=None fields[z] = D_z.  With a window,
    maps[z] = B_z o trend_z^-1, and the field is D_z interpolated at the node carried through the inverse trend,
    p' = (B_z^-1 o maps[z])(p); then the element-wise running lower median of the field over the same sections is taken
    out.  That treats the field's own trend to first order: the median field is subtracted, not inverted and composed
    as the maps' trend is.  ValueError as section_maps, for fields of another shape or dtype or not finite, a bad
    spacing."""
    maps = section_maps(pair_maps, window)
    ky, kx = _field_spacing(spacing)
    ny, nx = field_grid(vol_shape, spacing)
    Z = maps.shape[0]
    R = np.asarray(pair_fields)
    if R.shape != (Z - 1, ny, nx, 2) or R.dtype.kind != "f" or not np.isfinite(R).all():
        raise ValueError(f"pair_fields must be finite floats of shape {(Z - 1, ny, nx, 2)}, got {R.dtype} {R.shape}")
    R = R.astype(np.float64)
    T = np.asarray(pair_maps, np.float64)
    B = maps if window is None else section_maps(pair_maps)
    nodes = _field_nodes(ny, nx, ky, kx)
    D = np.zeros((Z, ny, nx, 2), np.float64)
    for z in range(Z - 1):
        at = nodes @ B[z][:, :2].T + B[z][:, 2] + D[z]
        D[z + 1] = D[z] @ T[z][:, :2].T + _field_interp(R[z], ky, kx, at)
    if window is None:
        return maps, D
    out = np.empty_like(D)
    for z in range(Z):
        L, b = B[z][:, :2], B[z][:, 2]
        q = nodes @ maps[z][:, :2].T + maps[z][:, 2] - b
        out[z] = _field_interp(D[z], ky, kx, q @ np.linalg.inv(L).T)
    h, trend = window // 2, np.empty_like(out)
    for z in range(Z):
        run = np.sort(out[max(z - h, 0):min(z + h + 1, Z)], axis=0)
        trend[z] = run[(run.shape[0] - 1) // 2]
    return maps, out - trend


def _check_qfield(U, ky, kx, what):
    """int32 [Z, ny, nx, 2] `U` inside tem_u8_warp_field's limits, or ValueError naming the section, node and limit."""
    V = U.astype(np.int64)
    bad = np.argwhere(np.abs(V) > FIELD_MAX)
    if bad.size:
        z, i, j, c = (int(v) for v in bad[0])
        raise ValueError(f"{what}: section {z}, node ({i}, {j}): the displacement {V[z, i, j, c] / WARP_UNIT:g} px is "
                         f"outside the limit of {FIELD_MAX // WARP_UNIT} px")
    for axis, k, name in ((1, ky, "y"), (2, kx, "x")):
        bad = np.argwhere(np.abs(np.diff(V, axis=axis)) > WARP_MAX_DEV << k)
        if bad.size:
            z, i, j, c = (int(v) for v in bad[0])
            raise ValueError(f"{what}: section {z}, node ({i}, {j}): the displacement changes by "
                             f"{np.diff(V, axis=axis)[z, i, j, c] / WARP_UNIT:g} px to the next node along {name}, above "
                             f"the limit of 1/8 of the spacing, {(1 << k) / 8:g} px")
    return U


def quantize_field(fields, spacing):
    """np.int32[Z, ny, nx, 2] = (u_y, u_x) in units of 2^-16 px, rounded with rint, of float fields [Z, ny, nx, 2] in
    pixels (section_fields'): what tem_u8_warp_field and volume_warp_field compute with.  ValueError for another shape
    or dtype, values that are not finite, a bad spacing, a displacement above 32 px (|U| > 2^21), and two adjacent nodes
    that differ by more than one eighth of the spacing (S 2^13) -- the gradient limit, the size of the matrix limit of
    quantize_maps, which is what bounds the kernel's staging hull; the message names the section, the node and the
    limit."""
    ky, kx = _field_spacing(spacing)
    f = np.asarray(fields)
    if f.ndim != 4 or f.shape[3] != 2 or f.shape[1] < 2 or f.shape[2] < 2 or f.dtype.kind != "f":
        raise ValueError(f"fields must be floats of shape [Z, ny, nx, 2], got {f.dtype} {f.shape}")
    if not np.isfinite(f).all():
        raise ValueError("fields must be finite")
    f = np.rint(np.clip(f.astype(np.float64), -1024.0, 1024.0) * WARP_UNIT)         # far outside the limit either way
    return _check_qfield(f.astype(np.int64), ky, kx, "fields").astype(np.int32)


def _field_table(fields, shape, ky, kx, one):
    """volume_warp_field's `fields` as the int32 table of `shape` [Z, ny, nx, 2]: float is quantised, int32 is checked;
    one image also takes one field [ny, nx, 2]."""
    f = np.asarray(fields)
    if one and f.ndim == 3:
        f = f[None]
    if f.dtype.kind == "f" and f.shape == shape:
        return np.ascontiguousarray(quantize_field(f, (1 << ky, 1 << kx)))
    if f.dtype == np.int32 and f.shape == shape:
        return _check_qfield(np.array(f), ky, kx, "fields")                          # a writable, dense copy
    raise ValueError(f"fields must be floats or int32 of shape {shape}, got {f.dtype} {f.shape}")


def _field_rows(M, U, ky, kx, x0, x1, Y):
    """_warp_rows with the field, as a function rows(z0, z1, y0, y1): per section the affine extremes over the box's
    corners plus the least and largest u_y over the nodes of the cells the box meets, [min iy, max iy + 2), unioned over
    the sections and clipped.  Runs of sections over the same rows (how a slab grows) share one pass over all sections."""
    memo = {}

    def per_section(z0, z1, y0, y1):
        u = U[z0:z1, y0 >> ky:((y1 - 1) >> ky) + 2, x0 >> kx:((x1 - 1) >> kx) + 2, 0].reshape(z1 - z0, -1).astype(np.int64)
        a, b, c = M[z0:z1, 0], M[z0:z1, 1], M[z0:z1, 2]
        s, ey, ex = a * y0 + b * x0 + c, a * (y1 - 1 - y0), b * (x1 - 1 - x0)
        return ((s + np.minimum(ey, 0) + np.minimum(ex, 0) + u.min(axis=1) + 128) >> 16,
                (s + np.maximum(ey, 0) + np.maximum(ex, 0) + u.max(axis=1) + 128) >> 16)

    def rows(z0, z1, y0, y1):
        if z1 - z0 == 1:
            lo, hi = per_section(z0, z1, y0, y1)
        else:
            if (y0, y1) not in memo:
                memo.clear()
                memo[y0, y1] = per_section(0, M.shape[0], y0, y1)
            lo, hi = (v[z0:z1] for v in memo[y0, y1])
        lo = min(max(int(lo.min()), 0), Y - 1)
        return lo, max(min(int(hi.max()) + 2, Y), lo + 1)
    return rows


def field_chunks(out_box, vol_shape, M, U, spacing, chunk_bytes=None, rank=0, world_size=1):
    """warp_chunks for volume_warp_field: the same cut of the (z, y, x) (lo, hi) box `out_box` into (output slab, read
    slab) under the maps `M`, quantize_maps' int64[Z, 6], and the fields `U`, quantize_field's int32[Z, ny, nx, 2] on the
    lattice of `spacing` -- the same budget, order, round-robin and refusals.  A read slab's rows bound every tap by
    tem_u8_warp_field's rule: per section the extremes of the affine sy over the output slab's corners plus the least
    and the largest u_y over the nodes of the cells the slab meets, [min iy, max iy + 2), unioned over the slab's
    sections and clipped to the section (one row at the least).  With U = 0 it is warp_chunks.  Pure host function;
    ValueError as warp_chunks, and for a bad spacing or fields of another shape or dtype or outside the limits."""
    budget = _budget(chunk_bytes, rank, world_size)
    vol_shape = tuple(int(v) for v in vol_shape)
    if len(vol_shape) != 3 or min(vol_shape) < 1:
        raise ValueError(f"field_chunks takes a non-empty volume shape [z, y, x], got {vol_shape}")
    Z, Y, X = vol_shape
    ky, kx = _field_spacing(spacing)
    M, U = np.asarray(M), np.asarray(U)
    if M.dtype != np.int64 or M.shape != (Z, 6):
        raise ValueError(f"M must be int64 of shape {(Z, 6)}, got {M.dtype} {M.shape}")
    _check_qmaps(M, "M")
    if U.dtype != np.int32 or U.shape != (Z,) + field_grid(vol_shape, spacing) + (2,):
        raise ValueError(f"U must be int32 of shape {(Z,) + field_grid(vol_shape, spacing) + (2,)}, got {U.dtype} {U.shape}")
    _check_qfield(U, ky, kx, "U")
    (z0, z1), (y0, y1), (x0, x1) = out_box
    if any(lo < 0 or hi > n for (lo, hi), n in zip(out_box, vol_shape)):
        raise ValueError(f"the box {tuple(out_box)} reaches outside the volume of shape {vol_shape}")
    if z1 <= z0 or y1 <= y0 or x1 <= x0:
        return []
    return _row_cut_slabs(_field_rows(M, U, ky, kx, x0, x1, Y), out_box, X, budget)[rank::world_size]


def volume_warp_field(volume, maps, fields, spacing, out=None, start=None, size=None, fill=0, nearest=False,
                      chunk_bytes=None, rank=0, world_size=1, device=None, stats=None):
    """volume_warp with a smooth displacement field on top of every section's map, on the device: out[z](p) =
    volume[z](B_z p + u_z(p)), B = `maps` as volume_warp takes them (float [Z, 2, 3] or quantize_maps' int64 [Z, 6]) and
    u_z = `fields`[z] interpolated bilinearly on the lattice of `spacing` (field_grid): float [Z, ny, nx, 2] in pixels
    (section_fields'; quantised inside with quantize_field) or quantize_field's int32 [Z, ny, nx, 2].  One image [y, x]
    takes one map and one field [ny, nx, 2].  This is the elastic link of the chain: section_shift_sums ->
    shift_subpixel -> fit_section_maps -> fit_section_fields -> section_fields -> volume_warp_field; with zero fields
    it reproduces volume_warp byte for byte.

    The field at a voxel is the bilinear blend of its cell's four nodes in integers, floored to 2^-16 px, added to the
    affine position; from there on everything is volume_warp's: rounded half up to 1/256 px, `fill` outside and never
    blended, one rounding of the blend, `nearest` for masks -- a defect mask moves through the same field
    (tem_u8_warp_field; include/tem_hip.h has the definition, numpy reproduces it bit for bit).  A displacement is at
    most 32 px and changes by at most one eighth of the spacing from node to node.  A voxel depends on its section, its
    map and its field alone, not on the slab, ROI or rank it was computed in.

    `out`, `start` / `size`, `fill`, `chunk_bytes`, `rank` / `world_size`, `device` and `stats` (`read_s`, `write_s`,
    `chunks`) are volume_warp's, and so is the pass: the ROI is cut into output slabs and the read slabs that hold
    their taps (field_chunks); host thread -> pinned -> H2D -> one tem_u8_warp_field launch per slab -> D2H -> host
    write, on double buffers, in the order write(k), read(k + 2) on the one host thread; both tables are uploaded once.

    Out of scope: resampling along z, majority resampling of labels (nearest is what masks get), and fields finer than
    16 px.  predict_cube / predict_volume take the same maps and fields as warp=Warp(maps, fields, spacing) and align
    on the way in, without the aligned copy.

    ValueError, before any GPU work: everything volume_warp refuses, a bad spacing, fields of a wrong shape or dtype
    or outside the limits."""
    _check_u8(volume)
    vshape = tuple(int(v) for v in volume.shape)
    if len(vshape) not in (2, 3) or min(vshape) < 1:
        raise ValueError(f"volume_warp_field needs a non-empty volume [z, y, x] or one image [y, x], got shape {vshape}")
    one = len(vshape) == 2
    vol3 = (1,) + vshape if one else vshape
    ky, kx = _field_spacing(spacing)
    ny, nx = field_grid(vshape, spacing)
    M = _warp_table(maps, vol3[0], one)
    U = _field_table(fields, (vol3[0], ny, nx, 2), ky, kx, one)
    fill = _index(fill, "fill")
    if not 0 <= fill <= 255:
        raise ValueError(f"fill must lie in 0...255, got {fill}")
    box = hist_box(vshape, start, size)
    out = _roi_out(out, box, one)
    chunks = field_chunks(box, vol3, M, U, (1 << ky, 1 << kx), chunk_bytes, rank, world_size)
    p = _SlabPass([volume], [hist_box(vshape)], chunk_bytes, rank, world_size, device, slabs=[r for _, r in chunks])
    lib = H.require_gpu()
    oslabs = [o for o, _ in chunks]
    per = ny * nx * 8                                                       # bytes of one section's field
    with p.streaming(stats):
        table, ftable = torch.from_numpy(M).to(p.dev), torch.from_numpy(U).to(p.dev)   # both tables, once
        with p.writing(out, box, oslabs) as outp:
            for k, ((z0, _), (y0, _), _), d, (src,) in p:
                _lib.check(lib.tem_u8_warp_field(src.data_ptr(), *d, y0, vol3[1], outp.device(k).data_ptr(),
                                                 *(hi - lo for lo, hi in oslabs[k]), oslabs[k][1][0], oslabs[k][2][0],
                                                 M.ctypes.data + 48 * z0, table.data_ptr() + 48 * z0,
                                                 U.ctypes.data + per * z0, ftable.data_ptr() + per * z0, ny, nx, ky, kx,
                                                 fill, int(bool(nearest)), p.compute.cuda_stream), "tem_u8_warp_field")
                p.put(k)
    return out


WARP_MAX_WGS = (1 << 24) - 1     # workgroups of one warp launch: 16 x 64 outputs of one plane each


class Warp(NamedTuple):
    """What the `warp=` keyword of predict_cube / predict_volume takes: how every section of a uint8 volume [z, y, x] is
    aligned ahead of the prediction.  `maps` are volume_warp's -- float [Z, 2, 3] (section_maps') or quantize_maps' int64
    [Z, 6], one image also takes one map --; `fields` with `spacing` are volume_warp_field's -- float or quantize_field's
    int32 [Z, ny, nx, 2] on the lattice of `spacing` (field_grid) --, both None for the maps alone; `fill` (0...255) is
    what a voxel reads whose position lies outside its section.  The prediction is that of the same call on
    volume_warp_field(volume, maps, fields, spacing, fill=fill) (volume_warp without a field), which is never made."""
    maps: object
    fields: object = None
    spacing: object = None
    fill: int = 0


class _WarpSpec(NamedTuple):
    """_check_warp's result: `M` np.int64[Z, 6], `U` np.int32[Z, ny, nx, 2] or None, the lattice (ny, nx, ky, kx), all 0
    without a field, and `fill`."""
    M: np.ndarray
    U: object
    ny: int
    nx: int
    ky: int
    kx: int
    fill: int


def _check_warp(warp, vol_shape):
    """None, or the _WarpSpec of `warp` (a Warp, or any (maps, fields, spacing, fill) tuple) for a volume of shape
    `vol_shape` [z, y, x] or one image [y, x]: the tables that volume_warp / volume_warp_field compute with, through
    _warp_table and _field_table, with their limits and messages.  ValueError also for fields without a spacing or a
    spacing without fields, and a fill outside 0...255."""
    if warp is None or isinstance(warp, _WarpSpec):
        return warp
    try:
        maps, fields, spacing, fill = warp
    except (TypeError, ValueError):
        raise ValueError(f"warp must be None or a Warp (maps, fields, spacing, fill), got {type(warp).__name__}")
    shape = tuple(int(v) for v in vol_shape)
    if len(shape) not in (2, 3) or min(shape) < 1:
        raise ValueError(f"warp needs a non-empty volume [z, y, x] or one image [y, x], got shape {shape}")
    one = len(shape) == 2
    Z = 1 if one else shape[0]
    M = _warp_table(maps, Z, one)
    if (fields is None) != (spacing is None):
        raise ValueError("warp: fields and spacing go together, give both or neither")
    U, ny, nx, ky, kx = None, 0, 0, 0, 0
    if fields is not None:
        ky, kx = _field_spacing(spacing)
        ny, nx = field_grid(shape, spacing)
        U = np.ascontiguousarray(_field_table(fields, (Z, ny, nx, 2), ky, kx, one))
    fill = _index(fill, "fill")
    if not 0 <= fill <= 255:
        raise ValueError(f"fill must lie in 0...255, got {fill}")
    return _WarpSpec(np.ascontiguousarray(M), U, ny, nx, ky, kx, fill)


def _warp_span(w, c, z0, z1, y0, y1, x0, x1, n, nearest):
    """tem_u8_warp_box's rule along one axis, per section of [z0, z1), for the outputs [y0, y1) x [x0, x1): c = 0 the
    rows (sy, U[..][0]) of a section of n rows, c = 1 the columns (sx, U[..][1]) of one of n columns.  The extremes of
    the affine position at the box's corners plus the least and largest node of the cells the box meets, the position
    in 1/256 px cut to [0, 256 (n - 1)].  Returns (some, first, last): whether that interval is not empty, and the
    first and last row (column) a tap of weight above 0 can lie in."""
    a, b, t = (w.M[z0:z1, 3 * c + i] for i in range(3))
    s, ey, ex = a * y0 + b * x0 + t, a * (y1 - 1 - y0), b * (x1 - 1 - x0)
    lo, hi = s + np.minimum(ey, 0) + np.minimum(ex, 0), s + np.maximum(ey, 0) + np.maximum(ex, 0)
    if w.U is not None:
        u = w.U[z0:z1, y0 >> w.ky:((y1 - 1) >> w.ky) + 2, x0 >> w.kx:((x1 - 1) >> w.kx) + 2, c]
        u = u.reshape(z1 - z0, -1).astype(np.int64)
        lo, hi = lo + u.min(axis=1), hi + u.max(axis=1)
    flo, fhi = np.maximum((lo + 128) >> 8, 0), np.minimum((hi + 128) >> 8, 256 * (n - 1))
    if nearest:
        return flo <= fhi, (flo + 128) >> 8, (fhi + 128) >> 8
    return flo <= fhi, flo >> 8, (fhi >> 8) + ((fhi & 255) != 0)


def warp_source_box(box, warp, vol_shape, nearest=False):
    """((y0, y1), (x0, x1)): the rows and columns of the raw volume of shape `vol_shape` [z, y, x] that hold every tap
    of the (z, y, x) (lo, hi) `box` of the volume aligned by `warp` (a Warp) -- what predict_volume(..., warp=) reads
    for a chunk whose footprint is `box`, in place of the footprint itself.  It is the union over the box's sections of
    exactly the rows and columns that tem_u8_warp_box demands of its source block (include/tem_hip.h: per section the
    extremes of the affine position at the box's corners plus the least and largest node of the cells the box meets,
    cut to the section; `nearest`: the rule for masks), so a launch on a planned box is never refused; a section that
    is wholly outside by the same bounds demands nothing, and None is returned where every section is.  With identity
    maps and a zero field the result is the box's own rows and columns, exactly.  Pure host function; ValueError for a
    box that is empty or leaves the volume, and _check_warp's."""
    vol_shape = tuple(int(v) for v in vol_shape)
    if len(vol_shape) != 3 or min(vol_shape) < 1:
        raise ValueError(f"warp_source_box takes a non-empty volume shape [z, y, x], got {vol_shape}")
    w = _check_warp(warp, vol_shape)
    if w is None:
        raise ValueError("warp_source_box needs a Warp")
    (z0, z1), (y0, y1), (x0, x1) = ((int(lo), int(hi)) for lo, hi in box)
    if any(lo < 0 or hi > n or hi <= lo for (lo, hi), n in zip(((z0, z1), (y0, y1), (x0, x1)), vol_shape)):
        raise ValueError(f"the box {tuple(box)} is empty or reaches outside the volume of shape {vol_shape}")
    ys, ya, yb = _warp_span(w, 0, z0, z1, y0, y1, x0, x1, vol_shape[1], nearest)
    xs, xa, xb = _warp_span(w, 1, z0, z1, y0, y1, x0, x1, vol_shape[2], nearest)
    need = ys & xs
    if not need.any():
        return None
    return ((int(ya[need].min()), int(yb[need].max()) + 1), (int(xa[need].min()), int(xb[need].max()) + 1))


def _warp_footprints(chunks, max_gap, wp, vol_shape, with_mask):
    """predict_volume's reads under `warp` (wp: _check_warp's spec), per chunk of `chunks` (chunk_plan's): (foot, sbox,
    mbox).  foot[k] is the (z, y, x) (lo, hi) box of the aligned volume that chunk k's device block holds -- its
    footprint `read`, with `max_gap` (repair's; 0 without) more sections on each side of z, clipped to the volume -- or
    None for a chunk wholly outside the volume; sbox[k] = warp_source_box(foot[k]) the rows and columns of the raw
    volume's same sections that are read for it (None: nothing is read, the block is `fill`); mbox[k] the same for a
    Repair's mask, which is moved with nearest (None without a mask)."""
    foot = [((max(c.read[0][0] - max_gap, 0), min(c.read[0][1] + max_gap, vol_shape[0])),) + tuple(c.read[1:])
            if min(c.block) > 0 else None for c in chunks]
    sbox = [None if f is None else warp_source_box(f, wp, vol_shape) for f in foot]
    mbox = [None if f is None or not with_mask else warp_source_box(f, wp, vol_shape, nearest=True) for f in foot]
    return foot, sbox, mbox


class _Warper:
    """The device leg of the `warp=` keyword, made once per call: the tables of `spec` (_check_warp's) are uploaded here,
    once, and box() resamples sections of a dense source box into a dense output box on `stream` (tem_u8_warp_box)."""

    def __init__(self, lib, spec, dev, stream, vol_shape):
        self.lib, self.w, self.stream, self.vol = lib, spec, stream, tuple(vol_shape)
        self.M_dev = torch.from_numpy(spec.M).to(dev)
        self.U_dev = None if spec.U is None else torch.from_numpy(spec.U).to(dev)
        self.per = spec.ny * spec.nx * 8                                     # bytes of one section's field

    def box(self, src, dst, zs, source, out, nearest=False, fill=None):
        """Sections [zs[0], zs[1]) of the volume: the dense block at `src` holds their rows and columns `source` =
        ((y0, y1), (x0, x1)), the dense block at `dst` receives the aligned sections' box `out` of the same form.  One
        launch per run of sections that stays within a launch's workgroups.  `fill` defaults to the spec's."""
        (z0, z1), ((sy0, sy1), (sx0, sx1)), ((oy0, oy1), (ox0, ox1)) = zs, source, out
        BH, BW, OH, OW, w = sy1 - sy0, sx1 - sx0, oy1 - oy0, ox1 - ox0, self.w
        run = max(WARP_MAX_WGS // (-(-OH // 16) * -(-OW // 64)), 1)
        for z in range(z0, z1, run):
            n, field = min(run, z1 - z), w.U is not None
            _lib.check(self.lib.tem_u8_warp_box(
                src + (z - z0) * BH * BW, n, BH, BW, sy0, sx0, self.vol[1], self.vol[2], dst + (z - z0) * OH * OW, n, OH, OW,
                oy0, ox0, w.M.ctypes.data + 48 * z, self.M_dev.data_ptr() + 48 * z,
                w.U.ctypes.data + self.per * z if field else None, self.U_dev.data_ptr() + self.per * z if field else None,
                w.ny, w.nx, w.ky, w.kx, w.fill if fill is None else fill, int(bool(nearest)), self.stream),
                "tem_u8_warp_box")


def _check_compare(compare, vol_shape, stats):
    """None, or `compare` itself: a uint8 array-like of the volume's shape, reported in a dict `stats`.  A _OneSection
    is the image that the single-image form has checked already and passes on as a one-section stack."""
    if compare is None or isinstance(compare, _OneSection):
        return compare
    if not isinstance(stats, dict):
        raise ValueError("compare= reports in stats['joint_histogram']: pass a dict as `stats`")
    shape, dtype = getattr(compare, "shape", None), getattr(compare, "dtype", None)
    if shape is None or dtype is None or dtype != np.uint8:
        raise ValueError(f"compare must be a uint8 array-like, got {type(compare).__name__} of dtype {dtype}")
    if tuple(int(v) for v in shape) != tuple(int(v) for v in vol_shape):
        raise ValueError(f"compare must have the volume's shape {tuple(vol_shape)}, got {tuple(shape)}")
    return compare


def _inside(lo, hi, shift, vol_shape):
    """The (z, y, x) (lo, hi) box [lo + shift, hi + shift) clipped to a volume of shape vol_shape, or None where it
    misses the volume."""
    box = tuple((max(l + s, 0), min(h + s, n)) for l, h, s, n in zip(lo, hi, shift, vol_shape))
    return box if all(h > l for l, h in box) else None


def meanstd_from_histogram(h):
    """(np.float32 mean, np.float32 std) of the SCALED values v / 127.5 - 1 of the voxels a 256-bin histogram `h`
    counts (a [Z, 256] per-section histogram is summed over its rows first): the unit `meanstd_x` / `meanstd_y` are
    in.  The standard deviation is the population one; both are computed in float64 from the counts and rounded once.
    This is datasets.get_meanstd of a dataset that holds the ROI as ONE tensor (which accumulates in float32, so the
    last bits may differ).  Over several tensors get_meanstd is another quantity: it averages the per-tensor means and
    the per-tensor variances, which leaves the spread of the tensors' means out of the variance.  ValueError on an
    empty histogram."""
    h = np.asarray(h)
    if h.ndim not in (1, 2) or h.shape[-1] != 256:
        raise ValueError(f"a histogram has 256 bins ([256] or [Z, 256]), got shape {h.shape}")
    h = h.reshape(-1, 256).astype(np.float64).sum(axis=0)
    n = h.sum()
    if not n > 0:
        raise ValueError("meanstd_from_histogram: the histogram is empty")
    v = np.arange(256, dtype=np.float64) / 127.5 - 1.0
    mean = (h * v).sum() / n
    var = (h * (v - mean) ** 2).sum() / n
    return np.float32(mean), np.float32(np.sqrt(var))


def _match_row(hs, hr):
    cs, cr, a = [], [], 0
    for c in hs:
        a += int(c)
        cs.append(a)
    a = 0
    for c in hr:
        a += int(c)
        cr.append(a)
    ns, nr = cs[-1], cr[-1]
    if nr == 0:
        raise ValueError("match_lut: the reference histogram is empty")
    if ns == 0:
        return list(range(256))
    lut, w = [], 0
    for v in range(256):                    # cs is non-decreasing, so w only moves up; cr[255] nr == nr ns ends it
        while cs[v] * nr > cr[w] * ns:
            w += 1
        lut.append(w)
    return lut


def match_lut(h_src, h_ref):
    """The classical histogram match as a lookup table: np.uint8[256] with lut[v] = the smallest w whose reference CDF
    reaches the source CDF of v, cdf_ref(w) >= cdf_src(v), decided in exact integer arithmetic on the cumulative
    counts (cs[v] N_ref <= cr[w] N_src, Python ints).  The table is non-decreasing, and the identity on the occupied
    bins when both histograms are the same.  Row-wise for an h_src of shape [Z, 256] (per-section histograms), against
    one h_ref [256] or [Z, 256] of them: returns [Z, 256], the form predict_cube / predict_volume take as `lut`.  A
    source row without voxels gets the identity; an empty reference raises ValueError, as negative counts do."""
    hs, hr = np.asarray(h_src), np.asarray(h_ref)
    for name, h in (("h_src", hs), ("h_ref", hr)):
        if h.ndim not in (1, 2) or h.shape[-1] != 256 or h.dtype.kind not in "iu":
            raise ValueError(f"match_lut: {name} must be integer counts of shape [256] or [Z, 256], got {h.dtype} "
                             f"{h.shape}")
        if h.size and int(h.min()) < 0:
            raise ValueError(f"match_lut: {name} has negative counts")
    if hs.ndim == 1:
        if hr.ndim != 1:
            raise ValueError("match_lut: a [Z, 256] h_ref needs a [Z, 256] h_src")
        return np.array(_match_row(hs, hr), np.uint8)
    if hr.ndim == 2 and hr.shape[0] != hs.shape[0]:
        raise ValueError(f"match_lut: h_src has {hs.shape[0]} rows, h_ref {hr.shape[0]}")
    return np.array([_match_row(hs[z], hr[z] if hr.ndim == 2 else hr) for z in range(hs.shape[0])],
                    np.uint8).reshape(hs.shape[0], 256)


def _check_lut(lut, vol_shape):
    """None, or `lut` as a C-contiguous np.uint8 array: [256], or [Z, 256] with Z the section count of the volume of
    shape `vol_shape` ([z, y, x]; one image [y, x] has one section).  ValueError for anything else."""
    if lut is None:
        return None
    if not isinstance(lut, np.ndarray) or lut.dtype != np.uint8:
        raise ValueError(f"lut must be a numpy uint8 array, got {getattr(lut, 'dtype', type(lut).__name__)}")
    Z = int(vol_shape[0]) if len(vol_shape) == 3 else 1
    if lut.shape != (256,) and lut.shape != (Z, 256):
        raise ValueError(f"lut must have shape (256,) or ({Z}, 256) -- one row per section of the volume -- got "
                         f"{lut.shape}")
    return np.ascontiguousarray(lut)


def _check_histogram(histogram, stats):
    if not isinstance(histogram, (bool, np.bool_)):
        raise ValueError(f"histogram must be True or False, got {histogram!r}")
    if histogram and not isinstance(stats, dict):
        raise ValueError("histogram=True reports in stats['histogram']: pass a dict as `stats`")
    return bool(histogram)


def _lut_host(vol, lut):
    """lut[vol], or lut[z][vol[z]] for a [Z, 256] table: what tem_u8_lut leaves on the device."""
    return lut[vol] if lut.ndim == 1 else lut[np.arange(vol.shape[0])[:, None, None], vol]


CLAHE_MAX_TILE = 2048            # th, tw of a CLAHE tile: the remap's numerator then stays below 2^32
CLAHE_ACC_BYTES = 1 << 30        # clahe_histograms: one device accumulator for the volume up to this size, else one per slab


class ClaheTables(NamedTuple):
    """What the `clahe=` keyword takes: the np.uint8[Z, gy, gx, 256] tables of clahe_tables and the tile they belong to."""
    tables: np.ndarray
    tile: tuple          # (th, tw), or an int for a square tile


def _clahe_tile(tile):
    """(th, tw) of `tile`, an int or a pair of ints in [1, CLAHE_MAX_TILE]."""
    import operator
    try:
        th, tw = (tile, tile) if not hasattr(tile, "__len__") else tile
        if isinstance(th, (bool, np.bool_)) or isinstance(tw, (bool, np.bool_)):
            raise TypeError
        th, tw = operator.index(th), operator.index(tw)
    except (TypeError, ValueError):
        raise ValueError(f"tile must be an int or (th, tw), got {tile!r}")
    if not (1 <= th <= CLAHE_MAX_TILE and 1 <= tw <= CLAHE_MAX_TILE):
        raise ValueError(f"tile {(th, tw)} is outside [1, {CLAHE_MAX_TILE}]")
    return th, tw


def clahe_grid(vol_shape, tile):
    """(gy, gx) = (ceil(Y / th), ceil(X / tw)): the tiles of (th, tw) pixels over (y, x) -- `tile`, an int or (th, tw) in
    [1, 2048] -- that cover a section of a volume of shape [Z, Y, X] or an image [Y, X].  The grid is anchored at the
    volume's (0, 0); its last row and column may be partial.  Pure host function."""
    th, tw = _clahe_tile(tile)
    shape = tuple(int(v) for v in vol_shape)
    if len(shape) not in (2, 3) or min(shape) < 1:
        raise ValueError(f"volume must be a non-empty [z, y, x] or one image [y, x], got shape {shape}")
    return -(-shape[-2] // th), -(-shape[-1] // tw)


def _check_u8(volume):
    if getattr(volume, "dtype", np.dtype(np.uint8)) != np.uint8:
        raise ValueError(f"volume must be uint8, got {volume.dtype}")


def clahe_histograms(volume, tile=128, chunk_bytes=None, rank=0, world_size=1, device=None, stats=None):
    """The tile histograms CLAHE starts from: np.uint32[Z, gy, gx, 256] with h[z, i, j, v] the count of value v in
    volume[z, i*th:(i+1)*th, j*tw:(j+1)*tw], over the WHOLE uint8 `volume` [z, y, x] (one image [y, x]: Z = 1), since
    the tiles outside an ROI still feed a prediction's halo and its folded boundaries.

    Out of core exactly as volume_histogram: slabs of at most `chunk_bytes` (hist_chunks; a slab of rows may cut a
    tile), one host thread -> pinned -> H2D -> tem_u8_hist_tiles adding into a device accumulator.  The accumulator
    holds the whole volume's Z*gy*gx*1024 bytes and is read back once where that is at most CLAHE_ACC_BYTES; else it
    holds one slab's sections and is read back, and added on the host, per slab.  Ranks take slabs round-robin and
    their results add up to the whole.  `stats` receives `read_s` and `chunks`."""
    th, tw = _clahe_tile(tile)
    gy, gx = clahe_grid(volume.shape, (th, tw))
    box = hist_box(volume.shape)
    p = _SlabPass([volume], [box], chunk_bytes, rank, world_size, device)
    lib = H.require_gpu()
    with p.streaming(stats):
        acc = _RowAccumulator(p.dev, box[0][1], (gy, gx, 256), _most_rows(s[0] for s in p.slabs), np.uint32)
        for k, ((z0, z1), (y0, _), (x0, _)), d, (src,) in p:
            _lib.check(lib.tem_u8_hist_tiles(src.data_ptr(), *d, y0, x0, th, tw, gy, gx, acc.ptr(z0, z1),
                                             p.compute.cuda_stream), "tem_u8_hist_tiles")
            acc.add(z0, z1)
        return acc.result()


def _clahe_params(clip_limit, z_radius):
    import operator
    try:
        if isinstance(z_radius, (bool, np.bool_)):
            raise TypeError
        r = operator.index(z_radius)
    except TypeError:
        raise ValueError(f"z_radius must be a non-negative integer, got {z_radius!r}")
    if r < 0:
        raise ValueError(f"z_radius must be a non-negative integer, got {z_radius!r}")
    if clip_limit is not None:
        clip_limit = float(clip_limit)
        if not clip_limit > 0:
            raise ValueError(f"clip_limit must be positive (None: no clipping), got {clip_limit!r}")
    return clip_limit, r


# _CLAHE_SPREAD[r, k] = 1 where bin k is one of the r bins {floor(j * 256 / r) : j < r} that take one count of a
# remainder of r
_CLAHE_SPREAD = np.zeros((256, 256), np.int64)
for _r in range(1, 256):
    _CLAHE_SPREAD[_r, (np.arange(_r) * 256) // _r] = 1
del _r


def clahe_tables(h, clip_limit=3.0, z_radius=0):
    """The equalisation tables np.uint8[Z, gy, gx, 256] of the tile histograms `h` (integer counts [Z, gy, gx, 256],
    clahe_histograms' result), in exact integer arithmetic on the host:

      * z_radius = r > 0 replaces h[z] by the sum of h[max(z - r, 0) : min(z + r + 1, Z)] (damps section-to-section
        flicker); n = h.sum(-1) is the tile's voxel count;
      * clip_limit = c clips every bin at clip = max(1, floor(c * n / 256)) (float64) and spreads the excess evenly:
        h = min(h, clip) + excess // 256, and with rem = excess % 256 the bins {floor(j * 256 / rem) : j < rem} get one
        more -- the total stays n.  c = 1 flattens the histogram (the identity, nearly), large c leaves it alone;
        clip_limit=None does not clip: plain adaptive equalisation;
      * T[v] = (cdf[v] * 255 + n // 2) // n with cdf = cumsum(h): non-decreasing, T[255] = 255.

    A tile without voxels (n = 0: only in the partial result of one rank) gets the identity.  ValueError for a negative
    or non-integer z_radius, clip_limit <= 0, and an `h` that is no integer array of shape [Z, gy, gx, 256]."""
    clip_limit, r = _clahe_params(clip_limit, z_radius)
    h = np.asarray(h)
    if h.ndim != 4 or h.shape[-1] != 256 or h.dtype.kind not in "iu":
        raise ValueError(f"clahe_tables: h must be integer counts of shape [Z, gy, gx, 256], got {h.dtype} {h.shape}")
    h = h.astype(np.int64)
    if h.size and int(h.min()) < 0:
        raise ValueError("clahe_tables: h has negative counts")
    Z = h.shape[0]
    if r > 0 and Z:
        c = np.concatenate([np.zeros((1,) + h.shape[1:], np.int64), np.cumsum(h, axis=0)])
        z = np.arange(Z)
        h = c[np.minimum(z + r + 1, Z)] - c[np.maximum(z - r, 0)]
    n = h.sum(-1)
    if clip_limit is not None:
        clip = np.maximum(1, np.floor(clip_limit * n.astype(np.float64) / 256.0).astype(np.int64))[..., None]
        excess = np.maximum(h - clip, 0).sum(-1)
        h = np.minimum(h, clip) + (excess // 256)[..., None] + _CLAHE_SPREAD[excess % 256]
    cdf = np.cumsum(h, axis=-1)
    n1 = np.maximum(n, 1)[..., None]
    T = (cdf * 255 + n1 // 2) // n1
    T = np.where(n[..., None] > 0, T, np.arange(256))
    return T.astype(np.uint8)


def _check_clahe(clahe, vol_shape):
    """None, or (tables, th, tw, gy, gx) of a ClaheTables (any (tables, tile) pair) for a volume of shape `vol_shape`
    ([z, y, x]; one image [y, x] has one section): tables as a C-contiguous np.uint8[Z, gy, gx, 256].  ValueError for
    anything else."""
    if clahe is None:
        return None
    try:
        tables, tile = clahe
    except (TypeError, ValueError):
        raise ValueError(f"clahe must be None or a ClaheTables (tables, tile), got {type(clahe).__name__}")
    th, tw = _clahe_tile(tile)
    if not isinstance(tables, np.ndarray) or tables.dtype != np.uint8:
        raise ValueError(f"clahe tables must be a numpy uint8 array, got {getattr(tables, 'dtype', type(tables).__name__)}")
    gy, gx = clahe_grid(vol_shape, (th, tw))
    Z = int(vol_shape[0]) if len(vol_shape) == 3 else 1
    if tables.shape != (Z, gy, gx, 256):
        raise ValueError(f"clahe tables must have shape {(Z, gy, gx, 256)} -- (Z, gy, gx, 256) of a volume of shape "
                         f"{tuple(vol_shape)} under tile {(th, tw)} -- got {tables.shape}")
    return np.ascontiguousarray(tables), th, tw, gy, gx


def clahe_fit(volume, tile=128, clip_limit=3.0, z_radius=0, **kw):
    """clahe_histograms(volume, tile, **kw) -> clahe_tables(..., clip_limit, z_radius) as a ClaheTables: what
    clahe_volume, predict_cube and predict_volume take as `clahe`.  The tables hold Z*gy*gx*256 bytes."""
    _clahe_params(clip_limit, z_radius)
    tile = _clahe_tile(tile)
    return ClaheTables(clahe_tables(clahe_histograms(volume, tile, **kw), clip_limit, z_radius), tile)


def clahe_volume(volume, clahe, out=None, start=None, size=None, chunk_bytes=None, histogram=False, stats=None, rank=0,
                 world_size=1, device=None):
    """Contrast-limited adaptive histogram equalisation of the ROI [start, start + size) ((x, y, z) order; default: the
    whole volume) of a uint8 array-like `volume` [z, y, x] (or one image [y, x] with 2-element start / size) by the
    tables `clahe` (a ClaheTables of the WHOLE volume: clahe_fit), written into `out`: a writable uint8 array-like of
    the ROI's shape (ndarray, memmap, h5py, zarr; allocated when None), which is returned.  This is how training
    volumes are prepared, so that the datasets crop equalised data, and what predict_*(clahe=...) sees without the copy.

    Every voxel of value v at (z, y, x) becomes the bilinear interpolation, in integers and rounded half up, of the
    tables of the four tiles whose centres surround it, at v (tem_u8_clahe; include/tem_hip.h has the formula).  The
    tile grid belongs to the volume, so the result of an ROI is the ROI of the whole result, however it is cut.

    Out of core: the ROI is cut into slabs of at most `chunk_bytes` (hist_chunks); host thread -> pinned -> H2D ->
    tem_u8_clahe in place -> D2H -> host write, on double buffers, the I/O of neighbouring slabs overlapped.  The
    tables are uploaded once: Z*gy*gx*256 bytes.  histogram=True adds one tem_u8_hist launch over each remapped slab
    and puts the 256 bins of the equalised ROI (np.int64) into stats["histogram"], so that a match_lut towards another
    domain can follow without another pass.  Ranks take slabs round-robin and write disjoint boxes of a shared `out`
    (each reports the histogram of its own slabs).  `stats` also receives `read_s`, `write_s` and `chunks`.
    ValueError, before any GPU work: an ROI outside the volume, a non-uint8 volume, tables of another dtype or shape,
    an `out` of another shape."""
    box = hist_box(volume.shape, start, size)
    p = _SlabPass([volume], [box], chunk_bytes, rank, world_size, device)
    cl = tuple(_check_clahe(clahe, tuple(volume.shape)))        # a TypeError for None: here the tables are no option
    histogram = _check_histogram(histogram, stats)
    out = _roi_out(out, box, len(volume.shape) == 2, any_dtype=True)
    lib = H.require_gpu()
    with p.streaming(stats):
        prepare = _Prepare(lib, cl, None, p.dev, p.compute.cuda_stream)          # the tables, once
        measure = _Measure(lib, histogram, False, p.dev, p.compute.cuda_stream)
        with p.writing(out, box, own_buffers=False):
            for k, slab, d, (buf,) in p:
                prepare.apply(buf.data_ptr(), d, tuple(lo for lo, _ in slab))
                measure.add(buf.data_ptr(), d, d)
                p.put(k, buf)                                                    # remapped in place
        measure.report(p.st)
    return out


U16_BINS = 1 << 16               # bins of a 16-bit histogram and bytes of a 16-bit table: indexed by u = v (uint16), v + 32768 (int16)


def _check_16(volume):
    """True for int16, False for uint16 voxels; ValueError for any other dtype and for the other byte order."""
    dt = getattr(volume, "dtype", None)
    if dt is None or np.dtype(dt) not in (np.dtype(np.uint16), np.dtype(np.int16)) or not np.dtype(dt).isnative:
        raise ValueError(f"volume must be native-endian uint16 or int16, got {dt}")
    return np.dtype(dt).kind == "i"


def volume_histogram16(volume, start=None, size=None, per_section=False, chunk_bytes=None, rank=0, world_size=1,
                       device=None, stats=None):
    """Intensity histogram of the ROI [start, start + size) ((x, y, z) order; default: the whole volume) of a
    native-endian uint16 or int16 array-like `volume` indexed [z, y, x] (ndarray, np.memmap, h5py / zarr dataset), or
    of one image [y, x] with 2-element start / size: volume_histogram's pass over 16-bit voxels.  A voxel v counts in
    bin u = v (uint16) or u = v + 32768 (int16: the order is kept).  Returns np.int64[65536], or with per_section
    np.int64[size_z, 65536] whose row i counts section start_z + i.  ValueError, before any GPU work: another dtype or
    byte order, an ROI outside the volume.

    Out of core: slabs of at most `chunk_bytes` BYTES (hist_chunks with itemsize=2); one host thread reads each slab
    into double-buffered pinned memory -> H2D -> tem_u16_hist, adding into ONE device accumulator that is read back
    once at the end -- a per-section table is 512 KiB per section; past CLAHE_ACC_BYTES the accumulator holds one
    slab's sections and is read back, and added on the host, per slab.  `stats` receives `read_s` and `chunks`.  Ranks
    take slabs round-robin and their results add up to the whole."""
    box = hist_box(volume.shape, start, size)
    p = _SlabPass([volume], [box], chunk_bytes, rank, world_size, device, itemsize=2)
    signed = int(_check_16(volume))
    lib = H.require_gpu()
    oz, nz = box[0][0], box[0][1] - box[0][0]
    spans = [(z0 - oz, z1 - oz) if per_section else (0, 1) for (z0, z1), _, _ in p.slabs]   # a slab's rows of the table
    with p.streaming(stats):
        acc = _RowAccumulator(p.dev, nz if per_section else 1, (U16_BINS,), _most_rows(spans))
        for k, slab, d, (src,) in p:
            _lib.check(lib.tem_u16_hist(src.data_ptr(), *d, 0, d[0], 0, d[1], 0, d[2], acc.ptr(*spans[k]),
                                        int(bool(per_section)), signed, p.compute.cuda_stream), "tem_u16_hist")
            acc.add(*spans[k])
        out = acc.result()
    return out if per_section else out[0]


def _check_hist16(h, who, bins=U16_BINS):
    h = np.asarray(h)
    if h.ndim not in (1, 2) or h.shape[-1] != bins or h.dtype.kind not in "iu":
        raise ValueError(f"{who} must be integer counts of shape [{bins}] or [Z, {bins}], got {h.dtype} {h.shape}")
    if h.size and int(h.min()) < 0:
        raise ValueError(f"{who} has negative counts")
    if h.dtype == np.uint64 and h.size and int(h.max()) >= 1 << 63:
        raise ValueError(f"{who} has counts of 2^63 and more")
    return h.astype(np.int64, copy=False)


def _unit_fraction(v, what):
    try:
        f = Fraction(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a fraction in [0, 1], got {v!r}")
    if not 0 <= f <= 1:
        raise ValueError(f"{what} must be a fraction in [0, 1], got {v!r}")
    return f


def window16(h, low=Fraction(1, 1000), high=Fraction(999, 1000)):
    """The quantile window (lo, hi), in index units, of a 16-bit histogram `h` (integer counts [65536]:
    volume_histogram16's result): with C the inclusive cumulative counts and N their total, lo is the smallest u with
    C[u] / N >= low and hi the smallest u with C[u] / N >= high, decided in exact integers (C[u] den >= num N for
    low = num / den: pass Fractions; a float stands for its exact binary value).  Hot and dead pixels, a fraction below
    `low` of the voxels, do not stretch it.  hi == lo is widened by one, hi = lo + 1 (lo = 65534 at lo == 65535), so
    that window_lut16 always takes the pair; a histogram without voxels gives (0, 65535).  Row-wise for [Z, 65536]
    (per-section histograms): two np.int64[Z].  ValueError unless 0 <= low <= high <= 1."""
    lo_f, hi_f = _unit_fraction(low, "low"), _unit_fraction(high, "high")
    if lo_f > hi_f:
        raise ValueError(f"low {low!r} is above high {high!r}")
    h = _check_hist16(h, "window16: h")
    rows = h.reshape(-1, U16_BINS)
    lo, hi = np.zeros(len(rows), np.int64), np.full(len(rows), U16_BINS - 1, np.int64)
    for z, r in enumerate(rows):
        c = np.cumsum(r)
        n = int(c[-1])
        if n == 0:
            continue
        if n >= 1 << 62:
            raise ValueError("window16: more than 2^62 voxels")
        for f, dst in ((lo_f, lo), (hi_f, hi)):             # C[u] den >= num N  <=>  C[u] >= ceil(num N / den)
            dst[z] = np.searchsorted(c, -((-f.numerator * n) // f.denominator), side="left")
        if hi[z] == lo[z]:
            if lo[z] == U16_BINS - 1:
                lo[z] -= 1
            else:
                hi[z] += 1
    return (int(lo[0]), int(hi[0])) if h.ndim == 1 else (lo, hi)


def window_lut16(lo, hi, invert=False):
    """The linear window [lo, hi] -> [0, 255] as a 16-bit table np.uint8[65536]: 0 for u <= lo, 255 for u >= hi and
    (2 * 255 (u - lo) + (hi - lo)) // (2 (hi - lo)) between, rounded half up in integers; invert=True gives 255 - t
    (a detector of the other polarity).  Arrays lo, hi of Z entries (window16 of per-section histograms) give
    [Z, 65536], the form volume_to_u8 takes per section.  ValueError unless 0 <= lo < hi <= 65535 (integers)."""
    a, b = np.asarray(lo), np.asarray(hi)
    if a.dtype.kind not in "iu" or b.dtype.kind not in "iu" or a.shape != b.shape or a.ndim > 1:
        raise ValueError(f"window_lut16: lo and hi must be integers, or integer arrays of one length; got {lo!r}, {hi!r}")
    a, b = a.astype(np.int64).reshape(-1, 1), b.astype(np.int64).reshape(-1, 1)
    if a.size and not ((0 <= a) & (a < b) & (b <= U16_BINS - 1)).all():
        raise ValueError(f"window_lut16: needs 0 <= lo < hi <= 65535, got {lo!r}, {hi!r}")
    u = np.arange(U16_BINS, dtype=np.int64)[None]
    w = b - a
    t = np.clip((2 * 255 * (np.clip(u, a, b) - a) + w) // (2 * w), 0, 255)
    if invert:
        t = 255 - t
    t = t.astype(np.uint8)
    return t[0] if np.ndim(lo) == 0 else t


def _match_row16(hs, hr):
    cs, cr = np.cumsum(hs), np.cumsum(hr)
    ns, nr = int(cs[-1]), int(cr[-1])
    if nr == 0:
        raise ValueError("match_lut16: the reference histogram is empty")
    if ns == 0:
        return np.arange(U16_BINS, dtype=np.int64) >> 8
    if ns * nr < 1 << 63:                   # the smallest w with cr[w] ns >= cs[u] nr; cr[255] ns == cs[65535] nr ends it
        return np.searchsorted(cr * ns, cs * nr, side="left")
    lut, w, cr = np.empty(U16_BINS, np.int64), 0, [int(c) * ns for c in cr]
    for u, c in enumerate(cs.tolist()):     # Python ints; cs is non-decreasing, so w only moves up
        c *= nr
        while cr[w] < c:
            w += 1
        lut[u] = w
    return lut


def match_lut16(h_src, h_ref):
    """match_lut from 65,536 source bins: np.uint8[65536] with lut[u] = the smallest w in 0...255 whose reference CDF
    reaches the source CDF of u, cr[w] N_src >= cs[u] N_ref, decided in exact integers (int64 where N_src N_ref < 2^63,
    Python ints otherwise).  `h_src` is a 16-bit histogram [65536] (volume_histogram16), `h_ref` the 256-bin histogram
    of the uint8 target domain (volume_histogram).  Taken from the 16-bit counts the match can split what an 8-bit
    window has already merged.  The table is non-decreasing.  Row-wise for an h_src [Z, 65536] against one h_ref [256]
    or [Z, 256]: returns [Z, 65536], the per-section form volume_to_u8 takes.  A source row without voxels gets the
    identity coarsening u >> 8; an empty reference raises ValueError, as negative counts and other shapes do."""
    hs, hr = _check_hist16(h_src, "match_lut16: h_src"), _check_hist16(h_ref, "match_lut16: h_ref", 256)
    if hs.ndim == 1:
        if hr.ndim != 1:
            raise ValueError("match_lut16: a [Z, 256] h_ref needs a [Z, 65536] h_src")
        return _match_row16(hs, hr).astype(np.uint8)
    if hr.ndim == 2 and hr.shape[0] != hs.shape[0]:
        raise ValueError(f"match_lut16: h_src has {hs.shape[0]} rows, h_ref {hr.shape[0]}")
    out = np.empty(hs.shape, np.uint8)
    for z in range(hs.shape[0]):
        out[z] = _match_row16(hs[z], hr[z] if hr.ndim == 2 else hr)
    return out


def _check_lut16(lut, vol_shape):
    """`lut` as a C-contiguous np.uint8 array: [65536], or [Z, 65536] with Z the section count of the volume of shape
    `vol_shape` ([z, y, x]; one image [y, x] has one section).  ValueError for anything else."""
    if not isinstance(lut, np.ndarray) or lut.dtype != np.uint8:
        raise ValueError(f"lut must be a numpy uint8 array, got {getattr(lut, 'dtype', type(lut).__name__)}")
    Z = int(vol_shape[0]) if len(vol_shape) == 3 else 1
    if lut.shape != (U16_BINS,) and lut.shape != (Z, U16_BINS):
        raise ValueError(f"lut must have shape ({U16_BINS},) or ({Z}, {U16_BINS}) -- one row per section of the volume "
                         f"-- got {lut.shape}")
    return np.ascontiguousarray(lut)


def volume_to_u8(volume, lut, out=None, start=None, size=None, chunk_bytes=None, histogram=False, stats=None, rank=0,
                 world_size=1, device=None):
    """The ROI [start, start + size) ((x, y, z) order; default: the whole volume) of a native-endian uint16 or int16
    array-like `volume` [z, y, x] (or one image [y, x] with 2-element start / size) brought to uint8 by the table
    `lut`, written into `out`: a writable uint8 array-like of the ROI's shape (ndarray, memmap, h5py, zarr; allocated
    when None), which is returned.  out[z, y, x] = lut[u] with u = v (uint16) or v + 32768 (int16); `lut` is
    np.uint8[65536] (window_lut16, match_lut16, any table: gamma, inversion) or [Z, 65536] with one row per section of
    the WHOLE volume, so that an ROI's bytes are the ROI of the whole result.  The first link of the preparation chain:
    everything after it -- volume_rescale, find_defects, volume_repair, clahe_fit, predict_volume -- takes uint8.

    Out of core, clahe_volume's pass: slabs of at most `chunk_bytes` source BYTES (hist_chunks with itemsize=2); host
    thread -> pinned -> H2D -> one tem_u16_lut_u8 launch per slab into an output buffer -> D2H -> host write, on double
    buffers, in the order write(k), read(k + 2).  The table is uploaded once.  histogram=True adds one tem_u8_hist
    launch per converted slab and puts the 256 bins of the converted ROI (np.int64) into stats["histogram"], for a
    match_lut or clahe_fit that follows.  Ranks take slabs round-robin and write disjoint boxes of a shared `out` (each
    reports the histogram of its own slabs).  `stats` also receives `read_s`, `write_s` and `chunks`.
    ValueError, before any GPU work: another dtype or byte order, a table of another dtype or shape, an `out` of
    another shape or dtype, an ROI outside the volume."""
    box = hist_box(volume.shape, start, size)
    p = _SlabPass([volume], [box], chunk_bytes, rank, world_size, device, itemsize=2)
    signed = int(_check_16(volume))
    lut = _check_lut16(lut, tuple(volume.shape))
    histogram = _check_histogram(histogram, stats)
    out = _roi_out(out, box, len(volume.shape) == 2)
    lib = H.require_gpu()
    with p.streaming(stats):
        lut_dev = torch.from_numpy(lut).to(p.dev)                                # the table(s), once
        measure = _Measure(lib, histogram, False, p.dev, p.compute.cuda_stream)
        with p.writing(out, box) as outp:
            for k, slab, d, (src,) in p:
                dst = outp.device(k)
                _lib.check(lib.tem_u16_lut_u8(src.data_ptr(), *d, dst.data_ptr(), lut_dev.data_ptr(), int(lut.ndim == 2),
                                              slab[0][0], signed, p.compute.cuda_stream), "tem_u16_lut_u8")
                measure.add(dst.data_ptr(), d, d)
                p.put(k)
        measure.report(p.st)
    return out


def predict_cube(volume, start, size, model, meanstd_x, meanstd_y, fetch_input=False, outdimsize=None, buffer=None,
                 rank=0, world_size=1, tile_batch=None, boundary="zeros", ensemble=None, mips=None, lut=None,
                 histogram=False, stats=None, clahe=None, warp=None, compare=None, repair=None, spread=None,
                 spread_gain=8.0):
    """Predict the subvolume [start, start+size) (x,y,z order as in the reference) of a uint8
    array `volume` indexed [z, y, x].  Voxels outside the array read as 0 (the reference fetches
    them from the store) or, with boundary="reflect" / "edge", the voxel that `fold` names on every axis: the result
    is that of the same call on numpy.pad(volume, P, mode=boundary) for any P the tiles stay within, without the padded
    copy.  Returns uint8 (zsize, ysize, xsize) [and the input block: the ROI of that padded volume].

    Device-side pipeline (utils.py:77-126 without the per-tile host round trips): the uint8 volume is uploaded
    once; one gather kernel cuts a batch of haloed tiles straight out of it (uint8 -> float, scaled and
    standardized, tem_u8_tiles_to_f32_std); the generator runs the batch as ONE launch sequence (batch = tile
    count: the small inner layers then fill the chip); one scatter kernel un-standardizes, rounds and writes
    every tile's interior into the uint8 output volume (tem_f32_tiles_unstd_to_u8).  Tile geometry, halo and
    the "multiple of 6" quirk are the reference's (tile_plan).

    `tile_batch` tiles run per launch sequence (default_tile_batch when None).  A request above stable_tile_batch(edge,
    is3d) is lowered to it, not refused: past it a layer's views outgrow a tiled kernel's 32-bit span, a full batch
    would run another kernel than the remainder batch, and the result would depend on the batch.  For every
    `tile_batch` the result is therefore bit-identical to tile_batch=1.

    A 2-D model (generator_g.is3d False) predicts every section of [start[2], start[2] + size[2]) on its own
    (tile_plan_2d) through the 2-D tile kernels; it also takes one image `volume` [y, x] with 2-element (x, y) `start`
    and `size`, and then returns [y, x] arrays.

    ensemble=None runs the generator once per tile.  ensemble="flips" | "all" | a sequence of symmetries (see
    `symmetries`; a 2-D model takes 2-axis members, or 3-axis ones that leave z alone) averages it over those
    orientations, per tile batch and on the device: for each member s in order the tiles are gathered as T_s(tile)
    (tem_u8_tiles*_to_f32_std_sym), the generator runs, and T_s^-1 of its output is accumulated in fp32
    (tem_f32_tiles*_sym_accum: the first member writes, the others add, the last also divides by the member count);
    the mean goes through the scatter kernel once.  No member is quantised before the mean and no copy of the volume
    is made.  ValueError, before any GPU work: an empty sequence, a perm that is no permutation, flips of another
    length, a member given twice, a member that moves z with a 2-D model.

    mips=None (or 0) returns the array above.  mips=L >= 1 returns the list [level0, ..., levelL] of a mip pyramid of
    it, built on the device: level 0 is that array, the same bytes, and level l + 1 is level l pooled by (2, 2, 2) over
    (z, y, x) -- (1, 2, 2) with a 2-D model, whose sections are not pooled -- to the shapes of `mip_shapes`.  A voxel is
    the mean of its children that exist in the level below (1, 2, 4 or 8 of them: fewer at the far face of an odd
    extent), rounded half up in integers, (sum + (cnt >> 1)) >> log2(cnt); levels cascade, and voxels past `size`
    never enter a mean (tem_u8_pool2, one launch per level after the tile loop -- and after the all-reduce of a
    multi-rank call).  The pyramid is relative to `start`: level-l voxel q covers ROI voxels [q 2^l, (q + 1) 2^l) on
    each pooled axis; choose `start` as a multiple of 2^L where it has to sit on a global grid.  L is at most
    max_mips(outdimsize) of the tile plan's outdimsize -- 5 for the 132 model (96), 2 for the 74 model (36), 1 for the
    260 model (222) -- so that predict_volume's chunks can pool on their own; a larger, negative or non-integer `mips`
    raises ValueError before any GPU work.  With fetch_input the result is (input block, list).

    lut=None reads the volume as it is.  lut = a np.uint8 table [256], or [Z, 256] with one row per section of the
    volume (match_lut builds either from histograms), remaps the intensities first: the result is, bit for bit, that of
    the same call on lut[volume] (lut[z][volume[z]]) for every boundary, ensemble, mips and tile_batch, without a
    remapped copy -- one tem_u8_lut launch runs in place on the uploaded bytes ahead of the first gather.  Only voxels
    of the volume are remapped: a voxel outside it still reads 0 under "zeros", not lut[0], and under the mirrored modes
    the remapped voxel it folds to.  fetch_input returns what the network saw, the remapped bytes.  A table of another
    dtype or shape raises ValueError before any GPU work.

    clahe=None reads the volume as it is.  clahe = a ClaheTables (clahe_fit of this volume: np.uint8 tables
    [Z, gy, gx, 256] and their tile; Z*gy*gx*256 bytes, uploaded once per call) equalises it first: one tem_u8_clahe
    launch runs in place on the uploaded bytes ahead of the first gather -- and ahead of `lut`, which then remaps the
    equalised bytes -- and the result is, bit for bit, that of the same call on clahe_volume(volume, clahe) for every
    boundary, ensemble, mips, tile_batch and lut.  As with `lut`, a voxel outside the volume still reads 0 under "zeros"
    and the equalised voxel it folds to under the mirrored modes, and fetch_input returns what the network saw.  Tables
    of another dtype or shape, a tile outside [1, 2048] and a non-uint8 volume raise ValueError before any GPU work.

    histogram=True puts the 256-bin histogram of the level-0 prediction into stats["histogram"] (np.int64[256]; `stats`
    must then be a dict): the voxels of the returned array and no others -- nothing past `size`, nothing from the
    rounded-up tile margin -- counted on the device by one tem_u8_hist launch over the cropped box of the result,
    after the all-reduce of a multi-rank call.  meanstd_from_histogram turns it into the unit of meanstd_y.

    compare=None compares nothing.  compare = gt, a uint8 array-like of the volume's own shape and in the volume's
    frame (the ground truth of the prediction), puts the joint histogram of (gt, level-0 prediction) into
    stats["joint_histogram"] (np.int64[256, 256], J[u, v] with u = ground truth, v = prediction; `stats` must then be
    a dict): compare_from_joint turns it into RMSE, MAE, PSNR, correlation and mutual information, regression_lut into
    the paired intensity map.  It is counted over the ROI voxels that lie inside the volume -- a voxel the ROI reaches
    outside the volume has no ground truth and is not compared, under every `boundary` -- by one tem_u8_hist2 launch on
    the cropped result against gt's ROI-within-the-volume box, uploaded once; after the all-reduce of a multi-rank
    call.  Anything else raises ValueError before any GPU work.

    repair=None reads the volume as it is and runs the launches above.  repair = a Repair (bad sections, a bad-voxel
    mask of the volume's shape, a missing grey level; max_gap) fills the volume's bad voxels along z first, each from
    the nearest good voxels of its column at most max_gap sections below and above (the rule is Repair's): one
    tem_u8_repair_z launch over the whole uploaded volume, in place, ahead of `clahe` and `lut`, with the mask uploaded
    next to it.  The result is, bit for bit, that of the same call on volume_repair(volume, repair), for 3-D and 2-D
    models and every boundary, ensemble, mips, lut, clahe, compare, spread, tile_batch and rank split.  Repair belongs
    to the volume, not to its padding: a voxel outside the volume reads the repaired voxel it folds to under the
    mirrored modes, and 0 under "zeros", which is not "missing" -- the same rule as `lut`.  fetch_input returns what the
    network saw, the repaired bytes.  _check_repair's ValueErrors (no source, max_gap outside 1...32, a section outside
    the volume, a mask of another shape or dtype, a missing_value outside 0...255, a single image, which has no z) come
    before any GPU work.

    spread=None measures nothing and runs the launches above.  spread = S, a writable np.uint8 ndarray of the result's
    shape -- (size[2], size[1], size[0]), or (size[1], size[0]) for one image -- needs an `ensemble` and receives how
    much its members disagree at every voxel, the test-time-augmentation uncertainty of the translation where there is
    no ground truth: the population standard deviation of the members' fp32 outputs (after T_s^-1, before any
    rounding to uint8) in grey levels of the output, times `spread_gain`, rounded and saturated at 255.  The default
    gain of 8 resolves 1/8 grey level and saturates from 31.9 grey levels on.  The accumulate that folds a member into
    the mean folds it, in the same launch, into two fp32 moments about the first member (tem_f32_tiles*_sym_accum_spread;
    the shift keeps fp32 sufficient) in three more batch-sized buffers, and tem_f32_tiles*_spread_to_u8 finishes them
    into a second device block behind the prediction's scatter: no further generator run, and every operation is one
    rounded fp32 operation in a fixed order, so numpy float32 reproduces the map bit for bit (include/tem_hip.h) and it
    stays within 1 of the float64 np.std form.  The prediction is bit-identical to the same call without `spread`; the
    return values stay as they are; `mips` pools the prediction only (the map has one level); a one-member ensemble
    gives an all-zero map.  When `stats` is a dict, stats["spread_histogram"] receives the map's np.int64[256]
    histogram over the ROI's voxels, counted on the device as `histogram` counts the prediction.  `spread` without
    `ensemble`, another shape or dtype, a read-only array and a `spread_gain` that is not a finite number above 0 raise
    ValueError before any GPU work.

    warp=None reads the volume as it is and runs the launches above.  warp = a Warp (per-section maps, optionally
    displacement fields on a lattice, a fill) aligns the sections first: the uploaded volume is resampled once into a
    second device buffer of its shape (tem_u8_warp_box over whole sections, in runs of sections that stay within a
    launch's workgroups; the raw buffer is then dropped), ahead of `repair`, `clahe` and `lut`, and the result is, bit
    for bit, that of the same call on A = volume_warp_field(volume, maps, fields, spacing, fill=fill) (volume_warp
    without fields), for 3-D and 2-D models, one image, and every boundary, ensemble, mips, lut, clahe, compare, repair,
    spread, tile_batch and rank split.  A has the volume's shape, so `start`, `size` and the boundary's folding are
    unchanged.  Frames, one rule: what has the volume's shape and is an input -- `volume`, and a Repair's `mask` --
    lives in the raw frame and goes through the warp (the mask with nearest=True and fill 0, as volume_warp_field(mask,
    ..., nearest=True) moves it); what is indexed by section or belongs to the result -- Repair.sections, the rows of
    a [Z, 256] `lut`, ClaheTables, `compare`'s ground truth, `spread` and the return values -- lives in the aligned
    frame.  Order on the device: warp, repair, clahe, lut, gather.  fetch_input returns what the network saw.
    _check_warp's ValueErrors (maps or fields of a wrong shape or dtype or outside volume_warp's and
    volume_warp_field's limits, fields without a spacing, a fill outside 0...255, a volume that is not uint8) come
    before any GPU work."""
    gen = getattr(model, "generator_g", None)
    is3d = getattr(gen, "is3d", True)
    syms = _check_ensemble(ensemble, is3d)
    gain = _check_spread(spread, spread_gain, syms, size, ndarray=True)
    lut = _check_lut(lut, np.shape(volume))
    if clahe is not None:
        _check_u8(volume)
    cl = _check_clahe(clahe, np.shape(volume))
    if repair is not None:
        _check_u8(volume)
    rp = _check_repair(repair, np.shape(volume))
    if warp is not None:
        _check_u8(volume)
    wp = _check_warp(warp, np.shape(volume))
    histogram = _check_histogram(histogram, stats)
    compare = _check_compare(compare, np.shape(volume), stats)
    if outdimsize is None:
        outdimsize = model.outdimsize
    if buffer is None:
        buffer = model.buffer
    L = _check_mips(mips, _plan_outdimsize(outdimsize))
    lib = H.require_gpu()
    if _single_image(model, start, size):
        res = predict_cube(np.asarray(volume)[None], tuple(start) + (0,), tuple(size) + (1,), model, meanstd_x,
                           meanstd_y, fetch_input=fetch_input, outdimsize=outdimsize, buffer=buffer, rank=rank,
                           world_size=world_size, tile_batch=tile_batch, boundary=boundary, ensemble=ensemble,
                           mips=mips, lut=lut, histogram=histogram, stats=stats, clahe=clahe,
                           compare=None if compare is None else np.asarray(compare)[None], repair=repair,
                           spread=None if spread is None else spread[None], spread_gain=spread_gain, warp=wp)
        one = lambda r: [v[0] for v in r] if isinstance(r, list) else r[0]
        return tuple(one(r) for r in res) if fetch_input else one(res)
    outdimsize, buffer, tpad, rois, index = _tile_plan(start, size, outdimsize, buffer, is3d)
    edge = outdimsize + buffer * 2
    z, y, x = size[2], size[1], size[0]
    rnd = lambda v: v + ((outdimsize - (v % outdimsize)) if (v % outdimsize) != 0 else 0)
    dev = model.device
    vol_host = np.ascontiguousarray(volume, dtype=np.uint8)
    _check_boundary(boundary, vol_host.shape)
    vol = torch.from_numpy(vol_host).to(dev, non_blocking=True)          # ONE upload of the whole volume
    Z, Y, X = vol_host.shape
    stream = H.current_stream()
    whole = ((0, Y), (0, X))
    if wp is not None:                                                   # first of all: the aligned volume, A, once
        warper = _Warper(lib, wp, dev, stream, (Z, Y, X))
        raw, vol = vol, torch.empty_like(vol)
        warper.box(raw.data_ptr(), vol.data_ptr(), (0, Z), whole, whole)
        del raw
    prepare = _Prepare(lib, cl, lut, dev, stream, repair=rp)
    if rp is not None:                                                   # then: one launch, the core is the whole volume
        mask_dev = None if rp.mask is None else torch.from_numpy(np.ascontiguousarray(rp.mask, dtype=np.uint8)).to(dev)
        if wp is not None and mask_dev is not None:                      # the mask lives in the raw frame: nearest, fill 0
            raw, mask_dev = mask_dev, torch.empty_like(mask_dev)
            warper.box(raw.data_ptr(), mask_dev.data_ptr(), (0, Z), whole, whole, nearest=True, fill=0)
            del raw
        prepare.repair_block(vol.data_ptr(), (Z, Y, X), 0, 0, Z, None if mask_dev is None else mask_dev.data_ptr())
    prepare.apply(vol.data_ptr(), (Z, Y, X), (0, 0, 0))                  # in place, once, behind the upload
    out_buffer = torch.zeros((rnd(z) if is3d else z, rnd(y), rnd(x)), dtype=torch.uint8, device=dev)
    OZ, OY, OX = out_buffer.shape
    mine = list(range(rank, len(rois), world_size))
    nb = _effective_batch(tile_batch, edge, is3d, len(mine) or 1)
    org = torch.tensor([rois[i][::-1] for i in mine], dtype=torch.int32).to(dev)       # this rank's (z, y, x), once
    idx = torch.tensor([index[i][::-1] for i in mine], dtype=torch.int32).to(dev)
    spread_buffer = None if gain is None else torch.zeros_like(out_buffer)
    runner = _TileRunner(lib, model, is3d, edge, tpad, outdimsize, boundary, syms, meanstd_x, meanstd_y, (Z, Y, X),
                         stream, gain)
    runner.run(vol.data_ptr(), (Z, Y, X), (0, 0, 0), org.data_ptr(), idx.data_ptr(), len(mine), nb,
               out_buffer.data_ptr(), (OZ, OY, OX), spread_dst=None if gain is None else spread_buffer.data_ptr())
    if world_size > 1 and torch.distributed.is_initialized():
        torch.distributed.all_reduce(out_buffer, op=torch.distributed.ReduceOp.MAX)   # disjoint tiles, zeros elsewhere
        if gain is not None:
            torch.distributed.all_reduce(spread_buffer, op=torch.distributed.ReduceOp.MAX)
    out = out_buffer[0:size[2], 0:size[1], 0:size[0]].cpu().numpy()
    measure, gt = _Measure(lib, histogram, compare is not None, dev, stream,
                           spread=gain is not None and isinstance(stats, dict)), None
    if gain is not None:
        measure.add_spread(spread_buffer.data_ptr(), (OZ, OY, OX), (size[2], size[1], size[0]))
        crop = spread_buffer[0:size[2], 0:size[1], 0:size[0]]
        try:
            torch.from_numpy(spread).copy_(crop)                             # the one download, straight into S
        except ValueError:                                                   # a view with a negative stride
            spread[...] = crop.cpu().numpy()
    box = None if compare is None else _inside((0, 0, 0), (size[2], size[1], size[0]), (start[2], start[1], start[0]),
                                               (Z, Y, X))
    if box is not None:                         # the ground truth where the ROI lies inside the volume, uploaded once
        (z0, z1), (y0, y1), (x0, x1) = box
        gt_dev = torch.from_numpy(np.ascontiguousarray(compare[z0:z1, y0:y1, x0:x1], dtype=np.uint8)).to(dev)
        gt = (gt_dev.data_ptr(), tuple(gt_dev.shape), (z0 - start[2], y0 - start[1], x0 - start[0]))
    measure.add(out_buffer.data_ptr(), (OZ, OY, OX), (size[2], size[1], size[0]), gt)   # the cropped box: `out`'s voxels
    measure.report(stats)
    if L:                                       # the pyramid of the resident result: one launch per level
        fz = 2 if is3d else 1
        shapes = mip_shapes(size, L, is3d)
        bufs, dims = [], (OZ, OY, OX)
        for _ in range(L):
            dims = (-(-dims[0] // fz), -(-dims[1] // 2), -(-dims[2] // 2))
            bufs.append(torch.empty(dims, dtype=torch.uint8, device=dev))
        _pool_levels(lib, out_buffer.data_ptr(), (OZ, OY, OX), shapes[0], L, is3d, [b.data_ptr() for b in bufs], stream)
        out = [out] + [b[:s[0], :s[1], :s[2]].cpu().numpy() for b, s in zip(bufs, shapes[1:])]
    if fetch_input:
        # the reference returns the RAW uint8 block here after a detour (utils.py:122-125: the standardized float
        # tile is un-standardized, rescaled and truncated into a uint8 buffer -- the original bytes up to float
        # rounding); the bytes themselves are returned instead
        if cl is not None or rp is not None or wp is not None:     # ... as the network saw them: the bytes the kernels left
            vol_host = vol.cpu().numpy()
        elif lut is not None:                    # ... remapped
            vol_host = _lut_host(vol_host, lut)
        if boundary != "zeros":                  # what the network saw: the ROI of the folded volume
            fz, fy, fx = (fold(np.arange(start[d], start[d] + size[d]), n, boundary) for d, n in ((2, Z), (1, Y), (0, X)))
            return vol_host[np.ix_(fz, fy, fx)], out
        inp = np.zeros((size[2], size[1], size[0]), np.uint8)
        z0, y0, x0 = max(start[2], 0), max(start[1], 0), max(start[0], 0)
        z1, y1, x1 = min(start[2] + size[2], Z), min(start[1] + size[1], Y), min(start[0] + size[0], X)
        inp[z0 - start[2]:z1 - start[2], y0 - start[1]:y1 - start[1], x0 - start[0]:x1 - start[0]] = \
            vol_host[z0:z1, y0:y1, x0:x1]
        return inp, out
    return out


class VolumeChunk(NamedTuple):
    """One box of whole tiles of a streamed prediction (chunk_plan).  Boxes are (z, y, x) (lo, hi) pairs."""
    tiles: tuple         # indices into tile_plan's rois / index
    origins: tuple       # per tile: (z, y, x) haloed-tile origin relative to read[*][0] (may be negative)
    offsets: tuple       # per tile: (z, y, x) of its interior in the chunk's output block
    read: tuple          # footprint in volume coordinates: union of the tiles' haloed boxes, clipped to the volume
    block: tuple         # footprint shape (a side is 0 when the chunk lies wholly outside the volume)
    base: tuple          # (z, y, x) of the output block's origin in `out` (before clipping)
    dims: tuple          # output block shape on the device: whole tiles
    out_box: tuple       # the part of the output block that lands in `out`: dims clipped to size


def _default_chunk_tiles(grid, cap):
    """(kz, ky, kx) with kz*ky*kx <= cap and fewest chunks over `grid`; ties go to the most cube-like box (least halo
    read per tile), then to more tiles per chunk."""
    best, key = (1, 1, 1), None
    for kz in range(1, min(grid[0], cap) + 1):
        for ky in range(1, min(grid[1], cap // kz) + 1):
            for kx in range(1, min(grid[2], cap // (kz * ky)) + 1):
                n = -(-grid[0] // kz) * -(-grid[1] // ky) * -(-grid[2] // kx)
                k = (n, max(kz, ky, kx), -kz * ky * kx)
                if key is None or k < key:
                    best, key = (kz, ky, kx), k
    return best


def _default_chunk_tiles_2d(grid, cap, od, halo):
    """(kz, ky, kx) sections x tiles with kz*ky*kx <= cap over `grid`.  Every distinct chunk tile count is a generator
    plan of its own (built per call once there are more than MAX_PLANS), so among the boxes within 1.5x of the fewest
    chunks the one with the fewest distinct tile counts wins; ties go to fewer chunks, then to the least footprint read
    per tile (the in-plane halo; there is none along z), then to more tiles per chunk."""
    ext = lambda g, k: {k} | ({g % k} if g % k else set())       # chunk extents along an axis: full, tail
    cands = []
    for kz in range(1, min(grid[0], cap) + 1):
        for ky in range(1, min(grid[1], cap // kz) + 1):
            for kx in range(1, min(grid[2], cap // (kz * ky)) + 1):
                n = -(-grid[0] // kz) * -(-grid[1] // ky) * -(-grid[2] // kx)
                cands.append((n, kz, ky, kx))
    if not cands:
        return 1, 1, 1
    n_min = min(c[0] for c in cands)
    best, key = (1, 1, 1), None
    for n, kz, ky, kx in cands:
        if n > 1.5 * n_min:
            continue
        shapes = len({a * b * c for a in ext(grid[0], kz) for b in ext(grid[1], ky) for c in ext(grid[2], kx)})
        k = (shapes, n, (ky * od + 2 * halo) * (kx * od + 2 * halo) / (ky * kx), -kz * ky * kx)
        if key is None or k < key:
            best, key = (kz, ky, kx), k
    return best


def _fold_hull(lo, hi, n, boundary):
    """[min, max + 1) of fold(i, n, boundary) over i in [lo, hi)."""
    if 0 <= lo and hi <= n:
        return lo, hi
    f = fold(np.arange(lo, hi), n, boundary)
    return int(f.min()), int(f.max()) + 1


def _chunk_plan(start, size, outdimsize, buffer, vol_shape, chunk_tiles, rank=0, world_size=1, is3d=True,
                boundary="zeros"):
    _check_boundary(boundary, vol_shape)
    outdimsize, buffer, tpad, rois, index = _tile_plan(start, size, outdimsize, buffer, is3d)
    od, edge = outdimsize, outdimsize + 2 * buffer
    # (z, y, x) extent of one tile's output (`step`) and haloed input (`ext`): a 2-D tile is one section thick
    step, ext = ((od, od, od), (edge, edge, edge)) if is3d else ((1, od, od), (1, edge, edge))
    size_zyx = (size[2], size[1], size[0])
    grid = tuple(len(range(0, n, s)) for n, s in zip(size_zyx, step))
    if chunk_tiles is None:
        chunk_tiles = (_default_chunk_tiles(grid, TILE_BATCH) if is3d else
                       _default_chunk_tiles_2d(grid, default_tile_batch(edge, False), od, buffer))
    kz, ky, kx = (int(v) for v in chunk_tiles)
    if min(kz, ky, kx) < 1:
        raise ValueError(f"chunk_tiles must be positive, got {chunk_tiles}")
    at = {(iz // step[0], iy // step[1], ix // step[2]): i for i, (ix, iy, iz) in enumerate(index)}   # grid cell -> tile
    chunks = []
    for gz in range(0, grid[0], kz):            # z-major: consecutive chunks read neighbouring slabs of the volume
        for gy in range(0, grid[1], ky):
            for gx in range(0, grid[2], kx):
                cells = [(a, b, c) for c in range(gx, min(gx + kx, grid[2])) for b in range(gy, min(gy + ky, grid[1]))
                         for a in range(gz, min(gz + kz, grid[0]))]
                tiles = tuple(sorted(at[c] for c in cells))            # tile_plan order
                org = [(rois[i][2], rois[i][1], rois[i][0]) for i in tiles]
                span = tuple((min(o[d] for o in org), max(o[d] for o in org) + ext[d]) for d in range(3))   # halo union
                if boundary == "zeros":
                    read = tuple((min(max(lo, 0), vol_shape[d]), max(min(hi, vol_shape[d]), 0))
                                 for d, (lo, hi) in enumerate(span))
                    read = tuple((lo, max(lo, hi)) for lo, hi in read)
                else:                       # mirrored coordinates leave the clipped union: the hull of where they land
                    read = tuple(_fold_hull(lo, hi, vol_shape[d], boundary) for d, (lo, hi) in enumerate(span))
                base = (gz * step[0], gy * step[1], gx * step[2])
                dims = tuple(k * s for k, s in zip((min(kz, grid[0] - gz), min(ky, grid[1] - gy), min(kx, grid[2] - gx)),
                                                   step))
                chunks.append(VolumeChunk(
                    tiles=tiles,
                    origins=tuple(tuple(o[d] - read[d][0] for d in range(3)) for o in org),
                    offsets=tuple((index[i][2] - base[0], index[i][1] - base[1], index[i][0] - base[2]) for i in tiles),
                    read=read, block=tuple(hi - lo for lo, hi in read), base=base, dims=dims,
                    out_box=tuple((base[d], min(base[d] + dims[d], size_zyx[d])) for d in range(3))))
    # same tile count => same generator batch: grouping them keeps the plan cache (MAX_PLANS) from rebuilding a plan
    # per chunk when the faces of the ROI leave tails along several axes
    chunks.sort(key=lambda c: -len(c.tiles))
    return outdimsize, buffer, tpad, chunks[rank::world_size]


def chunk_plan(start, size, outdimsize, buffer, vol_shape, chunk_tiles, rank=0, world_size=1, is3d=True,
               boundary="zeros"):
    """Group the tiles of tile_plan(start, size, outdimsize, buffer) into boxes of chunk_tiles = (kz, ky, kx) whole
    tiles (fewer at the ROI's far faces) over a volume of shape vol_shape = (Z, Y, X).  Chunks go round-robin to the
    ranks.  Returns this rank's list of VolumeChunk; chunk_tiles=None picks the box predict_volume uses by default
    (at most TILE_BATCH tiles, fewest chunks).

    The staging block of a chunk is exactly footprint = (union of its tiles' haloed boxes) n volume, and every tile
    voxel lies in that union.  So a tile voxel falls outside the block if and only if it falls outside the volume,
    and the resident-volume gather (tem_u8_tiles_to_f32_std) given the block, its dims and block-relative origins
    reads the same bytes as on the whole volume, zeros outside included.

    is3d=False groups tile_plan_2d's tiles instead: a chunk is a run of kz sections x (ky x kx) in-plane tiles, its
    footprint is haloed in y and x only (its z extent is exactly its sections, clipped to the volume), and
    chunk_tiles=None picks at most default_tile_batch(edge, False) tiles, fewest chunks, least halo read per tile.

    boundary="reflect" / "edge" (see `fold`): a voxel outside the volume reads a voxel inside it, which may lie outside
    the clipped union (a tile past the far face of a thin volume mirrors back beyond its own near side), so the rule
    above no longer holds.  A chunk's `read` is then, per axis, the hull [min, max + 1) of fold(i, n) over the union
    of its tiles' haloed extents: every folded coordinate lies in it, both ends are attained, and it is never empty.
    `origins` stay relative to read[*][0]; the `_bc` gather kernels get the block, read[*][0] and vol_shape, and fold
    l + origin + p themselves."""
    return _chunk_plan(start, size, outdimsize, buffer, tuple(int(v) for v in vol_shape), chunk_tiles, rank,
                       world_size, is3d, boundary)[3]


def predict_volume(volume, start, size, model, meanstd_x, meanstd_y, out=None, chunk_tiles=None, tile_batch=None,
                   outdimsize=None, buffer=None, rank=0, world_size=1, stats=None, boundary="zeros", ensemble=None,
                   mips=None, lut=None, histogram=False, clahe=None, warp=None, compare=None, repair=None,
                   spread=None, spread_gain=8.0):
    """Out-of-core predict_cube: the subvolume [start, start+size) (x,y,z order) of a uint8 array-like `volume`
    indexed [z, y, x] (ndarray, np.memmap, h5py / zarr dataset: `.shape` and basic slicing are all it needs) is
    predicted chunk by chunk (chunk_plan) into `out`, a writable uint8 array-like of shape (size[2], size[1], size[0])
    (allocated when None) that is returned.  Only the chunks' footprints are ever read from `volume`; device memory
    is bounded by the chunk, not by the ROI.  The result equals predict_cube's bit for bit, for every `boundary`
    ("zeros", "reflect", "edge": what a voxel outside the volume reads, see predict_cube; the mirrored modes read
    each chunk's footprint hull, chunk_plan).

    Pipeline per chunk: one host thread reads the footprint into a pinned staging buffer -> H2D on a copy stream ->
    gather + generator plan + scatter on the compute stream (the plan's buffers are reused run to run, so these stay
    in order on one stream) -> D2H on a second copy stream into a pinned output buffer -> the host thread writes the
    chunk's interior into `out`.  Staging is double-buffered (pinned and device, input and output), so the reads,
    copies and writes of neighbouring chunks run while the GPU computes.  Ranks (rank / world_size) take chunks
    round-robin and write disjoint boxes of a shared `out`; no collective is used.  `tile_batch` is predict_cube's: a
    chunk runs in batches of at most that many tiles, lowered to stable_tile_batch(edge, is3d) where it is larger.
    `stats` (a dict) receives the host thread's read and write seconds, the number of chunks and the tile batch used
    (`tile_batch`).

    A 2-D model streams chunks of chunk_plan(..., is3d=False) through the same pipeline with the 2-D tile kernels;
    it also takes one image `volume` [y, x] with 2-element (x, y) `start` / `size` (`out` is then [y, x]).

    `ensemble` is predict_cube's: every tile batch runs once per member between its gathers and its one scatter, with
    one fp32 accumulator of a batch's output for the whole call; a chunk's staging buffer is released for the next
    upload after the last member's gather of its last batch.  The rest of the pipeline, the chunk plan and the
    footprints are those of ensemble=None, and the result still equals predict_cube's bit for bit.

    `mips` is predict_cube's: mips=L >= 1 writes and returns the list of the L + 1 levels of the result's mip pyramid,
    equal to predict_cube's at every level.  `out` is then None (every level is allocated) or a sequence of L + 1
    writable uint8 array-likes of exactly mip_shapes(size, L, is3d) (memmap, h5py, zarr as for one array); anything else
    raises ValueError, as a `mips` beyond max_mips does, before any GPU work.  A chunk is a box of whole tiles whose
    origin and extents are multiples of 2^L on the pooled axes, so it pools on its own: after its last scatter the
    compute stream runs L launches of tem_u8_pool2 (level l + 1 from level l, valid extents = the chunk's `out_box`, so
    predictions past `size` never enter a mean) into the same device buffer, which holds the chunk's levels back to
    back; the one D2H copy moves them all and the host thread writes each level's box (`mip_box`).  The device and
    pinned output buffers grow by at most 1/7 (1/3 for a 2-D model); nothing else changes, and `boundary` and
    `ensemble` compose as they are (pooling comes after the scatter).  `stats["mips"]` reports L.

    `lut` is predict_cube's ([256], or [Z, 256] indexed by the volume's own section): each chunk's footprint is remapped
    in place on the device by one tem_u8_lut launch on the compute stream, behind the wait for the chunk's H2D and ahead
    of its first gather, with the footprint's first section as the table's row offset.  The one zero byte that stands in
    for a chunk wholly outside the volume is not remapped, so voxels outside the volume read 0 as before; under the
    mirrored modes the footprint hull holds real sections, remapped by their own rows.  The result equals
    predict_cube(lut=...)'s, i.e. that of the same call on the remapped volume, which is never made.

    `clahe` is predict_cube's (a ClaheTables of the whole volume; its Z*gy*gx*256 bytes are uploaded once per call, not
    per chunk): each chunk's footprint is equalised in place by one tem_u8_clahe launch on the compute stream, behind
    the wait for the chunk's H2D and ahead of `lut` and the first gather, with the footprint's `read` origin as the
    launch's (zsec0, y_org, x_org) -- the tile grid belongs to the volume, so a voxel's value does not depend on the
    chunk it arrives in.  The stand-in zero byte of a chunk wholly outside the volume is not touched.  The result equals
    predict_cube(clahe=...)'s, i.e. that of the same call on the equalised volume, which is never made.

    histogram=True puts the 256-bin histogram of the level-0 result (np.int64[256]) into stats["histogram"]: one
    tem_u8_hist launch per chunk behind its last scatter, over the chunk's `out_box` extents of its device block, adding
    into one device accumulator that is read back once at the end -- no voxel is copied for it, and predictions past
    `size` are not counted.  In a multi-rank call each rank reports the histogram of its own chunks: the ranks'
    histograms add up to that of the whole result.

    `compare` is predict_cube's (gt: a uint8 array-like of the volume's shape, e.g. a memmap): stats["joint_histogram"]
    receives the np.int64[256, 256] joint histogram of (gt, level-0 result) over the ROI voxels inside the volume.  Per
    chunk the host thread also reads gt's box -- the chunk's `out_box` shifted by `start` and clipped to the volume --
    through a second double-buffered input stream, and one tem_u8_hist2 launch behind the chunk's last scatter (and its
    tem_u8_hist, with `histogram`) adds it into one device table that is read back once at the end; a chunk whose box
    misses the volume launches nothing.  The table does not depend on chunk_tiles or tile_batch; each rank reports its
    own chunks, and the ranks' tables add up to that of the whole result.

    `repair` is predict_cube's (a Repair of the whole volume; its mask may be a memmap): the chunk plan and its
    footprints stay as they are, but the host thread reads each footprint with max_gap more sections on each side of z,
    clipped to the volume -- and the mask's same box through a second input stream, as `compare` reads its ground truth
    -- and one tem_u8_repair_z launch, ahead of `clahe` and `lut`, fills the footprint's planes in place as the core of
    that block (the section flags are uploaded once per call).  Everything behind it, clahe, lut and every gather, is
    given the pointer to the footprint's first plane and sees the block it sees without `repair`.  A voxel's result
    needs only the sections [z - max_gap, z + max_gap] of its column, which the block holds, so it does not depend on
    the chunk it arrives in: the result equals predict_cube(repair=...)'s, i.e. that of the same call on
    volume_repair(volume, repair), which is never made.  A chunk with an empty footprint launches nothing, and nothing
    is counted: footprints overlap, so counts would mean nothing (volume_repair reports them).

    `spread` / `spread_gain` are predict_cube's: spread = S, a writable uint8 array-like of `out`'s level-0 shape
    (ndarray, memmap, h5py, zarr), receives the map of the ensemble members' disagreement, equal to predict_cube's bit
    for bit.  A chunk's device and pinned output block grows by one block of its `dims`, behind the pyramid levels if
    there are any; the runner scatters the map there behind the prediction, the one D2H copy carries it, and the host
    thread writes the chunk's `out_box` of S with the chunk's `out`.  stats["spread_histogram"] receives the map's
    np.int64[256] histogram: one more tem_u8_hist launch per chunk into one device accumulator, read back once; each rank
    reports its own chunks and the ranks' histograms add up.  One read thread, one output stream and no collective, as
    before.

    `warp` is predict_cube's (a Warp of the whole volume; its tables are uploaded once per call): the chunk plan and its
    footprints stay as they are, but a footprint is no longer read, it is produced on the device.  Per chunk the host
    thread reads the raw volume's box volume[rz0:rz1, sy0:sy1, sx0:sx1] -- the footprint's sections (with `repair`:
    and its max_gap sections on each side of z) over warp_source_box of the footprint, the rows and columns that hold
    every tap, cut in y and in x -- into the pinned double buffers; behind its H2D one tem_u8_warp_box launch on the
    compute stream writes the aligned footprint into one device buffer that is reused in stream order, and the upload
    buffer is released behind that launch.  A Repair's mask, which lives in the raw frame, is read likewise (the
    planner's box for nearest) through the second input stream and moved by a second launch with nearest = 1 and fill
    0.  repair_block, clahe, lut and every gather then get the footprint exactly as they get the uploaded one without
    `warp`.  A footprint none of whose sections has a source (warp_source_box: None) is filled with `fill` without
    reading the volume.  A voxel of A depends on its section's map and field alone, so the result does not depend on
    the chunk: it equals predict_cube(warp=...)'s, i.e. that of the same call on the aligned volume, which is never
    made.  `stats` gains `warp_read_voxels`, the voxels of the volume that were read, and `footprint_voxels`, the
    voxels of the footprints they produced: their ratio is the read amplification."""
    gen = model.generator_g
    is3d = getattr(gen, "is3d", True)
    syms = _check_ensemble(ensemble, is3d)
    gain = _check_spread(spread, spread_gain, syms, size)
    L = _check_mips(mips, _plan_outdimsize(model.outdimsize if outdimsize is None else outdimsize))
    if L and len(size) in (2, 3):
        out = _check_mip_outs(out, size, L, is3d)
    lut = _check_lut(lut, tuple(volume.shape))
    if clahe is not None:
        _check_u8(volume)
    cl = _check_clahe(clahe, tuple(volume.shape))
    if repair is not None:
        _check_u8(volume)
    rp = _check_repair(repair, tuple(volume.shape))
    if warp is not None:
        _check_u8(volume)
    wp = _check_warp(warp, tuple(volume.shape))
    histogram = _check_histogram(histogram, stats)
    compare = _check_compare(compare, tuple(volume.shape), stats)
    lib = H.require_gpu()
    if not hasattr(gen, "plan"):
        raise TypeError("predict_volume needs a generator with launch plans (EM2EM or a saved model)")
    if _single_image(model, start, size):
        if len(volume.shape) != 2:
            raise ValueError(f"a 2-element start / size needs one image [y, x], got shape {tuple(volume.shape)}")
        if out is None:
            out = ([np.zeros(s, np.uint8) for s in mip_shapes(size, L, False)] if L else
                   np.zeros((size[1], size[0]), np.uint8))
        predict_volume(_OneSection(volume), tuple(start) + (0,), tuple(size) + (1,), model, meanstd_x, meanstd_y,
                       out=[_OneSection(o) for o in out] if L else _OneSection(out), chunk_tiles=chunk_tiles,
                       tile_batch=tile_batch, outdimsize=outdimsize, buffer=buffer, rank=rank, world_size=world_size,
                       stats=stats, boundary=boundary, ensemble=ensemble, mips=mips, lut=lut, histogram=histogram,
                       clahe=clahe, compare=None if compare is None else _OneSection(compare), repair=repair,
                       spread=None if spread is None else _OneSection(spread), spread_gain=spread_gain, warp=wp)
        return out
    vol_shape = tuple(int(v) for v in volume.shape)
    if len(vol_shape) != 3:
        raise ValueError(f"volume must be 3-D [z, y, x], got shape {vol_shape}")
    od, buf, tpad, chunks = _chunk_plan(start, size, model.outdimsize if outdimsize is None else outdimsize,
                                        model.buffer if buffer is None else buffer, vol_shape, chunk_tiles, rank,
                                        world_size, is3d, boundary)
    edge = od + 2 * buf
    if L:
        if out is None:
            out = [np.zeros(s, np.uint8) for s in mip_shapes(size, L, is3d)]
    elif out is None:
        out = np.zeros((size[2], size[1], size[0]), np.uint8)
    elif tuple(out.shape) != (size[2], size[1], size[0]):
        raise ValueError(f"out has shape {tuple(out.shape)}, expected {(size[2], size[1], size[0])}")
    st = {"read_s": 0.0, "write_s": 0.0, "chunks": len(chunks), "mips": L}
    if wp is not None:
        st["warp_read_voxels"] = st["footprint_voxels"] = 0
    if histogram:
        st["histogram"] = np.zeros(256, np.int64)
    if compare is not None:
        st["joint_histogram"] = np.zeros((256, 256), np.int64)
    if gain is not None:
        st["spread_histogram"] = np.zeros(256, np.int64)
    if stats is not None:
        stats.update(st)
    if not chunks:
        return out
    # a chunk wholly outside the volume has an empty footprint: it gathers from one zero byte (all voxels read 0);
    # with a mirrored boundary no footprint is empty
    gdims = [c.block if min(c.block) > 0 else (1, 1, 1) for c in chunks]
    # with `repair` a footprint is read with max_gap more sections on each side of z, clipped to the volume: rz[k] is
    # that z range, and the footprint itself -- the repair's core, what everything downstream sees -- its planes
    # [c.read[0][0] - rz[k][0], ...) of the block that is read
    R = 0 if rp is None else rp.max_gap
    rz = [(max(c.read[0][0] - R, 0), min(c.read[0][1] + R, vol_shape[0])) if min(c.block) > 0 else (0, 1) for c in chunks]
    rdims = [(z1 - z0,) + tuple(g[1:]) for (z0, z1), g in zip(rz, gdims)]
    in_bytes = [int(np.prod(g)) for g in rdims]
    with_mask = rp is not None and rp.mask is not None
    if wp is not None:
        # with `warp` the block that is read is not the footprint (with its halo along z) but the box of the raw volume
        # that holds its taps: sbox[k], the rows and columns of the same sections, or None where no section has any
        foot, sbox, mbox = _warp_footprints(chunks, R, wp, vol_shape, with_mask)
        sbytes = lambda boxes: [1 if b is None else (z1 - z0) * (b[0][1] - b[0][0]) * (b[1][1] - b[1][0])
                                for b, (z0, z1) in zip(boxes, rz)]
        foot_bytes, in_bytes, mask_bytes = in_bytes, sbytes(sbox), sbytes(mbox)
        st["warp_read_voxels"] = sum(n for n, b in zip(in_bytes, sbox) if b is not None)
        st["footprint_voxels"] = sum(n for n, f in zip(foot_bytes, foot) if f is not None)
        if stats is not None:
            stats.update(st)
    # a chunk's output block on the device and in pinned memory: its L + 1 levels back to back, level l at
    # lvl_off[k][l] with the dense dims lvl_dims[k][l] = c.dims divided by 2^l on the pooled axes (exact: dims are
    # whole tiles and outdimsize % 2^L == 0)
    lvl_dims = [[tuple(v >> (l if (is3d or d) else 0) for d, v in enumerate(c.dims)) for l in range(L + 1)]
                for c in chunks]
    lvl_off = [np.cumsum([0] + [int(np.prod(d)) for d in dd]) for dd in lvl_dims]
    # ... and, with a spread, one more block of c.dims behind them: the map, at lvl_off[k][-1]
    out_bytes = [int(o[-1]) + (int(np.prod(c.dims)) if gain is not None else 0) for o, c in zip(lvl_off, chunks)]
    nb = st["tile_batch"] = _effective_batch(tile_batch, edge, is3d, max(len(c.tiles) for c in chunks))
    dev = model.device
    compute = torch.cuda.current_stream(dev)
    first = np.cumsum([0] + [len(c.tiles) for c in chunks])
    org = torch.tensor([o for c in chunks for o in c.origins], dtype=torch.int32).to(dev)     # every chunk's, once
    idx = torch.tensor([o for c in chunks for o in c.offsets], dtype=torch.int32).to(dev)
    prepare = _Prepare(lib, cl, lut, dev, compute.cuda_stream, repair=rp)
    measure = _Measure(lib, histogram, compare is not None, dev, compute.cuda_stream, spread=gain is not None)
    runner = _TileRunner(lib, model, is3d, edge, tpad, od, boundary, syms, meanstd_x, meanstd_y, vol_shape,
                         compute.cuda_stream, gain)
    if compare is not None:
        # the ground truth of chunk k: its out_box in the volume's frame, clipped to the volume (None: it misses it)
        gt_box = [_inside(tuple(b[0] for b in c.out_box), tuple(b[1] for b in c.out_box),
                          (start[2], start[1], start[0]), vol_shape) for c in chunks]
        gt_dims = [None if b is None else tuple(hi - lo for lo, hi in b) for b in gt_box]
        gt_bytes = [1 if d is None else int(np.prod(d)) for d in gt_dims]

    def read_gt(k, flat):               # host thread: the ground-truth box of chunk k (one unused byte where none)
        if gt_box[k] is not None:
            (z0, z1), (y0, y1), (x0, x1) = gt_box[k]
            flat.reshape(gt_dims[k])[...] = compare[z0:z1, y0:y1, x0:x1]

    def read_box(src):                  # host thread: footprint of chunk k (with `repair`: and its halo along z)
        def read_into(k, flat):
            c, dst = chunks[k], flat.reshape(rdims[k])
            if min(c.block) > 0:
                (z0, z1), (_, (y0, y1), (x0, x1)) = rz[k], c.read
                dst[...] = src[z0:z1, y0:y1, x0:x1]
            else:
                dst[...] = 0
        return read_into

    def read_source(src, boxes):        # host thread, with `warp`: the raw box that holds the footprint's taps
        def read_into(k, flat):
            if boxes[k] is not None:
                (z0, z1), ((y0, y1), (x0, x1)) = rz[k], boxes[k]
                flat.reshape(z1 - z0, y1 - y0, x1 - x0)[...] = src[z0:z1, y0:y1, x0:x1]
        return read_into

    read_into = read_box(volume) if wp is None else read_source(volume, sbox)
    if wp is not None:                  # the aligned footprints, on the device: one buffer each, reused in stream order
        warper = _Warper(lib, wp, dev, compute.cuda_stream, vol_shape)
        foot_dev = torch.zeros(max(foot_bytes), dtype=torch.uint8, device=dev)
        mask_foot = torch.zeros(max(foot_bytes), dtype=torch.uint8, device=dev) if with_mask else None

    def align(k, buf, into, boxes, nearest, fill):      # compute stream: the footprint of chunk k from its raw box
        if foot[k] is None:             # the stand-in zero byte of a chunk wholly outside the volume
            into[:1].zero_()
        elif boxes[k] is None:          # no section has a source: `fill`, nothing was read
            into[:foot_bytes[k]].fill_(fill)
        else:
            warper.box(buf.data_ptr(), into.data_ptr(), rz[k], boxes[k], foot[k][1:], nearest, fill)

    def write_from(k, buf):             # host thread: the chunk's box of `out` (and of `spread`)
        c = chunks[k]
        if gain is not None:
            (z0, z1), (y0, y1), (x0, x1) = c.out_box
            spread[z0:z1, y0:y1, x0:x1] = buf[lvl_off[k][-1]:].reshape(c.dims)[:z1 - z0, :y1 - y0, :x1 - x0]
        if not L:
            (z0, z1), (y0, y1), (x0, x1) = c.out_box
            out[z0:z1, y0:y1, x0:x1] = buf[:lvl_off[k][1]].reshape(c.dims)[:z1 - z0, :y1 - y0, :x1 - x0]
        for l in range(L + 1 if L else 0):      # with a pyramid: each level's box into its own array
            src = buf[lvl_off[k][l]:lvl_off[k][l + 1]].reshape(lvl_dims[k][l])
            ((z0, z1), (y0, y1), (x0, x1)), (nz, ny, nx) = mip_box(c, l, is3d)
            out[l][z0:z1, y0:y1, x0:x1] = src[:nz, :ny, :nx]

    pool = ThreadPoolExecutor(max_workers=1)     # one thread for reads and writes: write(k), read(k + 2)
    outp = _OutputStream(out_bytes, write_from, dev, pool, st, own_buffers=True)
    with _InputStream(in_bytes, read_into, dev, pool, st) as inp, \
            (contextlib.nullcontext() if compare is None else _InputStream(gt_bytes, read_gt, dev, pool, st)) as gt_inp, \
            (contextlib.nullcontext() if not with_mask else
             _InputStream(in_bytes, read_box(rp.mask), dev, pool, st) if wp is None else
             _InputStream(mask_bytes, read_source(rp.mask, mbox), dev, pool, st)) as mask_inp, \
            outp:
        for k, c in enumerate(chunks):
            in_buf, dst = inp.get(k), outp.device(k).data_ptr()
            src, lo = in_buf.data_ptr(), tuple(r[0] for r in c.read)
            if with_mask:
                mask_buf = mask_inp.get(k)
            last_gather = lambda: inp.release(k, compute.record_event())
            if wp is not None:                               # first of all: the aligned footprint, from the raw box
                align(k, in_buf, foot_dev, sbox, False, wp.fill)
                inp.release(k, compute.record_event())
                src, last_gather = foot_dev.data_ptr(), None
                if with_mask:
                    align(k, mask_buf, mask_foot, mbox, True, 0)
                    mask_inp.release(k, compute.record_event())
                    mask_buf = mask_foot
            if rp is not None and min(c.block) > 0:          # first: the footprint is the core of the block that was read
                c0 = lo[0] - rz[k][0]
                prepare.repair_block(src, (rdims[k][0],) + tuple(c.block[1:]), rz[k][0], c0, c0 + c.block[0],
                                     mask_buf.data_ptr() if with_mask else None)
                src += c0 * c.block[1] * c.block[2]          # ... and what everything behind it sees
            if with_mask and wp is None:
                mask_inp.release(k, compute.record_event())
            prepare.apply(src, c.block, lo)                  # the footprint; never the stand-in zero byte
            t = 12 * int(first[k])
            # the staging buffer is free for the next upload once the chunk's last gather is enqueued
            sdst = None if gain is None else dst + int(lvl_off[k][-1])
            runner.run(src, gdims[k], lo, org.data_ptr() + t, idx.data_ptr() + t, len(c.tiles), nb, dst, c.dims,
                       last_gather, sdst)
            valid = tuple(hi - lo_ for lo_, hi in c.out_box)     # the chunk's part of the result
            if L:                                            # its pyramid, level by level behind its scatters
                _pool_levels(lib, dst, c.dims, valid, L, is3d, [dst + int(o) for o in lvl_off[k][1:L + 1]],
                             compute.cuda_stream)
            gt = None
            if compare is not None:                          # ... against its ground truth, where there is one
                gt_buf = gt_inp.get(k)
                if gt_box[k] is not None:
                    at = tuple(b[0] - s0 - o for b, s0, o in zip(gt_box[k], (start[2], start[1], start[0]), c.base))
                    gt = (gt_buf.data_ptr(), gt_dims[k], at)
            measure.add(dst, c.dims, valid, gt)
            if gain is not None:
                measure.add_spread(sdst, c.dims, valid)
            scattered = compute.record_event()
            if compare is not None:
                gt_inp.release(k, scattered)
            outp.put(k, scattered)
            inp.prefetch(k + 2)
            if compare is not None:
                gt_inp.prefetch(k + 2)
            if with_mask:
                mask_inp.prefetch(k + 2)
    measure.report(st)                                       # the one read-back of each
    if stats is not None:
        stats.update(st)
    return out


def save_model(name, ckpt_dir, meanstd_x, meanstd_y, size=132, is3d=True):
    """Export generator_g for inference (utils.py:133-167): weights + meta.json with the
    reference's keys (buffer, outdimsize, meanstd_x, meanstd_y)."""
    from .cgan import EM2EM
    model = EM2EM(size, name, is3d=is3d, ckpt_restore=ckpt_dir)
    os.makedirs(name, exist_ok=True)
    torch.save({"theta": model.generator_g.params.theta.detach().cpu(), "dimsize": size, "is3d": is3d},
               os.path.join(name, "generator_g.pt"))
    meta = {
        "buffer": model.buffer,
        "outdimsize": model.outdimsize,
        "meanstd_x": [float(meanstd_x[0]), float(meanstd_x[1])],
        "meanstd_y": [float(meanstd_y[0]), float(meanstd_y[1])]
    }
    with open(os.path.join(name, "meta.json"), 'w') as fout:
        fout.write(json.dumps(meta))


class _SavedGenerator:
    def __init__(self, gen, meta):
        self.generator_g, self.outdimsize, self.buffer, self.device = gen, meta["outdimsize"], meta["buffer"], gen.device
        self.meta = meta

    def predict(self, data):
        return self.generator_g(data)


def _local_volume(location):
    if isinstance(location, (str, bytes, os.PathLike)):
        raise NotImplementedError("cloud volume stores (neuroglancer precomputed, utils.py:62-90) are out of scope: "
                                  "pass the uint8 volume as an array indexed [z, y, x]")
    return location


def predict_ng_cube(location, start, size, model, meanstd_x, meanstd_y, cloudrun=None, fetch_input=False,
                    outdimsize=None, buffer=None):
    """Reference signature (utils.py:41): `location` is the uint8 volume itself (array indexed [z, y, x])
    instead of a cloud path; `cloudrun` is accepted and ignored.  The signature is the reference's, so voxels outside
    the array always read 0 here: predict_cube(..., boundary="reflect" | "edge") mirrors or clamps at the faces.
    It takes no `mips` either: predict_cube(..., mips=L) returns the mip pyramid of the prediction; nor `lut`, `clahe`,
    `compare`, `repair`, `spread` or `warp`."""
    return predict_cube(_local_volume(location), start, size, model, meanstd_x, meanstd_y, fetch_input=fetch_input,
                        outdimsize=outdimsize, buffer=buffer)


def predict_cube_from_saved_model(location, start, size, cloudrun, model_dir, fetch_input=False):
    """Reference signature (utils.py:12-38) over a local array: `location` is the uint8 volume,
    `cloudrun` is accepted and ignored, `model_dir` is a directory written by save_model.  The signature is the
    reference's, so voxels outside the array always read 0 here: for boundary="reflect" | "edge" call predict_cube, or
    predict_volume_from_saved_model, which takes the keyword.  The same holds for `mips` (the mip pyramid of the
    prediction): this signature has none and returns the full-resolution array alone."""
    volume = _local_volume(location)
    model = _load_saved(model_dir)
    return predict_cube(volume, start, size, model, model.meta["meanstd_x"], model.meta["meanstd_y"],
                        fetch_input=fetch_input, outdimsize=model.outdimsize, buffer=model.buffer)


def predict_volume_from_saved_model(volume, start, size, model_dir, out=None, **kw):
    """predict_volume with the generator and statistics exported by save_model to `model_dir` (the out-of-core
    sibling of predict_cube_from_saved_model); `kw` are predict_volume's chunk_tiles, tile_batch, rank, world_size,
    stats, boundary ("zeros", "reflect" or "edge": what a voxel outside the volume reads), ensemble (None, "flips",
    "all" or a sequence of symmetries: the orientations the generator's output is averaged over), mips (None, or
    the number of pooled levels of the result's mip pyramid: `out` and the return value are then lists of levels),
    lut (None, or a uint8 table [256] or [Z, 256] the volume's intensities are remapped by on the device),
    histogram (True: stats["histogram"] receives the 256-bin histogram of the result), clahe (None, or the
    ClaheTables of the volume, clahe_fit: the volume is equalised on the device, ahead of lut) and compare (None, or
    the ground truth as a uint8 array-like of the volume's shape: stats["joint_histogram"] receives the 256 x 256
    joint histogram of (ground truth, result), see compare_from_joint), repair (None, or a Repair: the volume's bad
    sections and voxels are filled along z on the device, ahead of clahe and lut) and spread / spread_gain (None, or a
    writable uint8 array-like of the result's shape that receives the map of the ensemble members' disagreement, see
    predict_cube) and warp (None, or a Warp: the sections are aligned on the device, chunk by chunk from the raw box
    that holds a footprint's taps, ahead of repair, clahe and lut).
    The reference's signatures, predict_ng_cube and predict_cube_from_saved_model, take none of these keywords; they
    run unensembled and return the full-resolution array alone."""
    model = _load_saved(model_dir)
    return predict_volume(_local_volume(volume), start, size, model, model.meta["meanstd_x"], model.meta["meanstd_y"],
                          out=out, outdimsize=model.outdimsize, buffer=model.buffer, **kw)


def _load_saved(model_dir):
    from .models.generator import unet_generator
    meta = json.load(open(os.path.join(model_dir, 'meta.json')))
    blob = torch.load(os.path.join(model_dir, "generator_g.pt"), map_location="cpu", weights_only=True)
    gen, _ = unet_generator(blob["dimsize"], blob["is3d"])
    gen.params.theta.copy_(blob["theta"])
    return _SavedGenerator(gen, meta)
