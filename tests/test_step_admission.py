"""Every launch of every supported train step is admitted by the library (no GPU).

EM2EM names three sizes as compatible -- 74, 132 and 260 -- in 3-D and 2-D, fp32 and bf16.  A compiled step is a flat
list of launches whose argument structs are built, and whose geometry is put to the library's dry queries, before
anything runs; the queries never dereference a pointer.  So the launch list builds on host tensors once the three
places that ask for a device are stubbed (`dry_step`): hip_ops.require_gpu, torch.cuda.Stream / Event, and
torch.cuda.current_device.  Nothing writes the host tensors: a 260^3 step is address space, not memory.

For every configuration the test asks each convolution, transposed convolution and kernel gradient again, from the
finished argument struct (a kernel gradient with the slab count its launch will pass), and wants its success code and
a kernel symbol on every launch.  The 260 steps are also held to a recorded list: the launches whose symbol differs
from the 132 step's.  A kernel that changes route at 260 fails here until someone has looked at it."""
import contextlib
import ctypes as C
import os
import sys
from collections import Counter

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fullsize_cases import launch_struct  # noqa: E402


class _Stub:
    def __init__(self, *a, **k):
        pass


@contextlib.contextmanager
def dry_step(monkeypatch, dimsize, is3d, precision, batch=1):
    """The compiled step of EM2EM(dimsize, is3d, precision) at `batch`, built on host tensors."""
    from transfer_em_amd import _lib, cgan, hip_ops
    with monkeypatch.context() as m:
        m.setattr(hip_ops, "require_gpu", _lib.load)
        m.setattr(torch.cuda, "Stream", _Stub)
        m.setattr(torch.cuda, "Event", _Stub)
        m.setattr(torch.cuda, "current_device", lambda: 0)
        model = cgan.EM2EM(dimsize, "dry", is3d=is3d, precision=precision, device="cpu",
                           checkpoint_root=os.path.join(os.sep, "nonexistent"))
        yield cgan._CompiledStep(model, batch)


def _requery(lib, launch):
    """The dry query of one convolution / kernel-gradient launch, from its finished struct -> return code."""
    from transfer_em_amd import _lib
    a, fn = launch_struct(launch), launch.fn.__name__
    name = C.create_string_buffer(96)
    if isinstance(a, _lib.tem_bww_args):
        if fn == "tem_conv_bwd_weight_bf16":
            n = lib.tem_conv_bwd_weight_bf16_nslab(C.byref(a), name, 96)
        elif fn == "tem_conv_bwd_weight_winograd":
            n = lib.tem_conv_bwd_weight_winograd_nslab(C.byref(a), name, 96)
        else:
            assert fn == "tem_conv_bwd_weight", fn
            n = lib.tem_conv_bwd_weight_nslab(C.byref(a))
        # the launch checks the count it is given against the query's: asked with that count the query must repeat it
        return 0 if n == a.nslab else (n if n < 0 else -1000 - n)
    if fn == "tem_conv_bf16":
        return lib.tem_conv_bf16_describe(C.byref(a), name, 96)
    if fn == "tem_conv_transpose_bf16":
        return lib.tem_conv_transpose_bf16_describe(C.byref(a), name, 96)
    assert fn in ("tem_conv", "tem_conv_transpose", "tem_conv_direct", "tem_conv_transpose_direct"), fn
    rc = lib.tem_conv_is_tiled(C.byref(a), int("transpose" in fn), name, 96)
    return min(rc, 0)


def symbols(step):
    """{launch name: [kernel symbol of each launch of that name, in step order]} of the convolution / kernel-gradient
    launches (a layer's launches at the three call sites of its network share a name); every one is asked again."""
    from transfer_em_amd import _lib
    lib = _lib.load()
    out, bad = {}, []
    for l in step.compute + step.update:
        if launch_struct(l) is None:
            continue
        rc = _requery(lib, l)
        if rc < 0:
            bad.append((l.name, l.fn.__name__, rc))
        assert l.meta.get("kernel"), f"launch {l.name} carries no kernel symbol"
        out.setdefault(l.name, []).append(l.meta["kernel"])
    assert not bad, bad
    return out


_CACHE = {}


def step_symbols(monkeypatch, dimsize, is3d, precision, batch=1):
    key = (dimsize, is3d, precision, batch)
    if key not in _CACHE:
        with dry_step(monkeypatch, *key) as st:
            _CACHE[key] = symbols(st)
    return _CACHE[key]


CONFIGS = [(n, is3d, prec, b) for n in (74, 132, 260) for is3d in (True, False) for prec in ("fp32", "bf16")
           for b in ((1,) if n == 260 else (1, 2))]


@pytest.mark.parametrize("dimsize,is3d,precision,batch", CONFIGS,
                         ids=[f"{n}-{'3d' if d else '2d'}-{p}-b{b}" for n, d, p, b in CONFIGS])
def test_every_launch_is_admitted(monkeypatch, dimsize, is3d, precision, batch):
    syms = step_symbols(monkeypatch, dimsize, is3d, precision, batch)
    assert sum(map(len, syms.values())) > 100, len(syms)


# Launches of the 260 step whose kernel symbols are not the 132 step's: {launch name: (at 132, at 260)}, each side
# {symbol: launches of that name that get it} (a generator layer has six launches: three call sites in G and in F, the
# cycle path's on the smaller cone).  Recorded from this tree.
ROUTES_260 = {
    (True, "fp32"): {
        "g.d1b": ({"conv_s2_k<8, 1, 4, true>": 6},
                  {"conv_direct_k<8, 0, 8, 0, false>": 4, "conv_s2_k<8, 1, 4, true>": 2}),
        "d.d3a": ({"conv_lds_k<32, 32, 3, 1, 8, 6, 1, false>": 4},
                  {"wino_conv_k<32, 32, 2, 0, 9>": 4}),
        "g.bww.u1a": ({"wino_bww_k<32, 16, 2, false, 9>": 6},
                      {"wino_bww_k<32, 16, 2, false, 17>": 6}),
        "g.bww.mid": ({"wino_bww_k<32, 32, 2, false, 17>": 4, "wino_bww_k<32, 32, 2, false, 9>": 2},
                      {"wino_bww_k<32, 32, 2, false, 17>": 6}),
        "g.bww.u2a": ({"wino_bww_k<16, 32, 2, false, 9>": 6},
                      {"wino_bww_k<16, 32, 2, false, 17>": 2, "wino_bww_k<16, 32, 2, false, 9>": 4}),
        "g.bd.d2a": ({"wino_conv_k<16, 8, 2, 1, 9>": 6},
                     {"wino_conv_k<16, 8, 2, 1, 17>": 2, "wino_conv_k<16, 8, 2, 1, 9>": 4}),
        "d.bww.d3a": ({"bww_s2_k<32, 32, 3, 1>": 4},
                      {"wino_bww_k<32, 32, 2, false, 9>": 4}),
    },
    (True, "bf16"): {},
    (False, "fp32"): {},
    (False, "bf16"): {},
}


@pytest.mark.parametrize("is3d,precision", list(ROUTES_260), ids=[f"{'3d' if d else '2d'}-{p}" for d, p in ROUTES_260])
def test_routes_that_change_at_260_are_the_recorded_ones(monkeypatch, is3d, precision):
    at132 = step_symbols(monkeypatch, 132, is3d, precision)
    at260 = step_symbols(monkeypatch, 260, is3d, precision)
    assert sorted(at132) == sorted(at260)                    # the same launches, by name
    got = {name: (dict(Counter(at132[name])), dict(Counter(at260[name]))) for name in at132 if Counter(at132[name]) != Counter(at260[name])}
    assert got == ROUTES_260[is3d, precision], got
