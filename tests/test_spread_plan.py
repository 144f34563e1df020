"""Host side of the self-ensemble's spread map: the argument checks of the `spread` / `spread_gain` keywords of
predict_cube and predict_volume, which are made before anything touches a GPU."""
import inspect
import types

import numpy as np
import pytest

from transfer_em_amd.utils import _check_spread, predict_cube, predict_volume


def _model(is3d):
    return types.SimpleNamespace(generator_g=types.SimpleNamespace(is3d=is3d), outdimsize=36, buffer=19, device="cpu")


def _case(is3d, single=False):
    """(volume, start, size, the shape of a valid map)."""
    if single:
        return np.zeros((40, 44), np.uint8), (0, 0), (36, 30), (30, 36)
    if is3d:
        return np.zeros((40, 40, 40), np.uint8), (0, 0, 0), (36, 30, 20), (20, 30, 36)
    return np.zeros((3, 40, 40), np.uint8), (0, 0, 0), (36, 30, 3), (3, 30, 36)


def _readonly(shape):
    a = np.zeros(shape, np.uint8)
    a.flags.writeable = False
    return a


# name -> (the keywords, given the shape of a valid map)
BAD = {
    "no ensemble": lambda s: dict(spread=np.zeros(s, np.uint8)),
    "ensemble None": lambda s: dict(spread=np.zeros(s, np.uint8), ensemble=None),
    "transposed shape": lambda s: dict(spread=np.zeros(s[::-1], np.uint8), ensemble="flips"),
    "one voxel short": lambda s: dict(spread=np.zeros(s[:-1] + (s[-1] - 1,), np.uint8), ensemble="flips"),
    "an axis more": lambda s: dict(spread=np.zeros((1,) + s, np.uint8), ensemble="flips"),
    "int8": lambda s: dict(spread=np.zeros(s, np.int8), ensemble="flips"),
    "float32": lambda s: dict(spread=np.zeros(s, np.float32), ensemble="flips"),
    "no array": lambda s: dict(spread=[[0]], ensemble="flips"),
    "gain 0": lambda s: dict(spread=np.zeros(s, np.uint8), ensemble="flips", spread_gain=0.0),
    "gain negative": lambda s: dict(spread=np.zeros(s, np.uint8), ensemble="flips", spread_gain=-8.0),
    "gain inf": lambda s: dict(spread=np.zeros(s, np.uint8), ensemble="flips", spread_gain=float("inf")),
    "gain nan": lambda s: dict(spread=np.zeros(s, np.uint8), ensemble="flips", spread_gain=float("nan")),
    "gain inf as float32": lambda s: dict(spread=np.zeros(s, np.uint8), ensemble="flips", spread_gain=1e39),
    "gain 0 as float32": lambda s: dict(spread=np.zeros(s, np.uint8), ensemble="flips", spread_gain=1e-60),
    "gain no number": lambda s: dict(spread=np.zeros(s, np.uint8), ensemble="flips", spread_gain="8"),
    "gain None": lambda s: dict(spread=np.zeros(s, np.uint8), ensemble="flips", spread_gain=None),
}
FORMS = [(True, False), (False, False), (False, True)]


@pytest.mark.parametrize("fn", [predict_cube, predict_volume], ids=["cube", "volume"])
@pytest.mark.parametrize("is3d, single", FORMS, ids=["3d", "2d", "2d-image"])
@pytest.mark.parametrize("name", list(BAD))
def test_bad_spread_raises_before_any_gpu_work(fn, is3d, single, name):
    """A ValueError, not the TemError / RuntimeError of a missing GPU or of the stand-in model: the check comes first."""
    vol, start, size, shape = _case(is3d, single)
    with pytest.raises(ValueError):
        fn(vol, start, size, _model(is3d), (0.0, 1.0), (0.0, 1.0), **BAD[name](shape))


@pytest.mark.parametrize("is3d, single", FORMS, ids=["3d", "2d", "2d-image"])
def test_predict_cube_wants_a_writable_ndarray(is3d, single):
    vol, start, size, shape = _case(is3d, single)
    like = types.SimpleNamespace(shape=shape, dtype=np.dtype(np.uint8))        # fine for predict_volume, not here
    for s in (_readonly(shape), like):
        with pytest.raises(ValueError):
            predict_cube(vol, start, size, _model(is3d), (0.0, 1.0), (0.0, 1.0), ensemble="flips", spread=s)
    with pytest.raises(ValueError):
        predict_volume(vol, start, size, _model(is3d), (0.0, 1.0), (0.0, 1.0), ensemble="flips", spread=_readonly(shape))


def test_accepted_forms():
    syms = [((0, 1, 2), (0, 0, 0))]
    S = np.zeros((20, 30, 36), np.uint8)
    assert _check_spread(None, 8.0, None, (36, 30, 20)) is None                # off: whatever the ensemble
    assert _check_spread(None, 8.0, syms, (36, 30, 20)) is None
    assert _check_spread(S, 8.0, syms, (36, 30, 20), ndarray=True) == 8.0      # a one-member ensemble is accepted
    assert _check_spread(S, 1, syms, (36, 30, 20)) == 1.0                      # an int is a number
    assert _check_spread(S, np.float32(0.25), syms, (36, 30, 20)) == 0.25
    assert _check_spread(S[0], 8.0, syms, (36, 30)) == 8.0                     # one image
    like = types.SimpleNamespace(shape=(20, 30, 36), dtype="uint8")            # h5py / zarr: shape and dtype
    assert _check_spread(like, 2.0, syms, (36, 30, 20)) == 2.0


def test_defaults_leave_the_signatures_alone():
    for fn in (predict_cube, predict_volume):
        p = inspect.signature(fn).parameters
        assert p["spread"].default is None and p["spread_gain"].default == 8.0
        assert p["ensemble"].default is None and p["mips"].default is None and p["boundary"].default == "zeros"
        assert list(p)[-2:] == ["spread", "spread_gain"]                       # behind every earlier keyword
    from transfer_em_amd.utils import predict_cube_from_saved_model, predict_ng_cube
    for fn in (predict_ng_cube, predict_cube_from_saved_model):                # the reference's signatures take none
        assert "spread" not in inspect.signature(fn).parameters


def test_without_spread_the_other_checks_are_as_before():
    """spread=None with its default gain changes nothing of what the call checks: a bad ensemble or `mips` still
    raises its own ValueError."""
    vol, start, size, _ = _case(True)
    for fn in (predict_cube, predict_volume):
        with pytest.raises(ValueError, match="ensemble"):
            fn(vol, start, size, _model(True), (0.0, 1.0), (0.0, 1.0), ensemble=[])
        with pytest.raises(ValueError, match="mips"):
            fn(vol, start, size, _model(True), (0.0, 1.0), (0.0, 1.0), ensemble="flips", mips=9)
