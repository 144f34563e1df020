"""Host side of the self-ensemble of tiled inference: the symmetry lists of utils.symmetries and the argument checks of
the `ensemble` keyword, which are made before anything touches a GPU."""
import itertools
import types

import numpy as np
import pytest

from transfer_em_amd.utils import predict_cube, predict_volume, symmetries


def T(v, s):
    perm, flips = s
    return np.flip(np.transpose(v, perm), [a for a, f in enumerate(flips) if f])


def _as_pairs(syms):
    return [(tuple(p), tuple(bool(f) for f in fl)) for p, fl in syms]


@pytest.mark.parametrize("is3d, kind, count", [(True, "flips", 8), (True, "all", 48), (False, "flips", 4),
                                               (False, "all", 8)])
def test_sizes_identity_first_members_distinct(is3d, kind, count):
    syms = _as_pairs(symmetries(is3d, kind))
    n = 3 if is3d else 2
    assert len(syms) == count and len(set(syms)) == count
    assert syms[0] == (tuple(range(n)), (False,) * n)
    assert all(len(p) == n and len(f) == n and sorted(p) == list(range(n)) for p, f in syms)
    if kind == "flips":
        assert all(p == tuple(range(n)) for p, _ in syms)
    cube = np.arange(4 ** n).reshape((4,) * n)
    assert len({T(cube, s).tobytes() for s in syms}) == count                # distinct as maps, not only as tuples


def test_defaults_and_the_documented_order():
    assert _as_pairs(symmetries()) == _as_pairs(symmetries(True, "flips"))
    for is3d in (True, False):
        n = 3 if is3d else 2
        want = [(p, f) for p in itertools.permutations(range(n)) for f in itertools.product((False, True), repeat=n)]
        assert _as_pairs(symmetries(is3d, "all")) == want
        assert _as_pairs(symmetries(is3d, "flips")) == want[:2 ** n]
    with pytest.raises(ValueError):
        symmetries(True, "rotations")


@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
def test_all_is_closed_under_inversion(is3d):
    n = 3 if is3d else 2
    syms = _as_pairs(symmetries(is3d, "all"))
    cube = np.arange(5 ** n).reshape((5,) * n)
    images = {T(cube, s).tobytes(): s for s in syms}
    for s in syms:
        # the inverse of T_s is the member u with T_u(T_s(cube)) == cube
        inv = [u for u in syms if np.array_equal(T(T(cube, s), u), cube)]
        assert len(inv) == 1, s
        assert np.array_equal(T(T(cube, inv[0]), s), cube)
        assert images[T(cube, inv[0]).tobytes()] == inv[0]


def _model(is3d):
    return types.SimpleNamespace(generator_g=types.SimpleNamespace(is3d=is3d), outdimsize=36, buffer=19, device="cpu")


ID3, ID2 = ((0, 1, 2), (False, False, False)), ((0, 1), (False, False))
BAD_3D = {
    "empty": [],
    "not a permutation": [((0, 0, 2), (False, False, False))],
    "perm out of range": [((0, 1, 3), (False, False, False))],
    "flips too short": [((0, 1, 2), (False, False))],
    "flips too long": [((0, 1, 2), (False, False, False, True))],
    "duplicate": [ID3, ((2, 1, 0), (True, False, False)), ID3],
    "2-axis member for a 3-D model": [ID2],
    "unknown name": "rotations",
}
BAD_2D = {
    "empty": (),
    "not a permutation": [((1, 1), (False, False))],
    "flips too long": [((0, 1), (False, False, False))],
    "duplicate": [ID2, ID2],
    "duplicate across the two spellings": [((1, 0), (False, True)), ((0, 2, 1), (False, False, True))],
    "moves z": [((1, 0, 2), (False, False, False))],
    "flips z": [((0, 1, 2), (True, False, False))],
    "3-cycle": [((1, 2, 0), (False, False, False))],
}


@pytest.mark.parametrize("fn", [predict_cube, predict_volume], ids=["cube", "volume"])
@pytest.mark.parametrize("is3d, name", [(True, k) for k in BAD_3D] + [(False, k) for k in BAD_2D])
def test_bad_ensembles_raise_before_any_gpu_work(fn, is3d, name):
    """A ValueError, not the TemError / RuntimeError of a missing GPU or of the stand-in model: the check comes first."""
    vol = np.zeros((3, 40, 40) if not is3d else (40, 40, 40), np.uint8)
    start, size = (0, 0, 0), ((36, 36, 3) if not is3d else (36, 36, 36))
    with pytest.raises(ValueError):
        fn(vol, start, size, _model(is3d), (0.0, 1.0), (0.0, 1.0), ensemble=(BAD_3D if is3d else BAD_2D)[name])


def test_accepted_forms():
    from transfer_em_amd.utils import _check_ensemble
    assert _check_ensemble(None, True) is None and _check_ensemble(None, False) is None
    assert len(_check_ensemble("flips", True)) == 8 and len(_check_ensemble("all", True)) == 48
    assert len(_check_ensemble("flips", False)) == 4 and len(_check_ensemble("all", False)) == 8
    assert _check_ensemble("all", True)[0] == ((0, 1, 2), (0, 0, 0))
    # a 2-D model: 2-axis members and 3-axis ones that leave z alone name the same symmetry
    two = _check_ensemble([((1, 0), (True, False))], False)
    three = _check_ensemble([((0, 2, 1), (False, True, False))], False)
    assert two == three == [((0, 2, 1), (0, 1, 0))]
    assert _check_ensemble(symmetries(False, "all"), False) == _check_ensemble("all", False)
    assert _check_ensemble([([2, 0, 1], [1, 0, 1])], True) == [((2, 0, 1), (1, 0, 1))]
