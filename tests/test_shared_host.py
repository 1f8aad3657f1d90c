"""etch_amd/_shared.py (the checked cache of shared tensors) and the scope of pointops._seed, on CPU tensors."""
import pytest
import torch

from etch_amd._shared import Shared, constant_value
from etch_amd.models import pointops


def _counting(value=1.0):
    made = []

    def make():
        made.append(1)
        return torch.full((2, 3), value)
    return made, make


def test_hit_and_rebuild_after_an_edit_also_through_a_view():
    made, make = _counting()
    s = Shared()
    t = s.get("k", make)
    assert s.get("k", make) is t and len(made) == 1
    t.add_(1)
    t2 = s.get("k", make)
    assert t2 is not t and len(made) == 2 and bool((t2 == 1).all())
    t2.view(6)[4:].zero_()                       # views share their base's version counter
    t3 = s.get("k", make)
    assert t3 is not t2 and len(made) == 3 and bool((t3 == 1).all())
    assert s.get("k", make) is t3 and len(made) == 3


def test_built_under_no_grad_and_keep_is_held():
    w = torch.ones(3, requires_grad=True)
    s = Shared()
    assert not s.get("k", lambda: w * 2).requires_grad
    key = torch.zeros(1)
    s.get(("p", key.data_ptr()), lambda: torch.zeros(1), keep=key)
    assert any(e[2] is key for e in s._d.values())


def test_limit_clears_when_exceeded_as_the_dicts_it_replaces_did():
    s = Shared(limit=2)
    first = s.get(0, lambda: torch.zeros(1))
    for k in (1, 2):
        s.get(k, lambda: torch.zeros(1))
    assert len(s._d) == 3 and s.get(0, None) is first            # limit + 1 entries fit
    s.get(3, lambda: torch.zeros(1))                          # the next new key clears first
    assert len(s._d) == 1 and s.get(0, lambda: torch.zeros(1)) is not first
    u = Shared()
    for k in range(300):
        u.get(k, lambda: torch.zeros(1))
    assert len(u._d) == 300


def test_constant_value():
    s = Shared()
    t = s.get("ones", lambda: torch.ones(4), fill=1.0)
    assert constant_value(t) == 1.0
    assert constant_value(torch.ones(4)) is None and constant_value(s.get("plain", lambda: torch.ones(4))) is None
    assert constant_value(t.view(2, 2)) is None              # only the registered object itself speaks for its contents
    t.view(2, 2)[0, 0] = 3.0
    assert constant_value(t) is None
    fresh = s.get("ones", lambda: torch.ones(4), fill=1.0)
    assert fresh is not t and constant_value(fresh) == 1.0


def test_wrote_bumps_versions_and_skips_none():
    from etch_amd import _lib
    a, b = torch.zeros(2), torch.nn.Parameter(torch.zeros(2))
    va, vb = a._version, b._version
    _lib.wrote(a, None, b)
    assert a._version == va + 1 and b._version == vb + 1
    _lib.wrote(None)
    s = Shared()
    t = s.get("k", lambda: torch.zeros(2))
    _lib.wrote(t)
    assert s.get("k", lambda: torch.zeros(2)) is not t


def test_seed_needs_a_scope_and_dies_with_it():
    x, value = torch.zeros(3), torch.arange(3)
    key = ("fps", x.data_ptr(), (3,), (1,))
    assert pointops._knn_cache is None
    with pytest.raises(RuntimeError, match="knn_scope"):
        pointops._seed(key, (x,), value)
    with pointops.knn_scope():
        pointops._seed(key, (x,), value)
        assert pointops._memo(key, (x,), lambda: 1 / 0) is value
        with pointops.knn_scope():                            # scopes nest: the inner one sees and leaves the outer one's entries
            assert pointops._memo(key, (x,), lambda: 1 / 0) is value
        assert pointops._memo(key, (x,), lambda: 1 / 0) is value
    assert pointops._knn_cache is None
    assert pointops._memo(key, (x,), lambda: "recomputed") == "recomputed"
    with pytest.raises(ValueError, match="half-way"):
        with pointops.knn_scope():
            pointops._seed(key, (x,), value)
            raise ValueError("half-way")
    assert pointops._knn_cache is None
    with pointops.knn_scope():
        assert pointops._memo(key, (x,), lambda: "recomputed") == "recomputed"
