"""The denoise loop's graph cache (``posetraj_amd.step_graphs``: ``GraphKey``, ``StepGraphs``) with stand-in states: exact-key lookup,
pool sharing within a geometry, at most one state per kind, one geometry at a time.  No device."""
from types import SimpleNamespace

import pytest

from posetraj_amd.step_graphs import GraphKey, StepGraphs


def key(kind="plain", scale=1.0, **kw):
    base = dict(Bc=1, F=14, hw=(8, 8), cond_shape=(2, 14, 3, 64, 64), cam_shape=None, kind=kind, scale=scale if kind == "plain" else None,
                unet=11, controlnet=12, unet_gen=0, controlnet_gen=0, overlap=True, networks_name=None, dispatch=(True, False))
    return GraphKey(**dict(base, **kw))


def state(pool=None):
    """What the cache reads of a state: ``graph`` (None until captured) and the graph's ``pool()``."""
    return SimpleNamespace(graph=None if pool is None else SimpleNamespace(pool=lambda: pool))


def test_fields_and_geometry():
    assert GraphKey._fields == ("Bc", "F", "hw", "cond_shape", "cam_shape", "kind", "scale", "unet", "controlnet", "unet_gen",
                                "controlnet_gen", "overlap", "networks_name", "dispatch")
    assert key("plain", 0.9).geometry() == key("weighted").geometry() == key("off").geometry() == key()._replace(kind=None, scale=None)
    assert key("plain", 0.9) != key("plain", 1.0) and key("weighted") != key("off")


def test_exact_key_hit_and_miss():
    c, s = StepGraphs(), state("p")
    assert len(c) == 0 and c.get(key()) is None and c.of_kind("plain") is None and c.pool_for(key()) is None
    c.insert(key(), s)
    assert c.get(key()) is s and c.of_kind("plain") is s and list(c) == [key()] and len(c) == 1
    assert c.get(key(scale=0.5)) is None and c.get(key("off")) is None and c.get(key(F=16)) is None and c.of_kind("off") is None


def test_another_kind_of_the_same_geometry_is_kept_and_shares_the_first_pool():
    c, w, o, p = StepGraphs(), state("pool-w"), state("pool-w"), state("pool-w")
    c.insert(key("weighted"), w)
    assert c.pool_for(key("off")) == "pool-w"
    c.insert(key("off"), o)
    assert c.get(key("weighted")) is w and c.get(key("off")) is o and len(c) == 2
    assert c.pool_for(key("plain", 0.9)) == "pool-w"
    c.insert(key("plain", 0.9), p)
    assert [c.of_kind(k) for k in ("weighted", "off", "plain")] == [w, o, p] and len(c) == 3


def test_plain_with_another_scale_replaces_the_plain_state_and_keeps_the_others():
    c, w, o, p, q = StepGraphs(), state("a"), state("a"), state("a"), state("a")
    for k, s in ((key("plain", 0.9), p), (key("weighted"), w), (key("off"), o)):
        c.insert(k, s)
    assert c.pool_for(key("plain", 0.5)) == "a"                       # of the other kinds: the state about to leave lends no pool
    c.insert(key("plain", 0.5), q)
    assert c.get(key("plain", 0.9)) is None and c.of_kind("plain") is q and c.get(key("plain", 0.5)) is q
    assert c.of_kind("weighted") is w and c.of_kind("off") is o and len(c) == 3
    only = StepGraphs()
    only.insert(key("plain", 0.9), p)
    assert only.pool_for(key("plain", 0.5)) is None


def test_another_geometry_leaves_only_the_new_state():
    c, n = StepGraphs(), state("b")
    for k in (key("plain", 0.9), key("weighted"), key("off")):
        c.insert(k, state("a"))
    assert c.pool_for(key("off", F=16)) is None
    c.insert(key("off", F=16), n)
    assert list(c) == [key("off", F=16)] and c.of_kind("off") is n and c.of_kind("plain") is None and c.of_kind("weighted") is None


def test_no_pool_without_a_captured_state_of_the_geometry():
    c = StepGraphs()
    c.insert(key("weighted"), state(None))                            # stored, not captured
    assert c.pool_for(key("off")) is None
    assert c.pool_for(key("off", hw=(8, 16))) is None and c.pool_for(key("off", cam_shape=(2, 14, 12))) is None


@pytest.mark.parametrize("field,value", [("dispatch", (False, False)), ("overlap", False), ("unet_gen", 1), ("controlnet_gen", 3)])
def test_keys_of_equal_geometry_fields_that_differ_in_an_identity_field(field, value):
    """Keys that differ only in ``dispatch``, ``overlap`` or a generation counter have the same geometry fields (``Bc, F, hw, cond_shape,
    cam_shape``) and are different keys: no hit.  As states they are not "of the same geometry" (that is equality after
    ``_replace(kind=None, scale=None)``, as before): the graphs were captured from other launches, so the old ones lend no pool and leave."""
    a, b = key("weighted"), key("weighted", **{field: value})
    assert a != b and (a.Bc, a.F, a.hw, a.cond_shape, a.cam_shape) == (b.Bc, b.F, b.hw, b.cond_shape, b.cam_shape)
    assert a.geometry() != b.geometry()
    c, new = StepGraphs(), state("b")
    c.insert(a, state("a"))
    assert c.get(b) is None and c.get(b._replace(kind="off")) is None and c.pool_for(b._replace(kind="off")) is None
    c.insert(b._replace(kind="off"), new)
    assert list(c) == [b._replace(kind="off")] and c.of_kind("off") is new
