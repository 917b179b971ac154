"""ops.GroupCache, the one cache of the launch groups (dit.py: ws.wgrad_groups, ws.bias_groups, _fp8_wgroup; unet.py: _wgrad_groups)."""
import copy

from vaw_amd import ops


def test_group_cache_bound_lru_order_and_counters():
    built = []

    def build(tag):
        def f():
            built.append(tag)
            return tag
        return f

    c = ops.GroupCache(3)
    assert len(c) == 0 and not c and (c.hits, c.misses) == (0, 0)
    for k in "abc":
        assert c.get(k, build(k)) == k
    assert list(c) == ["a", "b", "c"] and (c.hits, c.misses) == (0, 3) and built == ["a", "b", "c"]
    # a hit returns the resident group, does not call build and makes the key the most recently used
    assert c.get("a", build("never")) == "a" and built == ["a", "b", "c"] and (c.hits, c.misses) == (1, 3)
    assert list(c) == ["b", "c", "a"]
    # beyond the bound the least recently used key goes: b, not a
    assert c.get("d", build("d")) == "d" and list(c) == ["c", "a", "d"] and len(c) == 3
    assert c.get("b", build("b2")) == "b2" and list(c) == ["a", "d", "b"] and (c.hits, c.misses) == (1, 5)
    # the bound holds over any sequence, and alternating keys within it never rebuild
    for i in range(50):
        c.get(("k", i % 7), build(i))
        assert len(c) <= 3
    two = ops.GroupCache(2)
    for i in range(10):
        two.get(i % 2, build(("alt", i)))
    assert (two.hits, two.misses) == (8, 2) and list(two) == [0, 1]
    # a falsy group is still a resident group
    z = ops.GroupCache(1)
    assert z.get("k", lambda: 0) == 0 and z.get("k", build("never")) == 0 and (z.hits, z.misses) == (1, 1)
    assert "never" not in built
    # a model's copy starts with no group and the same bound
    d = copy.deepcopy(c)
    assert isinstance(d, ops.GroupCache) and len(d) == 0 and d.bound == 3 and len(c) == 3
    c.clear()
    assert len(c) == 0
