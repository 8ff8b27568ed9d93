"""Invalidation rules of the frozen-parameter cache (ctrlv_amd/frozen.py): pure host logic, checked on CPU tensors."""
import gc

import pytest
import torch

from ctrlv_amd import frozen as fc
from ctrlv_amd.frozen import frozen


@pytest.fixture(autouse=True)
def _empty_cache():
    fc.clear()
    yield
    fc.clear()


def _param(*shape, grad=False, dtype=torch.float32):
    return torch.nn.Parameter(torch.randn(*shape).to(dtype), requires_grad=grad)


class Builder:
    """build() of one value: counts its calls, returns twice the (concatenated) sources"""

    def __init__(self, *sources):
        self.sources, self.calls = sources, 0

    def __call__(self):
        self.calls += 1
        return torch.cat([s.detach().reshape(-1) for s in self.sources]) * 2


def test_hit_on_an_unchanged_frozen_source():
    p = _param(4, 3)
    b = Builder(p)
    v1, v2 = frozen((p,), "k", b), frozen((p,), "k", b)
    assert b.calls == 1 and v1 is v2
    assert torch.equal(v1, p.detach().reshape(-1) * 2)
    other = Builder(p)                                   # another kind of the same source is another entry
    assert frozen((p,), "k2", other) is not v1 and other.calls == 1 and len(fc._CACHE) == 2


def test_rebuild_after_an_in_place_update():
    p = _param(5)
    b = Builder(p)
    v1 = frozen((p,), "k", b)
    with torch.no_grad():
        p.add_(1.0)
    v2 = frozen((p,), "k", b)
    assert b.calls == 2 and torch.equal(v2, p.detach() * 2) and not torch.equal(v1, v2)
    assert frozen((p,), "k", b) is v2 and b.calls == 2 and len(fc._CACHE) == 1


def test_rebuild_after_a_data_storage_swap():
    p = _param(5)
    b = Builder(p)
    frozen((p,), "k", b)
    version = p._version
    p.data = torch.randn(5)                              # (what .to() / load_state_dict(assign=True) do: no version bump)
    assert p._version == version
    v2 = frozen((p,), "k", b)
    assert b.calls == 2 and torch.equal(v2, p.detach() * 2)
    p.data = p.data.to(torch.bfloat16)                   # ... and a dtype change
    assert frozen((p,), "k", b).dtype == torch.bfloat16 and b.calls == 3


@pytest.mark.parametrize("which", [0, 1, 2])
def test_never_cached_while_one_source_requires_grad_or_is_not_a_parameter(which):
    ps = [_param(3) for _ in range(3)]
    trainable = list(ps)
    trainable[which] = _param(3, grad=True)
    plain = list(ps)
    plain[which] = torch.randn(3)                        # a temporary: its address may be recycled
    for sources in (trainable, plain):
        b = Builder(*sources)
        v1, v2 = frozen(tuple(sources), "k", b), frozen(tuple(sources), "k", b, derived=True)
        assert b.calls == 2 and v1 is not v2 and not isinstance(v2, torch.nn.Parameter)
    assert not fc._CACHE


def test_requires_grad_flip_stops_and_restarts_caching():
    p = _param(4)
    b = Builder(p)
    frozen((p,), "k", b)
    p.requires_grad_(True)
    frozen((p,), "k", b), frozen((p,), "k", b)
    assert b.calls == 3
    with torch.no_grad():
        p.mul_(2.0)                                      # an optimizer step while it was trainable
    p.requires_grad_(False)
    v = frozen((p,), "k", b)
    assert b.calls == 4 and torch.equal(v, p.detach() * 2)      # (the stale entry of the first freeze is not served)
    assert frozen((p,), "k", b) is v and b.calls == 4


def test_multi_source_key():
    q, k, v = _param(2, 3), _param(2, 3), _param(2, 3)
    b = Builder(q, k, v)
    w = frozen((q, k, v), "cat", b)
    assert frozen((q, k, v), "cat", b) is w and b.calls == 1
    with torch.no_grad():
        v.zero_()                                        # a change of ANY source rebuilds
    w2 = frozen((q, k, v), "cat", b)
    assert b.calls == 2 and torch.equal(w2[-6:], torch.zeros(6))
    k2 = _param(2, 3)                                    # a replaced member is another key: q's entry is not served for it
    b2 = Builder(q, k2, v)
    w3 = frozen((q, k2, v), "cat", b2)
    assert b2.calls == 1 and torch.equal(w3[6:12], k2.detach().reshape(-1) * 2)
    assert frozen((q, k, v), "cat", b) is w2 and b.calls == 2


@pytest.mark.parametrize("dies", [0, 1])
def test_entry_is_gone_after_a_source_is_garbage_collected(dies):
    ps = [_param(3), _param(3)]
    frozen(tuple(ps), "k", Builder(*ps))
    frozen((ps[1 - dies],), "own", Builder(ps[1 - dies]))
    assert len(fc._CACHE) == 2
    del ps[dies]
    gc.collect()
    assert list(fc._CACHE) == [((id(ps[0]),), "own")]    # the survivor's own entry stays
    # a new parameter at a recycled address is never served a dead one's entry
    for _ in range(50):
        n = _param(3)
        b = Builder(n)
        assert torch.equal(frozen((n,), "k", b), n.detach() * 2) and b.calls == 1
        del n, b


def test_a_derived_frozen_parameter_gets_its_own_entries():
    q, k = _param(2, 3), _param(2, 3)
    b = Builder(q, k)
    w = frozen((q, k), "cat", b, derived=True)
    assert isinstance(w, torch.nn.Parameter) and not w.requires_grad
    assert frozen((q, k), "cat", b, derived=True) is w
    packs = []

    def packed_of(t):                                    # (holds no reference to t once it has run)
        return frozen((t,), "packed", lambda: (packs.append(1), t.detach() * 2)[1])

    packed = packed_of(w)
    assert packed_of(frozen((q, k), "cat", b, derived=True)) is packed and len(packs) == 1 and b.calls == 1
    with torch.no_grad():
        q.add_(1.0)                                      # a new derived parameter: its layouts are packed anew,
    w2 = frozen((q, k), "cat", b, derived=True)
    assert w2 is not w and packed_of(w2) is not packed and len(packs) == 2
    del w, packed
    gc.collect()                                         # and the old one's entries went with it
    assert sorted(kind for _, kind in fc._CACHE) == ["cat", "packed"]


def test_f32_of_an_fp32_parameter_is_not_an_entry():
    from ctrlv_amd.autograd import clear_pack_cache, f32
    p32, p16 = _param(4), _param(4, dtype=torch.bfloat16)
    assert f32(p32) is p32 and not fc._CACHE             # (the value would be its own source: the entry would pin it)
    v = f32(p16)
    assert v.dtype == torch.float32 and f32(p16) is v and len(fc._CACHE) == 1
    clear_pack_cache()
    assert not fc._CACHE
