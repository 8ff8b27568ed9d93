"""Values derived from FROZEN parameters (packed kernel layouts, fp32 forms, the fused q|k|v weight, a LoRA-merged weight),
built once.  The UNet of the training step never changes, and re-deriving all of this every step is ~10 ms of small
kernels; a trainable parameter's forms are rebuilt from the master on every use (autograd must see the master)."""
import weakref

import torch

_CACHE = {}          # (ids of the sources, kind) -> (weakrefs of the sources, their stamps, value)


def clear():
    _CACHE.clear()
    _MODULES.clear()


def _stamp(p):
    # in-place updates bump _version; .to() / load_state_dict / a `.data` assignment may swap the storage or the dtype
    return p._version, p.data_ptr(), p.dtype


def frozen(sources, kind, build, derived=False):
    """`build()`, cached while EVERY one of `sources` is a frozen nn.Parameter -- the same objects (ids are recycled after
    garbage collection: the entry holds weakrefs) at the same version, storage and dtype; anything else (a trainable
    source, a temporary) rebuilds on every use and caches nothing.  The entry goes when one of its sources is collected.
    derived: a cached value is itself wrapped as a frozen Parameter, so that the forms derived from IT are cached as well.
    The value must not be (or alias) one of its sources: the entry would keep that source alive for ever."""
    if any(p.requires_grad or not isinstance(p, torch.nn.Parameter) for p in sources):
        return build()
    key = (tuple(id(p) for p in sources), kind)
    stamps = tuple(_stamp(p) for p in sources)
    hit = _CACHE.get(key)
    if hit is not None and hit[1] == stamps and all(r() is p for r, p in zip(hit[0], sources)):
        return hit[2]
    value = build()
    if derived:
        value = torch.nn.Parameter(value.detach(), requires_grad=False)

    def drop(_ref, key=key):
        _CACHE.pop(key, None)
    _CACHE[key] = (tuple(weakref.ref(p, drop) for p in sources), stamps, value)
    return value


_MODULES = weakref.WeakKeyDictionary()      # module -> {kind: (stamps of its parameters, value)}


def frozen_module(module, kind, build):
    """`build()`, cached per MODULE while every parameter of it keeps its version, storage and dtype -- whether or not the
    parameters require grad: for values that are used without a gradient path only (an inference plan of the whole module),
    where an optimizer step, an in-place edit, `.to()` or `load_state_dict` must rebuild and nothing else may."""
    stamps = tuple(_stamp(p) for p in module.parameters())
    kinds = _MODULES.setdefault(module, {})
    hit = kinds.get(kind)
    if hit is not None and hit[0] == stamps:
        return hit[1]
    value = build()
    kinds[kind] = (stamps, value)
    return value
