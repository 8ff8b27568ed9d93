"""The fp64 references of tests/backward_ref.py and tests/autograd_ref.py on operands rounded to fp16 instead of bf16, for the
fp16-element tests (tests/test_backward_ops_f16_gpu.py, tests/test_autograd_ops_f16_gpu.py).  A helper module, not a conftest.

Both reference modules round through one module-level function `bf` and cache their seeded cases and references per process.
`fp16(module, name, *args)` calls `module.name(*args)` with `bf` rounding to fp16 and with fp16 TWINS of the cached functions in
place (the same code, caches of their own), and puts everything back: the bf16 cases and references that other tests share are
neither recomputed nor touched, and an fp16 reference is computed once per process too.  Same seeds, same formulas, same fp64
autograd -- only the rounding of the operands differs."""
import contextlib
import functools

import torch

_TWINS = {}         # module name -> {function name: lru_cache twin of the module's cached function}


def _half(x):
    return x.to(torch.float16)


def _twins(mod):
    if mod.__name__ not in _TWINS:
        _TWINS[mod.__name__] = {name: functools.lru_cache(maxsize=None)(f.__wrapped__) for name, f in vars(mod).items()
                                if callable(f) and hasattr(f, "cache_info") and hasattr(f, "__wrapped__")}
    return _TWINS[mod.__name__]


@contextlib.contextmanager
def fp16_operands(mod):
    saved = {name: getattr(mod, name) for name in list(_twins(mod)) + ["bf"]}
    try:
        for name, twin in _twins(mod).items():
            setattr(mod, name, twin)
        mod.bf = _half
        yield
    finally:
        for name, f in saved.items():
            setattr(mod, name, f)


def fp16(mod, name, *args):
    """mod.<name>(*args) on fp16-rounded operands (looked up INSIDE the context: the twin, not the bf16 original)."""
    with fp16_operands(mod):
        return getattr(mod, name)(*args)
