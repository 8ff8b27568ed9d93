"""Every test of tests/test_clip_plan_gpu.py again with fp16 ELEMENTS, i.e. against libctrlv_hip_f16.so: same cases, same fp32
references on the same (fp16-rounded) operands, the element bound scaled by `tol()` of that file; the model bound is relative to
the fp16 torch forward by construction.  The source is executed in THIS module's namespace with EL = torch.float16 (the pattern
of tests/test_clip_f16_gpu.py): one set of cases to maintain."""
import os

import torch

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_clip_plan_gpu.py")
exec(compile(open(_SRC).read(), _SRC, "exec"), globals())      # defines pytestmark (gpu), the fixtures and the tests
EL = torch.float16                                               # noqa: F811  (read by the tests at call time)
