"""Every test of tests/test_lpips_gpu.py again with fp16 ELEMENTS, i.e. against libctrlv_hip_f16.so: the operands are split in
fp16 (hi + lo keeps about 22 bits), so the emulation's own error a -- and with it the metric's tolerance 4 (a + b), which the test
computes for its element type -- is about fifty times smaller than with bf16.

The source of test_lpips_gpu.py is executed in THIS module's namespace with EL = torch.float16, as tests/test_ops_f16_gpu.py does
with tests/test_ops_gpu.py: one set of cases to maintain.
"""
import os

import torch

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_lpips_gpu.py")
exec(compile(open(_SRC).read(), _SRC, "exec"), globals())      # defines pytestmark (gpu), the fixtures and the tests
EL = torch.float16                                               # noqa: F811  (read by the tests at call time)
