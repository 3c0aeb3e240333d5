"""CPU arithmetic under which the bit-for-bit fixtures of tests/golden/ are recorded (oracle/gen_golden.py) and checked
(tests/conftest.py).

torch's CPU results differ in the last bits from host to host: oneDNN and ATen pick their kernels by instruction set,
MKL its code path by instruction set, and threaded reductions split their work by the thread count.  A fixture recorded
on one host then misses by an ulp on another.  Pinned as below, hosts compute the same bits: the AVX2 kernels of ATen,
oneDNN and MKL, one thread.

What no setting reaches: on CPUs of other vendors than Intel, MKL runs its generic sgemm whatever it is asked, and that
rounds the forcing product actions @ F differently from the fma chain the fixtures hold (the one MKL computes on Intel
CPUs, and the HIP stepper and the CPU twin compute everywhere).  Tests that form that product with torch check for it
first (tests/conftest.py::require_fma_sgemm).

``pin_env()`` must run before torch is imported; ``pin_torch()`` after."""
import os

ENV = {"MKL_CBWR": "AVX2", "ATEN_CPU_CAPABILITY": "avx2", "ONEDNN_MAX_CPU_ISA": "AVX2"}


def pin_env():
    os.environ.update(ENV)


def pin_torch():
    import torch
    torch.set_num_threads(1)
