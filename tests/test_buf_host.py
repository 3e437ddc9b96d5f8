"""The owning buffer type of the library (coloc_amd/csrc/clc_buf.h) on the host: Buf<Traits> over counting traits that can fail the k-th
allocation (tests/host/buf_host_lib.cpp).  What the context relies on: nothing leaks and nothing is freed twice whatever the sequence of
alloc / grow / move / reset / scope exit, a failed allocation leaves an empty buffer, and grow allocates exactly need + need * num / den
bytes -- and only when the buffer is too small."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(ROOT, "tests", "host", "libbuf_host.so")
    src = os.path.join(ROOT, "tests", "host", "buf_host_lib.cpp")
    hdr = os.path.join(ROOT, "coloc_amd", "csrc", "clc_buf.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-self-move", "-shared", "-fPIC", src, "-o", out])
    lib = C.CDLL(out)
    lib.buf_host_grow.restype = C.c_size_t
    lib.buf_host_grow.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_long)]
    return lib


def test_live_allocations_balance_over_every_operation(lib):
    assert lib.buf_host_lifetime() == 0          # (a non-zero value is the number of the CHECK that failed)


def test_a_failed_allocation_leaves_an_empty_buffer(lib):
    assert lib.buf_host_failure() == 0


def _grow(lib, have, need, num, den):
    re, live = C.c_int(-1), C.c_long(-1)
    bytes_ = lib.buf_host_grow(have, need, num, den, C.byref(re), C.byref(live))
    assert live.value == 0
    return bytes_, re.value


# the three policies in use: x1.25 (K2NN top-2 rows), x1.5 (pose scratch, pinned staging), exact (everything else)
@pytest.mark.parametrize("num,den", [(1, 4), (1, 2), (0, 1)])
@pytest.mark.parametrize("have", [0, 1, 4096])
@pytest.mark.parametrize("need", [1, 7, 4097, 10 ** 6 + 3])
def test_grow_arithmetic(lib, num, den, have, need):
    got, reallocated = _grow(lib, have, need, num, den)
    if need <= have:
        assert (got, reallocated) == (have, 0)
    else:
        assert (got, reallocated) == (need + need * num // den, 1)
    if need > have:
        assert got == {4: need + need // 4, 2: need + need // 2, 1: need}[den]


def test_grow_does_not_reallocate_at_or_below_the_capacity(lib):
    for need in (0, 1, 4095, 4096):
        for num, den in [(1, 4), (1, 2), (0, 1)]:
            assert _grow(lib, 4096, need, num, den) == (4096, 0)
    assert _grow(lib, 4096, 4097, 0, 1) == (4097, 1)
