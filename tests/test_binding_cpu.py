"""The binding's marshalling without libia_amd.so and without a GPU: _lib.load() on (tests/binding_stub.c built with gcc,
tests/binding_stub.h).  What an entry point RECEIVES is read back from the stub's echo block, for the plain form of the package
(tensors and numbers, no stream) and for the wrapped form of bench.py / tools (L.i64 / L.ptr / ..., an explicit stream, L.check)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from intrinsicavatar_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
STREAM = 0x5EED0                                                  # what the replaced _lib.stream() hands out


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("binding")), "libbinding_stub.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so, os.path.join(HERE, "binding_stub.c")])
    return L.load(so, os.path.join(HERE, "binding_stub.h"))


@pytest.fixture(autouse=True)
def sentinel_stream(monkeypatch):
    monkeypatch.setattr(L, "stream", lambda: C.c_void_p(STREAM))


def echo(stub, *args):
    out = (C.c_double * 9)(*[-1.0] * 9)
    assert stub.ia_stub_echo(*args[:7], out, *args[7:]) == 0
    return list(out)


def test_plain_form(stub):
    host = (C.c_float * 3)(0.5, 1.5, 2.5)
    got = echo(stub, 1 << 40, None, 0.25, 1e-300, 0xFFFFFFFF, 1 << 33, host)
    assert got == [float(1 << 40), 0.0, 0.25, 1e-300, float(0xFFFFFFFF), float(1 << 33), float(C.addressof(host)), 1.5, float(STREAM)]
    # a host block may be left out, a ctypes array may stand for the device pointer; ints convert to float parameters
    dev = (C.c_int * 4)()
    got = echo(stub, 65, dev, 2, 3, 0, 0, None)
    assert got == [65.0, float(C.addressof(dev)), 2.0, 3.0, 0.0, 0.0, 0.0, 0.0, float(STREAM)]


def test_explicit_stream_wins(stub):
    got = echo(stub, 1, None, 0.0, 0.0, 0, 0, None, C.c_void_p(0x77))
    assert got[8] == float(0x77)
    assert echo(stub, 1, None, 0.0, 0.0, 0, 0, None, None)[8] == 0.0           # the NULL stream, passed on purpose


def test_wrapped_form_gives_the_same_echo(stub):
    host = (C.c_float * 3)(0.5, 1.5, 2.5)
    dev = C.c_void_p(0x1000)
    plain = echo(stub, 7, dev, 0.25, 0.125, 9, 11, host)
    out = (C.c_double * 9)()
    L.check(stub.ia_stub_echo(L.i64(7), dev, L.f32(0.25), C.c_double(0.125), C.c_uint32(9), C.c_size_t(11), host, out, L.stream()),
            "ia_stub_echo")
    assert list(out) == plain and plain[1] == float(0x1000) and plain[8] == float(STREAM)
    assert echo(stub, L.i64(7), L.ptr(None), L.f32(0.25), 0.125, 9, 11, host)[:2] == [7.0, 0.0]


def test_status_becomes_an_error_with_the_entry_points_name(stub):
    with pytest.raises(L.IaError, match=r"^ia_stub_fail failed \(code -3\): stub: refused 42$"):
        stub.ia_stub_fail(42)
    with pytest.raises(L.IaError, match="ia_stub_fail failed"):
        stub.ia_stub_fail(L.i64(1), L.stream())


def test_host_only_query_returns_its_value(stub):
    assert stub.ia_stub_tmp_bytes(4) == 61
    assert stub.ia_stub_tmp_bytes(0) == -3                                      # a value, not a status: nothing raises
    assert stub.ia_stub_tmp_bytes(L.i64(4)) == 61
    assert stub.ia_stub_tmp_bytes is stub._cdll.ia_stub_tmp_bytes and stub._untimed == {"ia_last_error", "ia_stub_tmp_bytes"}
    assert isinstance(stub.ia_last_error(), bytes)


def test_argtypes_stay_as_the_header_declares_them(stub):
    fn = stub._cdll.ia_stub_echo
    assert list(fn.argtypes) == [C.c_int64, C.c_void_p, C.c_float, C.c_double, C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    assert fn.restype is C.c_int and stub._cdll.ia_stub_tmp_bytes.restype is C.c_int64


def test_cpu_tensor_for_a_pointer_is_an_iaerror(stub):
    with pytest.raises(L.IaError, match="need GPU tensors"):
        echo(stub, 1, torch.zeros(4), 0.0, 0.0, 0, 0, None)
    with pytest.raises(L.IaError, match="unit inner stride"):
        L.base_ptr(torch.zeros(4, 2))


OUT = object()                                                    # stands for the echo block in the argument lists below


@pytest.mark.parametrize("args", [
    (1, 0x1000, 0.0, 0.0, 0, 0, None, OUT),                 # a bare int for a pointer
    (1.0, None, 0.0, 0.0, 0, 0, None, OUT),                 # a float for int64_t
    (torch.tensor(1), None, 0.0, 0.0, 0, 0, None, OUT),     # a tensor for a scalar (ctypes alone would take it through __index__)
    (1, None, torch.tensor(0.5), 0.0, 0, 0, None, OUT),
    (1, None, 0.0, 0.0, 0, 0, OUT),                         # two arguments short: more than "the stream left out"
    (1, None, 0.0, 0.0, 0, 0, None, OUT, None, None),       # one too many
], ids=["int-for-pointer", "float-for-int64", "tensor-for-int64", "tensor-for-float", "two-short", "one-extra"])
def test_mistyped_or_miscounted_calls_raise(stub, args):
    out = (C.c_double * 9)()
    with pytest.raises((TypeError, C.ArgumentError)):
        stub.ia_stub_echo(*[out if a is OUT else a for a in args])
