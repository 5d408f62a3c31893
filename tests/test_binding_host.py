"""CPU: ``_lib.call``, the one helper the package makes its native calls with, on stand-in
functions (objects with ``argtypes`` / ``restype`` that record what they receive; no GPU, and the
library need not be built): what it converts, what it leaves alone and what it refuses."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from pano360_amd import _lib

I64P = C.POINTER(C.c_int64)


class StandIn:
    """A function object as ``lib()`` hands them out: records its arguments, returns ``status``."""

    def __init__(self, argtypes, restype=C.c_int, status=0):
        self.argtypes, self.restype, self.status, self.got = list(argtypes), restype, status, None

    def __call__(self, *args):
        self.got = args
        return self.status


@pytest.fixture
def bind(monkeypatch):
    """bind(name=function, ...): these are what ``lib()`` returns."""
    def bind(**functions):
        functions.setdefault("pano_last_error", lambda: b"the stand-in's message")
        monkeypatch.setattr(_lib, "_lib", types.SimpleNamespace(**functions))
    return bind


def memories():
    """(argument, its address) of a CPU tensor, a slice of one, a NumPy array and None."""
    t = torch.arange(12, dtype=torch.int64)
    a = np.arange(12, dtype=np.int64)
    return [(t, t.data_ptr()), (t[3:], t.data_ptr() + 24), (a, a.ctypes.data), (None, None)]


def test_memory_arrives_as_its_address_in_a_void_pointer(bind):
    fn = StandIn([C.c_void_p, C.c_int])
    bind(pano_fake=fn)
    for arg, address in memories():
        _lib.call("pano_fake", arg, 7)
        got, seven = fn.got
        assert seven == 7
        if arg is None:
            assert got is None
        else:
            assert type(got) is C.c_void_p and got.value == address


def test_memory_arrives_as_a_typed_pointer_of_equal_address(bind):
    fn = StandIn([I64P])
    bind(pano_fake=fn)
    for arg, address in memories():
        _lib.call("pano_fake", arg)
        got, = fn.got
        if arg is None:
            assert got is None
        else:
            assert isinstance(got, I64P) and C.cast(got, C.c_void_p).value == address
            assert got[1] == 1 if arg.shape[0] == 12 else got[1] == 4


def test_ctypes_takes_what_the_helper_hands_over(bind):
    """The same through a real foreign-function object: ctypes refuses an int or a c_void_p for a
    POINTER(c_int64) argument, so the callback only runs if the conversions are the right ones."""
    seen = []
    proto = C.CFUNCTYPE(C.c_int, C.c_void_p, I64P, C.c_float, C.c_int64)

    def callback(void, typed, scale, count):
        seen.append((void, C.cast(typed, C.c_void_p).value, typed[2], scale, count))
        return 0

    fn = proto(callback)
    assert fn.restype is C.c_int and len(fn.argtypes) == 4
    bind(pano_fake=fn)
    t = torch.arange(12, dtype=torch.int64)
    a = np.arange(12, dtype=np.int64)
    _lib.call("pano_fake", t[2:], a, np.float32(0.5), np.int64(1 << 40))
    assert seen == [(t.data_ptr() + 16, a.ctypes.data, 2, 0.5, 1 << 40)]


def test_ctypes_objects_and_plain_values_arrive_untouched(bind):
    fn = StandIn([C.POINTER(C.c_int), C.POINTER(_lib.FuseStack), C.c_void_p, C.c_void_p, C.c_int,
                  C.c_float])
    bind(pano_fake=fn)
    ints, word = (C.c_int * 3)(1, 2, 3), C.c_int(0)
    records, ref, handle = (_lib.FuseStack * 2)(), C.byref(word), C.c_void_p(64)
    scale = np.float32(1.5)
    _lib.call("pano_fake", ints, records, ref, 0x7F0000001000, 5, scale)
    assert fn.got[0] is ints and fn.got[1] is records and fn.got[2] is ref
    assert fn.got[3] == 0x7F0000001000 and fn.got[4] == 5 and fn.got[5] is scale
    _lib.call("pano_fake", ref, records, handle, None, np.int32(5), 2)
    assert fn.got[0] is ref and fn.got[2] is handle and fn.got[3] is None
    assert type(fn.got[4]) is np.int32 and fn.got[5] == 2


def test_via_calls_another_object_with_the_declaration_of_the_library(bind):
    """An engine calls through its ``lib`` attribute, which a caller may have wrapped."""
    fn, seen = StandIn([C.c_void_p, C.c_int]), []
    bind(pano_fake=fn)
    a = np.zeros(3)
    wrapped = types.SimpleNamespace(pano_fake=lambda *args: seen.append(args) or 0)
    _lib.call("pano_fake", a, 3, via=wrapped)
    assert fn.got is None and seen[0][0].value == a.ctypes.data and seen[0][1] == 3


def test_a_wrong_count_names_the_function_and_both_counts(bind):
    fn = StandIn([C.c_void_p, C.c_int, C.c_int])
    bind(pano_fake=fn)
    with pytest.raises(TypeError, match=r"pano_fake.*\b3\b.*\b2\b"):
        _lib.call("pano_fake", None, 1)
    with pytest.raises(TypeError, match=r"pano_fake.*\b3\b.*\b4\b"):
        _lib.call("pano_fake", None, 1, 2, 3)
    assert fn.got is None


def test_an_array_in_a_scalar_position_is_refused(bind):
    fn = StandIn([C.c_void_p, C.c_int, C.c_double])
    bind(pano_fake=fn)
    for bad in (np.zeros(3), torch.zeros(3), torch.zeros((2, 2))[0]):
        with pytest.raises(TypeError, match=r"pano_fake.*\b1\b"):
            _lib.call("pano_fake", None, bad, 0.5)
        with pytest.raises(TypeError, match=r"pano_fake.*\b2\b"):
            _lib.call("pano_fake", None, 1, bad)
    assert fn.got is None


def test_an_unknown_name_is_an_attribute_error(bind):
    bind()
    with pytest.raises(AttributeError):
        _lib.call("pano_no_such_function", 1)


def test_a_status_but_zero_raises_with_the_name_and_the_message(bind):
    bind(pano_fake=StandIn([C.c_int], status=_lib.EINVAL), pano_grow=StandIn([], status=1))
    with pytest.raises(_lib.PanoError, match=r"pano_fake failed \(-1\): the stand-in's message"):
        _lib.call("pano_fake", 3)
    with pytest.raises(_lib.PanoError, match="pano_grow"):
        _lib.call("pano_grow")


def test_value_results_are_int_exports():
    assert _lib.VALUE_RESULTS == {
        "pano_device_count", "pano_pitch", "pano_interior_block", "pano_kernel_count",
        "pano_blur_tile_grid", "pano_overlap_blocks", "pano_sift_detect_replaying"}
    for name in _lib.VALUE_RESULTS:
        assert _lib._SIGNATURES[name][0] is C.c_int, name


def test_the_guard_refuses_values_and_takes_every_status_function(bind):
    functions = {name: StandIn(args, res) for name, (res, args) in _lib._SIGNATURES.items()}
    bind(**functions)
    for name, (res, args) in _lib._SIGNATURES.items():
        zeros = [0] * len(args)
        if res is C.c_int and name not in _lib.VALUE_RESULTS:
            _lib.call(name, *zeros)
            assert functions[name].got == tuple(zeros)
        else:
            with pytest.raises(TypeError, match=name):
                _lib.call(name, *zeros)
