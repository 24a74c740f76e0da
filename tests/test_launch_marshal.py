"""The argument conversion of the one launch path into libgoat_hip.so (_plumbing.cargs) and its status check, without a GPU:
CPU tensors have a data_ptr() too, and the status check needs no library."""
import ctypes

import pytest
import torch

from vln_goat_amd import _lib
from vln_goat_amd._plumbing import _ptr, cargs


def test_tensor_becomes_its_data_pointer():
    t = torch.arange(12, dtype=torch.float32)
    p = torch.nn.Parameter(torch.zeros(3))
    v = t[4:]                                       # a view: its own first element, not the storage's
    out = cargs(t, p, v)
    assert out == (t.data_ptr(), p.data_ptr(), t.data_ptr() + 16)
    assert all(type(x) is int for x in out)


def test_tensor_subclass_becomes_its_data_pointer():
    class Tagged(torch.Tensor):
        pass
    t = torch.zeros(5).as_subclass(Tagged)
    assert type(t) is Tagged and cargs(t, True) == (t.data_ptr(), True)


def test_none_ints_floats_pass_through():
    out = cargs(None, 0, 7, -1, 1 << 40, 0.5, 1e-12)
    assert out == (None, 0, 7, -1, 1 << 40, 0.5, 1e-12)
    assert out[0] is None and type(out[1]) is int and type(out[5]) is float


def test_ctypes_arrays_and_structs_are_the_same_objects():
    arr = (ctypes.c_void_p * 3)(1, 2, 3)
    nb = (ctypes.c_int64 * 2)(16, 32)
    rec = _lib.LnPartial()
    out = cargs(arr, nb, rec)
    assert out[0] is arr and out[1] is nb and out[2] is rec


def test_offset_pointer_is_an_int_and_passes_through():
    t = torch.zeros(16, dtype=torch.bfloat16)
    p = _ptr(t, 5)
    assert type(p) is int and p == t.data_ptr() + 10
    assert cargs(p, t) == (p, t.data_ptr())


def test_mixed_call_keeps_order_and_length():
    t, u = torch.zeros(2), torch.zeros(2, dtype=torch.int64)
    arr = (ctypes.c_void_p * 1)(0)
    out = cargs(_lib.GOAT_F32, t, 4, None, arr, 0.25, u, _ptr(t, 1))
    assert out == (_lib.GOAT_F32, t.data_ptr(), 4, None, arr, 0.25, u.data_ptr(), t.data_ptr() + 4)
    assert cargs() == ()


def test_status_zero_is_silent():
    assert _lib.check(0, 'goat_colsum') is None


@pytest.mark.parametrize('status', [1, -1, 3])
def test_nonzero_status_names_the_symbol(status):
    with pytest.raises(RuntimeError) as e:
        _lib.check(status, 'goat_colsum')
    assert str(e.value) == 'libgoat_hip: goat_colsum failed with status %d' % status


def test_launch_reports_what_if_given_else_the_symbol(monkeypatch):
    """launch() itself, on a stand-in for the library handle: the stream comes first, then the converted arguments; the error
    names `what` when given and the symbol otherwise."""
    from vln_goat_amd import _plumbing
    seen = []

    class Handle:
        @staticmethod
        def goat_fake(*a):
            seen.append(a)
            return 0 if a[1] is not None else 2

    monkeypatch.setattr(_plumbing._lib, 'lib', lambda: Handle)
    monkeypatch.setattr(_plumbing, '_stream', lambda: 1234)
    t = torch.zeros(3)
    assert _plumbing.launch('goat_fake', t, 5) is None
    assert seen == [(1234, t.data_ptr(), 5)]
    with pytest.raises(RuntimeError) as e:
        _plumbing.launch('goat_fake', None)
    assert str(e.value) == 'libgoat_hip: goat_fake failed with status 2'
    with pytest.raises(RuntimeError) as e:
        _plumbing.launch('goat_fake', None, what='goat_fake(M=5,N=7)')
    assert str(e.value) == 'libgoat_hip: goat_fake(M=5,N=7) failed with status 2'
    # call(): the same, from a tuple that is converted already and goes in as the object it is
    del seen[:]
    ctuple = _plumbing.cargs(t, 5, 0.5)
    assert _plumbing.call('goat_fake', ctuple) is None
    assert seen == [(1234,) + ctuple]
    with pytest.raises(RuntimeError) as e:
        _plumbing.call('goat_fake', (None,), what='goat_fake(K=12)')
    assert str(e.value) == 'libgoat_hip: goat_fake(K=12) failed with status 2'
    with pytest.raises(RuntimeError) as e:
        _plumbing.call('goat_fake', (None,))
    assert str(e.value) == 'libgoat_hip: goat_fake failed with status 2'
