"""runtime.Workspace, the Python side of gsr_alloc_fn, and the pointer helpers; the callback is called through ctypes on CPU tensors."""
import ctypes
import gc
import weakref

import torch

from gauspcc_amd import runtime


def test_callback_returns_the_buffer_and_keeps_it():
    ws = runtime.Workspace("cpu")
    cb = ws.fn()
    p = cb(None, 300)
    assert p
    assert len(ws.buffers) == 1
    assert ws.buffers[0].dtype == torch.uint8 and ws.buffers[0].numel() == 300
    assert ws.buffers[0].data_ptr() == p
    q = cb(None, 7)
    assert q and q != p
    assert [b.numel() for b in ws.buffers] == [300, 7]


def test_zero_byte_request_gets_one_byte():
    ws = runtime.Workspace("cpu")
    assert ws.fn()(None, 0)
    assert ws.buffers[0].numel() == 1


def test_failed_allocation_returns_null(monkeypatch):
    def boom(*args, **kwargs):
        raise RuntimeError("out of memory")

    ws = runtime.Workspace("cpu")
    cb = ws.fn()
    monkeypatch.setattr(torch, "empty", boom)
    assert cb(None, 64) is None
    assert ws.buffers == []


def test_buffers_die_with_the_workspace_without_the_cycle_collector():
    gc.disable()
    try:
        ws = runtime.Workspace("cpu")
        cb = ws.fn()
        cb(None, 64)
        ref = weakref.ref(ws.buffers[0])
        del ws, cb
        assert ref() is None
    finally:
        gc.enable()


def test_ptr_and_ptrs():
    t = torch.zeros(4)
    assert runtime.ptr(None) is None
    assert runtime.ptr(t) == t.data_ptr()
    a = runtime.ptrs([t, None])
    assert isinstance(a, ctypes.Array) and len(a) == 2
    assert a[0] == t.data_ptr() and a[1] is None
    b = runtime.ptrs([t], 16)
    assert len(b) == 16 and b[0] == t.data_ptr() and all(b[i] is None for i in range(1, 16))
