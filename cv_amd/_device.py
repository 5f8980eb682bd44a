"""The one rule of the Python layer for what crosses into the rs_* / hm_* calls of include/akz.h that only enqueue: device
arguments, host index lists, the stream to wait for, and what has to stay alive behind a call that has returned.

  call(symbol, ...)       the foreign call: every argument through arg(), the status checked under the symbol's name
  arg(a)                  a d_* argument: None, an int (a device address) or anything with data_ptr(); a struct by reference
  tensor(...)             a host array uploaded, a device tensor checked and taken as it is
  index_list(blocks)      a host list of block indices -> (uint32 array, count)
  wait(stream)            a stream_to_wait value -> the handle the ABI takes
  wait_or_current(...)    the named stream, else the current torch stream of the device
  keep_alive(holder, ...) what an enqueued call still reads, held by what the caller gets back
  host_u32(t)             a device tensor of 4-byte words on the host
"""
import ctypes as C

import numpy as np

from . import _lib


def arg(a):
    """One argument of a foreign call.  A d_* argument is None, an int (a device address: ints pass as they are, so does
    every count) or anything with data_ptr() (a torch tensor); a ctypes.Structure goes by reference.  Context handles and
    the arrays of index_list() are ctypes objects already."""
    if isinstance(a, C.Structure):
        return C.byref(a)
    return a.data_ptr() if hasattr(a, "data_ptr") else a


def call(symbol, *args):
    """lib().symbol(*args) with every argument through arg(); a non-zero status raises AkzError under the symbol's name."""
    _lib.check(getattr(_lib.lib(), symbol)(*map(arg, args)), symbol)


def require_device(*tensors, itemsize=None):
    """THE test of a tensor the device reads where it lies: on the device, contiguous and, where `itemsize` is given, of
    elements that wide."""
    for t in tensors:
        if not (t.is_cuda and t.is_contiguous() and itemsize in (None, t.element_size())):
            raise ValueError("contiguous device tensors of the documented element type only")


def tensor(torch, a, dtype, dev):
    """a device tensor as it is (require_device, of dtype's width), a host array uploaded as `dtype`"""
    if isinstance(a, torch.Tensor):
        require_device(a, itemsize=np.dtype(dtype).itemsize)
        return a
    return _lib.device_bytes(torch, np.ascontiguousarray(a, dtype), dev)


def index_list(blocks):
    """A sequence of block indices (any nesting, flattened row by row) -> (uint32 ctypes array, count): the two arguments the
    ABI takes for a host index list.  The array has one word at the least, so that an empty list still has an address.  The
    call reads it before it returns: the caller keeps it in a local until then."""
    a = np.ascontiguousarray(blocks, np.uint32).reshape(-1)
    words = (C.c_uint32 * max(1, a.size))()
    C.memmove(words, a.ctypes.data, a.nbytes)
    return words, a.size


def wait(stream):
    """A stream_to_wait value -> what the ABI takes.  None: nothing to wait for.  A torch stream (anything with
    .cuda_stream): _lib.wait_handle, so that the legacy default stream, whose handle is 0, becomes AKZ_STREAM_LEGACY and
    never "nothing to wait for".  An int is a raw handle (rs_stream() / hm_stream() handed back in) and passes as it is."""
    return _lib.wait_handle(stream) if hasattr(stream, "cuda_stream") else stream


def wait_or_current(torch, stream, dev):
    """the named stream (as wait() takes it), else the current torch stream of `dev`"""
    return wait(stream) or wait(torch.cuda.current_stream(dev))


def keep_alive(holder, *reads):
    """THE keep-alive rule.  The calls enqueue on the consensus' stream, which torch's allocator does not know: a tensor that
    is dropped on the host while that stream still reads it is handed out again.  So whatever an enqueued call reads and
    the caller does not hold — an uploaded host array, a scratch table — stays referenced until the consensus' stream has
    been waited for: by the result object the caller gets back, which lives as long as the outputs are of interest, or,
    where the caller gets back a bare tensor or tuple, by the consensus, whose sync() lets go.  -> holder"""
    holder._inputs = getattr(holder, "_inputs", ()) + reads
    return holder


def host_u32(t):
    """a device tensor of 4-byte elements -> its words on the host, uint32"""
    return t.cpu().numpy().view(np.uint32)
