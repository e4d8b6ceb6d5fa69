"""The marshalling every entry of the binding shares, written once: numpy arrays and torch tensors to the addresses the C ABI takes, the stream
argument to its handle, the caller's output arrays, and the call of a host build (plp_model_*_host)."""

import ctypes as C

import numpy as np

from ._core import PLP_ERR_INVALID_ARG, PlpError, lib


def host_ptr(v, empty_null=True):
    """The address of a numpy array, or NULL (None) for None and for an array without an element.  empty_null=False passes the address of an
    empty array too, for the entries that check their pointers before their caps (match_context.hip: observe_check, last_frame_check, project_check,
    keylines_3d_check)."""
    return None if v is None or (empty_null and v.size == 0) else v.ctypes.data


def host_ptrs(empty_null=True, **arrays):
    """{field: host_ptr(array)}: the pointer fields of an args struct by name"""
    return {k: host_ptr(v, empty_null) for k, v in arrays.items()}


def dev_ptr(v):
    """The device address of None, of an int (already an address) or of a torch tensor"""
    return None if v is None else (int(v) if isinstance(v, int) else v.data_ptr())


def dev_ptrs(**tensors):
    """{field: dev_ptr(tensor)}: the pointer fields of an args struct by name"""
    return {k: dev_ptr(v) for k, v in tensors.items()}


def stream_handle(stream):
    """The hipStream_t of a stream argument: an int is the handle itself, None the current stream of torch"""
    import torch
    return stream if isinstance(stream, int) else (stream or torch.cuda.current_stream()).cuda_stream


def array_or_none(v, dtype, *shape):
    """None for None, else v as a C-contiguous array of dtype, reshaped when a shape is given"""
    if v is None:
        return None
    a = np.ascontiguousarray(v, dtype)
    return a.reshape(*shape) if shape else a


def wanted(k, optional, outputs):
    """An optional output is skipped when `outputs` is given and does not name it"""
    return not (optional and outputs is not None and k not in outputs)


def out_arrays(specs, out):
    """The output arrays of an entry from (name, full shape, dtype[, fill]) tuples: the caller's out[name] where given -- slots the library does
    not write keep their values --, else a fresh array of `fill` (default 0)."""
    o = {}
    for k, full, dt, *fill in specs:
        v = None if out is None else out.get(k)
        if v is not None and not (isinstance(v, np.ndarray) and v.dtype == dt and v.shape == full and v.flags.c_contiguous):
            raise PlpError(PLP_ERR_INVALID_ARG, f"out[{k!r}] must be a C-contiguous {np.dtype(dt).name} array of shape {full}")
        o[k] = v if v is not None else np.full(full, fill[0], dt) if fill else np.zeros(full, dt)
    return o


def set_outputs(a, names, o, ptr):
    """a.out_<name> = ptr(o[name]) for every name, NULL for the ones o does not hold"""
    for k in names:
        setattr(a, "out_" + k, ptr(o.get(k)))


def model_call(symbol, count, *extra, neg_status=False):
    """call(args struct) for the host build `symbol`, which returns the struct's count field `count` or, refused, less: raises INVALID_ARG, or
    with neg_status the status the entry returned negated."""
    def call(a):
        r = getattr(lib(), symbol)(C.byref(a), *extra)
        if r != getattr(a, count):
            raise PlpError(-r if neg_status else PLP_ERR_INVALID_ARG, lib().plp_last_error().decode())
    return call


def model_draw(symbol, message, seed, p, iters, iter0, width, *sizes):
    """(iters, width) i32: the draws of the host build `symbol`(seed, p, iter0, iters, *sizes, out), which returns iters or, refused, less:
    raises INVALID_ARG with `message`"""
    out = np.zeros((int(iters), int(width)), np.int32)
    if getattr(lib(), symbol)(int(seed) & 0xFFFFFFFFFFFFFFFF, int(p), int(iter0), int(iters), *map(int, sizes), host_ptr(out)) != int(iters):
        raise PlpError(PLP_ERR_INVALID_ARG, message)
    return out


def _rows_u8(a):
    """a 2-D uint8 image as the C ABI takes it: unit stride inside a row, any row step >= the row length -- a view into a larger image (cv::Mat ROI, a cropped numpy
    slice) is passed AS IT IS, with its step; anything else is copied to a contiguous array first"""
    a = np.asarray(a)
    if a.dtype == np.uint8 and a.ndim == 2 and a.size and a.strides[1] == 1 and a.strides[0] >= a.shape[1]:
        return a
    return np.ascontiguousarray(a, np.uint8)
