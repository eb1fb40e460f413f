"""Loader core of the binding: lib() (libltr_gpu.so, loaded at first use, every signature of _abi applied once), LtrError,
and the few helpers the subject modules share.  It imports none of them."""
import ctypes as C
import os

from . import _abi
from ._build import LIB_PATH


class LtrError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__(f"ltr error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback for the alignment path)")
    L = C.CDLL(LIB_PATH)
    _abi.bind(L)
    _lib = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Handle:
    """What the handle classes share: _h is the library's object (None once closed, or when __init__ did not finish) and
    close() gives it back through the function named _free."""

    _h = _free = None

    def close(self):
        if self._h:
            getattr(lib(), self._free)(self._h)
            self._h = None

    def __del__(self):
        try:                                                     # (interpreter shutdown, or an __init__ that did not finish)
            self.close()
        except Exception:
            pass


def open_handle(fn, *args, err_cap=4096):
    """The *_open entry points that end in (handle** out, char* err, int err_cap): the handle, or LtrError with the library's text."""
    h, err = C.c_void_p(), C.create_string_buffer(err_cap)
    rc = fn(*args, C.byref(h), err, len(err))
    if rc != 0:
        raise LtrError(rc, err.value.decode(errors="replace"))
    return h


def text_call(what, cap, call):
    """The entry points that write text into (char* out, int64 cap) and return its length: call(buf, cap) -> the text, or
    LtrError(the negative status, what)."""
    buf = C.create_string_buffer(cap)
    n = call(buf, cap)
    if n < 0:
        raise LtrError(int(n), what)
    return buf.raw[:n].decode()
