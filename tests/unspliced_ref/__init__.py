"""ctypes loader of the unspliced aligner's restatement (unspliced_ref.c), compiled on first use.  TEST INFRASTRUCTURE ONLY:
the product package never imports this module."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from spaln_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


class Stat(C.Structure):
    _fields_ = [("val", C.c_int32), ("mch", C.c_int32), ("mmc", C.c_int32), ("gap", C.c_float), ("unp", C.c_float),
                ("span", C.c_int32)]


def build() -> str:
    src = os.path.join(_HERE, "unspliced_ref.c")
    hdr = os.path.join(_HERE, "..", "..", "include")
    where = _HERE if os.access(_HERE, os.W_OK) else tempfile.gettempdir()
    so = os.path.join(where, "libunspliced_ref.so")
    newest = max(os.path.getmtime(src), os.path.getmtime(os.path.join(hdr, "spdp.h")))
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        tmp = f"{so}.{os.getpid()}.tmp"          # several test processes may get here at once: build aside, swap in
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I", hdr, "-o", tmp, src])
        os.replace(tmp, so)
    return so


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.ubr_cells.restype = C.c_int64
    return _lib


def stripe(p: abi.Problem, sh: int) -> abi.Window:
    w = abi.Window()
    lib().ubr_stripe(C.byref(p), C.c_int(sh), C.byref(w))
    return w


def cells(p: abi.Problem, sh: int) -> int:
    w = stripe(p, sh)
    return int(lib().ubr_cells(C.byref(p), C.byref(w)))


def align(sc, up, p):
    """globalB_ng: (score, skl) with skl = header row + corners ((0, 2) array when there is no alignment)"""
    cap = 2 * (p.a_len + p.b_len) + 16
    out = np.zeros((cap, 2), dtype=np.int32)
    score = C.c_int32(0)
    k = lib().ubr_align(C.byref(sc), C.byref(up), C.byref(p), out.ctypes.data_as(C.c_void_p), C.c_int(cap), C.byref(score))
    return int(score.value), out[:k].copy()


def scorealone(sc, up, p) -> int:
    return int(lib().ubr_scorealone(C.byref(sc), C.byref(up), C.byref(p)))


def rescore(sc, up, p, skl, fmt=0):
    """skl_rngB_ng: (stat dict, trimmed corners, edit records (k x 3), sam fields)"""
    skl = np.ascontiguousarray(skl, dtype=np.int32).reshape(-1, 2)
    st = Stat()
    cap = 2 * skl.shape[0] + 8
    ed = np.zeros((cap, 3), dtype=np.int32)
    sam = np.zeros(5, dtype=np.int32)
    trimmed = np.zeros((max(skl.shape[0], 1), 2), dtype=np.int32)
    nt = C.c_int32(0)
    ne = lib().ubr_rescore(C.byref(sc), C.byref(up), C.byref(p), skl.ctypes.data_as(C.c_void_p), C.c_int(skl.shape[0]), C.byref(st),
                           C.c_int(fmt), ed.ctypes.data_as(C.c_void_p), C.c_int(cap), sam.ctypes.data_as(C.c_void_p),
                           trimmed.ctypes.data_as(C.c_void_p), C.byref(nt))
    assert ne <= cap
    stat = dict(val=st.val, mch=st.mch, mmc=st.mmc, gap=st.gap, unp=st.unp, span=st.span)
    return stat, trimmed[:nt.value].copy(), ed[:ne].copy(), sam.tolist()
