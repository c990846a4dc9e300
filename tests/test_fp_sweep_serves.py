"""Which runs spdp_sweep_fp takes and which stay with the int32 sweeps: spdp_sweep_fp_serves(local, spj, nquant,
pen_cap, llmt), asked without a device.  pen_cap = qm_len[nquant - 2] + 1 is the index of the last entry the kernel's
{A, C} penalty table needs (every longer intron prices alike); the table has 992 entries, entries 0 .. llmt say "no
acceptor yet".  tests/test_gpu_fp_sweep_oracle.py checks on the device that the lengths admitted here really fit."""
import ctypes as C

import pytest

from spaln_amd import engine


@pytest.fixture(scope="module")
def serves():
    fn = C.CDLL(engine.LIB_PATH).spdp_sweep_fp_serves
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 5
    return lambda local=0, spj=1, nquant=5, pen_cap=960, llmt=20: fn(local, spj, nquant, pen_cap, llmt)


def test_default_scoring_is_served(serves):
    from spaln_amd import defaults
    sc = defaults.scoring()
    assert serves(0, sc.spj, sc.nquant, sc.qm_len[sc.nquant - 2] + 1, sc.llmt) == 1


def test_local_ends_are_not_served(serves):
    assert serves(local=1) == 0
    assert serves(local=1, spj=0) == 0
    assert serves(local=1, nquant=1, pen_cap=0) == 0


@pytest.mark.parametrize("nquant, pen_cap, llmt", [(1, 0, 20), (5, 960, 20), (8, 100000, 20), (5, 960, 0), (5, 960, -3),
                                                   (3, 992, 5000), (1, 0, 100000)])
def test_no_splice_signals_no_table(serves, nquant, pen_cap, llmt):
    assert serves(spj=0, nquant=nquant, pen_cap=pen_cap, llmt=llmt) == 1


def test_llmt_below_one_is_turned_away(serves):
    assert serves(llmt=1) == 1
    assert serves(llmt=0) == 0
    assert serves(llmt=-1) == 0
    assert serves(nquant=1, pen_cap=0, llmt=0) == 0
    assert serves(nquant=1, pen_cap=0, llmt=1) == 1


@pytest.mark.parametrize("pen_cap", [0, 991, 992, 30001, 1 << 30])
def test_flat_penalty_ignores_pen_cap(serves, pen_cap):
    assert serves(nquant=1, pen_cap=pen_cap) == 1


@pytest.mark.parametrize("nquant", [2, 5, 8])
def test_table_bound_on_pen_cap(serves, nquant):
    assert serves(nquant=nquant, pen_cap=990) == 1
    assert serves(nquant=nquant, pen_cap=991) == 1
    assert serves(nquant=nquant, pen_cap=992) == 0
    assert serves(nquant=nquant, pen_cap=993) == 0
    assert serves(nquant=nquant, pen_cap=1 << 20) == 0


@pytest.mark.parametrize("nquant, pen_cap", [(1, 0), (1, 5000), (5, 74), (5, 960)])
def test_table_bound_on_llmt(serves, nquant, pen_cap):
    """entries 0 .. llmt + 1 are needed whatever the quantiles say"""
    assert serves(nquant=nquant, pen_cap=pen_cap, llmt=989) == 1          # llmt + 1 = 990
    assert serves(nquant=nquant, pen_cap=pen_cap, llmt=990) == 1          # 991: the last index there is
    assert serves(nquant=nquant, pen_cap=pen_cap, llmt=991) == 0          # 992
    assert serves(nquant=nquant, pen_cap=pen_cap, llmt=100000) == 0
