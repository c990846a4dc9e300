"""spdp_chunk_plan (spaln_amd/csrc/spdp_chunk_plan.h): how a batch is cut into the chunks of the software pipeline.  A pure
host function, called here through ctypes on synthetic cell lists; no device is needed."""
import ctypes as C

import numpy as np
import pytest

from spaln_amd import engine

LEAST = 64


def _plan(cells, max_chunks, ratio, min_chunk=0):
    lib = C.CDLL(engine.LIB_PATH)
    lib.spdp_chunk_plan.restype = C.c_int
    lib.spdp_chunk_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p]
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    bounds = np.full(max(1, max_chunks) + 1, -7, dtype=np.int32)
    k = lib.spdp_chunk_plan(cells.ctypes.data, cells.size, max_chunks, ratio, min_chunk, bounds.ctypes.data)
    assert 1 <= k <= max(1, max_chunks)
    return bounds[:k + 1].tolist()


def _cell_lists():
    rng = np.random.default_rng(20261018)
    giant = np.full(1500, 1000, dtype=np.int64)
    giant[700] = 600000
    giant_first = giant.copy()
    giant_first[[0, 700]] = giant_first[[700, 0]]
    return {"equal": np.full(1000, 5000, dtype=np.int64),
            "equal_odd": np.full(1037, 77, dtype=np.int64),
            "span_1_4": rng.integers(1000, 4001, size=2311).astype(np.int64),
            "ascending": np.linspace(1000, 4000, 640).astype(np.int64),
            "descending": np.linspace(4000, 1000, 640).astype(np.int64),
            "giant_middle": giant, "giant_first": giant_first}


CELLS = _cell_lists()


@pytest.mark.parametrize("name", sorted(CELLS))
@pytest.mark.parametrize("ratio", [1.0, 0.7, 0.55, 0.25])
@pytest.mark.parametrize("max_chunks", [2, 3, 4, 6, 8])
def test_plan_invariants(name, ratio, max_chunks):
    cells = CELLS[name]
    b = _plan(cells, max_chunks, ratio)
    k = len(b) - 1
    assert b[0] == 0 and b[-1] == cells.size                            # covers [0, n)
    assert all(b[c + 1] > b[c] for c in range(k))                       # strictly increasing
    assert all(b[c + 1] - b[c] >= LEAST for c in range(k))              # no chunk below 64 problems
    assert k <= max_chunks
    held = [int(cells[b[c]:b[c + 1]].sum()) for c in range(k)]
    one = int(cells.max())
    assert all(held[c + 1] <= held[c] + one for c in range(k - 1)), held   # shares do not grow, up to one problem's cells


@pytest.mark.parametrize("name", ["equal", "span_1_4", "descending", "giant_first"])
@pytest.mark.parametrize("ratio", [0.7, 0.55])
def test_plan_follows_the_ratio(name, ratio):
    """where nothing stands in the way (many problems, none of them dominant past the first chunk) every boundary lies within
    one problem of its geometric target"""
    cells = CELLS[name]
    k = 4
    b = _plan(cells, k, ratio)
    assert len(b) == k + 1
    cum = np.concatenate([[0], np.cumsum(cells)])
    w = ratio ** np.arange(k)
    targets = cum[-1] * np.cumsum(w)[:-1] / w.sum()
    one = int(cells.max())
    for c in range(k - 1):
        assert targets[c] - 0.5 <= cum[b[c + 1]] < targets[c] + one + 0.5, (c, targets[c], cum[b[c + 1]])


def test_one_chunk_where_chunking_is_off_or_the_batch_is_small():
    assert _plan(CELLS["equal"], 1, 0.7) == [0, 1000]
    assert _plan(CELLS["equal"], 0, 0.7) == [0, 1000]
    for n in (1, 63, 64, 127):
        assert _plan(np.full(n, 1000), 8, 0.7) == [0, n]
    assert len(_plan(np.full(128, 1000), 8, 0.7)) == 3                  # 128 is the first size with two chunks of 64
    assert _plan(CELLS["equal"], 6, 0.7, min_chunk=501) == [0, 1000]    # a caller's larger minimum holds too
    b = _plan(CELLS["equal"], 6, 0.7, min_chunk=300)
    assert len(b) == 4 and all(y - x >= 300 for x, y in zip(b[:-1], b[1:]))


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8])
def test_ratio_one_gives_equal_cell_chunks(k):
    n = 1000
    assert _plan(CELLS["equal"], k, 1.0) == [-(-n * c // k) for c in range(k + 1)]   # equal cells: equal counts (rounded up)
    cells = CELLS["span_1_4"]
    b = _plan(cells, k, 1.0)
    assert len(b) == k + 1
    held = [int(cells[b[c]:b[c + 1]].sum()) for c in range(k)]
    # mixed cells: a boundary lies less than one problem past its target, and moves by at most one more problem where the
    # chunk behind it came out larger -- every chunk is within two problems of the equal share
    assert all(abs(h - cells.sum() / k) <= 2 * int(cells.max()) for h in held), held
    assert _plan(cells, k, float("nan")) == b and _plan(cells, k, 0.0) == b and _plan(cells, k, 1.5) == b   # not a ratio: 1


def test_cells_below_one_count_as_one():
    b = _plan(np.zeros(640, dtype=np.int64), 4, 1.0)
    assert b == [0, 160, 320, 480, 640]
    assert _plan(np.full(640, -5, dtype=np.int64), 4, 1.0) == b
