"""The chunk lanes of alignS_ng with blocking copies that wait for their own stream only (spdp_host.cpp: align_on_store,
SPDP_CHUNK_LANE_COPIES; spdp_internal.h: spdp_copy_sync).  A chunk's read-backs, slab sweeps and walk then run beside the next
chunk's linear-space sweep, and a lane's later rounds under the other lane's sweep.  No per-query computation depends on
that order, so every plan, with the knob on or off, gives the results of the batch in one piece; the gate counters
(spdp_chunk_stats) say that every gate was opened, and once.

Shapes: a few hundred 900-row queries under a MaxVmfSpace small enough that each takes the linear-space branch (as
tests/test_gpu_chunk_handover.py); no chunk is smaller than 64 problems (SPDP_CHUNK_LEAST), so 320 queries give up to four
chunks, i.e. both lanes run two chunks each.  SPDP_CHUNK_TEST_LAST cuts the last chunk down to one problem."""
import numpy as np
import pytest

from tests.envknobs import Env as _Env

pytestmark = pytest.mark.gpu

SHAPE = dict(mrna_len=900, n_exons=4, flank=300, intron_hi=2000)
SMALL_VMF = 2 * 1024 * 1024          # below twice the cells of any 900-row problem: every query takes the linear-space branch
TINY_VMF = 256 * 1024                # .. and below those of the slabs of a 3000-row query: a second linear-space round


def _problem_set(batches):
    from spaln_amd import abi
    ps = abi.ProblemSet()
    for b in batches:
        for w, q, s5, s3, _ in b:
            ps.add(q, w, s5, s3)
    return ps


class _Run:
    """one engine and one resident batch; align(**knobs) -> ([(score, skl rows)], step stats, chunk counters of the call)"""
    def __init__(self, batches, **scoring):
        from spaln_amd import defaults, engine
        self.eng = engine.Engine(0)
        self.sc = defaults.scoring(**scoring)
        self.ps = _problem_set(batches)
        self.batch = self.eng.upload(self.sc, self.ps)

    def align(self, **knobs):
        self.eng.chunk_stats(reset=True)
        with _Env(**knobs):
            res, _, _ = self.batch.align()
        return [(s, skl.tolist()) for s, skl in res], self.batch.stats(), self.eng.chunk_stats(reset=True).tolist()

    def close(self):
        self.batch.free()
        self.eng.close()


def _check_gates(cs, asked, all_linear=True):
    """every gate opened, by the signal, the event or (a chunk without a linear-space round) with nothing to wait for; none twice"""
    calls, n_chunks, by_signal, by_event, by_none, once = cs
    assert calls == 1 and 1 <= n_chunks <= asked
    assert by_signal + by_event + by_none == n_chunks - 1
    assert once == n_chunks - 1
    if all_linear:
        assert by_none == 0
    return n_chunks


@pytest.fixture(scope="module")
def linear():
    from spaln_amd import synth
    r = _Run([synth.make_batch(320, seed=20271, **SHAPE)], max_vmf_space=SMALL_VMF)
    r.whole = r.align(SPDP_CHUNKS=1)
    yield r
    r.close()


def test_whole_batch_is_linear_space_and_a_sample_is_the_oracles(linear):
    from oracle import host_logic
    res, stats, cs = linear.whole
    assert stats["udh_cells"] > 0 and stats["udh_problems"] >= 320
    assert cs == [1, 1, 0, 0, 0, 0]
    for i in (0, 63, 64, 200, 319):                                     # (the first and the last of chunks, and one inside)
        ws, wskl = host_logic.align_s(linear.sc, linear.ps.items[i])
        assert res[i][0] == ws and np.asarray(res[i][1]).ravel().tolist() == (wskl or []), i


@pytest.mark.parametrize("own", [1, 0])
@pytest.mark.parametrize("ratio", [1, 0.55])
@pytest.mark.parametrize("chunks", [1, 2, 3, 4])
def test_results_of_one_piece(linear, chunks, ratio, own):
    want, _, _ = linear.whole
    got, stats, cs = linear.align(SPDP_CHUNKS=chunks, SPDP_CHUNK_RATIO=ratio, SPDP_CHUNK_LANE_COPIES=own)
    print("chunks asked", chunks, "ratio", ratio, "own-stream copies", own, "counters", cs)
    assert stats["udh_problems"] >= 320
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, i                                                # score and SKL rows, query for query
    n_chunks = _check_gates(cs, chunks)
    assert n_chunks >= min(chunks, 2)
    if ratio == 1:
        assert n_chunks == chunks                                       # 320 equal-sized queries, at least 64 a chunk: as asked;
                                                                        # at four, both lanes run two chunks each


@pytest.mark.parametrize("own", [1, 0])
@pytest.mark.parametrize("chunks", [2, 3, 4])
def test_last_chunk_of_one_problem(linear, chunks, own):
    want, _, _ = linear.whole
    got, stats, cs = linear.align(SPDP_CHUNKS=chunks, SPDP_CHUNK_TEST_LAST=1, SPDP_CHUNK_LANE_COPIES=own)
    print("chunks asked", chunks, "own-stream copies", own, "counters", cs)
    assert got == want
    n_chunks = _check_gates(cs, chunks)
    assert n_chunks >= 2
    assert stats["udh_rounds"] >= n_chunks                              # the lone problem had a linear-space round of its own


@pytest.mark.parametrize("own", [1, 0])
def test_reuse_of_pools_and_staging(linear, own):
    """the same Batch three times in a row under one chunked plan, as bench.py runs it, then under other chunk counts, back,
    and in one piece: pools, staging and signal words are reused, the results identical each time"""
    want, _, _ = linear.whole
    plans = [dict(SPDP_CHUNKS=2)] * 3 + [dict(SPDP_CHUNKS=4), dict(SPDP_CHUNKS=3), dict(SPDP_CHUNKS=2, SPDP_CHUNK_RATIO=0.55),
                                        dict(SPDP_CHUNKS=4), dict(SPDP_CHUNKS=2)]
    for knobs in plans:
        got, _, cs = linear.align(SPDP_CHUNK_LANE_COPIES=own, **knobs)
        assert got == want, knobs
        assert _check_gates(cs, knobs["SPDP_CHUNKS"]) == (knobs["SPDP_CHUNKS"] if "SPDP_CHUNK_RATIO" not in knobs else 2), knobs
    got, _, cs = linear.align()                                         # no knob: 320 queries are below the default's 4096, one chunk
    assert got == want and cs == [1, 1, 0, 0, 0, 0]


def test_traceback_half_and_linear_space_half():
    """default MaxVmfSpace; the first half (900 rows) goes straight to the traceback, the second half (2000 rows against
    windows of some 20 kb) takes the linear-space branch: one lane fetches and sweeps slabs while the other is in its sweep"""
    from spaln_amd import synth
    short = synth.make_batch(128, seed=20272, **SHAPE)
    long_ = synth.make_batch(128, seed=20273, mrna_len=2000, n_exons=8, flank=1000, intron_lo=1500, intron_hi=3000)
    r = _Run([short, long_])
    try:
        want, wstats, _ = r.align(SPDP_CHUNKS=1)
        assert wstats["udh_problems"] == 128 and wstats["fwd_problems"] > 128
        assert all(len(skl) > 3 for _, skl in want[128:])
        for chunks in (2, 3, 4):
            for own in (1, 0):
                got, stats, cs = r.align(SPDP_CHUNKS=chunks, SPDP_CHUNK_LANE_COPIES=own)
                print("chunks asked", chunks, "own-stream copies", own, "counters", cs)
                assert got == want, (chunks, own)
                assert stats["udh_problems"] == 128
                assert _check_gates(cs, chunks, all_linear=False) >= 2
    finally:
        r.close()


def test_second_round_of_the_ladder():
    """one 3000-row query among 900-row ones and a MaxVmfSpace of 256 KiB: slabs are linear-space problems themselves, so a
    lane's later rounds -- launches no gate holds back -- run under the other lane's sweep"""
    from spaln_amd import synth
    from oracle import host_logic
    first = synth.make_batch(100, seed=20274, **SHAPE)
    tall = synth.make_batch(1, seed=20275, mrna_len=3000, n_exons=6, flank=300, intron_hi=2000)
    rest = synth.make_batch(155, seed=20276, **SHAPE)
    r = _Run([first, tall, rest], max_vmf_space=TINY_VMF)
    try:
        want, wstats, _ = r.align(SPDP_CHUNKS=1)
        assert wstats["udh_rounds"] >= 2 and wstats["udh_problems"] > 256
        ws, wskl = host_logic.align_s(r.sc, r.ps.items[100])
        assert want[100][0] == ws and np.asarray(want[100][1]).ravel().tolist() == (wskl or [])
        for chunks, ratio in ((2, 1), (3, 1), (4, 1), (4, 0.55)):
            for own in (1, 0):
                got, stats, cs = r.align(SPDP_CHUNKS=chunks, SPDP_CHUNK_RATIO=ratio, SPDP_CHUNK_LANE_COPIES=own)
                print("chunks asked", chunks, "ratio", ratio, "own-stream copies", own, "counters", cs)
                assert got == want, (chunks, ratio, own)
                assert stats["udh_rounds"] >= wstats["udh_rounds"] + _check_gates(cs, chunks) - 1
    finally:
        r.close()
