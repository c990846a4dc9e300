"""The chunk pipeline of alignS_ng (spdp_host.cpp: align_on_store): a batch cut into chunks by spdp_chunk_plan, the chunks on
two lanes, and the gate between consecutive chunks opened by the linear-space sweep's "all blocks started" signal.  Chunking
enters no per-query computation, so every plan gives the results of the batch in one piece; the gate counters
(spdp_chunk_stats) say which way each gate was opened."""
import os

import numpy as np
import pytest

from tests.envknobs import Env as _Env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = dict(mrna_len=900, n_exons=4, flank=300, intron_hi=2000)
SMALL_VMF = 2 * 1024 * 1024          # below twice the cells of any 900-row problem: every query takes the linear-space branch


def _problems(n, seed):
    from spaln_amd import abi, synth
    ps = abi.ProblemSet()
    for w, q, s5, s3, _ in synth.make_batch(n, seed=seed, **SHAPE):
        ps.add(q, w, s5, s3)
    return ps


class _Run:
    """one engine and one resident batch; align(**knobs) -> ([(score, skl rows)], step stats, chunk counters of the call)"""
    def __init__(self, n, seed, max_vmf_space=None):
        from spaln_amd import defaults, engine
        self.eng = engine.Engine(0)
        sc = defaults.scoring() if max_vmf_space is None else defaults.scoring(max_vmf_space=max_vmf_space)
        self.batch = self.eng.upload(sc, _problems(n, seed))

    def align(self, **knobs):
        self.eng.chunk_stats(reset=True)
        with _Env(**knobs):
            res, _, _ = self.batch.align()
        return [(s, skl.tolist()) for s, skl in res], self.batch.stats(), self.eng.chunk_stats(reset=True).tolist()

    def close(self):
        self.batch.free()
        self.eng.close()


@pytest.fixture(scope="module")
def linear():
    r = _Run(320, 20261, max_vmf_space=SMALL_VMF)
    r.whole = r.align(SPDP_CHUNKS=1)
    yield r
    r.close()


def test_whole_batch_takes_the_linear_space_branch(linear):
    res, stats, cs = linear.whole
    assert stats["udh_cells"] > 0 and stats["udh_problems"] >= 320
    assert cs == [1, 1, 0, 0, 0, 0]                                     # one call, one chunk, no gate
    assert sum(1 for s, skl in res if len(skl) > 3) > 300


@pytest.mark.parametrize("ratio", [1, 0.5])
@pytest.mark.parametrize("chunks", [2, 3, 5])
def test_chunks_give_the_results_of_one_piece(linear, chunks, ratio):
    want, wstats, _ = linear.whole
    got, stats, cs = linear.align(SPDP_CHUNKS=chunks, SPDP_CHUNK_RATIO=ratio)
    assert stats["udh_cells"] > 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, i                                                # score and SKL rows, query for query
    assert len(got) == len(want)
    calls, n_chunks, by_signal, by_event, by_none, once = cs
    print("chunks asked", chunks, "ratio", ratio, "counters", cs)
    assert calls == 1 and 2 <= n_chunks <= chunks


@pytest.mark.parametrize("ratio", [1, 0.5])
@pytest.mark.parametrize("chunks", [2, 3, 5])
def test_gate_accounting(linear, chunks, ratio):
    _, stats, cs = linear.align(SPDP_CHUNKS=chunks, SPDP_CHUNK_RATIO=ratio)
    calls, n_chunks, by_signal, by_event, by_none, once = cs
    print("chunks asked", chunks, "ratio", ratio, "counters", cs)
    assert stats["udh_cells"] > 0
    assert calls == 1 and 2 <= n_chunks <= chunks
    assert once == n_chunks - 1                                         # every chunk but the last opened its gate exactly once
    assert by_signal + by_event == n_chunks - 1                         # .. behind its sweep: every chunk has a linear-space round
    assert by_none == 0
    # the signal rides on 4-wave launches only, and a launch of at most half as many problems as the card has CUs (128 on
    # 256 CUs) runs as 16-wave blocks (DevRun::plan_blocks): of these plans the two-chunk ones are sure to have a first chunk
    # above that (160 queries at ratio 1, more at 0.5) -- there the gate must have been opened by the signal
    if chunks == 2:
        assert (by_signal, by_event) == (1, 0)


def test_forward_only_batch_opens_every_gate_with_nothing_to_wait_for():
    r = _Run(128, 20262)                                                # default MaxVmfSpace: straight to the traceback
    try:
        whole, wstats, _ = r.align(SPDP_CHUNKS=1)
        got, stats, cs = r.align(SPDP_CHUNKS=2)
    finally:
        r.close()
    assert stats["udh_cells"] == 0 and wstats["udh_cells"] == 0 and stats["fwd_problems"] >= 128
    assert got == whole
    assert cs == [1, 2, 0, 0, 1, 1]


def test_launch_without_a_gate_is_unchanged():
    """eng.wip_udh launches the linear-space sweep with no gate attached (null signal pointers): the output recorded from the
    kernels before the signal existed (tests/golden/wip_udh_24q_n3.npz: the 24-query batch of test_gpu_fp_sweep.py, three
    intermediate rows), and no chunk counter moves"""
    from spaln_amd import abi, defaults, engine, synth
    sc = defaults.scoring()
    ps = abi.ProblemSet()
    for w, q, s5, s3, _ in synth.make_batch(24, seed=99, **SHAPE):
        ps.add(q, w, s5, s3)
    want = np.load(os.path.join(ROOT, "tests", "golden", "wip_udh_24q_n3.npz"))
    eng = engine.Engine(0)
    try:
        eng.chunk_stats(reset=True)
        for fp in (1, 0):                                               # spdp_sweep_fp.hip, spdp_kernels.hip
            with _Env(SPDP_FP=fp):
                us, ucpos, urng = eng.wip_udh(sc, ps, 3)
            assert np.array_equal(us, want["scores"]) and np.array_equal(ucpos, want["cpos"]) and np.array_equal(urng, want["ranges"])
        assert eng.chunk_stats().tolist() == [0] * 6
    finally:
        eng.close()
