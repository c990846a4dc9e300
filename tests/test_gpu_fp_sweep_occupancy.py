"""The linear-space and traceback flavours of spdp_sweep_fp run five waves per SIMD (32-slot column rings, the feed
and the bottom-row results in one LDS block, 32-bit indices instead of carried 64-bit addresses).  Their results
must stay those of the int32 sweeps of spdp_kernels.hip (SPDP_FP=0), which the four-wave layout matched bit for
bit: on the headline C2 batch (bench.py's 10 000 x 2 kb queries) through the whole alignS_ng ladder and through
the linear-space entry point (scores, cpos rows, ranges), and on the shapes of test_gpu_fp_sweep.py."""
import numpy as np
import pytest

from tests.envknobs import Env as _Env

pytestmark = pytest.mark.gpu


def _problems(batch):
    from spaln_amd import abi
    ps = abi.ProblemSet()
    for w, q, s5, s3, _ in batch:
        ps.add(q, w, s5, s3)
    return ps


def _both(sc, ps, n_im=5):
    from spaln_amd import engine
    out = {}
    for fp in (0, 1):
        with _Env(SPDP_FP=fp, SPDP_CHUNKS=1):
            eng = engine.Engine(0)
            al = [(s, skl.tolist()) for s, skl in eng.align_s(sc, ps)]
            us, ucpos, urng = eng.wip_udh(sc, ps, n_im)
            eng.close()
        out[fp] = (al, us, ucpos, urng)
    return out


def _assert_same(out):
    al0, us0, cp0, rg0 = out[0]
    al1, us1, cp1, rg1 = out[1]
    np.testing.assert_array_equal(us1, us0)
    np.testing.assert_array_equal(cp1, cp0)
    np.testing.assert_array_equal(rg1, rg0)
    assert al1 == al0


def test_five_wave_sweeps_on_the_c2_bench_batch():
    from spaln_amd import defaults, synth
    ps = _problems(synth.make_batch(10000, seed=synth.SEED, intron_hi=20000))
    out = _both(defaults.scoring(), ps)
    _assert_same(out)
    assert sum(1 for s, skl in out[1][0] if len(skl) > 3) > 9000


@pytest.mark.parametrize("shape", [dict(mrna_len=700, n_exons=5, flank=400, intron_hi=1500),
                                   dict(mrna_len=2000, n_exons=8, flank=1000),
                                   dict(mrna_len=333, n_exons=3, flank=77, intron_hi=900)])
def test_five_wave_sweeps_on_the_fp_sweep_shapes(shape):
    from spaln_amd import defaults, synth
    ps = _problems(synth.make_batch(400, seed=4242, **shape))
    _assert_same(_both(defaults.scoring(), ps))


@pytest.mark.parametrize("variant", ["flat", "noll_spj_off"])
def test_five_wave_sweeps_variants(variant):
    """the flat -A3 penalty (a one-entry table) and splice signals off (no table at all)"""
    from spaln_amd import defaults, synth
    sc = defaults.scoring()
    if variant == "flat":
        sc.nquant = 1
    else:
        sc.spj = 0
    ps = _problems(synth.make_batch(200, seed=777, mrna_len=900, n_exons=5, flank=500, intron_hi=3000))
    _assert_same(_both(sc, ps))
