"""bench.py's one stdout line stays small enough for the driver to parse (round 5's grew to 22 KB and was lost)."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_compact_line_on_a_full_record():
    b = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_line_with_legs.json")))     # a real record with every leg
    assert len(json.dumps(full)) > 20000
    line = b.compact_line(full)
    assert "\n" not in line and len(line) <= b.LINE_LIMIT < 8192
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["value"] == full["value"] and d["ms_per_step"] == full["ms_per_step"]
    assert d["config"]["workload"].startswith("C2")
    rf = d["roofline"]
    assert rf["frac"] == full["roofline"]["frac"] and rf["bound"] == "hbm" and rf["peak"] == 8000.0
    assert rf["traffic"] == full["roofline"]["traffic"] and rf["kernel_ms"] > 0 and rf["valu"]["frac"] > 0
    cb = d["cpu_baseline"]
    assert cb["kind"] == "reference" and cb["cores"] == 16 and cb["value"] > 0
    legs = d["config"]["legs"]
    assert legs["a0"]["value"] == full["config"]["a0"]["value"]
    assert legs["c4_e2e"]["same"] == 9996 and legs["c4_e2e"]["of"] == 10000
    assert legs["dropin_q7_20k"]["Q7"]["x_ref"] > 1.0


def test_compact_line_never_exceeds_the_limit():
    b = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_line_with_legs.json")))
    for i in range(60):                                              # many more legs than exist: the line sheds them, keeps the contract
        full["config"][f"extra_{i}"] = dict(full["config"]["a0"])
    line = b.compact_line(full)
    assert len(line) <= b.LINE_LIMIT
    d = json.loads(line)
    assert d["roofline"]["frac"] and d["cpu_baseline"]["value"] and d["value"]


def test_the_round_record_is_within_the_limit():
    """profiles/r06_bench_legs.json (the full record of the round's last run) through the line builder, and the line kept beside it"""
    b = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_legs.json")))
    line = b.compact_line(full)
    assert len(line) <= b.LINE_LIMIT
    d = json.loads(line)
    assert d["steps"] == 20 and d["warmup"] == 5 and d["roofline"]["frac"] > 0 and d["cpu_baseline"]["kind"] == "reference"
    for leg in ("e2e_q7", "e2e_q7_p", "e2e_q7_s3", "c4_e2e"):
        assert d["config"]["legs"][leg]["same"] == d["config"]["legs"][leg]["of"], leg
    kept = open(os.path.join(ROOT, "profiles", "r06_bench_line.json")).read().strip()
    assert len(kept) <= b.LINE_LIMIT and json.loads(kept)["value"] == full["value"]


def test_a_plain_line_names_no_legs_and_no_record():
    """a run without --full has no legs and writes no full record: its line says neither, and keeps the contract's keys"""
    b = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_line_with_legs.json")))
    for k in list(full["config"]):
        if isinstance(full["config"][k], dict) and k != "with_h2d":
            del full["config"][k]
    full["cpu_baseline"] = None
    d = json.loads(b.compact_line(full, record=None))
    assert "legs" not in d["config"] and "full_record" not in d["config"]
    assert d["value"] == full["value"] and d["ms_per_step"] == full["ms_per_step"] and d["cpu_baseline"] is None
    assert json.loads(b.compact_line(full))["config"]["full_record"] == b.FULL_RECORD


def test_legs_need_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--legs", "c3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_a_plain_run_times_the_steps_and_nothing_else():
    """without --full: no CPU baseline, no upload-inclusive figures, no seeded leg, no legs, no full record written"""
    rec_path = os.path.join(ROOT, "bench_out", "r06_bench_legs.json")
    before = os.stat(rec_path).st_mtime_ns if os.path.exists(rec_path) else None
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--queries", "300"], capture_output=True, text=True, env=env, timeout=550)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["cpu_baseline"] is None and d["config"]["queries_per_gpu"] == 300
    assert not {"legs", "full_record", "queries_per_s_incl_upload", "seeded_q7"} & set(d["config"])
    assert (os.stat(rec_path).st_mtime_ns if os.path.exists(rec_path) else None) == before


def test_dump_outputs_of_an_align_step(tmp_path):
    """--dump-outputs: every query's score and SKL rows as the caller receives them, float64, within the size limit, the
    sample of a large batch fixed by its size alone, the library's arrays freed"""
    import ctypes as C
    import numpy as np
    from spaln_amd import abi
    b = _bench()
    rng = np.random.default_rng(3)
    for n, protein, rows_hi in ((40, False, 30), (b.DUMP_QUERIES + 5, True, 30), (30, False, 400000)):
        arr, keep = (abi.Alignment * n)(), []
        for i in range(n):
            k = int(rng.integers(-2, rows_hi))
            arr[i].score, arr[i].n_skl = 7 * i - 50, k
            if k > 0:
                s = (abi.Skl * k)()
                s_np = np.ctypeslib.as_array(C.cast(s, C.POINTER(C.c_int32)), shape=(k, 2))
                s_np[:, 0], s_np[:, 1] = i, np.arange(k)
                keep.append(s)
                arr[i].skl = C.cast(s, C.POINTER(abi.Skl))
        freed = []
        d = tmp_path / f"d{n}"
        b._dump_alignments(str(d), type("Lib", (), {"spdp_free_alignments": lambda self, a, m: freed.append(m)})(), arr, n, protein)
        assert freed == [n]
        out = {p.stem: np.load(p) for p in d.iterdir()}
        assert set(out) == {"query", "score", "skl", "skl_offset"} | ({"status"} if protein else set())
        assert all(a.dtype == np.float64 for a in out.values())
        assert sum(p.stat().st_size for p in d.iterdir()) <= 64 << 20
        q = out["query"].astype(np.int64)
        assert len(q) == min(n, b.DUMP_QUERIES) or rows_hi > 1000                  # (huge rows: a prefix of the sample)
        assert np.array_equal(q, b._dump_sample(n, b.DUMP_QUERIES)[:len(q)])
        for j, i in enumerate(q):
            k = max(arr[i].n_skl, 0)
            rows = out["skl"][int(out["skl_offset"][j]):int(out["skl_offset"][j + 1])]
            assert out["score"][j] == 7 * i - 50 and rows.shape == (k, 2)
            assert (rows[:, 0] == i).all() and np.array_equal(rows[:, 1], np.arange(k))
            assert not protein or out["status"][j] == min(arr[i].n_skl, 0)
