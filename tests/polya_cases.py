"""The queries the poly-A / poly-T scan is tried on (tests/test_polya_abi.py on the host entry, tests/test_gpu_polya.py on the
device entries), and the rule they are held to, restated here in a few lines from the description of PolyA::rmpolyA: score a
tail from the 3' end, +1 for A and -5 for anything else, remember the first position of the best score above thr, give up once
the score is more than thr below its best; the same for a T head from the 5' end; the better stays, A on ties; a T head turns
the query.  The set is made once and shared."""
import functools

import numpy as np

A, C, G, T, N = 2, 3, 5, 9, 16
# complcod: A <-> T, C <-> G inside every set of bases a code stands for
COMPL = np.array([0, 1, 9, 5, 13, 3, 11, 7, 15, 2, 10, 6, 14, 4, 12, 8, 16], dtype=np.uint8)
LENGTHS = (0, 1, 12, 13, 14, 63, 64, 65, 127, 128, 129, 200, 1000)
PARAMS = [(q_mns, thr) for q_mns in (1, 3) for thr in (12, 5, 0)]


def _one_way(seq, base, thr):
    """-> (best score, step of its first occurrence or None)"""
    score = best = 0
    at = None
    for i, c in enumerate(seq):
        score += 1 if c == base else -5
        if score > best:
            best = score
            at = i if score > thr else at
        if score < best - thr:
            break
    return best, at


def rule(q, q_mns, thr):
    """-> ((pol, tlen, left, right, ori), the normalised query)"""
    q = np.asarray(q, dtype=np.uint8)
    n = len(q)
    if thr <= 0:
        return (0, n, 0, n, q_mns), q
    sa, a = _one_way(q[::-1].tolist(), A, thr)
    st, t = _one_way(q.tolist(), T, thr) if q_mns != 1 else (0, None)
    if a is not None and t is not None:
        if sa >= st:
            t = None
        else:
            a = None
    if a is not None:
        return (1, n - 1 - a, 0, n - 1 - a, q_mns), q
    if t is not None:
        return (2, n - t, 0, n - t, q_mns), COMPL[q[::-1]]
    return (0, n, 0, n, q_mns), q


def _arr(*parts):
    return np.array([c for p in parts for c in p], dtype=np.uint8)


@functools.lru_cache(maxsize=1)
def queries():
    rng = np.random.default_rng(1402)
    acgt = np.array([A, C, G, T], dtype=np.uint8)
    body = lambda n: acgt[rng.integers(0, 4, size=n)]
    inner = lambda n: _arr([C], body(max(n - 2, 0)), [G])          # neither begins with T nor ends with A
    out = []
    # ---- random queries of every length: as they are, with an A tail, a T head, both, and tails with residues knocked out
    for n in LENGTHS:
        for _ in range(60):
            q = body(n)
            k, h = int(rng.integers(0, min(n, 90) + 1)), int(rng.integers(0, min(n, 90) + 1))
            tail, head, both, holes = q.copy(), q.copy(), q.copy(), q.copy()
            tail[n - k:] = A
            head[:h] = T
            both[n - k:] = A
            both[:h] = T
            holes[n - k:] = A
            holes[:h] = T
            for _ in range(3):
                if n:
                    holes[int(rng.integers(0, n))] = acgt[rng.integers(0, 4)]
            out += [q, tail, head, both, holes, COMPL[holes[::-1]]]
    # ---- constructed
    for n in LENGTHS:
        out += [np.full(n, A, np.uint8), np.full(n, T, np.uint8), np.full(n, N, np.uint8)]
    for t in (12, 5):
        for base, turn in ((A, False), (T, True)):
            def put(*tail_parts, front=200):
                """a query whose 3' end reads as given (A tail), or its mirror image with T (T head)"""
                q = _arr(inner(front), *tail_parts)
                out.append(COMPL[q[::-1]] if turn else q)
            run = lambda k: [A] * k
            put(run(t))                                             # exactly thr: no tail
            put(run(t + 1))                                         # one more: a tail
            put(run(16), [C], run(t + 1))                           # a mismatch the tail recovers from ...
            put(run(16), [C], run(t + 1), front=20)
            put(run(20), [C, C, C], run(t + 1))                     # ... and one it does not
            put(run(20), [C], run(2), [C], run(t + 1))
            put([C, C, C], run(5), [C], run(t + 2))                 # the best score reached twice: the first time counts
            put([C, C, C], run(5), [C], run(5), [C], run(t + 2))
            put(run(200), [C, C, C], run(t + 8))                    # nothing behind the break counts, however good
            put(run(70), [C, C], run(70))                           # a dip in the second chunk, the best in the third
            put(run(30), [N], run(30))                              # N and ambiguity codes inside a tail
            put(run(10), [N], run(10))
            put(run(20), list(range(17)), run(t + 1))
            for code in (4, 6, 7, 8, 10, 11, 12, 13, 14, 15):
                put(run(20), [code], run(20))
            for k in (62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 191, 192, 193):     # across the chunk boundaries
                put(run(k))
                put(run(k), front=0)
                put([C, C, C], run(k), front=3)
                put(run(40), [C], run(k - 1))                       # the mismatch right at the boundary
                put(run(40), [C], run(k))
                put(run(5), [C, C, C], run(k))                      # the break right behind it
        # an A tail and a T head together: equal scores (A stays), the T head stronger, the A tail stronger
        for ka, kt in ((20, 20), (20, 25), (25, 20), (t + 1, t + 1), (t + 1, t + 2), (70, 70), (64, 65), (130, 129)):
            out.append(_arr([T] * kt, inner(100), [A] * ka))
            out.append(_arr([T] * kt, [C], [A] * ka))
    return tuple(out)
