"""Problems and corner lists for the rescoring walks (spdp_skl_rng_s = skl_rngS_ng, spdp_skl_rng_h = skl_rngH_ng), shared by
tests/test_rescore_cases.py (generator + oracle, CPU) and tests/test_gpu_rescore.py (kernels against the oracle).

Sequences come from spaln_amd/synth.py (planted genes, synthetic signal tables); the corner lists are built by recipe, one
name per recipe, from a path of segments: ("M", d) a diagonal run, ("D", k) k genomic positions without a query residue (the
walks' `insert`), ("I", k) k query residues without a genomic position (`deletn`).  A walk scores whatever monotone corner list it
is given, so a recipe is free to put gaps and introns where it wants them and to plant the signal values that decide a
comparison.  Everything is a function of the seeds written here.

The scoring parameters are the ones two fixtures carry (s1_basic, h1_400aa: data read back from the reference); the protein
intron-length table is continued with its last value to cover the long regions of the window recipe.

Kept away from, because no fixture written by the reference pins these branches of the oracle (tests/test_oracle_rescore_census.py):
the GTGT....AGAG junction (both phase marks 2), a terminal gap in front of a stop codon, and a cDNA list whose
first two corners share n under b_exgl."""
import dataclasses
import functools

import numpy as np

from spaln_amd import abi, defaults, synth
from tests import spdg
from tests.conftest import golden_files

NEVSEL = abi.NEVSEL
JNEIBR = (1, 2, 10, 32)
F = {k: i for i, k in enumerate(["left", "right", "rleft", "rright", "mch", "mmc", "gap", "unp", "mch5", "mmc5", "gap5", "unp5",
                                 "mch3", "mmc3", "gap3", "unp3", "phs", "escr", "iscr", "sig3", "sig5"])}


def _fixture(prefix, name):
    return spdg.load([f for f in golden_files(prefix) if f.endswith(name + ".spdg")][0])


# ---- the two parameter sets -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def params_s():
    """(fixture, Scoring, rescoring keywords) of the cDNA walk; codonk1 is `never` there, the "k1" variant sets it to 7"""
    fx = _fixture("s1_", "s1_basic")
    intpen, t53 = defaults.exact_tables()
    return fx, spdg.scoring(fx, intpen=intpen, t53=t53), dict(codonk1=fx["prm"]["codonk1"], minl=fx["prm"]["minl"], lsg=1)


@functools.lru_cache(maxsize=None)
def params_h(codonk1=None):
    """(Scoring, oracle keywords without jneibr) of the protein walk"""
    fx = _fixture("h1_", "h1_400aa")
    h = dict(zip(spdg.HPARAM_NAMES, (int(x) for x in fx["hparams"])))
    rp = [int(x) for x in fx["rparams"]]
    intpen = np.concatenate([fx["intpen"], np.full(12400 - fx["intpen"].size, fx["intpen"][-1], dtype=fx["intpen"].dtype)])
    sc = spdg.scoring_h(fx, intpen=intpen, **({} if codonk1 is None else dict(codonk1=codonk1)))     # (`never` in the fixture)
    kw = dict(intpen=intpen, t53=fx["t53"], lgop=fx["prm"]["lgop"], diffu=rp[0], k1=h["k1"], gape1=h["gape1"], gape2=h["gape2"],
              extragop=h["extragop"], minl=fx["prm"]["minl"], lcl=h["lcl"], lsg=rp[5], sup_tcodon=0, many=rp[3])
    return sc, kw


# ---- cases ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    walk: str                   # "s" cDNA, "h" protein
    recipe: str
    name: str
    arrays: dict                # what ProblemSet(.H).add takes by keyword
    rng: tuple                  # a_left, a_right, b_left, b_right
    exg: tuple
    corners: list               # [(m, n)] or None: the aligners make the list
    kw: dict                    # keywords of the walk that are not the scoring bundle's (jneibr, codonk1, ...)
    info: dict = dataclasses.field(default_factory=dict)      # what the recipe promises (tests/test_rescore_cases.py checks it)

    def flat(self):
        """the list as align_s / align_h return it: [flags, n, m1, n1, ...]"""
        return [1, len(self.corners)] + [int(x) for mn in self.corners for x in mn]

    def rows(self):
        """... and as the engine wrappers take it: rows of (m, n) with the header row first"""
        return np.array(self.flat(), dtype=np.int32).reshape(-1, 2)

    def add_to(self, ps):
        a = self.arrays
        if self.walk == "s":
            p = ps.add(a["a"], a["b"], a["sig5"], a["sig3"], *self.rng, self.exg, cano5=a["cano5"], cano3=a["cano3"], dinc=a["dinc"])
        else:
            p = ps.add(a["a"], a["b"], a["sig5"], a["sig3"], a["sigS"], a["sigT"], a["sigE"], a["phs5"], a["phs3"], *self.rng, self.exg,
                       dinc=a["dinc"])
        return p

    def variant(self, name, pos, delta):
        """the same case with arrays[name][pos] moved by delta (the two sides of a planted tie)"""
        arr = dict(self.arrays)
        arr[name] = arr[name].copy()
        arr[name][pos] += delta
        return dataclasses.replace(self, arrays=arr)


def oracle_of(case, corners=None):
    """(score, fstat[5], records) of the oracle's restatement for one case"""
    from oracle import host_logic, host_logic_h
    flat = case.flat() if corners is None else [1, len(corners)] + [int(x) for mn in corners for x in mn]
    if case.walk == "s":
        _, sc, _ = params_s()
        ps = abi.ProblemSet()
        return host_logic.skl_rng_s(sc, case.add_to(ps), flat, **case.kw)
    sc, kw = params_h(case.kw.get("codonk1"))
    ps = abi.ProblemSetH()
    own = {k: v for k, v in case.kw.items() if k != "codonk1"}          # (the walk reads codonk1 from the scoring bundle)
    return host_logic_h.skl_rng_h(sc, case.add_to(ps), flat, dinc=case.arrays["dinc"], **{**kw, **own})


def corners_of(path, m0, n0, condensed=False, step=lambda op, k: {"M": (k, k), "D": (0, k), "I": (k, 0)}[op]):
    """the corner list of a path; condensed: without the corner where a diagonal run turns into a gap (the walks take a run and the
    gap behind it in one step)"""
    pts, m, n = [(m0, n0)], m0, n0
    for op, k in path:
        dm, dn = step(op, k)
        m, n = m + dm, n + dn
        pts.append((m, n))
    if condensed:
        drop = {j + 1 for j in range(len(path) - 1) if path[j][0] == "M" and path[j + 1][0] in "DI"}
        pts = [p for j, p in enumerate(pts) if j not in drop]
    return pts


def _span(path):
    return (sum(k for op, k in path if op in "MI"), sum(k for op, k in path if op in "MD"))


# ---- cDNA -------------------------------------------------------------------------------------------------------------------------
def _plant_s(rng, exon_lens, intron_lens, flank, extra_query=0):
    """window = flank, exons separated by GT....AG introns, flank; query = a random sequence long enough for the paths laid over it
    (rescoring scores what it is given; matches and mismatches both occur)"""
    parts, exons, pos = [synth.random_dna(rng, flank)], [], flank
    for k, L in enumerate(exon_lens):
        parts.append(synth.random_dna(rng, L))
        exons.append((pos, pos + L))
        pos += L
        if k < len(intron_lens):
            parts.append(synth._intron(rng, intron_lens[k]))
            pos += intron_lens[k]
    parts.append(synth.random_dna(rng, flank))
    window = np.concatenate(parts)
    tr = np.concatenate([window[s:e] for s, e in exons])
    hit = rng.random(tr.size) < 0.15
    tr = tr.copy()
    tr[hit] = synth.random_dna(rng, int(hit.sum()))
    query = np.concatenate([tr, synth.random_dna(rng, extra_query)])
    s5, s3 = synth.splice_signals(window)
    b = defaults.encode(window)
    arrays = dict(a=defaults.encode(query), b=b, sig5=s5.copy(), sig3=s3.copy(), **synth.exact_inputs(b))
    return arrays, exons


def _xi_s(arrays, n, n3):
    """sig5 + spjscr of the cDNA walk for an intron n .. n3"""
    _, sc, _ = params_s()
    intpen, t53 = defaults.exact_tables()
    d = arrays["dinc"]
    return int(arrays["sig5"][n]) + int(intpen[n3 - n]) + int(arrays["sig3"][n3]) + int(t53[16 * (d[n] >> 4) + (d[n3] & 15)])


def gap_penalty_s(i, codonk1):
    _, sc, _ = params_s()
    return 0 if i == 0 else (sc.lgop + i * sc.lgep if i > codonk1 else sc.gop + i * sc.gep)


def _case_s(recipe, name, arrays, path, m0, n0, *, jneibr=5, exg=(0, 0, 0, 0), condensed=False, codonk1=None, rng_pad=(0, 0, 0, 0), info=None):
    _, _, kw = params_s()
    kw = dict(kw, jneibr=jneibr)
    if codonk1 is not None:
        kw["codonk1"] = codonk1
    am, bn = _span(path)
    rng = (m0 - rng_pad[0], m0 + am + rng_pad[1], n0 - rng_pad[2], n0 + bn + rng_pad[3])
    assert 0 <= rng[0] and rng[1] <= arrays["a"].size and 0 <= rng[2] and rng[3] <= arrays["b"].size, (name, rng)
    info = dict(info or {})
    info.setdefault("candidates", sum(1 for op, k in path if op == "D" and k > kw["minl"]))
    info["path"] = path
    return Case("s", recipe, name, arrays, rng, tuple(exg), corners_of(path, m0, n0, condensed), kw, info)


def _gene_path(exons, rng=None, indels=0):
    """M over every exon, D over every intron; `indels` short gaps dropped into the exons"""
    path = []
    for k, (s, e) in enumerate(exons):
        L, cut = e - s, []
        if rng is not None and indels and L > 12:
            cut = sorted(int(x) for x in rng.choice(np.arange(3, L - 3), size=min(indels, (L - 6) // 4), replace=False))
        at = 0
        for c in cut:
            if c - at < 2:
                continue
            path.append(("M", c - at))
            g = int(rng.integers(1, 4))
            path.append(("D", g) if rng.random() < 0.5 else ("I", g))
            at = c + (g if path[-1][0] == "D" else 0)
            if at >= L - 1:
                break
        if L - at > 0:
            path.append(("M", L - at))
        if k + 1 < len(exons):
            path.append(("D", exons[k + 1][0] - e))
    # the genomic span must stay the exons' + introns': a D inside an exon shortens the run behind it (done above through `at`)
    return path


def _cases_s():
    out = []
    rng = np.random.default_rng(synth.SEED + 5101)
    # corner forms: the same path with every corner and condensed
    for k in range(12):
        ne = int(rng.integers(2, 6))
        lens = [int(x) for x in rng.integers(12, 60, size=ne)]
        arrays, exons = _plant_s(rng, lens, [int(x) for x in rng.integers(60, 400, size=ne - 1)], int(rng.integers(20, 200)), extra_query=40)
        path = _gene_path(exons, rng, indels=2)
        jn = JNEIBR[k % 4]
        for cond in (False, True):
            out.append(_case_s("forms", f"forms{k}{'c' if cond else 'f'}", arrays, path, 0, exons[0][0], jneibr=jn, condensed=cond,
                               info=dict(twin=f"forms{k}f")))
    # condensed at the bound: every step closes an exon (records = corners)
    for k, ne in enumerate((3, 6, 9, 14)):
        arrays, exons = _plant_s(rng, [int(x) for x in rng.integers(8, 24, size=ne)], [int(x) for x in rng.integers(60, 120, size=ne - 1)], 30)
        out.append(_case_s("bound", f"bound{k}", arrays, _gene_path(exons), 0, exons[0][0], jneibr=JNEIBR[k % 4], condensed=True,
                           info=dict(records=ne + 1)))
    # ties
    for k in range(12):
        jn = JNEIBR[k % 4]
        k1, k2 = int(rng.integers(3, 25)), int(rng.integers(60, 200))
        # xi == x (tested by >=): a short deletion, then an intron candidate, then the run that closes them
        arrays, exons = _plant_s(rng, [40, 40], [k1 + k2], 50)
        n = exons[0][1]
        want = gap_penalty_s(k1 + k2, 1 << 30) - gap_penalty_s(k1, 1 << 30)            # = rb[ISCR] at the tie
        arrays["sig5"][n + k1] += want - _xi_s(arrays, n + k1, n + k1 + k2)
        out.append(_case_s("tie_x", f"tie_x{k}", arrays, [("M", 40), ("D", k1), ("D", k2), ("M", 40)], 0, exons[0][0], jneibr=jn,
                           info=dict(tie=("sig5", n + k1), accepted_at=0, iscr=want)))
        # xi == gap_penalty(i): not a candidate
        arrays, exons = _plant_s(rng, [40, 40], [k2], 50)
        n = exons[0][1]
        arrays["sig5"][n] += gap_penalty_s(k2, 1 << 30) - _xi_s(arrays, n, n + k2)
        out.append(_case_s("tie_gap", f"tie_gap{k}", arrays, [("M", 40), ("D", k2), ("M", 40)], 0, exons[0][0], jneibr=jn,
                           info=dict(tie=("sig5", n), accepted_at=1)))
        # xi == rb[ISCR]: a second candidate behind a pending one, with the same score
        k3 = int(rng.integers(60, 200))
        arrays, exons = _plant_s(rng, [40, 40], [k2 + k3], 50)
        n = exons[0][1]
        arrays["sig5"][n + k2] += _xi_s(arrays, n, n + k2) - _xi_s(arrays, n + k2, n + k2 + k3)
        out.append(_case_s("tie_iscr", f"tie_iscr{k}", arrays, [("M", 40), ("D", k2), ("D", k3), ("M", 40)], 0, exons[0][0], jneibr=jn,
                           info=dict(tie=("sig5", n + k2), accepted_at=1)))
    # two deletions in a row (preint > 0); a deletion of minl and of minl + 1; gaps of codonk1 and codonk1 + 1
    minl = params_s()[2]["minl"]
    for k in range(8):
        k1 = int(rng.integers(2, minl))
        arrays, exons = _plant_s(rng, [30, 30], [k1 + 90], 40)
        out.append(_case_s("two_del", f"two_del{k}", arrays, [("M", 30), ("D", k1), ("D", 90), ("M", 30)], 0, exons[0][0], jneibr=JNEIBR[k % 4]))
        for L in (minl, minl + 1):
            arrays, exons = _plant_s(rng, [30, 30], [L], 40)
            arrays["sig5"][exons[0][1]] = 300                     # a candidate as soon as the length allows it
            arrays["sig3"][exons[0][1] + L] = 300
            out.append(_case_s("minl", f"minl{k}_{L}", arrays, [("M", 30), ("D", L), ("M", 30)], 0, exons[0][0], jneibr=JNEIBR[k % 4],
                               info=dict(records=2 + (L > minl))))
        for g in (7, 8):
            arrays, exons = _plant_s(rng, [60], [], 40, extra_query=20)
            s = exons[0][0]
            out.append(_case_s("codonk1", f"codonk1_{k}_{g}", arrays, [("M", 20), ("D", g), ("M", 15), ("I", g), ("M", 25 - g)], 0, s,
                               jneibr=JNEIBR[k % 4], codonk1=7, info=dict(gap=g)))
    # candidates at places without signals, short enough for the gap to be the cheaper reading: rejected
    for k in range(10):
        arrays, exons = _plant_s(rng, [200], [], 40)
        g = [int(x) for x in rng.integers(minl + 1, minl + 8, size=3)]
        for x in (25, 25 + g[0] + 25, 25 + g[0] + 25 + g[1] + 25):
            arrays["sig5"][exons[0][0] + x] = -400
        path = [("M", 25), ("D", g[0]), ("M", 25), ("D", g[1]), ("M", 25), ("D", g[2]), ("M", 200 - 75 - sum(g))]
        out.append(_case_s("rejected", f"rejected{k}", arrays, path, 0, exons[0][0], jneibr=JNEIBR[k % 4], condensed=bool(k % 2),
                           info=dict(records=2)))
    # exons of jneibr - 1, jneibr, jneibr + 1 aligned positions, first, inner and last
    for jn in JNEIBR:
        for d in (-1, 0, 1):
            L = jn + d
            if L < 1:
                continue
            for where in range(3):
                lens = [45, 45, 45]
                lens[where] = L
                arrays, exons = _plant_s(rng, lens, [80, 95], 30)
                out.append(_case_s("jneibr", f"jn{jn}_{L}_{where}", arrays, _gene_path(exons), 0, exons[0][0], jneibr=jn,
                                   info=dict(records=4, exon=where, exon_len=L)))
    # end gaps: every flag set; a gap at the range's end, and one position inside it
    for flags in range(16):
        exg = (flags & 1, flags >> 1 & 1, flags >> 2 & 1, flags >> 3 & 1)
        for v in range(4):
            arrays, exons = _plant_s(rng, [50, 40], [120], 40, extra_query=30)
            s = exons[0][0]
            g = int(rng.integers(1, 9))
            inner = [("M", 50 - 8), ("D", 120), ("M", 40)]
            # v 0 / 1: a genomic gap at the query's ends (a_exg*), flush and one residue in; v 2 / 3: a query gap at the window's
            # ends (b_exg*); a query gap flush with b_left under b_exgl is the unpinned branch (module docstring): one position in
            head = {0: [("D", g)], 1: [("M", 1), ("D", g)], 2: [("M", 1), ("I", g)] if exg[2] else [("I", g)], 3: [("M", 1), ("I", g)]}[v]
            tail = {0: [("D", g)], 1: [("D", g), ("M", 1)], 2: [("I", g)], 3: [("I", g), ("M", 1)]}[v]
            path = head + [("M", 8 - sum(k for op, k in head if op == "M"))] + inner[:-1] + [("M", 40 - sum(k for op, k in tail if op == "M"))] + tail
            gd = g if v < 2 else 0
            out.append(_case_s("end_gaps", f"exg{flags}_{v}", arrays, path, 0, s - gd, jneibr=JNEIBR[(flags + v) % 4], exg=exg,
                               info=dict(flags=flags)))
    # the aligners' own lists: the problems only
    for k in range(10):
        g = synth.make_gene(rng, n_exons=int(rng.integers(1, 5)), mrna_len=int(rng.integers(30, 300)), flank=int(rng.integers(40, 300)),
                            intron_lo=60, intron_hi=500, sub=0.04, indel=0.01, exon_min=10)
        s5, s3 = synth.splice_signals(g.window)
        b = defaults.encode(g.window)
        arrays = dict(a=defaults.encode(g.query), b=b, sig5=s5, sig3=s3, **synth.exact_inputs(b))
        _, _, kw = params_s()
        out.append(Case("s", "aligner", f"aligner{k}", arrays, (0, arrays["a"].size, 0, b.size), (1, 1, 1, 1), None,
                        dict(kw, jneibr=JNEIBR[k % 4])))
    return out


# ---- protein ----------------------------------------------------------------------------------------------------------------------
def _plant_h(rng, aa_len, n_exons, flank, intron_hi=300):
    g = synth.make_protein_gene(rng, n_exons=n_exons, aa_len=aa_len, flank=flank, sub=0.15, intron_lo=60, intron_hi=intron_hi)
    sg = synth.protein_signals(g.window, rng)
    arrays = dict(a=synth.encode_protein(g.query), dinc=synth.exact_inputs(defaults.encode(g.window))["dinc"], **sg)
    return arrays, g.exons


def _gene_corners_h(arrays, exons, condensed=False):
    """the corners of the planted structure: a junction behind p bases of a split codon sits at the donor (p = 0), one base before it
    (p = 1: phase -1) or one base behind it (p = 2: phase 1, the codon the run matched last is re-scored from its two halves)"""
    m, n = 0, exons[0][0]
    pts = [(m, n)]
    cds = 0
    for k, (s, e) in enumerate(exons):
        last = k + 1 == len(exons)
        cds_end = cds + (e - s) - (3 if last else 0)            # (the stop codon stays out of the alignment)
        if last:
            m_end, n_end = cds_end // 3, e - 3
        else:
            p = cds_end % 3
            m_end = cds_end // 3 + (1 if p == 2 else 0)
            n_end = e - p if p < 2 else e + 1
        if not condensed or last:
            pts.append((m_end, n_end))
        if not last:
            pts.append((m_end, n_end + exons[k + 1][0] - e))
        cds = cds_end
    return pts


def _phase2_free(arrays, corners):
    p5, p3 = arrays["phs5"], arrays["phs3"]
    for (m0, n0), (m1, n1) in zip(corners, corners[1:]):
        if m1 == m0 and p5[n0] == 2 and p3[n1] == 2:
            return False
    return True


def _case_h(recipe, name, arrays, corners, *, jneibr=5, exg=(0, 0, 0, 0), rng=None, info=None, codonk1=None, sup_tcodon=None):
    assert _phase2_free(arrays, corners), name
    rng = rng or (corners[0][0], corners[-1][0], corners[0][1], corners[-1][1])
    b_len = arrays["b"].size - 1
    assert 0 <= rng[0] and rng[1] <= arrays["a"].size and 0 <= rng[2] and rng[3] <= b_len, (name, rng)
    kw = dict(jneibr=jneibr) if codonk1 is None else dict(jneibr=jneibr, codonk1=codonk1)
    if sup_tcodon is not None:
        kw["sup_tcodon"] = sup_tcodon
    return Case("h", recipe, name, arrays, tuple(rng), tuple(exg), [tuple(int(x) for x in c) for c in corners], kw, dict(info or {}))


def _step_h(op, k):
    """protein paths: M k codons; D k nucleotides; I k nucleotides of query (k = 3 q + r: q + 1 residues over 3 - r positions when r)"""
    if op == "M":
        return (k, 3 * k)
    if op == "D":
        return (0, k)
    return (k // 3, 0) if k % 3 == 0 else (k // 3 + 1, 3 - k % 3)


def _xi_h(arrays, nb, n3):
    _, kw = params_h()
    d = arrays["dinc"]
    return int(arrays["sig5"][nb]) + int(kw["intpen"][n3 - nb]) + int(arrays["sig3"][n3]) + int(kw["t53"][16 * (d[nb] >> 4) + (d[n3] & 15)])


def gap_penalty3_h(i):
    sc, kw = params_h()
    assert i <= sc.codonk1
    return 0 if i == 0 else (0, kw["gape1"], kw["gape2"])[i % 3] + sc.gop + (i // 3) * sc.gep


def _junction(arrays, n, n3, ph):
    """plant a junction of phase ph between the corners at n and n3"""
    arrays["phs5"][n] = ph
    arrays["phs3"][n3] = ph


def _cases_h():
    out = []
    rng = np.random.default_rng(synth.SEED + 5102)
    minl = params_h()[1]["minl"]
    # corner forms: the planted structure, every corner and condensed
    k = 0
    while k < 14:
        arrays, exons = _plant_h(rng, int(rng.integers(15, 81)), int(rng.integers(2, 5)), int(rng.integers(40, 300)))
        full = _gene_corners_h(arrays, exons)
        if not _phase2_free(arrays, full) or any(b[0] < a[0] or b[1] < a[1] for a, b in zip(full, full[1:])):
            continue
        exg = tuple(int(x) for x in rng.integers(0, 2, size=4)) if k % 2 else (0, 0, 0, 0)
        for cond in (False, True):
            out.append(_case_h("h_forms", f"h_forms{k}{'c' if cond else 'f'}", arrays, _gene_corners_h(arrays, exons, cond),
                               jneibr=JNEIBR[k % 4], exg=exg, info=dict(twin=f"h_forms{k}f", introns=len(exons) - 1)))
        k += 1
    # gaps of every length mod 3 inside one exon: insertion and deletion frame shifts, extragop / gape1 / gape2
    for k in range(20):
        arrays, exons = _plant_h(rng, 60, 1, 60)
        g1, g2 = int(rng.integers(1, minl)), int(rng.integers(1, 20))
        if k < 6:
            g1, g2 = (1, 2, 3, 4, 5, 6)[k], (2, 1, 6, 5, 4, 3)[k]
        path = [("M", 12), ("D", g1), ("M", 10), ("I", g2), ("M", 9), ("D", g2), ("M", 5), ("I", g1), ("M", 4)]
        corners = corners_of(path, 0, exons[0][0], condensed=bool(k % 2), step=_step_h)
        out.append(_case_h("h_frameshift", f"h_fs{k}", arrays, corners, jneibr=JNEIBR[k % 4],
                           info=dict(ins_fs=(g1 % 3 != 0) + (g2 % 3 != 0), del_fs=(g2 % 3 != 0) + (g1 % 3 != 0))))
    # exons of jneibr - 1, jneibr, jneibr + 1 codons, first, inner and last; and of the lengths around jneibr nucleotides, since this walk
    # counts `psp` in nucleotides and asks `psp / 3 == jn` in one place, `psp < jn` and `n - LEFT <= jn` in the others
    for jn in JNEIBR:
        for L in sorted({jn - 1, jn, jn + 1, (jn - 1) // 3, (jn - 1) // 3 + 1, jn // 3 + 1} - {0}):
            for where in range(3):
                lens = [18, 18, 18]
                lens[where] = L
                arrays, exons = _plant_h(rng, 80, 1, 220)
                s = exons[0][0]
                for name in ("phs5", "phs3"):
                    arrays[name][s - 2:s + 3 * sum(lens) + 150] = -2
                corners, m, n = [(0, s)], 0, s
                for j, c in enumerate(lens):
                    m, n = m + c, n + 3 * c
                    corners.append((m, n))
                    if j < 2:
                        _junction(arrays, n, n + 70, 0)
                        arrays["sig5"][n], arrays["sig3"][n + 70] = 90, 110
                        n += 70
                        corners.append((m, n))
                out.append(_case_h("h_jneibr", f"h_jn{jn}_{L}_{where}", arrays, corners, jneibr=jn, info=dict(exon=where, exon_len=L)))
    # the list runs on over the stop codon behind the coding region, as the reference's aligner leaves it; with sup_tcodon the walk takes
    # the codon off the last corner (pinned by the h1_suptcodon fixture)
    k = 0
    while k < 6:
        arrays, exons = _plant_h(rng, int(rng.integers(15, 81)), int(rng.integers(1, 4)), int(rng.integers(40, 200)))
        full = _gene_corners_h(arrays, exons)
        if not _phase2_free(arrays, full) or any(b[0] < a[0] or b[1] < a[1] for a, b in zip(full, full[1:])):
            continue
        full.append((full[-1][0], exons[-1][1]))
        out.append(_case_h("h_suptcodon", f"h_suptcodon{k}", arrays, full, jneibr=JNEIBR[k % 4], sup_tcodon=1,
                           info=dict(right=exons[-1][1] - 3)))
        k += 1
    # a frame shift in front of a planted intron: what it leaves in `phs` decides the split-codon records the intron gets
    for k in range(8):
        g = (1, 2, 4, 5)[k % 4]
        arrays, exons = _plant_h(rng, 40, 1, 160)
        s = exons[0][0]
        path = [("M", 10), ("D" if k < 4 else "I", g), ("M", 8)]
        corners = corners_of(path, 0, s, step=_step_h)
        m, n = corners[-1]
        for name in ("phs5", "phs3"):
            arrays[name][n - 2:n + 103] = -2
        _junction(arrays, n, n + 100, 0)
        arrays["sig5"][n], arrays["sig3"][n + 100] = 90, 110
        corners += [(m, n + 100), (m + 10, n + 130)]
        out.append(_case_h("h_split", f"h_split{k}", arrays, corners, jneibr=JNEIBR[k % 4], info=dict(gap=g)))
    # gaps of codonk1 and codonk1 + 3 nucleotides under a codonk1 that gaps can exceed (the long-gap branch of GapPenalty3 and, for a gap
    # at the query's start under a_exgl, of UnpPenalty3)
    for k in range(8):
        g = (21, 24)[k % 2]
        arrays, exons = _plant_h(rng, 60, 1, 60)
        path = [("D", g), ("M", 15), ("D", g), ("M", 10), ("I", g), ("M", 5)]
        corners = corners_of(path, 0, exons[0][0] - g, step=_step_h)
        out.append(_case_h("h_codonk1", f"h_codonk1_{k}", arrays, corners, jneibr=JNEIBR[k % 4], exg=(k // 2 % 2, 0, 0, 0), codonk1=21,
                           info=dict(gap=g)))
    # junctions planted in each phase, accepted; and short ones with poor signals, rejected; the tie hi == h (tested by >=)
    for k in range(120):
        ph = (-1, 0, 1)[k % 3]
        kind = ("accept", "reject", "tie", "reject")[k // 3 % 4]
        L = int(rng.integers(minl, minl + 12)) if kind != "accept" else int(rng.integers(60, 300))
        arrays, exons = _plant_h(rng, 40, 1, 40 + L)
        s = exons[0][0]
        # 15 codons, the intron, 15 codons: the genomic side simply continues (rescoring scores what it is given)
        n = s + 45
        corners = [(0, s), (15, n), (15, n + L), (30, n + L + 45)]
        for name in ("phs5", "phs3"):
            arrays[name][n - 2:n + L + 3] = -2
        _junction(arrays, n, n + L, ph)
        nb = n - ph
        info = dict(phase=ph, kind=kind)
        if kind == "accept":
            arrays["sig5"][nb], arrays["sig3"][nb + L] = 90, 110
        else:
            # behind a matched codon a phase 1 junction re-scores it (hdlt): the tie is planted on phases 0 and -1 only
            arrays["sig5"][nb] += gap_penalty3_h(L) - _xi_h(arrays, nb, nb + L) - (1 if kind == "reject" else 0)
            if ph == 1:
                info["kind"] = kind = "reject"
                arrays["sig5"][nb] -= 400
            if kind == "tie":
                info["tie"] = ("sig5", nb)
        out.append(_case_h("h_junction", f"h_junc{k}", arrays, corners, jneibr=JNEIBR[k % 4], info=info))
    # a deletion of minl - 1 and of minl nucleotides at a planted junction (this walk asks `>= minl`, the cDNA one `> minl`)
    for k in range(6):
        L = minl - 1 + k % 2
        arrays, exons = _plant_h(rng, 40, 1, 40 + L)
        s = exons[0][0]
        n = s + 45
        for name in ("phs5", "phs3"):
            arrays[name][n - 2:n + L + 3] = -2
        _junction(arrays, n, n + L, 0)
        arrays["sig5"][n], arrays["sig3"][n + L] = 300, 300
        out.append(_case_h("h_minl", f"h_minl{k}", arrays, [(0, s), (15, n), (15, n + L), (30, n + L + 45)], jneibr=JNEIBR[k % 4],
                           info=dict(introns=k % 2)))
    # SER / SER2, stop codes and ambiguous bases in the four codons a junction reads (n5 - 2 .. n3 + 1)
    for k in range(12):
        ph = (-1, 0, 1)[k % 3]
        L = int(rng.integers(60, 200))
        arrays, exons = _plant_h(rng, 40, 1, 40 + L)
        s = exons[0][0]
        n = s + 45
        corners = [(0, s), (15, n), (15, n + L), (30, n + L + 45)]
        for name in ("phs5", "phs3"):
            arrays[name][n - 2:n + L + 3] = -2
        _junction(arrays, n, n + L, ph)
        nb = n - ph
        arrays["sig5"][nb], arrays["sig3"][nb + L] = 90, 110
        codes = ((2, 18, 23, 25), (23, 2, 18, 24), (25, 23, 2, 18), (18, 24, 25, 2))[k % 4]      # AMB, SER, SER2, TRM2, TRM
        arrays["b"] = arrays["b"].copy()
        for pos, code in zip((nb - 2, nb - 1, nb + L, nb + L + 1), codes):
            arrays["b"][pos] = code
        arrays["a"][14] = arrays["a"][15] = 18                                                # a serine on either side
        out.append(_case_h("h_codes", f"h_codes{k}", arrays, corners, jneibr=JNEIBR[k % 4], info=dict(phase=ph)))
    # junctions whose split codon lies outside the range: the donor at b_left, the acceptor at b_right - 1
    for k in range(6):
        L = int(rng.integers(60, 200))
        arrays, exons = _plant_h(rng, 40, 1, 40 + L)
        s = exons[0][0]
        for name in ("phs5", "phs3"):
            arrays[name][s - 2:s + 45 + L + 3] = -2
        if k % 2 == 0:
            corners, ph = [(0, s), (0, s + L), (15, s + L + 45)], 1
            _junction(arrays, s, s + L, ph)
            nb = s - ph
        else:
            n = s + 45
            corners, ph = [(0, s), (15, n), (15, n + L)], -1
            _junction(arrays, n, n + L, ph)
            nb = n - ph
        arrays["sig5"][nb], arrays["sig3"][nb + L] = 90, 110
        rng_ = (corners[0][0], corners[-1][0], corners[0][1], corners[-1][1] + (k % 2))
        out.append(_case_h("h_edge", f"h_edge{k}", arrays, corners, jneibr=JNEIBR[k % 4], rng=rng_, info=dict(phase=ph, side=k % 2)))
    # end gaps: every flag set, a genomic gap at the query's start and one at its end, flush with the range
    for flags in range(16):
        exg = (flags & 1, flags >> 1 & 1, flags >> 2 & 1, flags >> 3 & 1)
        arrays, exons = _plant_h(rng, 40, 1, 60)
        s = exons[0][0]
        g, g2, g3 = (int(x) for x in rng.integers(1, 12, size=3))
        # (the walk charges a gap at the query's end when a later step finds it pending: two steps)
        corners = [(0, s - g), (0, s), (30, s + 90), (30, s + 90 + g2), (30, s + 90 + g2 + g3)]
        arrays["b"] = arrays["b"].copy()
        for pos in (s + 90 + g2 - 1, s + 90 + g2 + 1):
            if arrays["b"][pos] >= 24:                   # no stop codon next to the last gap (unpinned, module docstring)
                arrays["b"][pos] = 3
        out.append(_case_h("h_end_gaps", f"h_exg{flags}", arrays, corners, jneibr=JNEIBR[flags % 4], exg=exg, info=dict(flags=flags)))
    # the end bonuses of `lcl & 20` / `lcl & 24`: an acceptor signal at the first corner above the start signal, a donor signal at the
    # last corner above the stop signal (pinned by the h1_local_inner fixture), and both one below: no bonus
    for k in range(8):
        arrays, exons = _plant_h(rng, 30, 1, 60)
        s = exons[0][0] + 3 * (k % 3)                     # (off the ATG for two in three)
        corners = [(k % 3, s), (20, s + 3 * (20 - k % 3))]
        e = corners[-1][1]
        top5 = max(int(arrays["sigT"][e - 2]), 0)
        top3 = max(int(arrays["sigS"][s + 1]), 0)
        d = 1 if k % 2 == 0 else 0
        arrays["sig3"][s], arrays["sig5"][e] = top3 + d, top5 + d
        out.append(_case_h("h_bonus", f"h_bonus{k}", arrays, corners, jneibr=JNEIBR[k % 4],
                           info=dict(sig3=top3 + d, sig5=top5 + d if d else top5 if arrays["sigT"][e - 2] > 0 else 0, on=d)))
    # two introns back to back whose phases leave an exon of one nucleotide between them (RIGHT - LEFT == 1: no record)
    for k in range(6):
        arrays, exons = _plant_h(rng, 40, 1, 300)
        s = exons[0][0]
        n, L1, L2 = s + 45, int(rng.integers(60, 120)), int(rng.integers(60, 120))
        corners = [(0, s), (15, n), (15, n + L1), (15, n + L1 + L2), (30, n + L1 + L2 + 45)]
        for name in ("phs5", "phs3"):
            arrays[name][n - 2:n + L1 + L2 + 3] = -2
        ph1, ph2 = ((0, -1), (1, 0), (0, 0))[k % 3]
        _junction(arrays, n, n + L1, ph1)
        arrays["phs5"][n + L1] = ph2
        arrays["phs3"][n + L1 + L2] = ph2
        for nb, L in ((n - ph1, L1), (n + L1 - ph2, L2)):
            arrays["sig5"][nb], arrays["sig3"][nb + L] = 90, 110
        out.append(_case_h("h_back_to_back", f"h_b2b{k}", arrays, corners, jneibr=JNEIBR[k % 4], info=dict(width=ph1 - ph2)))
    # the region window: an alignment deep inside a long region, and its ends closer to the region's ends than the margin
    for k, jn in enumerate(JNEIBR * 2):
        margin = 64 + 3 * jn
        arrays, exons = _plant_h(rng, 50, 3, 4500 if k < 4 else margin - 10 - 3 * k, intron_hi=200)
        if k < 4:
            assert 8000 <= arrays["b"].size - 1 <= 12000
        full = _gene_corners_h(arrays, exons)
        if not _phase2_free(arrays, full):
            for name in ("phs5", "phs3"):
                arrays[name][arrays[name] == 2] = -2
        out.append(_case_h("h_window", f"h_window{k}", arrays, full, jneibr=jn, rng=(0, arrays["a"].size, 0, arrays["b"].size - 1),
                           exg=(1, 1, 1, 1), info=dict(deep=k < 4, margin=margin)))
    # the aligner's own lists: the problems only
    for k in range(8):
        arrays, exons = _plant_h(rng, int(rng.integers(15, 81)), int(rng.integers(1, 4)), int(rng.integers(60, 300)))
        out.append(Case("h", "h_aligner", f"h_aligner{k}", arrays, (0, arrays["a"].size, 0, arrays["b"].size - 1), (1, 1, 1, 1), None,
                        dict(jneibr=JNEIBR[k % 4])))
    return out


@functools.lru_cache(maxsize=None)
def cases(walk):
    """every case of one walk ("s" / "h"), made once"""
    return tuple(_cases_s() if walk == "s" else _cases_h())


@functools.lru_cache(maxsize=None)
def expected(walk):
    """{case name: the oracle's (score, fstat, records)} for the cases that carry a corner list, computed once and shared"""
    return {c.name: oracle_of(c) for c in cases(walk) if c.corners is not None}
