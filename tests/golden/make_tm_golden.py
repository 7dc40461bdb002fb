#!/usr/bin/env python3
"""tests/golden/make_tm_golden.py -- generator of tests/golden/tm_v1 (TEST INFRASTRUCTURE).

Runs the WHOLE reference binary (oracle/_ref/bin/foldseek, built by oracle/build_ref_full.sh cpu) on the databases frozen in tests/golden/ca_v1 (db, db_pad,
pref, pref_pad: read from there, unchanged, not copied) and freezes what the TM-score path of this repository is held to:

  * `structurealign -a 1 -e 10 --alignment-type 2` with --sort-by-structure-bits 1 (thresholds 0; --lddt-threshold 0.5 --tmscore-threshold 0.7), with
    --sort-by-structure-bits 0 and --tmscore-threshold 0.7 in the modes 0 / 1 / 2 and 0.8 in mode 0, structure bits with the threshold 0.7 under
    --max-rejected 2, under --alt-ali 2 and on the padded target.  The line counts are asserted, so that a changed input is noticed; both thresholds drop
    some hits and keep others, and the three modes keep different numbers of hits.
  * `convertalis --format-output query,target,alnlen,alntmscore,qtmscore,ttmscore,rmsd` of ca_v1's unfiltered result aln_l0.
  * a CRAFTED database (written here) through the same `convertalis`: alignments of 1 to 5 columns (fewer than four pairs, a normalisation length of 0,
    NaN rotations that take the classical Kabsch()), the relief loop of score_fun8 entered and not entered, a self-alignment, leading and inner I / D
    runs, an alignment whose pairs all stay beyond score_d8 (score 0), and 39 / 40 / 41 / 80 / 81 / 161 columns (the step-40 start list, the forced last start,
    the sixth fragment length).  Which branch a record takes is asserted with the independent model tests/tm_model.py and written to the MANIFEST.

Every text field the reference printed is compared with the model here as well, and the model's raw answers for the task lists of tests/tm_cases.py
(these fixtures, a seeded corpus, edge cases) are frozen as model_*_raw.npy.  Running the generator twice gives identical files.
Needs the built reference binary only; it reads nothing else outside this repository.
"""
import json
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import lddt_model as M  # noqa: E402
import tm_model as T  # noqa: E402
from make_ca_golden import FS, align_par, count_lines, grid, read_db, run, write_db  # noqa: E402

CA = os.path.join(HERE, "ca_v1")
OUT = os.path.join(HERE, "tm_v1")
SUBMAT = "aa:3di.out,nucl:3di.out"
T1, T2 = 0.7, 0.8


def tm_par(bits, tm=0, mode=0, lddt=0, **kw):
    kw = dict(kw)
    kw.update({"--sort-by-structure-bits": bits, "--tmscore-threshold": tm, "--tmscore-threshold-mode": mode})
    return align_par(lddt, **kw)


# name -> (positional args, parameters, expected result lines)
ALIGN_RUNS = {
    "aln_sb1": (["db", "db", "pref"], tm_par(1), 144),
    "aln_sb1_l05_t07": (["db", "db", "pref"], tm_par(1, T1, 0, 0.5), 128),
    "aln_sb0_t07_m0": (["db", "db", "pref"], tm_par(0, T1, 0), 128),
    "aln_sb0_t07_m1": (["db", "db", "pref"], tm_par(0, T1, 1), 103),
    "aln_sb0_t07_m2": (["db", "db", "pref"], tm_par(0, T1, 2), 99),
    "aln_sb0_t08_m0": (["db", "db", "pref"], tm_par(0, T2, 0), 72),
    "aln_sb1_t07_maxrej": (["db", "db", "pref"], tm_par(1, T1, 0, **{"--max-rejected": 2}), 128),
    "aln_sb1_t07_altali": (["db", "db", "pref"], tm_par(1, T1, 0, **{"--alt-ali": 2}), 379),
    "aln_sb1_t07_pad": (["db", "db_pad", "pref_pad"], tm_par(1, T1, 0), 128),
}
CONVERT_PAR = ["--sub-mat", SUBMAT, "--format-mode", "0", "--format-output", "query,target,alnlen,alntmscore,qtmscore,ttmscore,rmsd",
               "--translation-table", "1", "--gap-open", "aa:10,nucl:10", "--gap-extend", "aa:1,nucl:1", "--db-output", "0", "--db-load-mode", "0",
               "--search-type", "0", "--threads", "1", "--compressed", "0", "-v", "1", "--exact-tmscore", "0"]


def crafted():
    """-> (coords {key: float32 [3, L]}, names {key: str}, alignments [(query key, target key, qStart, dbStart, cigar, what it is for)])"""
    rng = np.random.default_rng(20261017)

    def walk(L, step=3.8):
        v = rng.normal(size=(L, 3))
        v = v / np.linalg.norm(v, axis=1)[:, None] * step
        return np.cumsum(v, axis=0).T

    c, names = {}, {}
    c[0] = grid(walk(170)); names[0] = "qlong"
    noisy = np.array(c[0], np.float64) + rng.normal(scale=1.2, size=(3, 170))
    noisy[:, 100:] += rng.normal(scale=4.0, size=(3, 70))            # a tail that does not superpose: refinement rounds drop it
    c[1] = grid(noisy); names[1] = "tlong"
    c[2] = grid(walk(12)); names[2] = "qshort"
    c[3] = grid(np.array(c[2], np.float64) + rng.normal(scale=0.8, size=(3, 12))); names[3] = "tshort"
    far = np.zeros((3, 8))
    far[0] = np.arange(8) * 30.0                                      # residues 30 A apart (the int16 steps allow 32.767): nothing superposes within score_d8
    c[4] = grid(far); names[4] = "tfar"
    c[5] = grid(np.array([[0, 3.8, 7.6, 11.4, 15.2, 19.0], [0] * 6, [0] * 6], np.float64)); names[5] = "qline"          # collinear, on the grid
    c[6] = grid(np.array([[1.0] * 6, [2.0] * 6, [3.0] * 6], np.float64)); names[6] = "tpoint"                         # coincident residues
    aln = [(2, 3, 0, 0, "1M", "1 column: Lali < 4, normLen 0 in alntmscore"),
           (2, 3, 1, 0, "2M", "2 columns"),
           (2, 3, 0, 2, "3M", "3 columns"),
           (2, 3, 2, 2, "4M", "4 columns: one fragment length"),
           (2, 3, 0, 0, "5M", "5 columns"),
           (2, 2, 0, 0, "12M", "self-alignment: rmsd 0"),
           (2, 3, 0, 0, "3I4M2D3M2I", "leading I run, inner D run, trailing I run"),
           (2, 3, 0, 1, "2D5M1I4M", "leading D run, inner I"),
           (2, 4, 0, 3, "2M", "two pairs, both beyond score_d8 under every superposition: score 0"),
           (2, 4, 0, 0, "4M", "residues 30 A apart on 3.8 A apart: the relief loop walks far"),
           (2, 4, 2, 1, "7M", "the same with two fragment lengths"),
           (5, 6, 0, 0, "6M", "collinear query on coincident target residues: degenerate rotations"),
           (5, 5, 0, 0, "5M", "collinear self-alignment"),
           (0, 1, 0, 0, "39M", "39 columns"),
           (0, 1, 3, 2, "40M", "40 columns"),
           (0, 1, 0, 0, "41M", "41 columns: starts 0, 1 for the first halved length"),
           (0, 1, 5, 5, "80M", "80 columns"),
           (0, 1, 0, 0, "81M", "81 columns"),
           (0, 1, 0, 0, "161M", "161 columns: six fragment lengths, the dropped tail"),
           (0, 1, 2, 0, "50M3I60M4D40M", "inner gaps in a long alignment"),
           (0, 0, 0, 0, "170M", "long self-alignment")]
    return c, names, aln


def write_crafted(work):
    c, names, aln = crafted()
    write_db(os.path.join(work, "tmdb"), {k: ("A" * v.shape[1] + "\n").encode() for k, v in c.items()}, 0)
    write_db(os.path.join(work, "tmdb_ss"), {k: ("D" * v.shape[1] + "\n").encode() for k, v in c.items()}, 0)
    write_db(os.path.join(work, "tmdb_h"), {k: (names[k] + "\n").encode() for k in c}, 12)
    ca = {}
    for k, v in c.items():
        ca[k] = M.encode16(v) + b"\n"
        assert (M.decode(ca[k], v.shape[1]) == v).all(), k
    write_db(os.path.join(work, "tmdb_ca"), ca, 101)
    open(os.path.join(work, "tmdb.lookup"), "w").write("".join(f"{k}\t{names[k]}\t{k}\n" for k in sorted(c)))
    open(os.path.join(work, "tmdb.source"), "w").write("".join(f"{k}\t{names[k]}\n" for k in sorted(c)))
    per_q = {}
    for q, t, qs, ts, cig, _ in aln:
        bt = M.expand(cig)
        qe = qs + sum(ch in "MI" for ch in bt) - 1
        te = ts + sum(ch in "MD" for ch in bt) - 1
        assert qe < c[q].shape[1] and te < c[t].shape[1], (q, t, cig)
        per_q.setdefault(q, []).append(f"{t}\t100\t0.500\t1.000E-05\t{qs}\t{qe}\t{c[q].shape[1]}\t{ts}\t{te}\t{c[t].shape[1]}\t{cig}\n")
    write_db(os.path.join(work, "tmaln"), {q: "".join(v).encode() for q, v in per_q.items()}, 5)
    return c, names, aln


def model_fields(qc, tc, qs, ts, cig, stats=None):
    """the four text fields of the convertalis run for one record, and the three normalisation lengths"""
    bt = M.expand(cig)
    qe = qs + sum(ch in "MI" for ch in bt) - 1
    te = ts + sum(ch in "MD" for ch in bt) - 1
    norms = (min(qe - qs, te - ts), qc.shape[1], tc.shape[1])
    out = []
    for nl in norms:
        tm, rmsd = T.tmscore(qc, tc, qs, ts, bt, nl, stats)
        out.append(T.sstr(tm))
    out.append(T.sstr(rmsd))
    return out, norms


def parse_result_db(path):
    """{query key: [fields of every line]}"""
    return {k: [l.split("\t") for l in v.decode().splitlines()] for k, v in read_db(path).items()}


def main():
    if not os.path.exists(FS):
        raise SystemExit("build the reference first: bash oracle/build_ref_full.sh cpu")
    work = os.path.join(ROOT, "oracle", "_ref_full", "tm_work")
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    ca_manifest = json.load(open(os.path.join(CA, "MANIFEST.json")))
    for f in sorted(os.listdir(CA)):                                   # the inputs, as ca_v1 froze them (its links restored)
        if f.startswith(("db", "pref")):
            shutil.copy(os.path.join(CA, f), os.path.join(work, f))
    for link, target in ca_manifest["links"].items():
        if not os.path.lexists(os.path.join(work, link)):
            os.symlink(target, os.path.join(work, link))
    inputs = set(os.listdir(work))
    manifest = {"reference": "steineggerlab/foldseek, binary from oracle/build_ref_full.sh cpu", "inputs": "tests/golden/ca_v1: db*, pref*",
                "runs": {}, "convert_runs": {}, "thresholds": [T1, T2]}
    for name, (pos, par, lines) in ALIGN_RUNS.items():
        run([FS, "structurealign"] + pos + [name] + par, work)
        n = count_lines(os.path.join(work, name))
        assert n == lines, (name, n, lines)
        manifest["runs"][name] = {"module": "structurealign", "positional": pos, "parameters": par, "lines": n}
    shutil.copy(os.path.join(CA, "aln_l0"), os.path.join(work, "aln_l0"))
    shutil.copy(os.path.join(CA, "aln_l0.index"), os.path.join(work, "aln_l0.index"))
    shutil.copy(os.path.join(CA, "aln_l0.dbtype"), os.path.join(work, "aln_l0.dbtype"))
    inputs |= {"aln_l0", "aln_l0.index", "aln_l0.dbtype"}
    run([FS, "convertalis", "db", "db", "aln_l0", "conv_tm.m8"] + CONVERT_PAR, work)
    manifest["convert_runs"]["conv_tm.m8"] = {"module": "convertalis", "positional": ["db", "db", "aln_l0"], "parameters": CONVERT_PAR}
    c, names, aln = write_crafted(work)
    run([FS, "convertalis", "tmdb", "tmdb", "tmaln", "conv_tm_crafted.m8"] + CONVERT_PAR, work)
    manifest["convert_runs"]["conv_tm_crafted.m8"] = {"module": "convertalis", "positional": ["tmdb", "tmdb", "tmaln"], "parameters": CONVERT_PAR}

    # ---- the model against what the reference printed: the 144 pairs
    rows = [l.rstrip("\n").split("\t") for l in open(os.path.join(work, "conv_tm.m8"))]
    assert len(rows) == 144
    look = {l.split()[1]: int(l.split()[0]) for l in open(os.path.join(CA, "db.lookup"))}
    cadb = read_db(os.path.join(CA, "db_ca"))
    recs = parse_result_db(os.path.join(CA, "aln_l0"))
    flat = [(q, r) for q in sorted(recs) for r in recs[q]]
    assert len(flat) == len(rows)
    tms = []
    for row, (q, r) in zip(rows, flat):
        t, qs, ql, ts, tl, cig = int(r[0]), int(r[4]), int(r[6]), int(r[7]), int(r[9]), r[10]
        assert look[row[0]] == q and look[row[1]] == t
        got, _ = model_fields(M.decode(cadb[q], ql), M.decode(cadb[t], tl), qs, ts, cig)
        assert got == row[3:7], (row, got)
        tms.append([float(v) for v in row[3:6]])
    tms = np.array(tms)
    for thr in (T1, T2):                                               # each threshold drops some hits and keeps others
        assert 0 < (tms[:, 0] >= thr).sum() < 144
    assert len({int((tms[:, m] >= T1).sum()) for m in range(3)}) == 3  # the modes disagree

    # ---- the crafted records do what they were made for
    rows = [l.rstrip("\n").split("\t") for l in open(os.path.join(work, "conv_tm_crafted.m8"))]
    order = sorted(range(len(aln)), key=lambda i: aln[i][0])           # convertalis walks the queries in key order, records in file order
    assert len(rows) == len(aln)
    branches = []
    for row, i in zip(rows, order):
        q, t, qs, ts, cig, what = aln[i]
        assert row[0] == names[q] and row[1] == names[t], (row[:2], names[q], names[t])
        stats = {}
        got, norms = model_fields(c[q], c[t], qs, ts, cig, stats)
        assert got == row[3:7], (names[q], names[t], cig, row[3:7], got)
        n = M.expand(cig).count("M")
        branches.append({"query": names[q], "target": names[t], "qStart": qs, "dbStart": ts, "cigar": cig, "what": what, "pairs": n,
                         "fragment_lengths": T.frag_lengths(n), "relief_steps": stats.get("relief", 0), "kabsch_fallbacks": stats.get("fallback", 0),
                         "normLen": list(norms), "fields": row[3:7]})
    by = {(b["query"], b["target"], b["cigar"]): b for b in branches}
    for cig in ("1M", "2M", "3M"):
        assert by[("qshort", "tshort", cig)]["relief_steps"] == 0       # n_ali > 3 is false: the loop is never entered
    assert by[("qshort", "tshort", "1M")]["normLen"][0] == 0
    assert by[("qshort", "tshort", "1M")]["kabsch_fallbacks"] > 0       # a single pair: NaN rotation -> Kabsch()
    assert by[("qshort", "tfar", "4M")]["relief_steps"] > 10
    assert by[("qshort", "tfar", "2M")]["fields"][:3] == ["0.000E+00"] * 3
    assert by[("qshort", "qshort", "12M")]["fields"][3] == "0.000E+00"
    assert by[("qshort", "qshort", "12M")]["relief_steps"] == 0         # relief not entered although n_ali > 3
    assert len(by[("qlong", "tlong", "161M")]["fragment_lengths"]) == 6
    assert by[("qlong", "tlong", "41M")]["fragment_lengths"][:2] == [41, 20]
    manifest["crafted"] = {"records": branches,
                           "kabsch_fallback_records": [f'{b["query"]} {b["target"]} {b["cigar"]}' for b in branches if b["kabsch_fallbacks"] > 0]}

    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    for f in sorted(os.listdir(work)):
        p = os.path.join(work, f)
        if f in inputs or os.path.islink(p) or os.path.isdir(p) or "_tmp" in f or ".idx" in f:
            continue
        shutil.copy(p, os.path.join(OUT, f))
    json.dump(manifest, open(os.path.join(OUT, "MANIFEST.json"), "w"), indent=1, sort_keys=True)
    # ---- the model's raw answers for the fixed task lists of tests/tm_cases.py (the tests do not have the minutes this takes)
    import tm_cases as TC
    coords, tasks = TC.fixture_tasks()
    raw = TC.model_raw(coords, coords, tasks)
    text = [l.rstrip("\n").split("\t") for name in ("conv_tm.m8", "conv_tm_crafted.m8") for l in open(os.path.join(OUT, name))]
    assert len(text) * 3 == len(tasks)
    for r, row in enumerate(text):
        assert TC.text_fields(raw[3 * r:3 * r + 3], [t[5] for t in tasks[3 * r:3 * r + 3]]) == row[3:7], row
    np.save(os.path.join(OUT, "model_fixture_raw.npy"), raw)
    for which, lists in (("corpus", TC.corpus()), ("edge", TC.edge())):
        np.save(os.path.join(OUT, f"model_{which}_raw.npy"), TC.model_raw(*lists))
    n = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print(f"{len(os.listdir(OUT))} files, {n} bytes -> {OUT}")


if __name__ == "__main__":
    main()
