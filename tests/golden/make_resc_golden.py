#!/usr/bin/env python3
"""tests/golden/make_resc_golden.py -- generator of tests/golden/resc_v1 (TEST INFRASTRUCTURE).

  refs      runs the reference binary's structurerescorediagonal (oracle/_ref/bin/foldseek, built by oracle/build_ref_full.sh cpu) on the example
            structures' databases of tests/golden/scop_v1 with the parameter sets below and freezes what it reads and writes: the crafted prefilter DB
            pref_resc_edges, the result DBs, MANIFEST.json with the argument vectors.  Every result DB must equal the model's (tests/resc_model.py) byte
            for byte before it is frozen; CENSUS.md lists the model's outcome counts per run.
  world     the seeded world of tests/resc_cases.py through the live model: answers_t{0,2}.npz, sets_t{0,2}.json.

Without an argument both.  The base parameter string is rescore_par of make_scop_golden.py (what the cluster workflow hands the module)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import diag_model as D  # noqa: E402
import resc_cases as K  # noqa: E402
import resc_model as R  # noqa: E402
from make_scop_golden import override, rescore_par  # noqa: E402

FS = os.path.join(ROOT, "oracle", "_ref", "bin", "foldseek")
OUT = K.GOLD
EDGES = "pref_resc_edges"


def write_pref(work, name, pref):
    blob, index, off = b"", [], 0
    for q in sorted(pref):
        body = "".join(f"{t}\t{s}\t{d}\n" for t, s, d in pref[q]).encode() + b"\0"
        index.append(f"{q}\t{off}\t{len(body)}\n")
        blob += body; off += len(body)
    open(os.path.join(work, name), "wb").write(blob)
    open(os.path.join(work, name + ".index"), "w").write("".join(index))
    shutil.copy(os.path.join(K.SCOP, "pref_kmer_defined.dbtype"), os.path.join(work, name + ".dbtype"))


def make_edges():
    """the crafted prefilter lists: defined pairs only, in an order that is not score order.  Per query: the self hit on diagonal 0, on a far diagonal (four
    cells: its e-value fails) and on the near diagonal 1 .. 12 with the best score (low identity, a fair score); the best other target twice, on its diagonal
    and the next one; a run of three and a run of four lines the default gates reject (other targets on the last diagonals of the query: one to three cells; the
    second run begins with the far self hit), between lines they accept"""
    keys, seqs = K.scop_sequences()
    base = K.read_pref(os.path.join(K.SCOP, "pref_kmer_defined"))
    W = K._scop_world(2)
    idx = {k: i for i, k in enumerate(keys)}
    pref = {}
    for n, q in enumerate(keys):
        L = len(seqs[q][0])
        wq = W.query(*seqs[q])
        near = max(range(1, 13), key=lambda d: W.pair(wq, idx[q], d)["score"] - W.pair(wq, idx[q], d)["revScore"])
        others = [(t, d) for t, d in base.get(q, []) if t != q][::-1]
        ev = lambda t, d: W.evalue(wq, W.pair(wq, idx[t], d)["score"] - W.pair(wq, idx[t], d)["revScore"])  # noqa: E731
        first = [k for k, (t, d) in enumerate(others) if ev(t, d) <= 10.0]                   # the list opens with a line the default gates accept:
        others.insert(0, others.pop(first[0]) if first else (q, 0))                          # another target's, or the self hit where there is none
        rej = []                                                   # other targets on the last diagonals, those whose e-value the default gate rejects
        for j in range(1, len(keys)):
            t = keys[(n + 7 * j + 3) % len(keys)]
            d = L - 1 - (j % 3)
            p = W.pair(wq, idx[t], d)
            if t != q and len(rej) < 6 and W.evalue(wq, p["score"] - p["revScore"]) > 10.0:
                rej.append((t, d))
        assert len(rej) == 6, q
        lines = others[:1] + rej[:3] + ([(q, 0)] if first else []) + others[1:2]
        t, d = ([x for x in others if x[0] != q] or [(rej[0][0], -1)])[-1]                    # one target twice: on its diagonal and the next one
        assert K.defined(L, len(seqs[t][0]), d + 1), q
        lines += [(t, d + 1)]
        lines += [(q, L - 4)] + rej[3:6] + [(q, near)] + others[2:]
        assert all(K.defined(L, len(seqs[t][0]), d) for t, d in lines), q
        pref[q] = [(t, 100 - k, d) for k, (t, d) in enumerate(lines)]      # the score column is not read (:317-319)
    return pref


def fmt32(x):
    s = "%.9g" % float(np.float32(x))
    assert np.float32(float(s)) == np.float32(x) and "e" not in s
    return s


def ref_runs(edges):
    """-> {name: (positional, parameters, (query key, target key, what) of the line a threshold was read off, or None)}"""
    keys, _ = K.scop_sequences()
    named_q = keys[3]
    run = lambda par: K.model_db(dict(positional=["db", "db"], parameters=par), edges)[1]  # noqa: E731
    r = run(rescore_par(2, 1, "10", "0"))[named_q]
    mid = sorted(range(len(r.records)), key=lambda i: (r.records[i]["seqId"], i))[len(r.records) // 2]
    sid0 = fmt32(r.records[mid]["seqId"])
    r2 = run(override(rescore_par(2, 1, "10", "0"), **{"--seq-id-mode": "2"}))[named_q]
    sid2 = fmt32(r2.records[mid]["seqId"])
    ln = int(r.records[mid]["alnLength"])
    ev = "%.17g" % float(r.records[mid]["eval"])
    assert float(ev) == float(r.records[mid]["eval"])
    tkey = int(r.records[mid]["dbKey"])
    E, KD = ["db", "db", EDGES], ["db", "db", "pref_kmer_defined"]
    P = lambda atype=2, a=1, e="10", c="0", **kw: override(rescore_par(atype, a, e, c), **kw)  # noqa: E731
    runs = {
        "e_cov0": (E, P(c="0.5"), None),
        "e_cov1": (E, P(c="0.5", **{"--cov-mode": "1"}), None),
        "e_cov3": (E, P(c="0.7", **{"--cov-mode": "3"}), None),
        "e_cov4": (E, P(c="0.7", **{"--cov-mode": "4"}), None),
        "e_cov5": (E, P(c="0.7", **{"--cov-mode": "5"}), None),
        "k_cov1_t0": (KD, P(atype=0, c="0.6", **{"--cov-mode": "1"}), None),
        "k_cov4": (KD, P(c="0.8", **{"--cov-mode": "4"}), None),
        "e_sid0_eq": (E, P(**{"--min-seq-id": sid0, "--seq-id-mode": "0"}), (named_q, tkey, "seqId")),
        "e_sid2_eq": (E, P(**{"--min-seq-id": sid2, "--seq-id-mode": "2"}), (named_q, tkey, "seqId")),
        "k_sid2": (KD, P(**{"--min-seq-id": "0.3", "--seq-id-mode": "2"}), None),
        "e_minlen_eq": (E, P(**{"--min-aln-len": str(ln)}), (named_q, tkey, "alnLength")),
        "e_ev_eq": (E, P(e=ev), (named_q, tkey, "eval")),
        "e_acc2": (E, P(**{"--max-accept": "2"}), None),
        "e_rej3": (E, P(**{"--max-rejected": "3"}), None),
        # a run of three, an accepted line, a run of four: without the reset the second run would end the list at five
        "e_acc5_rej5": (E, P(**{"--max-accept": "5", "--max-rejected": "5"}), None),
        "e_e1e-3_t0": (E, P(atype=0, e="1e-3"), None),
        "e_e1e-3_t2": (E, P(e="1e-3"), None),
        "e_a0": (E, P(a=0), None),
        "e_sid05_noself": (E, P(**{"--min-seq-id": "0.5", "--add-self-matches": "0"}), None),
        "e_sid05_2path_noself": (["db", "db2", EDGES], P(**{"--min-seq-id": "0.5", "--add-self-matches": "0"}), None),
        "e_sid05_2path_self": (["db", "db2", EDGES], P(**{"--min-seq-id": "0.5", "--add-self-matches": "1"}), None),
        "e_cov0_2path_noself": (["db", "db2", EDGES], P(c="0.5", **{"--add-self-matches": "0"}), None),
    }
    return runs


def check_census(census):
    total = {}
    for c in census.values():
        for o, n in c.items():
            total[o] = total.get(o, 0) + n
    missing = [o for o in R.OUTCOMES if not o.startswith("skipped") and o not in total]
    assert not missing, missing
    return total


def refs():
    if not os.path.exists(FS):
        raise SystemExit("build the reference first: bash oracle/build_ref_full.sh cpu")
    work = os.path.join(ROOT, "oracle", "_ref_full", "resc_work")
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    for f in os.listdir(K.SCOP):
        if (f.startswith("db") and not f.startswith("db_pad")) or f.startswith("pref_kmer_defined"):
            shutil.copy(os.path.join(K.SCOP, f), os.path.join(work, f))
            if f.startswith("db"):                                  # the same database under a second path
                shutil.copy(os.path.join(K.SCOP, f), os.path.join(work, "db2" + f[2:]))
    crafted = make_edges()
    write_pref(work, EDGES, crafted)
    prefs = {EDGES: K.read_pref(os.path.join(work, EDGES)), "pref_kmer_defined": K.read_pref(os.path.join(work, "pref_kmer_defined"))}
    assert prefs[EDGES] == {q: [(t, d) for t, _, d in v] for q, v in crafted.items()}
    manifest = {"reference": "steineggerlab/foldseek, binary from oracle/build_ref_full.sh cpu; databases and pref_kmer_defined: tests/golden/scop_v1", "runs": {}}
    census = {}
    for name, (pos, par, named) in ref_runs(prefs[EDGES]).items():
        r = subprocess.run([FS, "structurerescorediagonal"] + pos + [name] + par, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise SystemExit(f"{name} failed:\n{r.stdout[-2000:]}")
        run = dict(module="structurerescorediagonal", positional=pos, parameters=par)
        db, res = K.model_db(run, prefs[pos[2]])
        want = D.read_db(os.path.join(work, name))
        bad = [q for q in sorted(want) if want[q] != db.get(q, b"")]
        assert not bad and sorted(want) == sorted(db), (name, bad[:3], want[bad[0]][:400], db[bad[0]][:400])
        if named:
            q, t, what = named
            _, P, _ = K.run_params(run)
            rec = [x for x in res[q].records if int(x["dbKey"]) == t]
            value = {"seqId": P["seqIdThr"], "alnLength": P["alnLenThr"], "eval": P["evalThr"]}[what]
            assert any(float(x[what]) == float(value) for x in rec), (name, "the named line no longer sits at the threshold")
            run["threshold_at"] = dict(query=int(q), target=int(t), field=what)
        manifest["runs"][name] = run
        census[name] = R.count_outcomes(res.values())
        print(name, census[name], flush=True)
    check_census(census)
    os.makedirs(OUT, exist_ok=True)
    for f in sorted(os.listdir(work)):
        if f.startswith(EDGES) or f.split(".")[0] in manifest["runs"]:
            shutil.copy(os.path.join(work, f), os.path.join(OUT, f))
    json.dump(manifest, open(os.path.join(OUT, "MANIFEST.json"), "w"), indent=1, sort_keys=True)
    return census


def world():
    census = {}
    for atype in K.ATYPES:
        live = K.Live(atype)
        sets, extra = K.derive(live)
        ans = K.answers(live, sets)
        n = K.check_pairs(live, sets)
        census[atype] = K.census(live, sets, ans)
        K.save(atype, sets, extra, ans)
        print(f"type {atype}: {len(sets)} sets, {n} pairs of sets at a threshold and beyond it", flush=True)
    return census


def write_census(ref_census, world_census):
    cols = [o for o in R.OUTCOMES]
    out = ["# What the frozen runs of resc_v1 reach", "", "Outcome of every listed pair, counted by the model (tests/resc_model.py); written by make_resc_golden.py.", "",
           "## Reference binary runs (example structures)", "", "| run | " + " | ".join(cols) + " |", "|---|" + "---|" * len(cols)]
    for name, c in ref_census.items():
        out.append(f"| {name} | " + " | ".join(str(c.get(o, 0)) for o in cols) + " |")
    for atype, cs in world_census.items():
        out += ["", f"## Seeded world, alignment type {atype}", "", "| set | " + " | ".join(cols) + " |", "|---|" + "---|" * len(cols)]
        for name, c in cs.items():
            out.append(f"| {name} | " + " | ".join(str(c.get(o, 0)) for o in cols) + " |")
    open(os.path.join(OUT, "CENSUS.md"), "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    rc = refs() if what in ("refs", "all") else None
    wc = world() if what in ("world", "all") else None
    if rc is not None and wc is not None:
        write_census(rc, wc)
