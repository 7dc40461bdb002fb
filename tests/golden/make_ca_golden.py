#!/usr/bin/env python3
"""tests/golden/make_ca_golden.py -- generator of tests/golden/ca_v1 (TEST INFRASTRUCTURE).

Runs the WHOLE reference binary (oracle/_ref/bin/foldseek, built by oracle/build_ref_full.sh cpu) on the 12 committed structures of
tests/golden/example_structures and freezes what the LDDT path of this repository is held to:

  * the databases the reference's `createdb` writes, INCLUDING the C-alpha database db_ca (int16-difference entries), and a padded target made by the
    reference's `makepaddedseqdb` workflow (db_pad*, its db_pad_ca keyed by the padded ids);
  * `ungappedprefilter --min-ungapped-score 0` (all 144 pairs) and `structurealign --sort-by-structure-bits 0 -a 1 -e 10 --lddt-threshold T` for
    T = 0 / 0.5 / 0.7 / 0.8 (144 / 143 / 24 / 14 result lines -- asserted here, so that a changed input is noticed), T = 0.7 with --max-rejected 2, with
    --alt-ali 2, and on the padded target;
  * `convertalis --format-output query,target,alnlen,lddt,lddtfull` of the T = 0 result;
  * a CRAFTED database (written here: sequences, headers, C-alpha entries and an alignment DB, no structure files) through the same reference
    `convertalis`: one raw-float32 entry, query residues without any neighbour inside 15 A (NaN columns, in the middle and at the end of an alignment),
    an alignment whose every column is isolated, residue pairs at exactly 15.0 A, pairs with |d_query - d_target| exactly 0.5 / 1 / 2 / 4, and pairs found
    by a seeded search for which the fused and the unfused dist() fall on different sides of the 15 A cutoff (the 12 structures cannot tell the two
    forms apart; this record pins the fused one -- asserted here with tests/lddt_model.py).

Needs the built reference binary only; it reads nothing else outside this repository.
"""
import gzip
import json
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lddt_model as M  # noqa: E402

FS = os.path.join(ROOT, "oracle", "_ref", "bin", "foldseek")
EXAMPLE = os.path.join(HERE, "example_structures")
OUT = os.path.join(HERE, "ca_v1")
SUBMAT = "aa:3di.out,nucl:3di.out"

UNGAPPED_PAR = ["--sub-mat", SUBMAT, "-c", "0", "-e", "1.79769e+308", "--cov-mode", "0", "--comp-bias-corr", "1",
                "--comp-bias-corr-scale", "0.15", "--min-ungapped-score", "0", "--max-seqs", "1000", "--db-load-mode", "0",
                "--gpu", "0", "--gpu-server", "0", "--gpu-server-wait-timeout", "600", "--prefilter-mode", "1",
                "--threads", "1", "--compressed", "0", "-v", "1"]


def align_par(lddt, **kw):
    par = ["--tmscore-threshold", "0", "--tmscore-threshold-mode", "0", "--lddt-threshold", str(lddt), "--sort-by-structure-bits", "0",
           "--alignment-type", "2", "--exact-tmscore", "0", "--sub-mat", SUBMAT, "-a", "1", "--alignment-mode", "3",
           "--alignment-output-mode", "0", "--wrapped-scoring", "0", "-e", "10", "--min-seq-id", "0", "--min-aln-len", "0",
           "--seq-id-mode", "0", "--alt-ali", "0", "-c", "0", "--cov-mode", "0", "--max-seq-len", "65535", "--comp-bias-corr", "1",
           "--comp-bias-corr-scale", "0.5", "--max-rejected", "2147483647", "--max-accept", "2147483647", "--add-self-matches", "0",
           "--db-load-mode", "0", "--pca", "substitution:1.100,context:1.400", "--pcb", "substitution:4.100,context:5.800",
           "--score-bias", "0", "--realign", "0", "--realign-score-bias", "-0.2", "--realign-max-seqs", "2147483647",
           "--corr-score-weight", "0", "--gap-open", "aa:10,nucl:10", "--gap-extend", "aa:1,nucl:1", "--zdrop", "40",
           "--threads", "1", "--compressed", "0", "-v", "1"]
    for flag, v in kw.items():
        par[par.index(flag) + 1] = str(v)
    return par


# name -> (positional args, parameters, expected result lines or None)
ALIGN_RUNS = {
    "aln_l0": (["db", "db", "pref"], align_par(0), 144),
    "aln_l05": (["db", "db", "pref"], align_par(0.5), 143),
    "aln_l07": (["db", "db", "pref"], align_par(0.7), 24),
    "aln_l08": (["db", "db", "pref"], align_par(0.8), 14),
    "aln_l07_maxrej": (["db", "db", "pref"], align_par(0.7, **{"--max-rejected": 2}), None),
    "aln_l07_altali": (["db", "db", "pref"], align_par(0.7, **{"--alt-ali": 2}), None),
    "aln_l07_pad": (["db", "db_pad", "pref_pad"], align_par(0.7), 24),
}
CONVERT_PAR = ["--sub-mat", SUBMAT, "--format-mode", "0", "--format-output", "query,target,alnlen,lddt,lddtfull",
               "--translation-table", "1", "--gap-open", "aa:10,nucl:10", "--gap-extend", "aa:1,nucl:1", "--db-output", "0", "--db-load-mode", "0",
               "--search-type", "0", "--threads", "1", "--compressed", "0", "-v", "1", "--exact-tmscore", "0"]


def run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout)
        raise SystemExit(f"FAILED: {' '.join(cmd)}")
    return r.stdout


def read_db(path):
    data = open(path, "rb").read()
    out = {}
    for line in open(path + ".index"):
        k, off, ln = line.split()
        out[int(k)] = data[int(off):int(off) + int(ln) - 1]
    return out


def write_db(path, entries, dbtype):
    """entries: {key: bytes without the terminator}"""
    blob, index, off = b"", [], 0
    for k in sorted(entries):
        body = entries[k] + b"\0"
        index.append(f"{k}\t{off}\t{len(body)}\n")
        blob += body
        off += len(body)
    open(path, "wb").write(blob)
    open(path + ".index", "w").write("".join(index))
    open(path + ".dbtype", "wb").write(int(dbtype).to_bytes(4, "little"))


def count_lines(path):
    return sum(len(v.decode().splitlines()) for v in read_db(path).values())


# ---- the crafted database ------------------------------------------------------------------------------------------------------------------
def grid(a):
    """coordinates on the 0.001 A grid of the compressed entry form, as the float32 values the decoder produces"""
    return (np.rint(np.asarray(a, np.float64) * 1000.0).astype(np.int32).astype(np.float32) / np.float32(1000.0)).astype(np.float32)


def straddling_partners(rng, anchor, want):
    """float32 points p with fused dist(anchor, p) and unfused dist(anchor, p) on different sides of 15.0: random direction, then a sweep of the
    last coordinate over neighbouring float32 values around the solution of |p - anchor| = 15"""
    found = []
    while len(found) < want:
        d0, d1 = rng.uniform(-9, 9, 2)
        d2 = np.sqrt(225.0 - d0 * d0 - d1 * d1)
        p = np.array([anchor[0] + d0, anchor[1] + d1, anchor[2] + d2], np.float32)
        z = p[2]
        for _ in range(40):
            z = np.nextafter(z, np.float32(-np.inf))
        for _ in range(80):
            z = np.nextafter(z, np.float32(np.inf))
            q = np.array([p[0], p[1], z], np.float32)
            fu, un = M.dist(anchor, q, True), M.dist(anchor, q, False)
            if (fu < M.CUTOFF) != (un < M.CUTOFF):
                found.append(q)
                break
    return found


def crafted():
    """-> (coords {key: float32 [3, L]}, raw {key: bool}, names {key: str}, alignments [(query key, target key, qStart, dbStart, cigar)])"""
    rng = np.random.default_rng(20251017)

    def walk(L, step=3.8):
        v = rng.normal(size=(L, 3))
        v = v / np.linalg.norm(v, axis=1)[:, None] * step
        return grid(np.cumsum(v, axis=0).T)

    def line(L, step, noise=0.4):
        p = np.zeros((3, L))
        p[0] = np.arange(L) * step
        p[1:] = rng.normal(scale=noise, size=(2, L))
        return p

    c, raw, names = {}, {}, {}
    c[0] = walk(40); names[0] = "qwalk"
    t = np.array(c[0], np.float64) + rng.normal(scale=0.9, size=(3, 40))
    c[1] = grid(np.concatenate([t[:, :10], t[:, 9:10] + [[1.5], [2.0], [1.0]], t[:, 9:10] + [[3.0], [3.5], [2.0]], t[:, 10:]], axis=1)); names[1] = "twalk"
    p = line(30, 3.8)
    p[2, 12] += 28.0            # residue 12: no neighbour inside 15 A
    p[0, 29] += 25.0            # the last residue neither
    c[2] = grid(p); names[2] = "qiso"
    c[3] = grid(line(6, 20.0, 0.0)); names[3] = "qalliso"
    c[4] = grid(np.array([[0, 10, 20, 30, 40, 49, 64], [0, 0, 0, 0, 0, 12, 12], [0, 0, 0, 0, 0, 0, 0]], np.float64)); names[4] = "qexact"
    c[5] = grid(np.array([[0, 10.5, 21.5, 33.5, 47.5, 56, 70], [0, 0, 0, 0, 0, 12, 12], [0, 0, 0, 0, 0, 0, 0]], np.float64)); names[5] = "texact"
    anchor = np.array([1.25, -2.5, 0.75], np.float32)
    partners = straddling_partners(rng, anchor, 6)
    filler = [anchor + np.array([3.8 * (i + 1), 0.5 * i, -0.25 * i], np.float32) for i in range(5)]
    c[6] = np.array([anchor] + partners + filler, np.float32).T.copy(); raw[6] = True; names[6] = "qrawfused"
    c[7] = grid(np.array(c[6], np.float64) + rng.normal(scale=0.7, size=c[6].shape)); names[7] = "trawfused"
    aln = [(0, 0, 0, 0, "40M"), (0, 1, 1, 1, "9M2D27M1I2M"), (0, 2, 3, 0, "5I20M"),
           (2, 0, 0, 2, "30M"), (2, 2, 0, 0, "30M"), (2, 1, 2, 0, "2D26M"),
           (3, 0, 0, 4, "6M"), (3, 3, 0, 0, "6M"),
           (4, 5, 0, 0, "7M"), (4, 4, 0, 0, "7M"), (4, 5, 0, 0, "5M"),
           (6, 7, 0, 0, "12M"), (6, 6, 0, 0, "12M"), (6, 7, 0, 1, "3M1D7M")]
    return c, raw, names, aln


def write_crafted(work):
    c, raw, names, aln = crafted()
    seq = {k: ("A" * v.shape[1] + "\n").encode() for k, v in c.items()}
    write_db(os.path.join(work, "cdb"), seq, 0)
    write_db(os.path.join(work, "cdb_ss"), {k: ("D" * v.shape[1] + "\n").encode() for k, v in c.items()}, 0)
    write_db(os.path.join(work, "cdb_h"), {k: (names[k] + "\n").encode() for k in c}, 12)
    ca = {}
    for k, v in c.items():
        ca[k] = (np.ascontiguousarray(v, "<f4").tobytes() if raw.get(k) else M.encode16(v)) + b"\n"
        assert (M.decode(ca[k], v.shape[1]) == v).all(), k
    write_db(os.path.join(work, "cdb_ca"), ca, 101)
    open(os.path.join(work, "cdb.lookup"), "w").write("".join(f"{k}\t{names[k]}\t{k}\n" for k in sorted(c)))
    open(os.path.join(work, "cdb.source"), "w").write("".join(f"{k}\t{names[k]}\n" for k in sorted(c)))
    per_q = {}
    for q, t, qs, ts, cig in aln:
        bt = M.expand(cig)
        qe = qs + sum(ch in "MI" for ch in bt) - 1
        te = ts + sum(ch in "MD" for ch in bt) - 1
        assert qe < c[q].shape[1] and te < c[t].shape[1], (q, t, cig)
        per_q.setdefault(q, []).append(f"{t}\t100\t0.500\t1.000E-05\t{qs}\t{qe}\t{c[q].shape[1]}\t{ts}\t{te}\t{c[t].shape[1]}\t{cig}\n")
    write_db(os.path.join(work, "caln"), {q: "".join(v).encode() for q, v in per_q.items()}, 5)
    return c, names, aln


def main():
    if not os.path.exists(FS):
        raise SystemExit("build the reference first: bash oracle/build_ref_full.sh cpu")
    work = os.path.join(ROOT, "oracle", "_ref_full", "ca_work")
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    run([FS, "createdb", EXAMPLE, "db", "--threads", "1", "-v", "1"], work)
    assert os.path.exists(os.path.join(work, "db_ca.dbtype"))
    run([FS, "makepaddedseqdb", "db", "db_pad", "--threads", "1", "-v", "1"], work)
    assert os.path.exists(os.path.join(work, "db_pad_ca.dbtype"))
    manifest = {"reference": "steineggerlab/foldseek, binary from oracle/build_ref_full.sh cpu", "links": {}, "runs": {}, "convert_runs": {}}
    for name, pos in (("pref", ["db_ss", "db_ss"]), ("pref_pad", ["db_ss", "db_pad_ss"])):
        run([FS, "ungappedprefilter"] + pos + [name] + UNGAPPED_PAR, work)
        manifest["runs"][name] = {"module": "ungappedprefilter", "positional": pos, "parameters": UNGAPPED_PAR}
        assert count_lines(os.path.join(work, name)) == 144
    for name, (pos, par, lines) in ALIGN_RUNS.items():
        run([FS, "structurealign"] + pos + [name] + par, work)
        n = count_lines(os.path.join(work, name))
        assert lines is None or n == lines, (name, n, lines)
        manifest["runs"][name] = {"module": "structurealign", "positional": pos, "parameters": par, "lines": n}
    run([FS, "convertalis", "db", "db", "aln_l0", "conv_lddt.m8"] + CONVERT_PAR, work)
    manifest["convert_runs"]["conv_lddt.m8"] = {"module": "convertalis", "positional": ["db", "db", "aln_l0"], "parameters": CONVERT_PAR}
    c, names, aln = write_crafted(work)
    run([FS, "convertalis", "cdb", "cdb", "caln", "conv_crafted.m8"] + CONVERT_PAR, work)
    manifest["convert_runs"]["conv_crafted.m8"] = {"module": "convertalis", "positional": ["cdb", "cdb", "caln"], "parameters": CONVERT_PAR}
    # the crafted records do what they were made for (checked with the independent model against what the reference printed)
    rows = [l.rstrip("\n").split("\t") for l in open(os.path.join(work, "conv_crafted.m8"))]
    order = sorted(range(len(aln)), key=lambda i: aln[i][0])          # stable: convertalis walks the queries in key order, records in file order
    told_apart = 0
    for row, i in zip(rows, order):
        q, t, qs, ts, cig = aln[i]
        assert row[0] == names[q] and row[1] == names[t], (row[:2], names[q], names[t])
        fused = M.columns(c[q], c[t], qs, ts, cig, True)
        unfused = M.columns(c[q], c[t], qs, ts, cig, False)
        avg, n = M.average(fused)
        if n > 0:
            assert row[3] == M.lddt_text(avg) and row[4] == M.lddtfull(fused), (names[q], names[t], cig, row[3], M.lddt_text(avg))
        if q == 6 and (np.nan_to_num(fused) != np.nan_to_num(unfused)).any():
            told_apart += 1
    assert told_apart > 0, "no crafted record tells the fused dist() from the unfused one"
    manifest["crafted"] = {"alignments": [[q, t, qs, ts, cig] for q, t, qs, ts, cig in aln], "records_that_pin_the_fused_distance": told_apart}
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    for f in sorted(os.listdir(work)):
        p = os.path.join(work, f)
        if os.path.islink(p):
            manifest["links"][f] = os.path.basename(os.readlink(p))
            continue
        if os.path.isdir(p) or "_tmp" in f or ".idx" in f:
            continue
        if f.endswith(".m8") and os.path.getsize(p) > 50000:      # large text outputs are frozen gzip-compressed (mtime 0: reproducible bytes)
            with open(os.path.join(OUT, f + ".gz"), "wb") as rawf, gzip.GzipFile(filename="", mode="wb", fileobj=rawf, mtime=0) as gz:
                gz.write(open(p, "rb").read())
            continue
        shutil.copy(p, os.path.join(OUT, f))
    json.dump(manifest, open(os.path.join(OUT, "MANIFEST.json"), "w"), indent=1, sort_keys=True)
    n = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print(f"{len(os.listdir(OUT))} files, {n} bytes -> {OUT}")


if __name__ == "__main__":
    main()
