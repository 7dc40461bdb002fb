"""tests/lddt_cases.py -- the frozen LDDT fixtures of tests/golden/ca_v1 (generator: tests/golden/make_ca_golden.py) as Python objects, and the model's
answers for them, computed once per test session and shared by test_lddt_model.py / test_lddt_gpu.py (TEST INFRASTRUCTURE: no project code in here)."""
import functools
import gzip
import json
import os

import numpy as np

import lddt_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ca_v1")
MANIFEST = json.load(open(os.path.join(GOLD, "MANIFEST.json")))


def gold(name):
    """path of a frozen file; a data file that the reference left as a link (padded DBs) resolves to its target"""
    return os.path.join(GOLD, MANIFEST["links"].get(name, name))


def read_db(name):
    """{key: entry bytes without the terminator} of a frozen DB"""
    data = open(gold(name), "rb").read()
    out = {}
    for line in open(os.path.join(GOLD, name + ".index")):
        k, off, ln = line.split()
        out[int(k)] = data[int(off):int(off) + int(ln) - 1]
    return out


def frozen_text(name):
    p = os.path.join(GOLD, name)
    return gzip.open(p + ".gz", "rb").read() if os.path.exists(p + ".gz") else open(p, "rb").read()


def lengths(db):
    return {int(l.split()[0]): int(l.split()[2]) - 2 for l in open(os.path.join(GOLD, db + ".index"))}


def names(db):
    return {k: v.decode().split()[0] for k, v in read_db(db + "_h").items()}


@functools.lru_cache(maxsize=None)
def coords(db):
    """{key: float32 [3, L]} decoded by the MODEL's decoder"""
    L = lengths(db)
    return {k: M.decode(e, L[k]) for k, e in read_db(db + "_ca").items()}


def records(aln):
    """[(query key, target key, qStart, dbStart, cigar)] of a frozen alignment DB, queries in key order, records in file order"""
    out = []
    for q, entry in sorted(read_db(aln).items()):
        for line in entry.decode().splitlines():
            c = line.split("\t")
            out.append((q, int(c[0]), int(c[4]), int(c[7]), c[10]))
    return out


@functools.lru_cache(maxsize=None)
def model_columns(db, aln):
    """the model's per-column values of every record of a frozen alignment DB (the query's distance matrix is computed once per query)"""
    C = coords(db)
    norms = {}
    out = []
    for q, t, qs, ts, cig in records(aln):
        if q not in norms:
            norms[q] = M.query_norm(C[q])
        out.append(M.columns(C[q], C[t], qs, ts, cig, True, norms[q]))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    # NaN payloads are not part of the contract (0 * inf on the device and in numpy are both quiet NaNs; only "is NaN" is read)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
