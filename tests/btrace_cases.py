"""The frozen block-aligner cases as the DEVICE aligner sees them (TEST INFRASTRUCTURE; shared by tests/test_btrace_model.py, which needs no GPU, and
tests/test_btrace_model_gpu.py).  Everything a case expects comes from the independent model (tests/ba_model.py) -- its frozen answers
(oracle/ba_kat/ours_v3.txt, which the CPU suite ties to the model line for line; tests/golden/ba_long/long_model.txt, written by the model) and the
class the generator oracle/ba_kat/make_long_cases.py derived from the model's block sizes -- never from host/block_aligner.cpp."""
import gzip
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "oracle", "ba_kat")
LONG = os.path.join(ROOT, "tests", "golden", "ba_long")
sys.path.insert(0, KAT)
import make_long_cases as G  # noqa: E402

LETTERS = G.LETTERS
CODE = {c: k for k, c in enumerate(LETTERS)}


def matrix_text(path):
    """mat_aa.txt / mat_3di.txt -> (letters, int [n, n] as written)"""
    toks = open(path).read().split()
    n = len(toks[0])
    return toks[0], np.array(list(map(int, toks[1:])), np.int64).reshape(n, n)


def device_tables():
    """(tblAA, tbl3Di int8 [27, 32], letAA, let3Di uint8 [21]) in numpy from the two matrix files: what the crate's AAMatrix::new_simple(1, -1) followed by
    one set() per letter pair leaves (each call writes both orders, so the later call wins), and code k -> LETTERS[k] - 'A'"""
    out = []
    for fn in ("mat_aa.txt", "mat_3di.txt"):
        letters, m = matrix_text(os.path.join(KAT, fn))
        t = np.full((27, 32), -128, np.int8)
        t[:26, :26] = -1
        t[np.arange(26), np.arange(26)] = 1
        for a in range(len(letters)):
            for b in range(len(letters)):
                ia, ib = ord(letters[a]) - 65, ord(letters[b]) - 65
                t[ia, ib] = t[ib, ia] = m[a, b]
        out.append(t)
    let = np.array([ord(c) - 65 for c in LETTERS], np.uint8)
    return out[0], out[1], let, let.copy()


def expand(cigar):
    """'3M1D' -> 'MMMD'"""
    ops, n = "", ""
    for ch in ("" if cigar == "-" else cigar):
        if ch.isdigit():
            n += ch
        else:
            ops += ch * int(n); n = ""
    return ops


def identical_under_m(ops, qa, ta):
    """equal letters under the M operations of a path that starts at the first letters of both strings"""
    i = j = n = 0
    for op in ops:
        if op == "M":
            n += qa[i] == ta[j]; i += 1; j += 1
        elif op == "I":
            i += 1
        else:
            j += 1
    return n


class Case:
    """one call sequence of alignStartPosBacktraceBlock: the reversed prefixes, the gap costs, the requested score, and what the model answers"""

    def __init__(self, line, answer, cls, largest, lowered, long):
        self.name, self.go, self.ge, self.rqa, self.rq3, self.rbias, self.rta, self.rt3, self.target = G.parse_case(line)
        f = answer.rstrip("\n").split("\t")
        assert f[0] == self.name, (f[0], self.name)
        self.answer = f
        self.score, self.i, self.j, self.cigar = int(f[1]), int(f[2]), int(f[3]), f[4]
        self.attempts = len(f[5].split(","))
        self.cls, self.largest, self.lowered, self.long = cls, largest, lowered, long

    def expected(self, q_end, db_end):
        """the device's record for this case as a task that ends in (q_end, db_end): dict without blockSizes"""
        if self.cls == "C":
            return dict(status=0, qStart=-1, dbStart=-1, identicalAA=0, backtrace="")
        if self.score != self.target:
            return dict(status=2, qStart=-1, dbStart=-1, identicalAA=0, backtrace="")
        ops = expand(self.cigar)
        return dict(status=1, qStart=q_end + 1 - self.i, dbStart=db_end + 1 - self.j, identicalAA=identical_under_m(ops, self.rqa, self.rta), backtrace=ops[::-1])


def short_cases():
    """the 3di cases of cases.txt with the answers of ours_v3.txt and the classes of cases_classes.txt"""
    lines = [ln for ln in open(os.path.join(KAT, "cases.txt")) if ln.strip() and ln[0] != "#"]
    answers = open(os.path.join(KAT, "ours_v3.txt")).read().splitlines()
    assert len(lines) == len(answers)
    classes = dict((f[0], (f[1], int(f[2]))) for f in (ln.split() for ln in open(os.path.join(KAT, "cases_classes.txt"))))
    out = []
    for ln, ans in zip(lines, answers):
        if ln.startswith("3di "):
            cls, largest = classes[ln.split()[1]]
            out.append(Case(ln, ans, cls, largest, 0, False))
    assert len(out) == len(classes)
    return out


def long_lines():
    with gzip.open(os.path.join(LONG, "long_cases.txt.gz"), "rt") as f:
        return [ln for ln in f if ln.startswith("3di ")]


def long_cases():
    lines = long_lines()
    answers = open(os.path.join(LONG, "long_model.txt")).read().splitlines()
    assert len(lines) == len(answers)
    out = []
    for ln, ans in zip(lines, answers):
        cls, largest, lowered = G.name_info(ln.split()[1])
        out.append(Case(ln, ans, cls, largest, lowered, True))
    return out


def model_case(name, qa, q3, bias, ta, t3, score, go=10, ge=1):
    """a handcrafted pair (FORWARD codes, the end cell is the last residue of both) through the model, now: the Case the device is held to"""
    rev = lambda x: "".join(LETTERS[c] for c in x[::-1])  # noqa: E731
    rqa, rq3, rta, rt3, rbias = rev(qa), rev(q3), rev(ta), rev(t3), [int(b) for b in bias[::-1]]
    fA, _ = G.load_matrix(os.path.join(KAT, "mat_aa.txt"))
    f3, _ = G.load_matrix(os.path.join(KAT, "mat_3di.txt"))
    attempts, res, cigar = G.ladder(rqa, rq3, rbias, rta, rt3, go, ge, score, fA, f3)
    name = f"{name}@{score}"
    line = f"3di {name} {go} {ge} {rqa} {rq3} {','.join(map(str, rbias))} {rta} {rt3}"
    return Case(line, G.answer_line(name, res, cigar, attempts), G.classify(attempts, score), max(a[2] for a in attempts), 0, False)
