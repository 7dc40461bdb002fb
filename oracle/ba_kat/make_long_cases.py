#!/usr/bin/env python3
"""oracle/ba_kat/make_long_cases.py -- writes tests/golden/ba_long/long_cases.txt.gz and long_model.txt (TEST INFRASTRUCTURE ONLY).

The 3di cases of cases.txt stop at 180 residues and almost never leave block size 32.  What the DEVICE aligner (foldseek_amd/csrc/k_btrace.hpp)
adds over the host restatement only shows on longer inputs: its 128-row first pass, its 512-row second pass, the hand-back to the host path.  This
generator plants such inputs -- the families and gap-cost pairs of tools/ba_model_sweep.py, plus single long insertions / deletions between strong
flanks, pairs of 1000 residues and more, a few X residues -- in the 3di line format of cases.txt, and freezes for each the answer of the independent
model (tests/ba_model.py: BlockModel), NOT of the restatement, in the line format of ours_v3.txt.

From the model alone it also works out what the device must do with a case, and writes that into the case's name:
    <family>_<trial>_<class><largest block>[_lo<d>]@<requested score>
  class A   answered by the first pass: the requested score is reached with a starting size of 128 or less and no attempt places a block beyond 128
  class B   not A, answered by the second pass (it restarts at 32): reached with a starting size of 512 or less, no block beyond 512
  class C   neither: the device hands the hit back (status 0)
  largest block = the largest block size the model places in any attempt of the ladder 32, 64, ... until the requested score is reached
  _lo<d>    the requested score is the true SW score lowered by d = 1..5: the aligner overshoots it, the expected status is 2 (structurealign.cpp:83)
The census printed at the end is what tests/test_block_aligner.py asserts on the frozen files.

It also writes cases_classes.txt: class and largest block of every 3di case of cases.txt, whose names carry none.

usage: make_long_cases.py [processes=8] [all|short]      (deterministic: every trial draws from its own seeded generator; a few minutes on 8 cores;
       short: cases_classes.txt only)"""
import gzip
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LONG = os.path.join(ROOT, "tests", "golden", "ba_long")          # fixtures: the gzip file is binary
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, HERE)

LETTERS = "ACDEFGHIKLMNPQRSTVWYX"
SEED = 20261017
GAPS = [(10, 1), (10, 1), (8, 2), (3, 1), (15, 3)]          # tools/ba_model_sweep.py
MINIMA = {"A, starting size 32": 250, "A, starting size 64 or 128": 40, "A, largest block >= 128": 40, "B": 40, "C": 8, "status 2": 20,
          "pairs of >= 1000 residues": 10}


def load_matrix(path):
    """mat_aa.txt / mat_3di.txt -> (score(a, b) on letters as the model wants it, int64 [21, 21] on codes)"""
    toks = open(path).read().split()
    letters, vals = toks[0], list(map(int, toks[1:]))
    n = len(letters)
    tab = {}
    for a in range(n):
        for b in range(n):
            tab[(letters[a], letters[b])] = vals[a * n + b]
            tab[(letters[b], letters[a])] = vals[a * n + b]          # block_set_aamatrix sets both orders; the later call wins
    arr = np.array([[tab[(LETTERS[a], LETTERS[b])] for b in range(21)] for a in range(21)], np.int64)
    return (lambda x, y: tab.get((x, y), 1 if x == y else -1)), arr


def best_local_end(S, go, ge):
    """make_cases.best_local_end (score and end cell of the best local alignment: the first cell in row-major order that holds the maximum and was
    reached by a match), one numpy row at a time.  The horizontal gap state of a row is a running maximum: with go >= ge a gap opened from a cell that
    was itself reached by that gap never beats the gap extended, so E[j] = max over k < j of H'[k] - go - (j - 1 - k) ge with H' = max(0, diagonal, F)."""
    assert go >= ge
    n, m = S.shape
    NEG = -10 ** 9
    Hp, Fp = np.zeros(m + 1, np.int64), np.full(m + 1, NEG, np.int64)
    jj = np.arange(m + 1, dtype=np.int64)
    best, qe, te = -1, -1, -1
    for i in range(1, n + 1):
        F = np.maximum(Fp[1:] - ge, Hp[1:] - go)
        d = Hp[:-1] + S[i - 1]
        Ht = np.maximum(0, np.maximum(d, F))
        A = np.concatenate(([0], Ht)) + jj * ge
        E = np.maximum.accumulate(A)[:-1] - go - (jj[1:] - 1) * ge
        H = np.maximum(Ht, E)
        Hc = np.where(H == d, H, -1)
        mx = int(Hc.max())
        if mx > best:
            best, qe, te = mx, i - 1, int(np.argmax(Hc))
        Hp = np.concatenate(([0], H)); Fp = np.concatenate(([NEG], F))
    return best, qe, te


def ladder(qa, q3, qbias, ta, t3, go, ge, target, fA, f3):
    """the call sequence of alignStartPosBacktraceBlock through the model: [(starting size, score, largest block placed)], result, CIGAR"""
    from ba_model import BlockModel
    attempts, res, ms, M = [], (-10 ** 9, 0, 0), 32, None
    while ms <= 4096 and res[0] < target:
        M = BlockModel(qa, ta, fA, -go, -ge, ms, 4096, x_drop=-(ms * (-ge) + (-go)), q_bias=qbias, r_bias=[0] * len(ta), score2=f3, q2=q3, r2=t3)
        res = M.align()
        attempts.append((ms, res[0], max(bs for _d, _i, _j, bs in M.steps)))
        ms *= 2
    return attempts, res, (M.trace.cigar(res[1], res[2]) or "-")


def classify(attempts, target):
    """what the device does with this ladder (k_btrace.hpp: a pass ends an alignment whose block wants to grow beyond the pass's limit and does not try
    a larger starting size; the second pass restarts at 32)"""
    def answered(limit):
        for ms, score, mb in attempts:
            if ms > limit or mb > limit:
                return False
            if score >= target:
                return True
        return False
    return "A" if answered(128) else ("B" if answered(512) else "C")


def answer_line(name, res, cigar, attempts):
    return "\t".join([name, str(res[0]), str(res[1]), str(res[2]), cigar, ",".join(f"{ms}:{sc}" for ms, sc, _mb in attempts)])


def parse_case(line):
    """3di line -> (name, go, ge, qAA, q3Di, bias list, tAA, t3Di, requested score); the strings are the REVERSED prefixes"""
    f = line.split()
    assert f[0] == "3di"
    name, go, ge = f[1], int(f[2]), int(f[3])
    qa, q3, qb, ta, t3 = f[4:9]
    qbias = ([0] * len(qa) if qb == "-" else [int(x) for x in qb.split(",")] + [0] * len(qa))[:len(qa)]
    return name, go, ge, qa, q3, qbias, ta, t3, int(name.split("@")[1])


def name_info(name):
    """-> (class, largest block, lowered by) from a long case's name"""
    f = name.split("@")[0].split("_")
    lo = int(f[3][2:]) if len(f) > 3 else 0
    return f[2][0], int(f[2][1:]), lo


_W = {}


def _init():
    from foldseek_amd import api
    _W["m3"], _W["mA"] = api.Matrix(0, 2.1, 0.0), api.Matrix(1, 1.4, 0.0)
    _W["fA"], _W["sA"] = load_matrix(os.path.join(HERE, "mat_aa.txt"))
    _W["f3"], _W["s3"] = load_matrix(os.path.join(HERE, "mat_3di.txt"))
    # the committed matrix files are what every consumer of the cases reads
    assert (np.clip(_W["mA"].scores(), -128, 127) == _W["sA"]).all() and (np.clip(_W["m3"].scores(), -128, 127) == _W["s3"]).all()


def _pair(rng, fam, trial):
    """one query / target pair of a family; sweep = the families of tools/ba_model_sweep.py"""
    from foldseek_amd import synth
    p3, pA = synth.BACK_3DI / synth.BACK_3DI.sum(), synth.BACK_AA / synth.BACK_AA.sum()
    draw = lambda n: (rng.choice(20, size=n, p=p3).astype(np.uint8), rng.choice(20, size=n, p=pA).astype(np.uint8))  # noqa: E731
    if fam in ("swp", "ind"):
        sub = trial % 4
        Lq = int(rng.integers(32, 400)) if fam == "swp" else int(rng.integers(150, 400))
        q3, qa = draw(Lq)
        if sub == 1:
            a = int(rng.integers(0, Lq - 12)); n = int(rng.integers(6, 30)); q3[a:a + n] = q3[a]; qa[a:a + n] = qa[a]
        elif sub == 2:
            u = int(rng.integers(2, 6)); a = int(rng.integers(0, max(1, Lq - 8 * u)))
            for k in range(min(8 * u, Lq - a)):
                q3[a + k] = q3[a + k % u]; qa[a + k] = qa[a + k % u]
        elif sub == 3 and fam == "swp":
            q3 = rng.choice(q3[:2], size=Lq).astype(np.uint8); qa = rng.choice(qa[:3], size=Lq).astype(np.uint8)
        t3, ta = synth._mutate(rng, q3, qa, float(rng.choice([0.1, 0.2, 0.35])), float(rng.choice([0.03, 0.10, 0.2])))
        if fam == "ind" or rng.random() < 0.4:        # a long insertion / deletion: the x-drop run of a small block gives up, the caller retries with the next size
            n = int(rng.integers(20, 160)) if fam == "swp" else int(rng.integers(30, 126))
            a = int(rng.integers(1, max(2, len(t3) - 1))) if fam == "swp" else int(rng.integers(40, max(41, len(t3) - 40)))
            if rng.random() < 0.5:
                i3, ia = draw(n)
                t3 = np.concatenate([t3[:a], i3, t3[a:]]); ta = np.concatenate([ta[:a], ia, ta[a:]])
            elif len(t3) > n + 40:
                t3 = np.concatenate([t3[:a], t3[a + n:]]); ta = np.concatenate([ta[:a], ta[a + n:]])
        pad = int(rng.integers(0, 40))
    elif fam in ("gapB", "gapC"):
        # one insertion or deletion of 130 .. 500 residues (B) / more than 520 (C) between flanks strong enough to carry it
        n = int(rng.integers(130, 501)) if fam == "gapB" else int(rng.integers(521, 1000))
        fl1, fl2 = int(rng.integers(90, 150)), int(rng.integers(90, 150))
        if fam == "gapC":
            fl1, fl2 = fl1 + 40, fl2 + 40
        c3, cA = draw(fl1 + fl2)
        m3_, mA_ = synth._mutate(rng, c3, cA, 0.08, 0.02)
        cut = int(round(len(m3_) * fl1 / (fl1 + fl2)))
        i3, ia = draw(n)
        if trial % 2:                                  # insertion in the target
            q3, qa = c3, cA
            t3 = np.concatenate([m3_[:cut], i3, m3_[cut:]]); ta = np.concatenate([mA_[:cut], ia, mA_[cut:]])
        else:                                          # ... in the query
            q3 = np.concatenate([c3[:fl1], i3, c3[fl1:]]); qa = np.concatenate([cA[:fl1], ia, cA[fl1:]])
            t3, ta = m3_, mA_
        pad = int(rng.integers(0, 20))
    else:                                              # "kilo": pairs of 1000 residues and more
        Lq = int(rng.integers(1080, 1400))
        q3, qa = draw(Lq)
        t3, ta = synth._mutate(rng, q3, qa, float(rng.choice([0.1, 0.2])), float(rng.choice([0.03, 0.10])))
        if trial % 3 == 0:
            n = int(rng.integers(20, 120)); a = int(rng.integers(100, len(t3) - 100))
            i3, ia = draw(n)
            t3 = np.concatenate([t3[:a], i3, t3[a:]]); ta = np.concatenate([ta[:a], ia, ta[a:]])
        pad = int(rng.integers(0, 40))
    p3_, pa_ = draw(pad)
    t3 = np.concatenate([p3_, t3]); ta = np.concatenate([pa_, ta])
    if trial % 5 == 0:                                 # a few X residues (code 20) in both strings of both sequences
        for s3_, sa_ in ((q3, qa), (t3, ta)):
            for p in rng.integers(0, len(s3_), size=1 + len(s3_) // 120):
                s3_[p] = 20; sa_[p] = 20
    return q3, qa, t3, ta


def make(job):
    """one trial -> None or (case line, model answer line, class, largest block, lowered by, attempts, shorter prefix length)"""
    fam, trial, lower = job
    if not _W:
        _init()
    from foldseek_amd import api
    rng = np.random.default_rng([SEED, sum(ord(c) for c in fam), trial, lower])
    q3, qa, t3, ta = _pair(rng, fam, trial)
    if len(t3) < 10:
        return None
    _, _, cbA, cbS = api.align_profiles(_W["mA"], _W["m3"], qa, q3, comp_bias=True, scale=0.5)
    bias = cbA.astype(np.int64) + cbS.astype(np.int64)
    go, ge = GAPS[int(rng.integers(0, 5))]
    S = _W["s3"][q3][:, t3] + _W["sA"][qa][:, ta] + bias[:, None]
    best, qe, te = best_local_end(S, go, ge)
    if best < 25 or best >= 32767:
        return None
    if fam == "kilo" and min(qe, te) + 1 < 1000:
        return None
    d = int(rng.integers(1, 6)) if lower else 0
    target = best - d
    rev = lambda x, e: "".join(LETTERS[c] for c in x[:e + 1][::-1])  # noqa: E731
    rqa, rq3, rta, rt3 = rev(qa, qe), rev(q3, qe), rev(ta, te), rev(t3, te)
    rbias = [int(b) for b in bias[:qe + 1][::-1]]
    attempts, res, cigar = ladder(rqa, rq3, rbias, rta, rt3, go, ge, target, _W["fA"], _W["f3"])
    cls = classify(attempts, target)
    mb = max(a[2] for a in attempts)
    if lower and (res[0] == target or cls == "C"):
        return None                                    # a smaller block happened to land on the lowered score / the device would not answer: not a status-2 case
    name = f"{fam}_{trial}_{cls}{mb}" + (f"_lo{d}" if lower else "") + f"@{target}"
    line = f"3di {name} {go} {ge} {rqa} {rq3} {','.join(map(str, rbias))} {rta} {rt3}"
    return line, answer_line(name, res, cigar, attempts), cls, mb, d, len(attempts), min(qe, te) + 1


def census(names_and_attempts):
    """[(name, number of attempts, shorter prefix length)] -> the table of MINIMA"""
    c = {k: 0 for k in MINIMA}
    for name, nat, shorter in names_and_attempts:
        cls, mb, lo = name_info(name)
        c["pairs of >= 1000 residues"] += shorter >= 1000
        if lo:
            c["status 2"] += 1
            continue
        if cls == "A":
            c["A, starting size 32"] += nat == 1
            c["A, starting size 64 or 128"] += nat in (2, 3)
            c["A, largest block >= 128"] += mb >= 128
        else:
            c[cls] += 1
    return c


def short_class(line):
    """a 3di line of cases.txt -> 'name class largest-block' (the model's ladder, classified as above)"""
    if not _W:
        _init()
    name, go, ge, qa, q3, qbias, ta, t3, target = parse_case(line)
    attempts, _res, _cigar = ladder(qa, q3, qbias, ta, t3, go, ge, target, _W["fA"], _W["f3"])
    return f"{name} {classify(attempts, target)} {max(a[2] for a in attempts)}"


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    what = sys.argv[2] if len(sys.argv) > 2 else "all"
    if what in ("all", "short"):
        # the 3di cases of cases.txt carry no class in their names: the model's verdict on each goes to cases_classes.txt
        lines = [ln for ln in open(os.path.join(HERE, "cases.txt")) if ln.startswith("3di ")]
        with Pool(procs, initializer=_init) as pool:
            out = pool.map(short_class, lines, chunksize=8)
        with open(os.path.join(HERE, "cases_classes.txt"), "w") as f:
            f.write("".join(x + "\n" for x in out))
        tally = {}
        for x in out:
            k = " ".join(x.split()[1:])
            tally[k] = tally.get(k, 0) + 1
        print(f"cases.txt: {len(out)} 3di cases, class and largest block {dict(sorted(tally.items()))}", flush=True)
        if what == "short":
            return
    kept, rows = [], []
    # (family, lowered, what a case of it must still fill to be kept, trials at most, cases at most)
    plans = [("kilo", 0, ("pairs of >= 1000 residues",), 60, 99), ("gapC", 0, ("C",), 60, 99), ("gapB", 0, ("B",), 400, 99), ("gapB", 1, ("status 2",), 40, 6),
             ("ind", 0, ("A, starting size 64 or 128", "A, largest block >= 128"), 1500, 999), ("ind", 1, ("status 2",), 100, 6), ("swp", 1, ("status 2",), 200, 99),
             ("swp", 0, ("A, starting size 32", "A, starting size 64 or 128", "A, largest block >= 128"), 3000, 999)]
    quota = dict(MINIMA)
    quota["status 2"] = 26
    quota["B"], quota["C"], quota["pairs of >= 1000 residues"] = 44, 10, 12
    quota["A, starting size 64 or 128"], quota["A, largest block >= 128"] = 48, 48
    with Pool(procs, initializer=_init) as pool:
        for fam, lower, fills, most, cap in plans:
            own = 0
            for t0 in range(0, most, 4 * procs):
                c = census(rows)
                if all(c[k] >= quota[k] for k in fills) or own >= cap:
                    break
                for out in pool.map(make, [(fam, t, lower) for t in range(t0, min(most, t0 + 4 * procs))]):
                    if out is None or own >= cap:
                        continue
                    line, ans, cls, mb, d, nat, shorter = out
                    c = census(rows)
                    row = (ans.split("\t")[0], nat, shorter)
                    c2 = census(rows + [row])
                    if not any(c2[k] > c[k] and c[k] < quota[k] for k in fills):
                        continue
                    kept.append((line, ans)); rows.append(row); own += 1
            print(f"{fam}{' lowered' if lower else ''}: {own} cases kept; census {census(rows)}", flush=True)
    os.makedirs(LONG, exist_ok=True)
    with open(os.path.join(LONG, "long_cases.txt.gz"), "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as f:
            f.write(("# generated by make_long_cases.py -- 3di lines as in cases.txt\n" + "".join(ln + "\n" for ln, _a in kept)).encode())
    with open(os.path.join(LONG, "long_model.txt"), "w") as f:
        f.write("".join(a + "\n" for _ln, a in kept))
    c = census(rows)
    print(f"{len(kept)} long cases; census (minimum):")
    for k in MINIMA:
        print(f"  {k:32s} {c[k]:4d} ({MINIMA[k]})")
    for fn in ("long_cases.txt.gz", "long_model.txt"):
        print(f"  {fn}: {os.path.getsize(os.path.join(LONG, fn))} bytes")
    assert all(c[k] >= MINIMA[k] for k in MINIMA), "a class is below its minimum"


if __name__ == "__main__":
    main()
