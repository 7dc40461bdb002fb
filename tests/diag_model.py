"""Independent model of single-diagonal rescoring, written from the reference's ungappedAlignment + ungappedAlignStructure
(structurerescorediagonal.cpp:23-104) alone: plain Python / numpy ints, no call into foldseek_amd.  tests/test_diag_model.py holds it to what the
reference binary wrote (tests/golden/scop_v1/resc_*), tests/test_diag_gpu.py holds k_diag_rescore to it.

Sequences are code arrays 0..20; matrices are [21][21] integer arrays indexed [query code][target code]."""
import os

import numpy as np

OK, NO_OVERLAP, UNDEFINED, BAD_ID = 0, 1, 2, 3
FIELDS = ("score", "startPos", "endPos", "revScore", "diagonalLen", "identicalAA", "status", "reserved")
LETTERS = "ACDEFGHIKLMNPQRSTVWYX"


def scan(cells):
    """ungappedAlignment (:31-49): (maxScore, maxStartPos, maxEndPos) of the running sum over `cells`; the sum resets when it is <= 0, a new
    maximum is taken only when it is strictly greater"""
    max_score, max_end, max_start, min_pos, score = 0, 0, 0, -1, 0
    for pos, c in enumerate(cells):
        score += c
        if score <= 0:
            score = 0
            min_pos = pos
        if score > max_score:
            max_end, max_start, max_score = pos, min_pos + 1, score
    return max_score, max_start, max_end


def scan_events(cells):
    """what the tie rules of `scan` met on this diagonal: (the sum returned to exactly 0 after a positive stretch, times the final maximum was reached,
    first position at which it was reached or -1)"""
    score, back_to_zero, sums = 0, False, []
    for c in cells:
        prev = score
        score += c
        if score <= 0:
            back_to_zero = back_to_zero or (prev > 0 and score == 0)
            score = 0
        sums.append(score)
    top = max(sums) if sums else 0
    return back_to_zero, (sums.count(top) if top > 0 else 0), (sums.index(top) if top > 0 else -1)


def _cells(m3, mA, s3a, sAa, s3b, sAb, n):
    return [int(m3[s3a[p]][s3b[p]]) + int(mA[sAa[p]][sAb[p]]) for p in range(n)]


def rescore(qA, q3, tA, t3, diagonal, m3, mA):
    """one (query, target, diagonal): dict of the eight fields of fsgpu_diag_res.  With status UNDEFINED the forward fields are valid and revScore is
    not defined (the reference reads past the query there, :96-99)."""
    Lq, Lt = len(q3), len(t3)
    diagonal = int(diagonal)
    dist = abs(diagonal)
    r = dict(score=0, startPos=-1, endPos=-1, revScore=0, diagonalLen=0, identicalAA=0, status=NO_OVERLAP, reserved=0)
    qA, q3, tA, t3 = ([int(x) for x in s] for s in (qA, q3, tA, t3))
    qrA, qr3 = qA[::-1], q3[::-1]
    if diagonal >= 0 and dist < Lq:
        n = min(Lt, Lq - dist)
        r["diagonalLen"] = n
        r["score"], r["startPos"], r["endPos"] = scan(_cells(m3, mA, q3[dist:], qA[dist:], t3, tA, n))
        r["revScore"] = scan(_cells(m3, mA, qr3[dist:], qrA[dist:], t3, tA, n))[0]
        r["identicalAA"] = sum(qA[dist + p] == tA[p] for p in range(r["startPos"], r["endPos"] + 1))
        r["status"] = OK
    elif diagonal < 0 and dist < Lt:
        n = min(Lt - dist, Lq)
        r["diagonalLen"] = n
        r["score"], r["startPos"], r["endPos"] = scan(_cells(m3, mA, q3, qA, t3[dist:], tA[dist:], n))
        r["identicalAA"] = sum(qA[p] == tA[dist + p] for p in range(r["startPos"], r["endPos"] + 1))
        if dist + n > Lq:
            r["status"] = UNDEFINED
        else:
            # literally (:96-99): seq3Di1 = qRev3Di, seqAA1 = qAA, seq3Di2 = qRevAA + dist, seqAA2 = tAA + dist
            r["revScore"] = scan(_cells(m3, mA, qr3, qA, qrA[dist:], tA[dist:], n))[0]
            r["status"] = OK
    return r


def rescore_pair(queries, targets, pair, m3, mA):
    """queries / targets: lists of (AA codes, 3Di codes); pair = (query, target, diagonal) with ids as unsigned 32-bit numbers"""
    q, t, d = int(pair[0]), int(pair[1]), int(pair[2])
    if q >= len(queries) or t >= len(targets):
        return dict(score=0, startPos=-1, endPos=-1, revScore=0, diagonalLen=0, identicalAA=0, status=BAD_ID, reserved=0)
    return rescore(queries[q][0], queries[q][1], targets[t][0], targets[t][1], d, m3, mA)


def forward_events(qA, q3, tA, t3, diagonal, m3, mA):
    """scan_events of the forward pass of an OK / UNDEFINED pair"""
    Lq, Lt, dist = len(q3), len(t3), abs(int(diagonal))
    if diagonal >= 0:
        n = min(Lt, Lq - dist)
        cells = _cells(m3, mA, q3[dist:], qA[dist:], t3, tA, n)
    else:
        n = min(Lt - dist, Lq)
        cells = _cells(m3, mA, q3, qA, t3[dist:], tA[dist:], n)
    return scan_events(cells)


def module_columns(r, diagonal):
    """what the module prints of an OK result (:82, :102, :116-127): score, qStart, qEnd, dbStart, dbEnd, alnLen"""
    dist = abs(int(diagonal))
    s, e = r["startPos"], r["endPos"]
    qs, qe, ds, de = (s + dist, e + dist, s, e) if diagonal >= 0 else (s, e, s + dist, e + dist)
    return r["score"] - r["revScore"], qs, qe, ds, de, max(abs(qe - qs), abs(de - ds)) + 1


def encode(letters):
    """letters -> codes in the order ACDEFGHIKLMNPQRSTVWYX, anything else -> 20"""
    return np.array([LETTERS.index(c) if c in LETTERS else 20 for c in letters], np.uint8)


def read_db(path):
    """{key: entry bytes without the terminator} straight from the files of a reference-written database"""
    if os.path.exists(path):
        data = open(path, "rb").read()
    else:
        data, k = b"", 0
        while os.path.exists(f"{path}.{k}"):
            data += open(f"{path}.{k}", "rb").read()
            k += 1
    out = {}
    for line in open(path + ".index"):
        k, off, ln = line.split()
        out[int(k)] = data[int(off):int(off) + int(ln) - 1]
    return out
