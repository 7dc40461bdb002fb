"""Known-answer tests for the C++ restatement of the block aligner, ported from the Rust crate's own unit tests
(reference lib/mmseqs/lib/block-aligner/src/scan_block.rs:2337-2413: test_x_drop, test_trace).  The crate's BLOSUM62 /
NW1 constants are replaced by matrices that agree with them on the letters the tests use (A, R / A, T, G, C).

Ported: test_x_drop, test_trace, test_no_x_drop (:2267-2334; its one case with the nucleotide wildcard N needs NucMatrix).
NOT portable: test_bytes (:2414-2431, ByteMatrix) and test_profile (:2433-2478, AAProfile) exercise matrix / profile types
that Foldseek's path never instantiates and the restatement therefore does not contain (their C entry points are
die()-stubs in oracle/ref_block_stub.cpp).  The 3Di + AA entry point Foldseek DOES use has no known answers in the crate;
it is covered by the independent property test at the end of this file."""
import ctypes as C
import numpy as np
import pytest
from foldseek_amd import api


class OpLen(C.Structure):
    _fields_ = [("op", C.c_uint8), ("len", C.c_size_t)]


class Gaps(C.Structure):
    _fields_ = [("open", C.c_int8), ("extend", C.c_int8)]


class SizeRange(C.Structure):
    _fields_ = [("min", C.c_size_t), ("max", C.c_size_t)]


class AlignResult(C.Structure):
    _fields_ = [("score", C.c_int32), ("query_idx", C.c_size_t), ("reference_idx", C.c_size_t)]


def _scalar_build():
    """the portable (non-AVX2) statement of the same lane semantics, compiled on the fly with g++"""
    import os, subprocess, tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.join(tempfile.gettempdir(), f"fs_block_aligner_scalar_{os.getuid()}.so")
    src = os.path.join(root, "foldseek_amd", "csrc", "host", "block_aligner.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mno-avx2", "-o", out, src])
    return out


@pytest.fixture(scope="module", params=["avx2-product", "scalar"])
def ba(request):
    L = C.CDLL(api.LIB_PATH if request.param == "avx2-product" else _scalar_build())
    vp = C.c_void_p
    L.block_new_simple_aamatrix.restype = vp
    L.block_new_simple_aamatrix.argtypes = [C.c_int8, C.c_int8]
    L.block_set_aamatrix.argtypes = [vp, C.c_uint8, C.c_uint8, C.c_int8]
    L.block_new_cigar.restype = vp
    L.block_new_cigar.argtypes = [C.c_size_t, C.c_size_t]
    L.block_get_cigar.restype = OpLen
    L.block_get_cigar.argtypes = [vp, C.c_size_t]
    L.block_len_cigar.restype = C.c_size_t
    L.block_len_cigar.argtypes = [vp]
    L.block_new_padded_aa.restype = vp
    L.block_new_padded_aa.argtypes = [C.c_size_t, C.c_size_t]
    L.block_set_bytes_padded_aa.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_size_t]
    for pre in ("block_new_aa_trace_xdrop", "block_new_aa_trace"):
        getattr(L, pre).restype = vp
        getattr(L, pre).argtypes = [C.c_size_t] * 3
    for pre in ("block_align_aa_trace_xdrop", "block_align_aa_trace"):
        getattr(L, pre).argtypes = [vp, vp, vp, vp, Gaps, SizeRange, C.c_int32]
    for pre in ("block_res_aa_trace_xdrop", "block_res_aa_trace"):
        getattr(L, pre).restype = AlignResult
        getattr(L, pre).argtypes = [vp]
    for pre in ("block_cigar_aa_trace_xdrop", "block_cigar_aa_trace"):
        getattr(L, pre).argtypes = [vp, C.c_size_t, C.c_size_t, vp]
    for pre in ("block_cigar_eq_aa_trace_xdrop", "block_cigar_eq_aa_trace"):
        getattr(L, pre).argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp]
    return L


def padded(L, s, size):
    p = L.block_new_padded_aa(len(s), size)
    L.block_set_bytes_padded_aa(p, s, len(s), size)
    return p


def cigar_str(L, cg):
    names = {1: "M", 2: "=", 3: "X", 4: "I", 5: "D"}
    out = ""
    for i in range(L.block_len_cigar(cg)):
        o = L.block_get_cigar(cg, i)
        out += f"{o.len}{names[o.op]}"
    return out


def blosum_ar(L):
    m = L.block_new_simple_aamatrix(1, -1)
    L.block_set_aamatrix(m, ord("A"), ord("A"), 4)
    L.block_set_aamatrix(m, ord("A"), ord("R"), -1)
    L.block_set_aamatrix(m, ord("R"), ord("R"), 5)
    return m


def test_x_drop(ba):
    L = ba
    m = blosum_ar(L)
    g = Gaps(-11, -1)
    a = L.block_new_aa_trace_xdrop(100, 100, 16)
    L.block_align_aa_trace_xdrop(a, padded(L, b"AAAAAA", 16), padded(L, b"AAARRA", 16), m, g, SizeRange(16, 16), 1)
    r = L.block_res_aa_trace_xdrop(a)
    assert (r.score, r.query_idx, r.reference_idx) == (14, 6, 6)
    L.block_align_aa_trace_xdrop(a, padded(L, b"A" * 44, 16), padded(L, b"A" * 15 + b"R" * 16 + b"A" * 13, 16), m, g, SizeRange(16, 16), 1)
    r = L.block_res_aa_trace_xdrop(a)
    assert (r.score, r.query_idx, r.reference_idx) == (60, 15, 15)
    a = L.block_new_aa_trace_xdrop(2048, 2048, 2048)
    s = b"A" * 2048
    L.block_align_aa_trace_xdrop(a, padded(L, s, 2048), padded(L, s, 2048), m, g, SizeRange(2048, 2048), 100)
    r = L.block_res_aa_trace_xdrop(a)
    assert (r.score, r.query_idx, r.reference_idx) == (8192, 2048, 2048)


def test_trace(ba):
    L = ba
    m = blosum_ar(L)
    g = Gaps(-11, -1)
    cg = L.block_new_cigar(100, 100)
    a = L.block_new_aa_trace(100, 100, 16)
    q, r = padded(L, b"AAAAAA", 16), padded(L, b"AAARRA", 16)
    L.block_align_aa_trace(a, q, r, m, g, SizeRange(16, 16), 0)
    res = L.block_res_aa_trace(a)
    assert (res.score, res.query_idx, res.reference_idx) == (14, 6, 6)
    L.block_cigar_eq_aa_trace(a, q, r, res.query_idx, res.reference_idx, cg)
    assert cigar_str(L, cg) == "3=2X1="
    q, r = padded(L, b"AAA", 16), padded(L, b"AAAA", 16)
    L.block_align_aa_trace(a, q, r, m, g, SizeRange(16, 16), 0)
    res = L.block_res_aa_trace(a)
    assert (res.score, res.query_idx, res.reference_idx) == (1, 3, 4)
    L.block_cigar_aa_trace(a, res.query_idx, res.reference_idx, cg)
    assert cigar_str(L, cg) == "3M1D"
    nw = L.block_new_simple_aamatrix(1, -1)
    g2 = Gaps(-2, -1)
    q, r = padded(L, b"TTTTTTTTAAAAAAATTTTTTTTT", 16), padded(L, b"TTAAAAAAATTTTTTTTTTTT", 16)
    L.block_align_aa_trace(a, q, r, nw, g2, SizeRange(16, 16), 0)
    res = L.block_res_aa_trace(a)
    assert (res.score, res.query_idx, res.reference_idx) == (7, 24, 21)
    L.block_cigar_aa_trace(a, res.query_idx, res.reference_idx, cg)
    assert cigar_str(L, cg) == "2M6I16M3D"
    a = L.block_new_aa_trace(100, 100, 32)
    q, r = padded(L, b"AAAAAAAAATTGCGCT", 32), padded(L, b"AAAAAAAAAGCGC", 32)
    L.block_align_aa_trace(a, q, r, nw, g2, SizeRange(32, 32), 0)
    res = L.block_res_aa_trace(a)
    assert (res.score, res.query_idx, res.reference_idx) == (8, 16, 13)
    L.block_cigar_eq_aa_trace(a, q, r, res.query_idx, res.reference_idx, cg)
    assert cigar_str(L, cg) == "9=2I4=1I"
    m2 = L.block_new_simple_aamatrix(2, -1)
    L.block_align_aa_trace(a, q, r, m2, Gaps(-5, -2), SizeRange(32, 32), 0)
    res = L.block_res_aa_trace(a)
    assert (res.score, res.query_idx, res.reference_idx) == (14, 16, 13)
    L.block_cigar_eq_aa_trace(a, q, r, res.query_idx, res.reference_idx, cg)
    assert cigar_str(L, cg) == "9=2I4=1I"


def test_no_x_drop_scores(ba):
    """scan_block.rs:2267-2334 (test_no_x_drop), the AA and the N-free nucleotide cases"""
    L = ba
    m = blosum_ar(L)
    g = Gaps(-11, -1)
    a = L.block_new_aa_trace(100, 100, 16)

    def score(q, r, mat=m, gaps=g):
        L.block_align_aa_trace(a, padded(L, q, 16), padded(L, r, 16), mat, gaps, SizeRange(16, 16), 0)
        return L.block_res_aa_trace(a).score

    assert score(b"AARA", b"AAAA") == 11
    assert score(b"AARAAAA", b"AAAAAAAA") == 12
    assert score(b"AAAA", b"AAAA") == 16
    assert score(b"RRRR", b"AAAA") == -4
    assert score(b"AAA", b"AAAA") == 1
    nw = L.block_new_simple_aamatrix(1, -1)
    g2 = Gaps(-2, -1)
    assert score(b"A" * 32, b"A" * 32, nw, g2) == 32
    assert score(b"T" * 32, b"A" * 32, nw, g2) == -32
    assert score(b"TA" * 16, b"A" * 32, nw, g2) == 0
    assert score(b"TTTTTTTTAAAAAAATTTTTTTTT", b"TTAAAAAAATTTTTTTTTTTT", nw, g2) == 7
    assert score(b"C", b"AAAA", nw, g2) == -5
    assert score(b"AAAA", b"C", nw, g2) == -5


# ---- independent property test of the 3Di + AA path (align_3di: the one Foldseek uses) ---------------------------------
# CIGAR parity against the Rust crate cannot be pinned in this environment (no cargo / rustc: the crate cannot be built, and
# the compiled reference links THIS restatement for its block_* symbols).  What can be checked independently of the
# restatement: every backtrace it emits, re-scored position by position against the 3Di + AA matrices, the position bias and
# the affine gap costs, must add up to the optimum of a plain O(n^2) scalar Gotoh recurrence (written here, sharing no code
# with the aligner) for the best alignment ENDING at the given cell -- and the start positions must be the ones the path
# implies.  Ties between co-optimal paths stay unpinned (that is exactly what the crate's tie rules decide).
def _gotoh_end_anchored(S, go, ge):
    """best score of an alignment that ends exactly at the last cell of S (local start): scalar affine-gap DP, int64"""
    n, m = S.shape
    NEG = -10 ** 9
    H = np.zeros((n + 1, m + 1), np.int64)
    E = np.full((n + 1, m + 1), NEG, np.int64)
    F = np.full((n + 1, m + 1), NEG, np.int64)
    best_end = NEG
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            E[i, j] = max(E[i, j - 1] - ge, H[i, j - 1] - go)
            F[i, j] = max(F[i - 1, j] - ge, H[i - 1, j] - go)
            d = H[i - 1, j - 1] + S[i - 1, j - 1]
            H[i, j] = max(0, d, E[i, j], F[i, j])
    # value of the best path ending at (n, m) with a match: a path may START anywhere (local start = restart at 0)
    return int(H[n - 1, m - 1] + S[n - 1, m - 1]) if n and m else 0


def _rescore(bt, S, q0, t0, go, ge):
    """score of the backtrace string (M / I = query only / D = target only) walked from (q0, t0)"""
    i, j, score, prev = q0, t0, 0, "M"
    for op in bt:
        if op == "M":
            score += int(S[i, j]); i += 1; j += 1
        elif op == "I":
            score -= go if prev != "I" else ge; i += 1
        else:
            score -= go if prev != "D" else ge; j += 1
        prev = op
    return score, i, j


@pytest.mark.parametrize("atype", [2, 0])
def test_align_3di_backtraces_rescore_to_the_scalar_optimum(atype):
    from foldseek_amd import synth
    rng = np.random.default_rng(20260924 + atype)
    m3 = api.Matrix(0, 2.1, 0.0)
    mA = api.Matrix(1, 1.4 if atype == 2 else 0.0, 0.0)
    s3, sA = m3.scores().astype(np.int64), mA.scores().astype(np.int64)
    checked = gapped = 0
    for trial in range(140):
        Lq, Lt = int(rng.integers(20, 90)), int(rng.integers(20, 90))
        q3 = rng.choice(20, size=Lq, p=synth.BACK_3DI / synth.BACK_3DI.sum()).astype(np.uint8)
        qa = rng.choice(20, size=Lq, p=synth.BACK_AA / synth.BACK_AA.sum()).astype(np.uint8)
        # target = mutated copy of a query window (substitutions + an indel or two), so alignments are long and gapped
        a, b = sorted(rng.integers(0, Lq, size=2))
        if b - a < 12:
            a, b = 0, Lq
        t3, ta = synth._mutate(rng, q3[a:b], qa[a:b], 0.25, 0.12)
        pad = int(rng.integers(0, 12))
        t3 = np.concatenate([rng.integers(0, 20, pad).astype(np.uint8), t3]); ta = np.concatenate([rng.integers(0, 20, pad).astype(np.uint8), ta])
        if len(t3) < 8:
            continue
        _, _, cbA, cbS = api.align_profiles(mA, m3, qa, q3, comp_bias=True, scale=0.5)
        S = s3[q3][:, t3] + sA[qa][:, ta] + (cbA.astype(np.int64) + cbS.astype(np.int64))[:, None]
        # pick the end cell of the best local alignment (textbook recurrence) and the best score ending there
        best, qe, te = -1, -1, -1
        NEG = -10 ** 9
        n, m = S.shape
        H = np.zeros((n + 1, m + 1), np.int64); E = np.full((n + 1, m + 1), NEG, np.int64); F = np.full((n + 1, m + 1), NEG, np.int64)
        for i in range(1, n + 1):
            for j in range(1, m + 1):
                E[i, j] = max(E[i, j - 1] - 1, H[i, j - 1] - 10); F[i, j] = max(F[i - 1, j] - 1, H[i - 1, j] - 10)
                H[i, j] = max(0, H[i - 1, j - 1] + S[i - 1, j - 1], E[i, j], F[i, j])
                if H[i, j] > best and H[i, j] == H[i - 1, j - 1] + S[i - 1, j - 1]:
                    best, qe, te = int(H[i, j]), i - 1, j - 1
        if best < 25:
            continue
        assert best == _gotoh_end_anchored(S[:qe + 1, :te + 1], 10, 1)
        ok, qs, ds, ident, bt = api.block_backtrace(mA, m3, qa, q3, cbA, cbS, ta, t3, qe, te, best, 10, 1)
        assert ok, (trial, best, qe, te)
        score, qi, tj = _rescore(bt, S, qs, ds, 10, 1)
        assert (qi, tj) == (qe + 1, te + 1), "the backtrace must end in the end cell"
        assert score == best, (trial, score, best, bt)
        assert ident == sum(1 for k, (i, j) in enumerate(_walk(bt, qs, ds)) if qa[i] == ta[j])
        assert bt[0] == "M" and bt[-1] == "M"
        checked += 1
        gapped += ("I" in bt) or ("D" in bt)
    assert checked >= 100 and gapped >= 30


def _walk(bt, i, j):
    for op in bt:
        if op == "M":
            yield i, j
            i += 1; j += 1
        elif op == "I":
            i += 1
        else:
            j += 1


# ---- the crate's tie rules, stated independently, against the restatement on tie-rich inputs ---------------------------------------
# When the block covers the whole DP matrix (block size >= both lengths, global variant) the crate computes ONE `right` block
# (scan_block.rs:268-330: the first Grow step places a block of the full width with right = true), so the adaptive trajectory plays no role
# and the backtrace is a function of the recurrences and of three documented tie rules (scan_block.rs:1492-1576, 1870-1925):
#   C (gap consuming the reference, op D) = max(C[i][j-1] + ext, D[i][j-1] + open); "gap beginning" bit = (C == open candidate): ties -> open
#   R (gap consuming the query, op I)     = max(R[i-1][j] + ext, D'[i-1][j] + open) (inclusive prefix scan); bit likewise: ties -> open
#   D = max(D[i-1][j-1] + s, C, R); trace bits (D == C), (D == R); OP_LUT for right blocks: C before R before the diagonal.
# _rule_model below is a scalar statement of exactly that, written from the crate's source and sharing no code with block_aligner.cpp.  It is
# first held against the crate's OWN known answers (test_trace: "3M1D", "2M6I16M3D", the two "9=2I4=1I"), then the restatement is held
# against it on homopolymers, tandem repeats and equal-score substitution / gap alternatives -- inputs where co-optimal paths abound.
def _rule_model(q, r, score, go, ge, first_down=None):
    """global alignment of q vs r with the crate's tie rules; returns (score, cigar with M/I/D runs).  Cells of DP rows >= first_down lie in
    `down` blocks (right = false), where OP_LUT mirrors the precedence: R (op I) before C (op D) before the diagonal"""
    n, m = len(q), len(r)
    NEG = -10 ** 6
    D = [[NEG] * (m + 1) for _ in range(n + 1)]
    Cm = [[NEG] * (m + 1) for _ in range(n + 1)]
    Rm = [[NEG] * (m + 1) for _ in range(n + 1)]
    c_open = [[False] * (m + 1) for _ in range(n + 1)]
    r_open = [[False] * (m + 1) for _ in range(n + 1)]
    t_c = [[False] * (m + 1) for _ in range(n + 1)]
    t_r = [[False] * (m + 1) for _ in range(n + 1)]
    for j in range(m + 1):
        pre_above = NEG                       # D' (before the max with R) of the cell above in this column
        for i in range(n + 1):
            if i == 0 and j == 0:
                D[0][0] = 0
                pre_above = 0
                continue
            c = NEG
            if j > 0:
                oc, ec = D[i][j - 1] + go, Cm[i][j - 1] + ge
                c = max(oc, ec)
                c_open[i][j] = c == oc
            Cm[i][j] = c
            diag = D[i - 1][j - 1] + score(q[i - 1], r[j - 1]) if i > 0 and j > 0 else NEG
            pre = max(diag, c)
            rr = NEG
            if i > 0:
                orr, er = pre_above + go, Rm[i - 1][j] + ge
                rr = max(orr, er)
                r_open[i][j] = rr == orr
            Rm[i][j] = rr
            D[i][j] = max(pre, rr)
            t_c[i][j] = D[i][j] == c
            t_r[i][j] = D[i][j] == rr
            pre_above = pre
    ops, i, j, table = [], n, m, "D"
    while i > 0 or j > 0:
        if table == "D":
            down = first_down is not None and i >= first_down
            first, second = (("R", t_r), ("C", t_c)) if down else (("C", t_c), ("R", t_r))
            take = first[0] if first[1][i][j] else (second[0] if second[1][i][j] else "M")
            if take == "C":
                ops.append("D"); table = "D" if c_open[i][j] else "C"; j -= 1
            elif take == "R":
                ops.append("I"); table = "D" if r_open[i][j] else "R"; i -= 1
            else:
                ops.append("M"); i -= 1; j -= 1
        elif table == "C":
            ops.append("D"); table = "D" if c_open[i][j] else "C"; j -= 1
        else:
            ops.append("I"); table = "D" if r_open[i][j] else "R"; i -= 1
    ops.reverse()
    out, k = "", 0
    while k < len(ops):
        e = k
        while e < len(ops) and ops[e] == ops[k]:
            e += 1
        out += f"{e - k}{ops[k]}"
        k = e
    return D[n][m], out


def _simple(match, mismatch):
    return lambda a, b: match if a == b else mismatch


def _blosum_ar_score(a, b):
    return {("A", "A"): 4, ("R", "R"): 5}.get((a, b), -1)


def test_rule_model_reproduces_the_crates_own_known_answers():
    """the independent statement of the tie rules is itself pinned: scan_block.rs:2366-2412 (test_trace)"""
    assert _rule_model("AAA", "AAAA", _blosum_ar_score, -11, -1) == (1, "3M1D")
    assert _rule_model("TTTTTTTTAAAAAAATTTTTTTTT", "TTAAAAAAATTTTTTTTTTTT", _simple(1, -1), -2, -1) == (7, "2M6I16M3D")
    assert _rule_model("AAAAAAAAATTGCGCT", "AAAAAAAAAGCGC", _simple(1, -1), -2, -1)[0] == 8
    assert _rule_model("AAAAAAAAATTGCGCT", "AAAAAAAAAGCGC", _simple(1, -1), -2, -1)[1].replace("M", "=") == "9=2I4=1I"
    assert _rule_model("AAAAAAAAATTGCGCT", "AAAAAAAAAGCGC", _simple(2, -1), -5, -2) == (14, "9M2I4M1I")
    assert _rule_model("AAAAAA", "AAARRA", _blosum_ar_score, -11, -1) == (14, "6M")


def _tie_rich_cases():
    rng = np.random.default_rng(7)
    cases = [("AAAA", "AAA"), ("AAA", "AAAA"), ("AAAAAAAA", "AAAAA"), ("ATATATAT", "ATATAT"), ("ATATAT", "ATATATATAT"), ("AATTAATT", "AATT"),
             ("ACGTACGTACGT", "ACGTACGT"), ("A", "AAAA"), ("AAAA", "A"), ("AT", "TA"), ("ATAT", "TATA"), ("AAAT", "TAAA"), ("GATTACA", "GCATGCT"),
             ("AAAAAAAAAAAAAAAAAAAAAAAAAAAAAA", "AAAAAAAAAAAAAAAAAAAAAAAA"), ("ACACACACACACACAC", "CACACACACACACA"), ("AGAGAGAG", "GAGAGAGAGAGA")]
    for _ in range(160):
        unit = "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 4))))
        a = unit * int(rng.integers(1, 12)) + "".join(rng.choice(list("AC"), size=int(rng.integers(0, 4))))
        b = unit * int(rng.integers(1, 12)) + "".join(rng.choice(list("AC"), size=int(rng.integers(0, 4))))
        if rng.random() < 0.5:
            a, b = a[::-1], b[::-1]
        if 0 < len(a) <= 60 and 0 < len(b) <= 60:
            cases.append((a, b))
    return cases


@pytest.mark.parametrize("scheme", [(1, -1, -2, -1), (2, -1, -5, -2), (1, -1, -3, -1), (3, -2, -4, -2), (1, -3, -2, -1)])
def test_restatement_follows_the_crates_tie_rules_on_tie_rich_inputs(ba, scheme):
    """homopolymers, tandem repeats, shifted repeats: every co-optimal choice (which gap, where it opens, gap vs substitution) must come out
    the way the crate's rules decide it"""
    L = ba
    match, mismatch, go, ge = scheme
    m = L.block_new_simple_aamatrix(match, mismatch)
    g = Gaps(go, ge)
    cg = L.block_new_cigar(128, 128)
    a = L.block_new_aa_trace(128, 128, 64)
    checked = gapped = 0
    for q, r in _tie_rich_cases():
        pq, pr = padded(L, q.encode(), 64), padded(L, r.encode(), 64)
        L.block_align_aa_trace(a, pq, pr, m, g, SizeRange(64, 64), 0)
        res = L.block_res_aa_trace(a)
        L.block_cigar_aa_trace(a, res.query_idx, res.reference_idx, cg)
        want_score, want_cigar = _rule_model(q, r, _simple(match, mismatch), go, ge)
        assert (res.score, res.query_idx, res.reference_idx) == (want_score, len(q), len(r)), (q, r, scheme)
        assert cigar_str(L, cg) == want_cigar, (q, r, scheme, cigar_str(L, cg), want_cigar)
        checked += 1
        gapped += ("I" in want_cigar) or ("D" in want_cigar)
    assert checked >= 150 and gapped >= 100


@pytest.mark.parametrize("scheme", [(1, -1, -2, -1), (2, -1, -5, -2), (1, -3, -2, -1)])
def test_restatement_follows_the_mirrored_rules_in_down_blocks(ba, scheme):
    """block size 16 and a reference of at most 15 residues: the first block spans every column, so every later step is forced DOWN
    (scan_block.rs:412-421) -- DP rows from 16 on lie in `down` blocks, whose OP_LUT half prefers R (op I) to C (op D)"""
    L = ba
    match, mismatch, go, ge = scheme
    m = L.block_new_simple_aamatrix(match, mismatch)
    g = Gaps(go, ge)
    cg = L.block_new_cigar(128, 128)
    a = L.block_new_aa_trace(128, 128, 16)
    rng = np.random.default_rng(11)
    checked = differs = 0
    for k in range(4000):
        if k % 12 == 0:         # repeats
            unit = "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 4))))
            r = (unit * 8)[: int(rng.integers(3, 16))]
            q = (unit * 30)[: int(rng.integers(17, 60))]
        else:                   # three-letter strings: equal-score gap / substitution alternatives in every region of the matrix
            r = "".join(rng.choice(list("ATC"), size=int(rng.integers(3, 16))))
            q = "".join(rng.choice(list("ATC"), size=int(rng.integers(17, 40))))
        want_score, want_cigar = _rule_model(q, r, _simple(match, mismatch), go, ge, first_down=16)
        decisive = want_cigar != _rule_model(q, r, _simple(match, mismatch), go, ge)[1]
        if not decisive and k % 8:
            continue            # the aligner runs on every case the mirrored rule decides and on a sample of the others
        pq, pr = padded(L, q.encode(), 16), padded(L, r.encode(), 16)
        L.block_align_aa_trace(a, pq, pr, m, g, SizeRange(16, 16), 0)
        res = L.block_res_aa_trace(a)
        L.block_cigar_aa_trace(a, res.query_idx, res.reference_idx, cg)
        assert res.score == want_score, (q, r, scheme)
        assert cigar_str(L, cg) == want_cigar, (q, r, scheme, cigar_str(L, cg), want_cigar)
        differs += decisive
        checked += 1
    assert checked >= 450 and differs >= 15          # the mirrored rule decides the path on these inputs


# ---- the block TRAJECTORY and the X-drop stop rule, stated a second time ----------------------------------------------------------------
# tests/ba_model.py is a cell-level Python model of align_core / place_block / Trace written from scan_block.rs alone: which region is
# computed next (Right / Down by 8, Grow from the checkpoint, Shrink), the offsets, the per-lane best cell and the crate's choice between
# lanes, the X-drop counter, the stack of regions and the traceback through it.  It is pinned to the crate's own known answers first; then
# block_aligner.cpp (the lane-exact restatement: a different decomposition of the same source) is held to it on thousands of inputs --
# score, end cell, CIGAR and the complete list of computed regions -- with the inputs counted by how many DECISIONS sat exactly on their
# boundary (equal border maxima in the direction rule, equality in the shrink rule, the X-drop threshold met exactly or missed by one,
# a Grow that had to grow again).  What neither can show: that both did not misread the same line of the crate the same way.
def test_trajectory_model_reproduces_the_crates_known_answers():
    """scan_block.rs:2267-2413 (test_no_x_drop, test_x_drop, test_trace) through the independent model"""
    from ba_model import BlockModel
    nw = _simple(1, -1)

    def run(q, r, sc, go, ge, lo, hi, x=None):
        m = BlockModel(q, r, sc, go, ge, lo, hi, x_drop=x)
        res = m.align()
        return res, m.trace.cigar(res[1], res[2])

    assert run("AAAAAA", "AAARRA", _blosum_ar_score, -11, -1, 16, 16, 1)[0] == (14, 6, 6)
    assert run("A" * 44, "A" * 15 + "R" * 16 + "A" * 13, _blosum_ar_score, -11, -1, 16, 16, 1)[0] == (60, 15, 15)
    assert run("A" * 2048, "A" * 2048, _blosum_ar_score, -11, -1, 2048, 2048, 100)[0] == (8192, 2048, 2048)
    assert run("AAAAAA", "AAARRA", _blosum_ar_score, -11, -1, 16, 16) == ((14, 6, 6), "6M")
    assert run("AAA", "AAAA", _blosum_ar_score, -11, -1, 16, 16) == ((1, 3, 4), "3M1D")
    assert run("TTTTTTTTAAAAAAATTTTTTTTT", "TTAAAAAAATTTTTTTTTTTT", nw, -2, -1, 16, 16) == ((7, 24, 21), "2M6I16M3D")
    assert run("AAAAAAAAATTGCGCT", "AAAAAAAAAGCGC", nw, -2, -1, 32, 32) == ((8, 16, 13), "9M2I4M1I")
    assert run("AAAAAAAAATTGCGCT", "AAAAAAAAAGCGC", _simple(2, -1), -5, -2, 32, 32) == ((14, 16, 13), "9M2I4M1I")
    for q, r, want in (("AARA", "AAAA", 11), ("AARAAAA", "AAAAAAAA", 12), ("AAAA", "AAAA", 16), ("RRRR", "AAAA", -4), ("AAA", "AAAA", 1)):
        assert run(q, r, _blosum_ar_score, -11, -1, 16, 16)[0][0] == want
    for q, r, want in (("A" * 32, "A" * 32, 32), ("T" * 32, "A" * 32, -32), ("TA" * 16, "A" * 32, 0), ("C", "AAAA", -5), ("AAAA", "C", -5)):
        assert run(q, r, nw, -2, -1, 16, 16)[0][0] == want


def _trajectory_inputs(seed, n):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        ln = int(rng.integers(5, 150))
        if rng.integers(0, 4) == 0:
            unit = "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 5))))
            q, r = (unit * 80)[:ln], (unit * 80)[:int(rng.integers(5, 150))]
        else:
            q = "".join(rng.choice(list("ACG"), size=ln))
            r = list(q)
            for _e in range(int(rng.integers(0, 8))):
                p = int(rng.integers(0, max(1, len(r))))
                c = int(rng.integers(0, 3))
                if c == 0 and r:
                    r[p] = str(rng.choice(list("ACG")))
                elif c == 1 and len(r) > 3:
                    del r[p:p + int(rng.integers(1, 12))]
                else:
                    r[p:p] = list(rng.choice(list("ACG"), size=int(rng.integers(1, 12))))
            r = "".join(r) or "A"
        scheme = [(1, -1, -2, -1), (2, -1, -5, -2), (1, -1, -3, -1), (3, -2, -4, -2), (1, -3, -2, -1), (4, -1, -11, -1)][int(rng.integers(0, 6))]
        sizes = [(16, 16), (16, 32), (16, 64), (32, 128), (16, 128), (32, 32)][int(rng.integers(0, 6))]
        xdrop = None if rng.random() < 0.35 else int(rng.integers(0, 30))
        yield q, r, scheme, sizes, xdrop


def test_restatement_follows_the_trajectory_model(ba):
    """1500 seeded inputs (mutated copies with indels of up to 11 residues, periodic strings; six score schemes, six block size ranges, global and
    X-drop 0 .. 29): result, CIGAR and every computed region of the restatement against the model; every boundary class hit many times"""
    from ba_model import BlockModel
    L = ba
    L.block_trace_blocks.restype = C.c_size_t
    L.block_trace_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    for fn in ("block_free_aa_trace", "block_free_aa_trace_xdrop", "block_free_padded_aa", "block_free_cigar", "block_free_aamatrix"):
        getattr(L, fn).argtypes = [C.c_void_p]
        getattr(L, fn).restype = None
    ties, n = {}, 0
    buf = np.zeros(5 * 8192, np.uint32)
    for q, r, (match, mismatch, go, ge), (lo, hi), xdrop in _trajectory_inputs(20260925, 1500):
        M = BlockModel(q, r, _simple(match, mismatch), go, ge, lo, hi, x_drop=xdrop)
        want = M.align()
        want_cigar = M.trace.cigar(want[1], want[2])
        m = L.block_new_simple_aamatrix(match, mismatch)
        pq, pr = padded(L, q.encode(), hi), padded(L, r.encode(), hi)
        cg = L.block_new_cigar(len(q) + 8, len(r) + 8)
        if xdrop is None:
            a = L.block_new_aa_trace(len(q) + 8, len(r) + 8, hi)
            L.block_align_aa_trace(a, pq, pr, m, Gaps(go, ge), SizeRange(lo, hi), 0)
            res = L.block_res_aa_trace(a)
            L.block_cigar_aa_trace(a, res.query_idx, res.reference_idx, cg)
        else:
            a = L.block_new_aa_trace_xdrop(len(q) + 8, len(r) + 8, hi)
            L.block_align_aa_trace_xdrop(a, pq, pr, m, Gaps(go, ge), SizeRange(lo, hi), xdrop)
            res = L.block_res_aa_trace_xdrop(a)
            L.block_cigar_aa_trace_xdrop(a, res.query_idx, res.reference_idx, cg)
        nb = L.block_trace_blocks(a, buf.ctypes.data, 8192)
        blocks = [tuple(int(x) for x in buf[5 * k:5 * k + 5]) for k in range(nb)]
        what = (q, r, (match, mismatch, go, ge), (lo, hi), xdrop)
        assert (res.score, res.query_idx, res.reference_idx) == want, what
        assert cigar_str(L, cg) == want_cigar, what
        assert blocks == M.trace.rectangles(), what
        (L.block_free_aa_trace if xdrop is None else L.block_free_aa_trace_xdrop)(a)
        for x in (pq, pr):
            L.block_free_padded_aa(x)
        L.block_free_cigar(cg)
        L.block_free_aamatrix(m)
        for k, v in M.ties.items():
            ties[k] = ties.get(k, 0) + (1 if v else 0)
        n += 1
    assert n == 1500
    assert ties["dir_equal"] >= 800 and ties["grow_at_limit"] >= 400 and ties["best_equal"] >= 150, ties
    assert ties["xdrop_at_threshold"] >= 50 and ties["xdrop_one_below"] >= 40 and ties["xdrop_second_step"] >= 100, ties
    assert ties["shrink_equal"] >= 20 and ties["grow_twice"] >= 15, ties


def test_trajectory_model_reproduces_the_kat_answers():
    """the model over all of oracle/ba_kat/cases.txt -- the 397 call sequences of alignStartPosBacktraceBlock (both matrices, position biases,
    block sizes 32, 64, ... until the target score is reached, x-drop = -(size * extend + open)), the 300 single-matrix strings, the 219
    boundary cases and (round 5) 189 call sequences of up to 180 residues taken from tools/ba_model_sweep.py runs on which a RARE decision fired (x-drop
    threshold met exactly / missed by one, second bad x-drop step, shrink with equality, a Grow that grew again; names swp<seed>_<boundaries>_...): every line of the restatement's frozen answers (score, end cell, CIGAR, block sizes tried)"""
    import os
    import sys
    from ba_model import BlockModel
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    kat = os.path.join(root, "oracle", "ba_kat")

    def load(path):
        toks = open(path).read().split()
        letters, vals = toks[0], list(map(int, toks[1:]))
        n = len(letters)
        tab = {}
        for a in range(n):
            for b in range(n):
                tab[(letters[a], letters[b])] = vals[a * n + b]
                tab[(letters[b], letters[a])] = vals[a * n + b]          # block_set_aamatrix sets both orders; the later call wins
        return lambda x, y: tab.get((x, y), 1 if x == y else -1)

    mAA, m3 = load(os.path.join(kat, "mat_aa.txt")), load(os.path.join(kat, "mat_3di.txt"))
    want = [ln.rstrip("\n").split("\t") for ln in open(os.path.join(kat, "ours_v3.txt"))]
    sys.path.insert(0, kat)
    import make_long_cases as long_cases
    classes = dict((f[0], f[1:]) for f in (ln.split() for ln in open(os.path.join(kat, "cases_classes.txt"))))
    k = 0
    for line in open(os.path.join(kat, "cases.txt")):
        if not line.strip() or line[0] == "#":
            continue
        f = line.split()
        kind, name, go, ge = f[0], f[1], int(f[2]), int(f[3])
        if kind == "3di":
            qa, q3, qb, ta, t3 = f[4:9]
            target = int(name.split("@")[1])
            qbias = ([0] * len(qa) if qb == "-" else [int(x) for x in qb.split(",")] + [0] * len(qa))[:len(qa)]
            res, sizes, ms, placed = (-10 ** 9, 0, 0), [], 32, []
            while ms <= 4096 and res[0] < target:
                M = BlockModel(qa, ta, mAA, -go, -ge, ms, 4096, x_drop=-(ms * (-ge) + (-go)), q_bias=qbias, r_bias=[0] * len(ta), score2=m3, q2=q3, r2=t3)
                res = M.align()
                sizes.append(f"{ms}:{res[0]}")
                placed.append((ms, res[0], max(step[3] for step in M.steps)))
                ms *= 2
            got = [name, str(res[0]), str(res[1]), str(res[2]), M.trace.cigar(res[1], res[2]) or "-", ",".join(sizes)]
            # what the device aligner must do with the case (tests/test_btrace_model_gpu.py), from the model's block sizes: the frozen verdict is this one
            assert classes[name] == [long_cases.classify(placed, target), str(max(x[2] for x in placed))], (name, placed)
        else:
            rest = f[4:]
            sc = mAA
            if kind == "nw":
                sc, rest = _simple(int(rest[0]), int(rest[1])), rest[2:]
            lo, hi, xd, q, r = int(rest[0]), int(rest[1]), int(rest[2]), rest[3], rest[4]
            M = BlockModel(q, r, sc, -go, -ge, lo, hi, x_drop=(xd if xd >= 0 else None))
            res = M.align()
            got = [name, str(res[0]), str(res[1]), str(res[2]), M.trace.cigar(res[1], res[2]) or "-", "-"]
        assert got == want[k], (k, got, want[k])
        k += 1
    assert k == 1105


# ---- oracle/ba_kat: the C-ABI harness that runs on the restatement here and on the Rust crate wherever cargo exists -----------------
def test_ba_kat_harness_and_crate_answers_when_present(tmp_path):
    """oracle/ba_kat/ba_kat.cpp (block aligner C ABI only) over the 1105 committed cases (397 + 189 align_3di call sequences of
    alignStartPosBacktraceBlock on homolog pairs incl. homopolymer / tandem-repeat / low-complexity families, 300 single-matrix tie-rich
    strings over four block-size ranges with and without x-drop, 219 trajectory cases on which a decision of align_core sits on its
    boundary): the restatement reaches the target score in every 3di case and reproduces its frozen answers (ours_v3.txt); and when somebody with a Rust toolchain has run `make -C oracle/ba_kat crate.txt
    CRATE=.../lib/block-aligner` and committed crate.txt, every line (score, end cell, CIGAR, block sizes tried) must equal the crate's.
    Without crate.txt the co-optimal-path choices of the ADAPTIVE trajectory stay unpinned against the crate -- said here, in
    DESIGN.md 2 and in the test's skip message, not hidden."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    kat = os.path.join(root, "oracle", "ba_kat")
    exe = str(tmp_path / "ba_kat_ours")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-mavx2", "-mfma", "-I" + os.path.join(root, "foldseek_amd", "csrc", "host"), "-o", exe,
                           os.path.join(kat, "ba_kat.cpp"), os.path.join(root, "foldseek_amd", "csrc", "host", "block_aligner.cpp")])
    ours = subprocess.run([exe, kat], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    assert len(ours) == 1105
    for ln in ours:
        name, score = ln.split("\t")[:2]
        if "@" in name:
            assert int(score) == int(name.split("@")[1]), ln
    assert ours == open(os.path.join(kat, "ours_v3.txt")).read().splitlines()
    crate = os.path.join(kat, "crate.txt")
    if not os.path.exists(crate):
        pytest.skip("oracle/ba_kat/crate.txt absent (no Rust toolchain in this image): CIGAR tie-breaks of the adaptive block trajectory are NOT pinned "
                    "against the crate; run `make -C oracle/ba_kat crate.txt CRATE=<reference>/lib/mmseqs/lib/block-aligner` where cargo exists")
    want = open(crate).read().splitlines()
    assert len(want) == len(ours)
    bad = [(a, b) for a, b in zip(ours, want) if a != b]
    assert not bad, bad[:5]


def test_restatement_follows_the_model_in_the_foldseek_call_shape_on_long_pairs():
    """tools/ba_model_sweep.py on a fresh seed: 80 homolog pairs of up to 500 residues with long insertions / deletions in the call shape of
    alignStartPosBacktraceBlock (both matrices, composition bias, block sizes 32, 64, ... until the SW score is reached) -- the restatement through
    oracle/ba_kat/ba_kat.cpp against tests/ba_model.py: score, end cell, CIGAR and the block sizes tried, every case.  (The committed KAT cases stop at
    110 residues; 8000 such cases over 20 other seeds up to 600 residues: 0 mismatches)"""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "ba_model_sweep.py"), "7", "80", "500"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert "80 cases" in last and " 0 mismatches" in last and "target score missed 0x" in last, r.stdout[-2000:]
    attempts = eval(re.search(r"attempts per case (\{[^}]*\})", last).group(1))
    assert sum(v for k, v in attempts.items() if k >= 2) >= 3, attempts            # the retry with a larger block happened
