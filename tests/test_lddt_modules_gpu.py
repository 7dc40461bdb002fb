"""--lddt-threshold and the lddt / lddtfull columns at module level, on REFERENCE-WRITTEN databases with a C-alpha database (tests/golden/ca_v1, generator
tests/golden/make_ca_golden.py): `fsgpu-modules` runs with the positional arguments and the complete parameter strings the reference binary was run with,
and every entry of every result DB / every byte of the text output must be the reference's.  The LDDT itself never reaches the alignment DB (10 or 11
columns): it shows in WHICH hits survive -- 144 / 143 / 24 / 14 lines at thresholds 0 / 0.5 / 0.7 / 0.8, one pair at 0.49996 (printed as 5.000E-01) dropped at 0.5."""
import os
import shutil
import subprocess

import pytest

import lddt_cases as K

pytestmark = pytest.mark.gpu

BIN = os.path.join(K.ROOT, "foldseek_amd", "bin", "fsgpu-modules")
WARNING = "Cannot use --lddt-threshold with --sort-by-structure-bits 0\nDisabling --lddt-threshold\n"


def read_db(path):
    t = int.from_bytes(open(path + ".dbtype", "rb").read(4), "little", signed=True)
    data = open(path, "rb").read()
    out = {}
    for line in open(path + ".index"):
        k, off, ln = line.split()
        out[int(k)] = data[int(off):int(off) + int(ln) - 1]
    return t, out


@pytest.fixture()
def work(tmp_path):
    """a private copy of the frozen DBs with the links the reference's makepaddedseqdb workflow makes (AA / header / C-alpha data -> source DB)"""
    w = tmp_path / "ca"
    shutil.copytree(K.GOLD, w)
    for link, target in K.MANIFEST["links"].items():
        os.symlink(str(w / target), str(w / link))
    return w


def _run(cmd, dev=None):
    env = dict(os.environ, FSGPU_BT_PASS2="1")
    if dev is not None:
        env["FSGPU_DEVICE_BACKTRACE"] = str(dev)
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)


def _same_db(got_path, want_path):
    want_t, want = read_db(want_path)
    got_t, got = read_db(got_path)
    assert got_t == want_t and sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k] == want[k], f"entry {k}\nwant {want[k][:300]!r}\ngot  {got[k][:300]!r}"
    return sum(len(v.decode().splitlines()) for v in got.values())


_ALIGN = sorted(n for n, r in K.MANIFEST["runs"].items() if r["module"] == "structurealign")


@pytest.mark.parametrize("dev", [0, 1])
@pytest.mark.parametrize("name", _ALIGN)
def test_structurealign_equals_reference_result_db(work, name, dev):
    """every frozen parameter set (thresholds 0 / 0.5 / 0.7 / 0.8, --max-rejected 2: the one-by-one path, --alt-ali 2: alternative alignments are not
    filtered, the padded target: _ca looked up by the padded ids), backtraces by the host (dev 0) and by the device (dev 1) block aligner"""
    run = K.MANIFEST["runs"][name]
    out = str(work / f"mine_{dev}_{name}")
    r = _run([BIN, "structurealign"] + [str(work / p) for p in run["positional"]] + [out] + run["parameters"], dev)
    assert r.returncode == 0, r.stderr
    assert _same_db(out, str(work / name)) == run["lines"]
    assert "Disabling --lddt-threshold" not in r.stderr


@pytest.mark.parametrize("dev", [0, 1])
@pytest.mark.parametrize("name", _ALIGN)
def test_fused_search_equals_reference_result_db(work, name, dev):
    """`search` at every frozen parameter set: with the ungapped prefilter at --min-ungapped-score 0 it hands the aligner the 144 pairs the frozen prefilter DB
    holds, in its order (checked: --max-rejected 2 depends on it).  aln_l07_maxrej drives the one-by-one LDDT path through the module's query hand-over,
    aln_l07_pad the padded target whose _ca is keyed by the padded ids."""
    run = K.MANIFEST["runs"][name]
    par = run["parameters"]
    get = lambda flag: par[par.index(flag) + 1]  # noqa: E731
    target, pref = run["positional"][1], run["positional"][2]
    out, outp = str(work / f"mine_search_{dev}_{name}"), str(work / f"mine_search_{dev}_{name}_pref")
    r = _run([BIN, "search", str(work / "db"), str(work / target), out, outp, "--prefilter-mode", "1", "--min-ungapped-score", "0", "-a", "1", "--alignment-type", "2",
              "--sort-by-structure-bits", "0", "--threads", "2", "--max-seqs", "1000", "-e", "10", "--lddt-threshold", get("--lddt-threshold"),
              "--alt-ali", get("--alt-ali"), "--max-rejected", get("--max-rejected")], dev)
    assert r.returncode == 0, r.stderr
    assert read_db(outp) == read_db(str(work / pref))
    assert _same_db(out, str(work / name)) == run["lines"]
    assert "Disabling --lddt-threshold" not in r.stderr


def test_kmer_search_filters_like_structurealign_on_its_own_hits(work):
    """the k-mer prefilter path of `search` (fshost_search_kmer_batch) hands the C-alpha entries of the queries that reach the aligner on in ITS order:
    search at 0.7 == structurealign at 0.7 on the prefilter DB the same search wrote"""
    out, outp = str(work / "ks"), str(work / "ks_pref")
    common = ["-a", "1", "--alignment-type", "2", "--sort-by-structure-bits", "0", "-e", "10", "--lddt-threshold", "0.7"]
    r = _run([BIN, "search", str(work / "db"), str(work / "db"), out, outp, "--prefilter-mode", "0", "-s", "9.5", "--max-seqs", "1000", "--threads", "2"] + common)
    assert r.returncode == 0, r.stderr
    r = _run([BIN, "structurealign", str(work / "db"), str(work / "db"), outp, str(work / "ks_two")] + common)
    assert r.returncode == 0, r.stderr
    n = _same_db(out, str(work / "ks_two"))
    r = _run([BIN, "structurealign", str(work / "db"), str(work / "db"), outp, str(work / "ks_all")] + common[:-1] + ["0"])
    assert r.returncode == 0, r.stderr
    assert 0 < n < sum(len(v.decode().splitlines()) for v in read_db(str(work / "ks_all"))[1].values())


def test_convertalis_lddt_columns_equal_reference_text(work):
    for name in ("conv_lddt.m8", "conv_crafted.m8"):
        run = K.MANIFEST["convert_runs"][name]
        out = str(work / ("mine_" + name))
        r = _run([BIN, "convertalis"] + [str(work / p) for p in run["positional"]] + [out] + run["parameters"])
        assert r.returncode == 0, r.stderr
        want, got = K.frozen_text(name), open(out, "rb").read()
        if got != want:
            for i, (a, b) in enumerate(zip(want.split(b"\n"), got.split(b"\n"))):
                assert a == b, f"{name}: line {i + 1}\nwant {a[:300]!r}\ngot  {b[:300]!r}"
        assert got == want
    # the issue's own check: query,target,lddt,lddtfull
    out = str(work / "mine_short.m8")
    r = _run([BIN, "convertalis", str(work / "db"), str(work / "db"), str(work / "aln_l0"), out, "--format-output", "query,target,lddt,lddtfull"])
    assert r.returncode == 0, r.stderr
    want = b"".join(b"\t".join(l.split(b"\t")[i] for i in (0, 1, 3, 4)) + b"\n" for l in K.frozen_text("conv_lddt.m8").splitlines())
    assert open(out, "rb").read() == want


def test_convertalis_lddt_needs_backtrace_and_ca(work):
    """backtrace columns: a record without one gets the existing failure; without <db>_ca the columns are refused by name and nothing is written"""
    noa = str(work / "aln_noa")
    par = list(K.MANIFEST["runs"]["aln_l0"]["parameters"])
    par[par.index("-a") + 1] = "0"
    r = _run([BIN, "structurealign", str(work / "db"), str(work / "db"), str(work / "pref"), noa] + par)
    assert r.returncode == 0, r.stderr
    r = _run([BIN, "convertalis", str(work / "db"), str(work / "db"), noa, str(work / "o1.m8"), "--format-output", "query,target,lddt"])
    assert r.returncode == 1 and "Backtrace cigar is missing in the alignment result" in r.stderr
    for f in os.listdir(work):
        if f.startswith("db_ca"):
            os.remove(work / f)
    r = _run([BIN, "convertalis", str(work / "db"), str(work / "db"), str(work / "aln_l0"), str(work / "o2.m8"), "--format-output", "query,target,lddtfull"])
    assert r.returncode == 1 and "column lddtfull is not implemented on this path" in r.stderr and "no <db>_ca" in r.stderr
    assert not os.path.exists(work / "o2.m8")


@pytest.mark.parametrize("module", ["structurealign", "search"])
def test_missing_ca_warns_and_runs_without_the_filter(work, module):
    """structurealign.cpp:216-224: without a C-alpha database the reference prints two warning lines and disables the threshold"""
    for f in os.listdir(work):
        if f.startswith("db_ca"):
            os.remove(work / f)
    out = str(work / "mine_noca")
    if module == "structurealign":
        run = K.MANIFEST["runs"]["aln_l07"]
        cmd = [BIN, "structurealign"] + [str(work / p) for p in run["positional"]] + [out] + run["parameters"]
    else:
        cmd = [BIN, "search", str(work / "db"), str(work / "db"), out, "--prefilter-mode", "1", "--min-ungapped-score", "0", "-a", "1", "--alignment-type", "2",
               "--sort-by-structure-bits", "0", "--max-seqs", "1000", "-e", "10", "--lddt-threshold", "0.7"]
    r = _run(cmd)
    assert r.returncode == 0, r.stderr
    assert WARNING in r.stderr
    assert _same_db(out, str(work / "aln_l0")) == 144


def test_index_target_reads_ca_from_inside_the_idx(work):
    """`createindex` appends the C-alpha database to <db>.idx under the user keys 500 / 501; with the plain target files gone, structurealign against db.idx
    takes sequences AND C-alpha entries from inside the index"""
    for f in os.listdir(work):
        if f.startswith("db") and not f.startswith("db_pad") and not os.path.islink(work / f):
            shutil.copy(work / f, work / ("q" + f))
    os.makedirs(work / "tmp")
    r = _run([BIN, "createindex", str(work / "db"), str(work / "tmp"), "--threads", "1", "-v", "1"])
    assert r.returncode == 0, r.stderr
    keys = [l.split()[0] for l in open(work / "db.idx.index")]
    assert "500" in keys and "501" in keys
    run = K.MANIFEST["runs"]["aln_l07"]
    for gone in (False, True):
        if gone:
            for f in os.listdir(work):
                if f.startswith("db") and not f.startswith("db_pad") and ".idx" not in f:
                    os.remove(work / f)
        out = str(work / f"mine_idx_{int(gone)}")
        r = _run([BIN, "structurealign", str(work / "qdb"), str(work / "db.idx"), str(work / "pref"), out] + run["parameters"])
        assert r.returncode == 0, r.stderr
        assert "Disabling --lddt-threshold" not in r.stderr
        # query and target DB names differ, so no pair is treated as the identity: the frozen run accepted the 12 self hits as ordinary hits too
        assert _same_db(out, str(work / "aln_l07")) == run["lines"]
