"""bench.py's contract is ONE JSON line on stdout.  Libraries write there too (librccl prints its version banner to the C stdout when the first communicator
comes up -- round 5 made the one-rank RCCL communicator the default at N = 1 and found a six-line stdout): the run points file descriptor 1 at stderr and
writes its line to a private duplicate of the real stdout.  No GPU needed."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_only_the_result_line_reaches_stdout():
    code = ("import os, sys, bench\n"
            "bench._claim_stdout()\n"
            "os.write(1, b'RCCL version : banner from a C library\\n')\n"
            "print('a python print')\n"
            "bench.emit_line({'metric': 'x', 'value': 1.5, 'big': 'y' * 200000})\n"
            "os.write(1, b'printed at exit by a library\\n')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith('{"metric": "x", "value": 1.5') and len(lines[0]) > 200000
    assert "banner from a C library" in r.stderr and "a python print" in r.stderr and "printed at exit" in r.stderr


def test_without_the_claim_the_line_still_goes_to_stdout():
    r = subprocess.run([sys.executable, "-c", "import bench; bench.emit_line({'a': 1})"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == '{"a": 1}\n'


def test_dump_outputs_writes_float64_fields(tmp_path):
    """--dump-outputs: one .npy per field of the returned records (no padding, no CIGAR-buffer offsets), float64, one query's records after the other"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from foldseek_amd import api
    res = [np.zeros(n, api.RESULT_DT) for n in (2, 0, 3)]
    for i, r in enumerate(res):
        r["dbKey"] = np.arange(len(r)) + 10 * i
        r["eval"] = 1e-30 * (i + 1)
    hits = [np.array([(7, -3)], api.HIT_DT), np.zeros(0, api.HIT_DT), np.array([(1, 5), (2, 4)], api.HIT_DT)]
    bench.dump_outputs(str(tmp_path / "d"), {**bench.result_arrays("prefilter", hits), **bench.result_arrays("align", res)})
    names = sorted(os.listdir(tmp_path / "d"))
    assert "align_backtraceOff.npy" not in names and not any("_pad" in n for n in names)
    assert {"prefilter_per_query.npy", "prefilter_id.npy", "prefilter_score.npy", "align_per_query.npy", "align_dbKey.npy", "align_eval.npy"} <= set(names)
    for n in names:
        assert np.load(tmp_path / "d" / n).dtype == np.float64
    assert np.load(tmp_path / "d" / "prefilter_score.npy").tolist() == [-3, 5, 4]
    assert np.load(tmp_path / "d" / "align_per_query.npy").tolist() == [2, 0, 3]
    assert np.load(tmp_path / "d" / "align_dbKey.npy").tolist() == [0, 1, 20, 21, 22]
    assert np.load(tmp_path / "d" / "align_eval.npy").tolist() == np.concatenate(res)["eval"].tolist()


def test_plain_and_full_options():
    """--full is off by default; --dump-outputs takes a directory"""
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
