"""The gpuserver protocol's CLIENT half against the reference's own client, no GPU needed: a scripted server (this test) owns the
shared-memory block under the name both binaries derive from (database path, visible devices, version string) and answers every READY with a
result list that depends on the query.  The reference binary (oracle/_ref/bin/foldseek-fsgpu: its unmodified ungappedprefilter.cpp /
GpuUtil.cpp) and `fsgpu-modules ungappedprefilter --gpu-server 1` must
  * hand over the same bytes for every query -- residue codes and the 21 x L int8 profile incl. the composition bias -- and
  * write byte-identical prefilter DBs from the same answers (threshold, order, --max-seqs cut, text format)."""
import ctypes as C
import json
import mmap
import os
import shutil
import struct
import subprocess
import threading
import time

import numpy as np
import pytest

from foldseek_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS_GPU = os.path.join(ROOT, "oracle", "_ref", "bin", "foldseek-fsgpu")
BIN = os.path.join(ROOT, "foldseek_amd", "bin", "fsgpu-modules")
GOLD = os.path.join(ROOT, "tests", "golden", "scop_v1")
pytestmark = pytest.mark.skipif(not os.path.exists(FS_GPU), reason="oracle/_ref/bin/foldseek-fsgpu not built (oracle/build_ref_full.sh gpu)")


class ScriptedServer:
    """GPUSharedMemory (M/src/commons/GpuUtil.h:9-49) driven from Python: IDLE 0, RESERVED 1, READY 2, DONE 3"""
    def __init__(self, name, max_len=65535, max_res=1000):
        self.qoff, self.roff = 36, 36 + max_len
        self.poff = self.roff + 16 * max_res
        self.size = self.poff + 21 * max_len
        self.path = "/dev/shm/" + name
        with open(self.path, "wb") as f:
            f.write(struct.pack("<IIiB3xIIIII", max_len, max_res, 0, 0, self.qoff, 0, self.roff, 0, self.poff) + bytes(self.size - 36))
        self.fd = os.open(self.path, os.O_RDWR)
        self.mm = mmap.mmap(self.fd, self.size)
        self.seen, self.stop = [], threading.Event()
        self.th = threading.Thread(target=self.run, daemon=True)
        self.th.start()

    @staticmethod
    def answer(codes, n_targets):
        """made up, a function of the query: ties, scores at / below / above the threshold, more entries than --max-seqs"""
        s = int(codes.astype(np.int64).sum())
        res = [((s + 7 * i) % n_targets, 20 + (s * (i + 3)) % 236) for i in range(12)]
        res += [((s + 1) % n_targets, 150), ((s + 2) % n_targets, 150), (s % n_targets, 30), ((s + 5) % n_targets, 31)]
        out, used = [], set()
        for t, sc in res:                      # one entry per target, like a real scan
            if t not in used:
                used.add(t); out.append((t, sc))
        return out

    def run(self):
        mm = self.mm
        while not self.stop.is_set():
            if struct.unpack_from("<i", mm, 8)[0] != 2:
                time.sleep(0.0003)
                continue
            L = struct.unpack_from("<I", mm, 20)[0]
            codes = np.frombuffer(mm[self.qoff:self.qoff + L], np.uint8).copy()
            prof = np.frombuffer(mm[self.poff:self.poff + 21 * L], np.int8).copy()
            self.seen.append((codes, prof))
            res = self.answer(codes, self.n_targets)
            for i, (tid, sc) in enumerate(res):
                struct.pack_into("<Iiii", mm, self.roff + 16 * i, tid, sc, 0, 0)
            struct.pack_into("<I", mm, 28, len(res))
            struct.pack_into("<i", mm, 8, 3)

    def close(self):
        self.stop.set(); self.th.join(timeout=5)
        self.mm.close(); os.close(self.fd); os.remove(self.path)


# (the reference's client copies `resultLen` entries into a list sized by ITS --max-seqs: an answer longer than that corrupts its heap --
#  "free(): invalid pointer" with --max-seqs 3 here -- so the scripted answers stay below the smaller value; ours clamps)
@pytest.mark.parametrize("bias,max_seqs", [("1", "1000"), ("0", "20")])
def test_both_clients_speak_the_same_protocol(tmp_path, bias, max_seqs):
    w = str(tmp_path)
    for f in os.listdir(GOLD):
        if f.startswith("db"):
            shutil.copy(os.path.join(GOLD, f), os.path.join(w, f))
    manifest = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
    for link, target in manifest["links"].items():
        if not os.path.exists(os.path.join(w, link)):
            os.symlink(target, os.path.join(w, link))
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "foldseek_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    env.pop("HIP_VISIBLE_DEVICES", None); env.pop("CUDA_VISIBLE_DEVICES", None)
    version = subprocess.run([FS_GPU, "version"], capture_output=True, text=True, env=env).stdout.strip()
    L = C.CDLL(api.LIB_PATH)
    L.fshost_gpu_shm_name.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(256)
    assert L.fshost_gpu_shm_name(os.path.join(w, "db_pad_ss").encode(), None, version.encode(), buf, 256) > 0
    par = list(manifest["runs"]["pref_ung_pad"]["parameters"])
    for k, v in (("--gpu", "1"), ("--gpu-server", "1"), ("--prefilter-mode", "0"), ("--comp-bias-corr", bias), ("--max-seqs", max_seqs), ("--threads", "1")):
        par[par.index(k) + 1] = v
    n_targets = sum(1 for _ in open(os.path.join(w, "db_pad_ss.index")))
    runs = {}
    for who, cmd in (("ref", [FS_GPU, "ungappedprefilter", "db_ss", "db_pad_ss", "ref_out"] + par),
                     ("mine", [BIN, "ungappedprefilter", "db_ss", "db_pad_ss", "mine_out", "--gpu-server-version", version] + [p for p in par])):
        srv = ScriptedServer(buf.value.decode())
        srv.n_targets = n_targets
        try:
            r = subprocess.run(cmd, cwd=w, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
        finally:
            srv.close()
        assert r.returncode == 0, (who, r.stdout[-2000:])
        runs[who] = srv.seen
    assert len(runs["ref"]) == len(runs["mine"]) > 20
    key = lambda cp: (len(cp[0]), cp[0].tobytes())              # the two clients may walk the queries in a different order
    for (c1, p1), (c2, p2) in zip(sorted(runs["ref"], key=key), sorted(runs["mine"], key=key)):
        assert (c1 == c2).all()
        assert (p1 == p2).all()                                   # the int8 profile, bias included, bit for bit
    for ext in ("", ".index", ".dbtype"):
        assert open(os.path.join(w, "ref_out" + ext), "rb").read() == open(os.path.join(w, "mine_out" + ext), "rb").read(), ext
    assert os.path.getsize(os.path.join(w, "ref_out")) > 200
