"""The end of a call: one sample's chunks cross the bus without pair offsets and entropies and with four-byte frequencies (the emitter
makes them up: csrc/emit_fill.h), and the last prefix of a call hands its set to the copy stream while its fills are still running.
Every batch of every call must be the oracle's: its text through dsm_format_batch, entropies bit for bit, with one sample pair offsets
0, 1, 2, ... and ids all zero.  The calls end in a prefix of four chunks, of two, of a single tuple, of none (the set before it must
still arrive, in order), or consist of one prefix; all run one after the other on one Miner.  DSM_EMIT_CHUNK_TUPLES (read once per
process: every case runs in a child process of its own) cuts the small golden prefixes into chunks.  The prefixes are picked from the
oracle's output on the CPU."""
import ctypes as C
import itertools
import math
import os
import subprocess
import sys
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# (samples of toy3 or a crafted frequency, miner settings, extra environment)
CASES = {
    "one": (["toy-1"], dict(fmin=2, pmin=1), {}),
    "one-wide": (["toy-1"], dict(fmin=2, pmin=1, wide=1), {}),           # 64-bit positions: the frequencies keep eight bytes on the bus
    "one-fallback": (["toy-1"], dict(fmin=2, pmin=1), {"DSM_CAND_ARENA": "256"}),  # the fallback candidate store
    "two": (["toy-1", "toy-2"], dict(fmin=2, pmin=1), {}),               # arrays unchanged, the last prefix's copies start early
    "crafted-65535": (65535, None, {}),  # A^K0 at the last entry of the term table: the host pass reads it
    "crafted-65536": (65536, None, {}),  # ... and one beyond: libm decides that tuple, the pass the ones around it, in the same chunks
}


def _count(oidx, names, prefix, kw):
    import orc
    return orc.mine(oidx, names, [prefix], emax=-1.0, **kw)[0].count(b"\n")


def _pick_prefixes(oidx, names, kw):
    """from the oracle: prefixes with many tuples (four chunks), with 2-3 (two chunks), with one and with none"""
    want = {"two": None, "single": None, "none": None}
    for p in itertools.product("ACGT", repeat=6):
        p = "".join(p)
        n = _count(oidx, names, p, kw)
        key = "none" if n == 0 else ("single" if n == 1 else ("two" if n <= 3 else None))
        if key and want[key] is None:
            want[key] = p
        if all(want.values()):
            break
    assert all(want.values()), want
    assert _count(oidx, names, "G", kw) >= 4 and _count(oidx, names, "AC", kw) >= 4
    return want


class Sink:
    def __init__(self, pydsm):
        self.pydsm, self.text, self.tuples, self.nbatch = pydsm, [], [], 0
        self.one_pair_ok = True

    def __call__(self, b):
        import numpy as np
        L = self.pydsm.lib()
        t, n = C.c_void_p(), C.c_size_t(0)
        self.pydsm._check(L.dsm_format_batch(C.byref(b), C.byref(t), C.byref(n)))
        self.text.append(C.string_at(t, n.value))
        L.dsm_free(t)
        nt = int(b.ntuples)
        assert nt > 0
        self.nbatch += 1
        arr = np.ctypeslib.as_array
        po, qo = arr(b.path_off, (nt + 1,)), arr(b.pair_off, (nt + 1,))
        assert po[0] == 0 and qo[0] == 0
        ids, freqs = arr(b.ids, (int(qo[nt]),)), arr(b.freqs, (int(qo[nt]),)).tolist()
        self.one_pair_ok = self.one_pair_ok and bool((qo == np.arange(nt + 1, dtype=np.uint32)).all()) and not ids.any()
        poff, qoff, ids = po.tolist(), qo.tolist(), ids.tolist()
        paths = C.string_at(b.path_bytes, poff[nt])
        ent = arr(b.entropy, (nt,)).tolist()
        for r in range(nt):
            self.tuples.append((paths[poff[r]:poff[r + 1]], ent[r], ids[qoff[r]:qoff[r + 1]], freqs[qoff[r]:qoff[r + 1]]))


def _chunks(n):
    return 4 if n >= 4 else (2 if n >= 2 else (1 if n else 0))


def _run_case(case):
    import entlib
    import orc
    import pydsm
    from goldenlib import Golden
    what, kw, _ = CASES[case]
    tmp = None
    if isinstance(what, int):  # one crafted sample under prefix A
        tmp = tempfile.TemporaryDirectory()
        paths = entlib.build_crafted(tmp.name, "tail%d" % what, entlib.freq_targets(1, what), device=0)
        names = [entlib.sample_name(p) for p in paths]
        kw = dict(entlib.CRAFT_KW)
        # emin one ulp above 0 drops the tuples of entropy 0.0, A^K0 among them: beyond the table that is the host's verdict
        settings = [(0.0, -1.0), (0.0, 2.0), (math.nextafter(0.0, math.inf), entlib.BIG)]
    else:
        g = Golden()
        names = what
        paths = [g.fmi("toy3", n) for n in names]
        settings = [(0.0, -1.0), (0.0, 2.0)]
    d = len(names)
    okw = {k: v for k, v in kw.items() if k != "wide"}
    idx = [pydsm.Index(p) for p in paths]
    oidx = [orc.Index(p) for p in paths]
    try:
        if tmp is not None:
            calls = [["A"], ["A"]]
            lines = entlib.parse(orc.mine(oidx, names, ["A"], emax=0.0, **okw)[0])
            assert entlib.boundary_line(lines, [what]).freqs == [what]
            assert any(ln.freqs[0] >= entlib.TERM_TAB for ln in lines) and any(ln.freqs[0] < entlib.TERM_TAB - 1 for ln in lines)
        elif d == 1:
            pk = _pick_prefixes(oidx, names, okw)
            calls = [["AC", "G"], ["G", pk["two"]], ["G", pk["single"]], ["G", pk["none"]], ["G"], [pk["single"]], ["T", "AC"]]
        else:
            calls = [["GT", "A"], ["A"]]
        for emin, emax in settings:
            with pydsm.Miner(idx, emin=emin, emax=emax, **kw) as m:
                for prefixes in calls:  # (calls in a row on one Miner)
                    tag = (case, emin.hex(), emax, prefixes)
                    want, ost = orc.mine(oidx, names, prefixes, emin=emin, emax=emax, threads=4, **okw)
                    lines = entlib.parse(want)
                    sink = Sink(pydsm)
                    _, st = m.mine_many(prefixes, text=False, on_batch=sink)
                    assert b"".join(sink.text) == want, tag       # (every set arrived, in order)
                    assert (st.tuples, st.pairs) == ost[4:], tag
                    assert len(sink.tuples) == len(lines), tag
                    for (path, e, ids, freqs), ln in zip(sink.tuples, lines):
                        assert (path, ids, freqs) == (ln.path, ln.ids, ln.freqs), tag + (ln.raw,)
                        assert e == entlib.exact_entropy(d, ln.freqs), tag + (ln.raw, e.hex())
                    if d == 1:
                        assert sink.one_pair_ok, tag
                    if emax < 0:  # nothing dropped: one batch per chunk
                        per = [_chunks(_count(oidx, names, p, okw)) for p in prefixes]
                        assert sink.nbatch == sum(per), tag + (per, sink.nbatch)
                        if tmp is None and len(prefixes) > 1 and prefixes[-1] in ("G", "A"):
                            assert per[-1] == 4, tag
                    got, st = m.mine_many(prefixes)  # the device text takes the same early hand-over
                    assert got == want and (st.tuples, st.pairs) == ost[4:], tag
    finally:
        for ix in idx:
            ix.close()
        for o in oidx:
            o.close()
        if tmp is not None:
            tmp.cleanup()


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_call_tails_match_oracle(case):
    env = dict(os.environ)
    env["DSM_EMIT_CHUNK_TUPLES"] = "1"
    env.update(CASES[case][2])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=240)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-4000:]
    assert b"case ok" in r.stdout


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(ROOT, "dsm-framework_amd"))
    _run_case(sys.argv[1])
    print("case ok", sys.argv[1])
