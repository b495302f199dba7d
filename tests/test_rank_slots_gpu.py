"""The finish of a mined prefix: every candidate leaves its index in its level and its level side by side at its post-order rank (one
8-byte slot, whose level the scan of the path offsets reads), and with one sample and binary batches no pair counts at all: every
tuple has one pair, the pair offset of rank r is r.  DSM_EMIT_CHUNK_TUPLES (read once per process: every case runs in a child process
of its own) cuts the tuples into four chunks, two, or one.  Device text (which keeps the pair offsets) and binary batches (paths,
entropies bit for bit, ids, frequencies) must equal the oracle for one sample (its candidate records, and its fallback store), two
samples and eight."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# (set, samples, prefixes, miner settings, an emax that drops some of the tuples, extra environment)
CASES = {
    "one-records": ("toy3", ["toy-1"], ["G", "AC", "T"], dict(fmin=2, pmin=1), 2.0, {}),
    "one-fallback": ("toy3", ["toy-2"], ["T", "GT"], dict(fmin=2, pmin=1), 2.0, {"DSM_CAND_ARENA": "256"}),
    "two": ("toy3", ["toy-1", "toy-2"], ["A", "GT"], dict(fmin=2), 2.0, {}),
    "eight": ("many30", ["m00", "m01", "m02", "m03", "m04", "m05", "m06", "m07"], ["AC", "G"], dict(fmin=3, maxdepth=14), 2.85, {}),
}
# tuples per chunk unit: four chunks per prefix, two for most, one
SWEEPS = {"four": "1", "two": "9", "one": "1000000"}


def _run_case(case):
    import entlib
    import numpy as np
    import orc
    import pydsm
    from goldenlib import Golden
    g = Golden()
    setname, names, prefixes, kw, emax_drop, _ = CASES[case]
    d = len(names)
    idx = [pydsm.Index(g.fmi(setname, n)) for n in names]
    oidx = [orc.Index(g.fmi(setname, n)) for n in names]
    try:
        for emax in (-1.0, emax_drop):
            want, ost = orc.mine(oidx, names, prefixes, emax=emax, threads=4, **kw)
            lines = entlib.parse(want)
            assert len(lines) > 20, (case, emax)
            with pydsm.Miner(idx, emax=emax, **kw) as m:
                got, st = m.mine_many(prefixes)  # device text
                assert got == want, (case, emax)
                assert (st.tuples, st.pairs) == ost[4:], (case, emax)
                tuples = []

                def on_batch(b):
                    nt = int(b.ntuples)
                    arr = np.ctypeslib.as_array
                    poff, qoff = arr(b.path_off, (nt + 1,)).tolist(), arr(b.pair_off, (nt + 1,)).tolist()
                    assert poff[0] == 0 and qoff[0] == 0
                    paths = C.string_at(b.path_bytes, poff[nt])
                    ids, freqs = arr(b.ids, (qoff[nt],)).tolist(), arr(b.freqs, (qoff[nt],)).tolist()
                    ent = arr(b.entropy, (nt,)).tolist()
                    for r in range(nt):
                        tuples.append((paths[poff[r]:poff[r + 1]], ent[r], ids[qoff[r]:qoff[r + 1]], freqs[qoff[r]:qoff[r + 1]]))

                _, st = m.mine_many(prefixes, text=False, on_batch=on_batch)
                assert (st.tuples, st.pairs) == ost[4:], (case, emax)
                assert len(tuples) == len(lines), (case, emax)
                for (path, e, ids, freqs), ln in zip(tuples, lines):
                    assert (path, ids, freqs) == (ln.path, ln.ids, ln.freqs), (case, emax, ln.raw)
                    assert e == entlib.exact_entropy(d, ln.freqs), (case, emax, ln.raw, e.hex())
    finally:
        for ix in idx:
            ix.close()
        for o in oidx:
            o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sweep", sorted(SWEEPS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_rank_slots_match_oracle(case, sweep):
    env = dict(os.environ)
    env["DSM_EMIT_CHUNK_TUPLES"] = SWEEPS[sweep]
    env.update(CASES[case][5])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=240)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-4000:]
    assert b"case ok" in r.stdout


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(ROOT, "dsm-framework_amd"))
    _run_case(sys.argv[1])
    print("case ok", sys.argv[1])
