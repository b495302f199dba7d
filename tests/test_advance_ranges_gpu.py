"""Mined levels of one sample: the level's tiles are cut into ranges (csrc/ranges.h), range_sums_kernel adds up the children and candidates
of every range and of every wave's part of it, and advance_single_kernel walks the ranges -- three launches between two LF-step
launches, no per-tile counts, no scan.  DSM_ADVANCE_RANGES (read once per process: every case runs in a child process of its own) caps
the number of ranges: with 1, 3 or 7 of them a level of about 79 tiles has some twenty tiles per wave, a short last range and a wave
without tiles; unset, every range is one tile per wave or less.  Both position widths; with three ranges also a candidate block too
small for a level (fallback store) and an arena so small that the prefix splits (a level wider than its window is reported through
the two published words and not written).

The split case differs from the others in two points, both by the engine's definition and the same on the parent commit: the
pieces of a split prefix are narrower than 8192 nodes (5291, 21 tiles: three ranges of eight, the last one short with an empty wave),
and a split run's cost counters (lf_steps, rank_ops, union_nodes) count the prefix's own path once per piece, so they are above the
oracle's: 41 413 930 / 93 171 864 / 3 924 966 against 41 413 218 / 93 170 262 / 3 919 454 for the four prefixes.  That case asserts
reported, tuples and pairs against the oracle and all six against the parent commit's figures.

Input: builder.synth_reads(7, 20000, 60, 40000, 0.005), fmin 2, pmin 1, emax 2.0; the prefixes A, C, G, T in one call and G alone.  The
oracle's answer is computed once per session (3 919 454 nodes and 82 199 tuples; G alone 983 077 and 20 635) and shared through files.
Every case: device text equals the oracle's, the six counters equal the oracle's, the binary batches give the same paths, entropies
and frequencies in the same order.

The CPU part: the range arithmetic against its definition for every number of tiles 2..5000 (tests/native/ranges_check.cpp), once more
as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "tests", "native", "ranges_check.cpp")

KW = dict(fmin=2, pmin=1, emax=2.0)
PREFIX_SETS = {"all": ["A", "C", "G", "T"], "g": ["G"]}
EXPECT = {"all": (3919454, 82199), "g": (983077, 20635)}   # nodes, tuples: the oracle's, checked when the reference is made
SPLIT_ARENA = 8 << 20   # bytes: with it the parent commit splits every one-letter prefix of this input once (1 to 6 MiB: 5 times each)
# A split run walks the prefix's own path once per piece (engine.hip, run_auto: "union_nodes and the cost counters still count the
# enforced path once per sub-run"), so its lf_steps, rank_ops and union_nodes are not the oracle's; reported, tuples and pairs are.
# These are the six counters of the parent commit's library for this input and arena (32-bit positions), text and binary alike.
SPLIT_COUNTERS = {"all": (3919454, 41413930, 93171864, 3924966, 82199, 82199), "g": (983077, 10389304, 23373082, 984455, 20635, 20635)}
SPLIT_WIDEST = 5291     # the widest level of a piece (the parent's figure); unsplit: 20763

# (DSM_ADVANCE_RANGES or None, wide, extra environment, arena_bytes)
CASES = {}
for _r in ("1", "3", "7", None):
    for _w in (0, 1):
        CASES["ranges%s-wide%d" % (_r or "unset", _w)] = (_r, _w, {}, 0)
CASES["ranges3-fallback"] = ("3", 0, {"DSM_CAND_ARENA": "256"}, 0)
CASES["ranges3-split"] = ("3", 0, {}, SPLIT_ARENA)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_range_arithmetic_on_the_cpu(tmp_path, flags):
    exe = str(tmp_path / "ranges_check")
    subprocess.run(["g++", "-std=c++17"] + flags + ["-o", exe, SRC], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.startswith("ok "), out
    assert int(out.split()[1]) > 4 * 4999 * 4, out   # at least one range of four waves per (cap, number of tiles)


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """The index and the oracle's text and counters of both prefix sets, in a directory the child processes read."""
    import orc
    from pydsm import builder
    d = tmp_path_factory.mktemp("advance_ranges")
    fmi = str(d / "one.fasta.fmi")
    builder.build_from_codes(builder.synth_reads(7, 20000, 60, 40000, 0.005), fmi)
    o = orc.Index(fmi)
    try:
        name = os.path.basename(fmi).split(".")[0]   # (a sample's name ends at the first dot of its file's)
        meta = {}
        for key, prefixes in PREFIX_SETS.items():
            want, ost = orc.mine([o], [name], prefixes, threads=4, **KW)
            assert (ost[0], ost[4]) == EXPECT[key], (key, ost)
            with open(str(d / ("want_%s.txt" % key)), "wb") as f:
                f.write(want)
            meta[key] = list(ost)
        with open(str(d / "counters.json"), "w") as f:
            json.dump(meta, f)
    finally:
        o.close()
    return str(d)


def _run_case(workdir, case):
    import entlib
    import numpy as np
    import pydsm
    _, wide, _, arena = CASES[case]
    counters = json.load(open(os.path.join(workdir, "counters.json")))
    widest, splits = 0, 0
    with pydsm.Index(os.path.join(workdir, "one.fasta.fmi")) as ix:
        with pydsm.Miner([ix], wide=wide, arena_bytes=arena, **KW) as m:
            for key, prefixes in PREFIX_SETS.items():
                want = open(os.path.join(workdir, "want_%s.txt" % key), "rb").read()
                ost = tuple(counters[key])
                if arena:   # what the oracle and a split run share, then all six as the parent commit gives them
                    assert (SPLIT_COUNTERS[key][0],) + SPLIT_COUNTERS[key][4:] == (ost[0],) + ost[4:], (case, key)
                    assert all(a >= b for a, b in zip(SPLIT_COUNTERS[key], ost)), (case, key)
                    ost = SPLIT_COUNTERS[key]
                got, st = m.mine_many(prefixes)   # device text
                assert got == want, (case, key)
                assert (st.reported, st.lf_steps, st.rank_ops, st.union_nodes, st.tuples, st.pairs) == ost, (case, key)
                widest, splits = max(widest, st.max_frontier), splits + st.splits
                lines = entlib.parse(want)
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
                assert (st.reported, st.lf_steps, st.rank_ops, st.union_nodes, st.tuples, st.pairs) == ost, (case, key)
                assert len(tuples) == len(lines), (case, key)
                for (path, e, ids, freqs), ln in zip(tuples, lines):
                    assert (path, ids, freqs) == (ln.path, ln.ids, ln.freqs), (case, key, ln.raw)
                    assert e == entlib.exact_entropy(1, ln.freqs), (case, key, ln.raw, e.hex())
                widest, splits = max(widest, st.max_frontier), splits + st.splits
    if arena:   # (a level too wide for its window was met, reported and not written: the pieces are narrower)
        assert splits > 0 and widest == SPLIT_WIDEST, (splits, widest)
    else:
        assert splits == 0 and widest > 8192, (splits, widest)   # levels of more than 32 tiles: the range sweep took them
    print("widest level %d, splits %d" % (widest, splits))


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_range_sweep_matches_oracle(reference, case):
    env = dict(os.environ)
    env.pop("DSM_ADVANCE_RANGES", None)
    if CASES[case][0]:
        env["DSM_ADVANCE_RANGES"] = CASES[case][0]
    env.update(CASES[case][2])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), reference, case], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=240)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-4000:]
    assert b"case ok" in r.stdout


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(ROOT, "dsm-framework_amd"))
    _run_case(sys.argv[1], sys.argv[2])
    print("case ok", sys.argv[2])
