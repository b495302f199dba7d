#!/usr/bin/env python3
"""Distance-matrix goldens: the UNMODIFIED reference smtxt2entropy (oracle/_ref/smtxt2entropy, built by
oracle/Makefile.ref from wrapper-distance-matrix/smtxt2entropy.c) run on the committed reference-server outputs.
Writes tests/golden/<set>/distmat.<case>.{count,log,sqrt,lgamma}.gz and the case table into MANIFEST.json.
The set "synth" holds synthetic inputs from seeded generators (SYNTH_CASES), committed as distmat.<case>.input.gz: more than 64
samples, frequencies at the 32-bit edges and non-finite cells, which the server outputs do not reach.
Run in the build container only (needs /root/reference through oracle/_ref)."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TOOL = os.path.join(ROOT, "oracle", "_ref", "smtxt2entropy")

CASES = {
    # set: {case: (server cfg, prefixes, tool arguments without -s / -F)}
    "toy3": {"m4": ("default", ["A", "C", "G", "T"], ["-m", "0.25,0.5,0.75,1.0"]),
             "step": ("default", ["A", "C"], ["-e", "0.3"])},
    "five": {"m3": ("default", ["A", "C", "G", "T"], ["-m", "0.4,0.8,1.0"]),
             "minfreq": ("default", ["A", "C", "G", "T"], ["-m", "0.5,1.0", "-M", "12"])},
    "many30": {"m2": ("default", ["AC", "G"], ["-m", "0.7,1.0"])},
}
# cases with the -S run-to-sample file and / or the -N dataset-size file: {set: {case: (cfg, prefixes, args, mapping, sizes)}}
FILE_CASES = {
    "five": {"smap": ("default", ["A", "C", "G", "T"], ["-m", "0.5,1.0"], [0, 1, 1, 2, 0], None),
             "norm": ("default", ["A", "C", "G", "T"], ["-m", "0.4,0.8,1.0"], None, [1.0, 2.5, 0.5, 4.0, 1.5]),
             "smap_norm": ("default", ["A", "C"], ["-e", "0.5"], [2, 0, 1, 1, 0], [3.0, 1.0, 2.0])},
    "many30": {"smap": ("default", ["AC", "G"], ["-m", "0.6,1.0", "-M", "4"], [i % 7 for i in range(30)], None)},
}

ROWLEN = 10000   # smtxt2entropy.c:32: longer lines are split by fgets
MAXSMPLS = 220   # smtxt2entropy.c:33: at most 219 samples (and pairs per line)


def synth_lines(seed, runs, nlines, maxk, big=0.0, wrap=0.0, dup=0.0, edges=(), infsum=0.0):
    """Random server lines "<path> <entropy> id:freq ...": ids from range(runs), mostly small frequencies, a share of
    frequencies >= 1e5 (the tool's direct-call path), lines with two frequencies >= 2^31 (wrap) or with two frequencies that
    add up to 2^32 - 1 (infsum: freq[j] + freq[k] + 1 wraps to 0 and lgamma(0) is inf), repeated ids (dup) and frequencies
    drawn from edges."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nlines):
        k = int(rng.integers(1, maxk + 1))
        ids = [int(x) for x in rng.choice(runs, k, replace=False)]
        fr = [int(x) for x in np.where(rng.random(k) < big, rng.integers(100000, 3000000, k), rng.integers(0, 400, k))]
        if k >= 2 and rng.random() < wrap:
            fr[0], fr[1] = (int(x) for x in rng.integers(2 ** 31, 2 ** 32 - 1, 2))
        if k >= 2 and rng.random() < infsum:
            f = int(rng.integers(2 ** 31, 2 ** 32 - 1))
            fr[0], fr[1] = f, 2 ** 32 - 1 - f
        if edges and rng.random() < 0.3:
            fr[int(rng.integers(0, k))] = int(rng.choice(edges))
        if rng.random() < dup:
            j = int(rng.integers(0, k))
            ids.append(ids[j])
            fr.append(int(rng.integers(0, 400)))
        line = "%s 0.5 " % "".join("ACGT"[int(x)] for x in rng.integers(0, 4, 6)) + " ".join("%d:%d" % p for p in zip(ids, fr))
        assert len(line) + 1 < ROWLEN and len(ids) <= MAXSMPLS
        out.append(line + "\n")
    return "".join(out).encode()


# synthetic cases: {case: (samples, tool arguments without -s / -S / -N / -F, mapping, sizes, synth_lines arguments)}
SYNTH_CASES = {
    # 70 samples: diagonal counts past 64 lanes; lines with two frequencies >= 2^31 (the unsigned sums of add() :187-188 wrap)
    "s70": (70, ["-m", "0.3,0.5,0.7,1.0", "-M", "3"], None, None,
            dict(seed=70, runs=70, nlines=1500, maxk=70, big=0.05, wrap=0.1, dup=0.05)),
    # 150 runs onto 100 samples by -S, repeated ids in a line
    "smap100": (100, ["-m", "0.5,1.0"], [int(x) for x in np.random.default_rng(100).integers(0, 100, 150)], None,
                dict(seed=101, runs=150, nlines=800, maxk=120, big=0.03, dup=0.3)),
    # -N with a negative size: sqrt of a negative normalised frequency, "-nan" cells
    "norm_neg": (9, ["-m", "0.5,1.0"], None, [1.0, 4.0, 0.25, -250.0, 2.5, 16.0, 1e-3, 64.0, 3.0],
                 dict(seed=9, runs=9, nlines=1500, maxk=9, big=0.02)),
    # 12 samples, 7 buckets: 66 pairs (more than the 64 lanes of a tuple) and 1008 cells (the LDS path)
    "s12m7": (12, ["-m", "0.1,0.2,0.35,0.5,0.65,0.8,1.0"], None, None, dict(seed=12, runs=12, nlines=3000, maxk=12, big=0.05, dup=0.05)),
    # frequencies at the 32-bit edges: 2^31, 2^32 - 2, 2^32 - 1 (1 + freq wraps to 0; the tool's entropy is nan and the line
    # lands in no bucket), 2^32 and more (atoi keeps the low 32 bits); pairs whose lgamma term is inf
    "edges": (6, ["-m", "0.2,0.6,1.0"], None, None,
              dict(seed=6, runs=6, nlines=600, maxk=6, infsum=0.02,
                   edges=(2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 5000000000))),
}


def run_tool(text, targs, smpls, mapping, sizes, outdir):
    with tempfile.TemporaryDirectory() as td:
        args = [TOOL, "-F", "out"] + targs
        if mapping is not None:
            open(os.path.join(td, "map.txt"), "w").write("".join("%d\n" % x for x in mapping))
            args += ["-S", "map.txt"]
        else:
            args += ["-s", str(smpls)]
        if sizes is not None:
            open(os.path.join(td, "sizes.txt"), "w").write("".join("d%d\t%r\n" % (i, x) for i, x in enumerate(sizes)))
            args += ["-N", "sizes.txt"]
        subprocess.run(args, input=text, cwd=td, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for kind in ("count", "log", "sqrt", "lgamma"):
            data = open(os.path.join(td, "%s.out" % kind), "rb").read()
            with gzip.GzipFile(outdir % kind, "wb", mtime=0) as g:
                g.write(data)


def main():
    if not os.path.exists(TOOL):
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "-f", "Makefile.ref"], check=True)
    man_path = os.path.join(HERE, "MANIFEST.json")
    man = json.load(open(man_path))
    out_cases = {}
    for setname, cases in CASES.items():
        names = man["sets"][setname]["names"]
        for case, (cfg, prefixes, targs) in cases.items():
            if cfg not in man["sets"][setname]["server_cfgs"]:
                continue
            prefixes = prefixes or man["sets"][setname]["prefixes"]
            text = b""
            for p in prefixes:
                f = os.path.join(HERE, setname, "server.%s.%s.txt.gz" % (cfg, p))
                if os.path.exists(f):
                    text += gzip.open(f, "rb").read()
            if not text:
                continue
            with tempfile.TemporaryDirectory() as td:
                subprocess.run([TOOL, "-s", str(len(names)), "-F", "out"] + targs, input=text, cwd=td, check=True,
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                for kind in ("count", "log", "sqrt", "lgamma"):
                    data = open(os.path.join(td, "%s.out" % kind), "rb").read()
                    with gzip.GzipFile(os.path.join(HERE, setname, "distmat.%s.%s.gz" % (case, kind)), "wb", mtime=0) as g:
                        g.write(data)
            out_cases.setdefault(setname, {})[case] = {"server_cfg": cfg, "prefixes": prefixes, "args": targs, "lines": text.count(b"\n")}
            print(setname, case, text.count(b"\n"), "lines")
    for setname, cases in FILE_CASES.items():
        for case, (cfg, prefixes, targs, mapping, sizes) in cases.items():
            text = b"".join(gzip.open(os.path.join(HERE, setname, "server.%s.%s.txt.gz" % (cfg, p)), "rb").read() for p in prefixes)
            smpls = max(mapping) + 1 if mapping is not None else len(man["sets"][setname]["names"])
            run_tool(text, targs, smpls, mapping, sizes, os.path.join(HERE, setname, "distmat.%s.%%s.gz" % case))
            out_cases.setdefault(setname, {})[case] = {"server_cfg": cfg, "prefixes": prefixes, "args": targs, "lines": text.count(b"\n"),
                                                        "mapping": mapping, "sizes": sizes}
            print(setname, case, text.count(b"\n"), "lines")
    os.makedirs(os.path.join(HERE, "synth"), exist_ok=True)
    for case, (smpls, targs, mapping, sizes, gen) in SYNTH_CASES.items():
        assert smpls < MAXSMPLS and (mapping is None or max(mapping) + 1 == smpls)
        text = synth_lines(**gen)
        with gzip.GzipFile(os.path.join(HERE, "synth", "distmat.%s.input.gz" % case), "wb", mtime=0) as g:
            g.write(text)
        run_tool(text, targs, smpls, mapping, sizes, os.path.join(HERE, "synth", "distmat.%s.%%s.gz" % case))
        out_cases.setdefault("synth", {})[case] = {"input": "distmat.%s.input.gz" % case, "samples": smpls, "args": targs,
                                                  "lines": text.count(b"\n"), "mapping": mapping, "sizes": sizes}
        print("synth", case, text.count(b"\n"), "lines")
    man["distmat"] = out_cases
    json.dump(man, open(man_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    sys.exit(main())
