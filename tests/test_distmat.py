"""distance matrices of smtxt2entropy.
CPU: the oracle restatement reproduces the reference tool's four output files byte for byte on the committed goldens.
GPU: dsm_distmat_* (csrc/distmat.hip) against the oracle -- counts and substring totals exact, the double matrices
within 1e-9 relative (the GPU adds the same terms in a different order; the tool prints them with %f)."""
import ctypes as C
import gzip
import json
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MAN = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
CASES = [(s, c) for s, cs in sorted(MAN.get("distmat", {}).items()) for c in sorted(cs)]


def _olib():
    so = os.path.join(ROOT, "oracle", "_build", "libdistmat_oracle.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), so], check=True, stdout=subprocess.DEVNULL)
    L = C.CDLL(so)
    L.orc_distmat_new.restype = C.c_void_p
    L.orc_distmat_new.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint]
    L.orc_distmat_free.argtypes = [C.c_void_p]
    L.orc_distmat_add_text.restype = C.c_long
    L.orc_distmat_add_text.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.orc_distmat_finish.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 4 + [C.c_void_p] * 5
    L.orc_distmat_steps.argtypes = [C.c_double, C.c_void_p, C.c_int]
    L.orc_distmat_options.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.orc_free_text.argtypes = [C.c_void_p]
    return L


def case_input(setname, case):
    info = MAN["distmat"][setname][case]
    if "input" in info:   # synthetic lines (make_golden_distmat.py SYNTH_CASES)
        text = gzip.open(os.path.join(GOLD, setname, info["input"]), "rb").read()
    else:
        text = b"".join(gzip.open(os.path.join(GOLD, setname, "server.%s.%s.txt.gz" % (info["server_cfg"], p)), "rb").read()
                        for p in info["prefixes"])
    args = info["args"]
    minfreq = int(args[args.index("-M") + 1]) if "-M" in args else 0
    if "-m" in args:
        maxent = [float(x) for x in args[args.index("-m") + 1].split(",")]
    else:
        buf = (C.c_double * 256)()
        n = _olib().orc_distmat_steps(float(args[args.index("-e") + 1]), buf, 256)
        maxent = list(buf[:n])
    mapping, sizes = info.get("mapping"), info.get("sizes")
    smpls = info["samples"] if "samples" in info else max(mapping) + 1 if mapping else len(MAN["sets"][setname]["names"])
    return text, smpls, maxent, minfreq, mapping, sizes


def oracle_run(text, smpls, maxent, minfreq, mapping=None, sizes=None):
    L = _olib()
    me = (C.c_double * len(maxent))(*maxent)
    h = L.orc_distmat_new(smpls, me, len(maxent), minfreq)
    assert h
    mp = (C.c_int * len(mapping))(*mapping) if mapping else None
    sz = (C.c_double * len(sizes))(*sizes) if sizes else None
    L.orc_distmat_options(h, mp, len(mapping) if mapping else 0, sz)
    rows = L.orc_distmat_add_text(h, text, len(text))
    assert rows == text.count(b"\n")
    outs = [C.c_void_p() for _ in range(4)]
    nm = len(maxent)
    nout = np.zeros(nm, np.uint32)
    cnt = np.zeros((nm, smpls, smpls), np.uint32)
    mats = [np.zeros((nm, smpls, smpls), np.float64) for _ in range(3)]
    L.orc_distmat_finish(h, *[C.byref(o) for o in outs], nout.ctypes.data, cnt.ctypes.data, *[m.ctypes.data for m in mats])
    texts = [C.string_at(o.value) for o in outs]
    for o in outs:
        L.orc_free_text(o)
    L.orc_distmat_free(h)
    return texts, nout, cnt, mats


@pytest.mark.parametrize("setname,case", CASES)
def test_oracle_reproduces_reference_tool_output(setname, case):
    text, smpls, maxent, minfreq, mapping, sizes = case_input(setname, case)
    texts, nout, cnt, mats = oracle_run(text, smpls, maxent, minfreq, mapping, sizes)
    for kind, got in zip(("count", "log", "sqrt", "lgamma"), texts):
        want = gzip.open(os.path.join(GOLD, setname, "distmat.%s.%s.gz" % (case, kind)), "rb").read()
        assert got == want, (setname, case, kind)
    assert nout.max() <= text.count(b"\n")


@pytest.fixture(scope="module")
def pydsm_mod():
    import pydsm
    pydsm.lib()
    return pydsm


def _cmp(res, nout, cnt, mats):
    assert (res["noutput"] == nout).all()
    assert (res["count"] == cnt).all()
    for k, want in zip(("log", "sqrt", "lgamma"), mats):
        got = res[k]
        fin = np.isfinite(want)     # the tool's inf and -nan cells: the same value, the sign of a NaN included
        assert np.array_equal(np.isfinite(got), fin) and np.array_equal(np.isnan(got), np.isnan(want)), k
        assert np.array_equal(np.signbit(got[~fin]), np.signbit(want[~fin])), k
        assert np.allclose(got[fin], want[fin], rtol=1e-9, atol=1e-6), (k, np.abs(got[fin] - want[fin]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("setname,case", CASES)
def test_gpu_distmat_matches_oracle_on_goldens(setname, case, pydsm_mod):
    text, smpls, maxent, minfreq, mapping, sizes = case_input(setname, case)
    texts, nout, cnt, mats = oracle_run(text, smpls, maxent, minfreq, mapping, sizes)
    with pydsm_mod.DistMat(smpls, maxent=maxent, minfreq=minfreq, run_to_sample=mapping, sizes=sizes) as dm:
        half = text.rfind(b"\n", 0, len(text) // 2) + 1
        dm.add_text(text[:half])          # two batches: accumulation across calls
        dm.add_text(text[half:])
        res = dm.finish()
    _cmp(res, nout, cnt, mats)
    # the sums are exact 128-bit fixed-point sums, rounded once (distmat.hip, Fix128): they do not depend on how the lines are cut
    # into batches, on the order the blocks run in, or on the run -- bit for bit
    with pydsm_mod.DistMat(smpls, maxent=maxent, minfreq=minfreq, run_to_sample=mapping, sizes=sizes) as dm:
        cuts = [0] + [text.rfind(b"\n", 0, len(text) * k // 5) + 1 for k in range(1, 5)] + [len(text)]
        for a, b in zip(cuts, cuts[1:]):
            if b > a:
                dm.add_text(text[a:b])
        res2 = dm.finish()
    _same_bits(res, res2)                 # (NaN cells included)
    got = pydsm_mod.DistMat.format(res)
    assert got[0] == texts[0]             # the count file is exact
    for g, w in zip(got[1:], texts[1:]):  # the double files agree line for line up to the last printed digits
        assert g.count(b"\n") == w.count(b"\n")
        for a, b in zip(g.split(), w.split()):
            if a != b:
                assert abs(float(a) - float(b)) <= 1e-9 * max(1.0, abs(float(b))) + 2e-6, (a, b)


@pytest.mark.gpu
def test_gpu_distmat_fused_with_mining_and_many_samples(golden, pydsm_mod):
    """Tuples go from the miner's sink straight into the accumulator (no text round trip); 30 samples use the global-atomic
    path (the matrices do not fit LDS)."""
    for setname, prefixes, kw, maxent in (("five", ["A", "C", "G", "T"], dict(fmin=10, emax=2.0), [0.4, 0.8, 1.0]),
                                         ("many30", ["AC", "G"], dict(fmin=3, maxdepth=14, emax=5.0), [0.7, 0.9, 1.0])):
        names = golden.manifest["sets"][setname]["names"]
        idx = [pydsm_mod.Index(golden.fmi(setname, n)) for n in names]
        with pydsm_mod.DistMat(len(names), maxent=maxent) as dm, pydsm_mod.Miner(idx, **kw) as m:
            text, st = m.mine_many(prefixes, on_batch=dm.add)
            res = dm.finish()
        texts, nout, cnt, mats = oracle_run(text, len(names), maxent, 0)
        _cmp(res, nout, cnt, mats)
        assert int(res["noutput"][0]) <= st.tuples
        for ix in idx:
            ix.close()


@pytest.mark.gpu
def test_gpu_distmat_large_frequencies_and_errors(pydsm_mod):
    rng = np.random.default_rng(5)
    lines = []
    for _ in range(20000):
        k = int(rng.integers(1, 7))
        ids = rng.choice(6, k, replace=False)
        fr = [int(x) for x in np.where(rng.random(k) < 0.02, rng.integers(100000, 3000000, k), rng.integers(1, 400, k))]
        lines.append("ACGT 0.5 " + " ".join("%d:%d" % (i, f) for i, f in zip(ids, fr)))
    text = ("\n".join(lines) + "\n").encode()
    maxent = [0.2, 0.5, 0.9, 1.0]
    texts, nout, cnt, mats = oracle_run(text, 6, maxent, 3)
    with pydsm_mod.DistMat(6, maxent=maxent, minfreq=3) as dm:
        dm.add_text(text)
        _cmp(dm.finish(), nout, cnt, mats)
    with pytest.raises(pydsm_mod.DsmError):
        pydsm_mod.DistMat(1, maxent=[1.0])
    with pytest.raises(pydsm_mod.DsmError):
        pydsm_mod.DistMat(4, maxent=[1.5])
    with pydsm_mod.DistMat(3, maxent=[1.0]) as dm:
        with pytest.raises(pydsm_mod.DsmError):
            dm.add_text(b"ACG 0.1 7:3\n")          # sample id out of range


@pytest.mark.gpu
def test_cli_dropin_writes_the_tools_files(tmp_path):
    """smtxt2entropy_hip with the reference's options: the count file is byte-identical to the reference tool's, the double
    files agree to the printed precision; an existing output file is refused like the tool does."""
    exe = os.path.join(ROOT, "dsm-framework_amd", "host", "smtxt2entropy_hip")
    text, smpls, maxent, minfreq, _, _ = case_input("five", "minfreq")
    args = [exe, "-s", str(smpls), "-m", ",".join(str(x) for x in maxent), "-M", str(minfreq), "-F", "o"]
    r = subprocess.run(args, input=text, cwd=tmp_path, capture_output=True)
    assert r.returncode == 0, r.stderr
    for kind in ("count", "log", "sqrt", "lgamma"):
        got = open(os.path.join(tmp_path, kind + ".o"), "rb").read()
        want = gzip.open(os.path.join(GOLD, "five", "distmat.minfreq.%s.gz" % kind), "rb").read()
        if kind == "count":
            assert got == want
        else:
            assert len(got.split()) == len(want.split())
            for a, b in zip(got.split(), want.split()):
                if a != b:
                    assert abs(float(a) - float(b)) <= 1e-9 * max(1.0, abs(float(b))) + 2e-6, (kind, a, b)
    r = subprocess.run(args, input=text, cwd=tmp_path, capture_output=True)
    assert r.returncode == 1 and b"already exists" in r.stderr
    # -e steps
    text, smpls, maxent, _, _, _ = case_input("toy3", "step")
    r = subprocess.run([exe, "-s", str(smpls), "-e", "0.3", "-F", "s"], input=text, cwd=tmp_path, capture_output=True)
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(tmp_path, "count.s"), "rb").read() == gzip.open(os.path.join(GOLD, "toy3", "distmat.step.count.gz"), "rb").read()


@pytest.mark.gpu
def test_cli_samplefile_and_normalize(tmp_path):
    """-S and -N through the drop-in CLI, files in the tool's formats."""
    exe = os.path.join(ROOT, "dsm-framework_amd", "host", "smtxt2entropy_hip")
    text, smpls, maxent, minfreq, mapping, sizes = case_input("five", "smap_norm")
    open(os.path.join(tmp_path, "map.txt"), "w").write("".join("%d\n" % x for x in mapping))
    open(os.path.join(tmp_path, "sizes.txt"), "w").write("".join("d%d\t%r\n" % (i, x) for i, x in enumerate(sizes)))
    r = subprocess.run([exe, "-S", "map.txt", "-N", "sizes.txt", "-e", "0.5", "-F", "o"], input=text, cwd=tmp_path, capture_output=True)
    assert r.returncode == 0, r.stderr
    for kind in ("count", "log", "sqrt", "lgamma"):
        got = open(os.path.join(tmp_path, kind + ".o"), "rb").read()
        want = gzip.open(os.path.join(GOLD, "five", "distmat.smap_norm.%s.gz" % kind), "rb").read()
        if kind in ("count", "lgamma"):      # lgamma stays zero under -N
            assert got == want, kind
        else:
            for a, b in zip(got.split(), want.split()):
                if a != b:
                    assert abs(float(a) - float(b)) <= 1e-9 * max(1.0, abs(float(b))) + 2e-6, (kind, a, b)
    r = subprocess.run([exe, "-s", "3", "-S", "map.txt", "-m", "1.0", "-F", "x"], input=text, cwd=tmp_path, capture_output=True)
    assert r.returncode == 1


def _gpu_run(pydsm, text, smpls, maxent, minfreq=0, mapping=None, sizes=None, pieces=1):
    """dsm_distmat on the lines of text, cut into `pieces` batches at line ends."""
    with pydsm.DistMat(smpls, maxent=maxent, minfreq=minfreq, run_to_sample=mapping, sizes=sizes) as dm:
        cuts = [0] + [text.rfind(b"\n", 0, len(text) * k // pieces) + 1 for k in range(1, pieces)] + [len(text)]
        for a, b in zip(cuts, cuts[1:]):
            if b > a:
                dm.add_text(text[a:b])
        return dm.finish()


def _same_bits(r1, r2):
    for k in ("noutput", "count", "log", "sqrt", "lgamma"):
        assert r1[k].tobytes() == r2[k].tobytes(), k


def _random_lines(rng, runs, n, maxk, big=0.05, wrap=0.0, dup=0.0):
    """Server lines with random ids, frequencies mostly below 400 (zeros included), a share >= 1e5, lines with two
    frequencies >= 2^31 (wrap) and repeated ids (dup)."""
    out = []
    for _ in range(n):
        k = int(rng.integers(1, maxk + 1))
        ids = rng.choice(runs, k, replace=False).tolist()
        fr = np.where(rng.random(k) < big, rng.integers(100000, 3000000, k), rng.integers(0, 400, k)).tolist()
        if k >= 2 and rng.random() < wrap:
            fr[0], fr[1] = rng.integers(2 ** 31, 2 ** 32 - 1, 2).tolist()
        if rng.random() < dup:
            ids.append(ids[0])
            fr.append(int(rng.integers(0, 400)))
        out.append("GATTACA 0.5 " + " ".join("%d:%d" % p for p in zip(ids, fr)) + "\n")
    return "".join(out).encode()


# (samples, buckets, mode, lines): every sample count on both sides of the 64 lanes of a tuple group and of the 2 * 32 pair
# limit, buckets on both sides of the 1024 cells that go to LDS, the plain mode, -N (one case with a negative size: -nan cells)
# and -S.  s = 4 with 70000 lines: G = 8, 2048 blocks of 32 groups, so the grid-stride loop runs twice (and the host pass
# runs in several threads).
SWEEP = [(2, 1, "plain", 3000), (3, 3, "S", 3000), (4, 2, "plain", 70000), (8, 16, "plain", 20000), (8, 17, "N", 3000),
         (11, 8, "N", 3000), (12, 7, "plain", 3000), (12, 8, "S", 3000), (18, 3, "S", 2000), (19, 3, "plain", 2000),
         (32, 1, "plain", 2000), (33, 1, "N", 2000), (63, 2, "S", 1000), (64, 1, "plain", 1000), (65, 2, "Nneg", 1000),
         (70, 3, "plain", 1000), (128, 2, "S", 500), (219, 2, "plain", 300), (273, 1, "N", 200)]


@pytest.mark.gpu
@pytest.mark.parametrize("s,nm,mode,n", SWEEP, ids=["s%d_nm%d_%s" % c[:3] for c in SWEEP])
def test_gpu_distmat_sample_and_bucket_sweep(s, nm, mode, n, pydsm_mod):
    rng = np.random.default_rng(1000 * s + nm)
    mapping = sizes = None
    runs = s
    if mode == "S":
        runs = s + s // 2 + 1
        mapping = rng.permutation(np.concatenate([np.arange(s), rng.integers(0, s, runs - s)])).tolist()
    if mode.startswith("N"):
        sizes = (2.0 ** rng.integers(-3, 8, s) * rng.choice([1.0, 1.5, 3.0], s)).tolist()
        if mode == "Nneg":
            sizes[s // 3] = -1e6
    maxent = sorted(rng.uniform(0.2, 0.95, nm - 1).tolist()) + [1.0]
    minfreq = 3 if s % 2 else 0
    text = _random_lines(rng, runs, n, min(runs, 120), wrap=0.05 if mode == "plain" else 0.0, dup=0.1)
    texts, nout, cnt, mats = oracle_run(text, s, maxent, minfreq, mapping, sizes)
    res = _gpu_run(pydsm_mod, text, s, maxent, minfreq, mapping, sizes)
    _cmp(res, nout, cnt, mats)
    assert np.diagonal(res["count"][0]).min() > 0 or s > 100     # every sample occurs: the diagonal is not trivially 0
    if mode == "Nneg":
        assert np.isnan(mats[1]).any()
    _same_bits(res, _gpu_run(pydsm_mod, text, s, maxent, minfreq, mapping, sizes, pieces=5))


def _bucket_of(freqs, s, maxent, nfactor=None):
    """Bucket of one tuple ({sample: freq}, duplicates resolved) as smtxt2entropy.c:128-165, 690-703 pick it; also returns the
    distance of the entropy to the nearest bound."""
    L2 = math.log(2)
    if nfactor is None:
        sumN, sumNlogN = s, 0.0
        for x in sorted(freqs):
            f = freqs[x]
            sumN = (sumN + f) % 2 ** 32
            sumNlogN += float(f + 1) * math.log(f + 1) / L2
        entropy = math.log(sumN) / L2 - sumNlogN / float(sumN)
    else:
        sumN, sumNlogN = float(s), 0.0
        for x in sorted(freqs):
            f = float(freqs[x]) * nfactor[x]
            sumN += f
            sumNlogN += (f + 1) * math.log(f + 1) / L2
        entropy = math.log(sumN) / L2 - sumNlogN / sumN
    entr = L2 * entropy / math.log(s)
    me = sorted(maxent, reverse=True)   # the order of the returned matrices
    b = -1
    for i in range(len(me) - 1, -1, -1):
        if entr <= me[i]:
            b = i
            break
    return b, min(abs(entr - m) for m in me)


def _cumulate(per_bucket):
    """The cumulative matrices of dsm_distmat_finish / smtxt2entropy.c:230-242 from each bucket's sum rounded once."""
    out = [m.copy() for m in per_bucket]
    for i in range(len(out) - 1, 0, -1):
        out[i - 1] = out[i - 1] + out[i]
    return np.stack(out)


@pytest.mark.gpu
@pytest.mark.parametrize("s,nm", [(8, 3), (70, 2)], ids=["lds", "global"])
@pytest.mark.parametrize("kind", ["onehot", "dyadic"])
def test_gpu_distmat_sums_are_exact(s, nm, kind, pydsm_mod):
    """Terms the device computes exactly, summed with Python integers and rounded to a double once: the sums must match bit for
    bit.  onehot: one non-zero frequency per tuple, a perfect square f = r^2, the other samples present with 0 -- the sqrt term is
    f and the lgamma term -(f + 1) (negative totals).  dyadic (-N): sizes 4^k, perfect squares, several non-zero samples -- the
    sqrt terms are dyadic fractions down to 2^-32 whose sums carry through the low 64 bits.  The counts, diagonal included, come
    from numpy.  rtol 1e-9 would hide an error of 1.0 in a 1e10 sum; this does not."""
    rng = np.random.default_rng(s * 10 + nm)
    maxent = [0.35, 0.7, 1.0][3 - nm:]
    nfactor = sizes = None
    if kind == "dyadic":
        sizes = [4.0 ** int(k) for k in rng.integers(-4, 17, s)]
        nfactor = [1.0 / x for x in sizes]
    iu = np.triu_indices(s, 1)
    cnt = np.zeros((nm, s, s), np.int64)
    ip = np.zeros((nm, s, s), object)          # exact sums, in units of 2^-64
    ig = np.zeros((nm, s, s), object)
    lg_log = np.zeros((nm, s, s), np.float64)  # (the log matrix: libm results, compared with a tolerance)
    lines, nout = [], np.zeros(nm, np.int64)
    ntup = 2500 if s < 64 else 800
    while len(lines) < ntup:
        k = int(rng.integers(1, min(s, 12) + 1))
        ids = rng.choice(s, k, replace=False)
        if kind == "onehot":
            fr = np.zeros(k, np.int64)
            fr[0] = int(rng.choice([rng.integers(1, 300), rng.integers(300, 65535)])) ** 2
        else:
            fr = rng.integers(0, 2 ** 16, k) ** 2 * (rng.random(k) < 0.7)
        freqs = {int(i): int(f) for i, f in zip(ids, fr)}
        b, margin = _bucket_of(freqs, s, maxent, nfactor)
        if margin < 1e-9:
            continue                             # (no tuple at a bucket bound: the rounding of the entropy cannot matter)
        lines.append("ACGT 0.5 " + " ".join("%d:%d" % p for p in zip(ids.tolist(), fr.tolist())) + "\n")
        if b < 0:
            continue
        nout[b] += 1
        pres = np.zeros(s, np.int64)
        pres[ids] = 1
        cnt[b] += np.triu(np.outer(pres, pres))
        f = np.zeros(s, np.float64)
        f[ids] = fr
        nz = (f[iu[0]] != 0) | (f[iu[1]] != 0)
        j, kk = iu[0][nz], iu[1][nz]
        if kind == "onehot":
            fu = int(fr[0])
            for a, c in zip(j.tolist(), kk.tolist()):
                ip[b, a, c] += fu << 64
                ig[b, a, c] += -(fu + 1) << 64
                lg_log[b, a, c] += (math.log(fu + 1) - math.log(1)) ** 2
        else:
            sq = np.sqrt(f * np.array(nfactor))
            d = sq[j] - sq[kk]
            t = d * d                             # IEEE products, as on the device; exact dyadic values
            for a, c, x in zip(j.tolist(), kk.tolist(), t.tolist()):
                num, den = x.as_integer_ratio()
                assert (1 << 64) % den == 0
                ip[b, a, c] += num * ((1 << 64) // den)
    text = "".join(lines).encode()
    rnd = lambda m: np.array([float(Fraction(int(v), 1 << 64)) for v in m.ravel()]).reshape(m.shape)
    want_sqrt = _cumulate([rnd(ip[b]) for b in range(nm)])
    want_lgam = _cumulate([rnd(ig[b]) for b in range(nm)])
    want_cnt = np.cumsum(cnt[::-1], axis=0)[::-1]
    want_nout = np.cumsum(nout[::-1])[::-1]
    assert (nout > 0).all() and (np.abs(want_sqrt) > 1e10).any()
    for pieces in (1, 3):
        res = _gpu_run(pydsm_mod, text, s, maxent, sizes=sizes, pieces=pieces)
        assert (res["noutput"] == want_nout).all()
        assert (res["count"] == want_cnt).all()
        assert res["sqrt"].tobytes() == want_sqrt.tobytes(), np.abs(res["sqrt"] - want_sqrt).max()
        assert res["lgamma"].tobytes() == want_lgam.tobytes(), np.abs(res["lgamma"] - want_lgam).max()
        if kind == "onehot":
            assert np.allclose(res["log"], _cumulate(list(lg_log)), rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_gpu_distmat_fused_with_mining_past_64_samples(pydsm_mod, tmp_path):
    """70 samples mined together feed the accumulator batch by batch (no text round trip): the diagonal counts of samples 64 and
    up, and the global-atomic path (4 * 70^2 cells do not fit LDS)."""
    import torch
    from pydsm import builder
    rng = np.random.default_rng(70)
    genome = rng.integers(0, 4, 1500)
    paths = []
    for s in range(70):
        starts = rng.integers(0, len(genome) - 40, 60)
        codes = np.stack([genome[a:a + 40] for a in starts]).astype(np.uint8)
        flip = rng.random(codes.shape) < 0.01
        codes = np.where(flip, (codes + rng.integers(1, 4, codes.shape)) % 4, codes).astype(np.uint8)
        p = tmp_path / ("s%03d.fasta.fmi" % s)
        builder.build_from_codes(torch.from_numpy(codes), str(p))
        paths.append(str(p))
    idx = [pydsm_mod.Index(p) for p in paths]
    maxent = [0.6, 0.8, 0.9, 1.0]
    with pydsm_mod.DistMat(70, maxent=maxent) as dm, pydsm_mod.Miner(idx, fmin=2, maxdepth=12, pmin=1, emax=9.0) as m:
        text, st = m.mine_many(["A", "GT"], on_batch=dm.add)
        res = dm.finish()
    for ix in idx:
        ix.close()
    assert st.tuples > 100
    texts, nout, cnt, mats = oracle_run(text, 70, maxent, 0)
    _cmp(res, nout, cnt, mats)
    assert np.diagonal(cnt[0])[64:].min() > 0


def _cmp_text(got, want):
    """The tool's double files: the same tokens up to the last printed digits; nan, -nan and inf tokens exactly."""
    assert got.count(b"\n") == want.count(b"\n")
    g, w = got.split(), want.split()
    assert len(g) == len(w)
    for a, b in zip(g, w):
        if a != b:
            assert not (b"nan" in a + b or b"inf" in a + b), (a, b)
            assert abs(float(a) - float(b)) <= 1e-9 * max(1.0, abs(float(b))) + 2e-6, (a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["s70", "smap100", "norm_neg", "edges"])
def test_cli_on_synthetic_goldens(case, tmp_path):
    """smtxt2entropy_hip on the reference tool's synthetic goldens: 70 samples, 150 runs onto 100 samples (-S), a negative size
    (-N, -nan cells) and the 32-bit edges (inf cells).  The count file is byte-identical."""
    exe = os.path.join(ROOT, "dsm-framework_amd", "host", "smtxt2entropy_hip")
    info = MAN["distmat"]["synth"][case]
    text, smpls, maxent, minfreq, mapping, sizes = case_input("synth", case)
    args = [exe, "-F", "o"] + info["args"]
    if mapping:
        open(os.path.join(tmp_path, "map.txt"), "w").write("".join("%d\n" % x for x in mapping))
        args += ["-S", "map.txt"]
    else:
        args += ["-s", str(smpls)]
    if sizes:
        open(os.path.join(tmp_path, "sizes.txt"), "w").write("".join("d%d\t%r\n" % (i, x) for i, x in enumerate(sizes)))
        args += ["-N", "sizes.txt"]
    r = subprocess.run(args, input=text, cwd=tmp_path, capture_output=True)
    assert r.returncode == 0, r.stderr
    for kind in ("count", "log", "sqrt", "lgamma"):
        got = open(os.path.join(tmp_path, kind + ".o"), "rb").read()
        want = gzip.open(os.path.join(GOLD, "synth", "distmat.%s.%s.gz" % (case, kind)), "rb").read()
        if kind == "count":
            assert got == want
        else:
            _cmp_text(got, want)


def _batch(lines):
    """A TupleBatch (u64 frequencies) of [(id, freq), ...] lines; the arrays are kept alive with it."""
    import pydsm
    off = np.zeros(len(lines) + 1, np.uint32)
    off[1:] = np.cumsum([len(x) for x in lines])
    ids = np.array([i for x in lines for i, _ in x], np.uint32)
    fr = np.array([f for x in lines for _, f in x], np.uint64)
    b = pydsm.TupleBatch()
    b.ntuples = len(lines)
    b.pair_off = off.ctypes.data_as(C.POINTER(C.c_uint32))
    b.ids = ids.ctypes.data_as(C.POINTER(C.c_uint32))
    b.freqs = fr.ctypes.data_as(C.POINTER(C.c_uint64))
    return b, (off, ids, fr)


@pytest.mark.gpu
@pytest.mark.parametrize("s", [5, 70])
def test_gpu_distmat_32bit_frequency_edges(s, pydsm_mod):
    """Frequencies 2^31, 2^32 - 2, 2^32 - 1, 2^32 and more: the tool reads them with atoi into an unsigned and its sums
    1 + freq and freq[j] + freq[k] + 1 wrap modulo 2^32 (lgamma of a wrapped 0 is inf).  add_text, add with u64 frequencies
    and the oracle agree."""
    rng = np.random.default_rng(32 + s)
    edges = [2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 5000000000, 0, 1, 399]
    lines = []
    for t in range(3000):
        k = int(rng.integers(1, min(s, 8) + 1))
        ids = rng.choice(s, k, replace=False).tolist()
        fr = [int(rng.choice(edges)) if rng.random() < 0.5 else int(rng.integers(0, 400)) for _ in range(k)]
        if k >= 2 and t % 10 == 0:
            f = int(rng.integers(2 ** 31, 2 ** 32 - 1))
            fr[0], fr[1] = f, 2 ** 32 - 1 - f          # freq[j] + freq[k] + 1 wraps to 0
        lines.append(list(zip(ids, fr)))
    text = "".join("AC 0.5 " + " ".join("%d:%d" % p for p in x) + "\n" for x in lines).encode()
    maxent = [0.1, 0.5, 1.0]
    texts, nout, cnt, mats = oracle_run(text, s, maxent, 0)
    assert (nout > 0).all() and np.isinf(mats[2]).any()
    with pydsm_mod.DistMat(s, maxent=maxent) as dm:
        dm.add_text(text)
        r_text = dm.finish()
    with pydsm_mod.DistMat(s, maxent=maxent) as dm:
        b, keep = _batch(lines)
        dm.add(b)
        r_batch = dm.finish()
    _cmp(r_text, nout, cnt, mats)
    _same_bits(r_text, r_batch)
    got = pydsm_mod.DistMat.format(r_text)
    assert got[0] == texts[0]
    for g, w in zip(got[1:], texts[1:]):
        _cmp_text(g, w)
