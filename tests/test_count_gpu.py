"""Pattern counts (dsm_counter_*, pydsm.Counter, host/dsm_count) on the GPU:
  * pinned by the reference's own output: every id:freq of every committed server output line equals the count in that sample,
    and every sample absent from a line counts below the client's fmin -- with and without the k-mer table;
  * edge cases on toy3 against a plain count over the reads and their reverse complements and against chained Index.lf_batch;
  * the CLI fed a golden server output;
  * full size: the configs[1] index (mined tuples, random patterns) and an index of n > 2^32."""
import gzip
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "dsm-framework_amd", "host", "dsm_count")
U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def _lines(setname, cfg, prefix):
    with gzip.open(os.path.join(GOLD, setname, "server.%s.%s.txt.gz" % (cfg, prefix)), "rb") as f:
        return f.read().splitlines()


def _golden_sets(golden):
    """(set, names, client fmin, [(cfg, prefix)]) for every committed server output"""
    m = golden.manifest["sets"]
    toy = [(cfg, p) for cfg in m["toy3"]["server_cfgs"] for p in m["toy3"]["prefixes"]
           if os.path.exists(os.path.join(GOLD, "toy3", "server.%s.%s.txt.gz" % (cfg, p)))]
    return [("toy3", m["toy3"]["names"], 2, toy),
            ("toy3", m["toy3"]["names"], 1, [("p1_fmin1_M24", p) for p in "ACGT"]),
            ("five", m["five"]["names"], 10, [("default", p) for p in m["five"]["prefixes"]]),
            ("many30", m["many30"]["names"], 3, [(cfg, p) for cfg in m["many30"]["server_cfgs"] for p in m["many30"]["prefixes"]])]


def chained_lf(ix, patterns):
    """(count, sp) per pattern by pushing its bytes through Index.lf_batch, one batched call per position"""
    pats = [p if isinstance(p, bytes) else p.encode("latin-1") for p in patterns]
    k = len(pats)
    sp = np.zeros(k, np.uint64)
    ep = np.full(k, ix.n - 1, np.uint64)
    live = np.ones(k, bool)
    lens = np.array([len(p) for p in pats])
    for t in range(int(lens.max()) if k else 0):
        j = np.flatnonzero(live & (lens > t))
        if len(j) == 0:
            break
        c = np.array([pats[q][t] for q in j], np.uint8)
        lo = ix.lf_batch(np.concatenate([c, c]), np.concatenate([sp[j] - np.uint64(1), ep[j]]))   # (sp - 1 wraps: rank(-1) = 0)
        nsp, nep = lo[:len(j)], lo[len(j):] - np.uint64(1)
        sp[j], ep[j] = nsp, nep
        live[j] = nep + np.uint64(1) > nsp
    cnt = np.where(live, ep + np.uint64(1) - sp, np.uint64(0)).astype(np.uint64)
    return cnt, sp


def test_counts_pinned_by_reference_server_outputs(golden):
    import pydsm
    total = 0
    for setname, names, fmin, outs in _golden_sets(golden):
        ixs = [pydsm.Index(golden.fmi(setname, n)) for n in names]
        paths, listed = [], []
        for cfg, p in outs:
            for ln in _lines(setname, cfg, p):
                f = ln.split()
                paths.append(f[0])
                listed.append({int(a): int(b) for a, b in (x.split(b":") for x in f[2:])})
        assert paths, setname
        res = []
        for k in (0, None):
            with pydsm.Counter(ixs, kmer=k) as c:
                res.append(c.count(paths))
        assert (res[0] == res[1]).all(), "k = 0 and the default table disagree on %s" % setname
        got = res[0]
        for r, want in enumerate(listed):
            for i in range(len(names)):
                if i in want:
                    assert got[r, i] == want[i], (setname, paths[r], i, int(got[r, i]), want[i])
                else:
                    assert got[r, i] < fmin, (setname, paths[r], i, int(got[r, i]), "unlisted sample reaches fmin")
        total += len(paths)
        for x in ixs:
            x.close()
    print("pinned: %d server lines" % total)


def _naive_strings(golden, names):
    from pydsm import builder
    out = []
    for n in names:
        reads = builder.read_fasta(golden.fasta("toy3", n))
        rs = []
        for r in reads:
            a = builder._NORM[np.frombuffer(r.encode("latin-1"), np.uint8)].tobytes()
            rc = builder._COMP[np.frombuffer(a, np.uint8)][::-1].tobytes()
            rs.append(a + b"-" + rc)
        out.append(rs)
    return out


def _naive(strings, p):
    if not p:
        return None
    tot = 0
    for s in strings:
        i = s.find(p)
        while i >= 0:
            tot += 1
            i = s.find(p, i + 1)
    return tot


def _revcomp(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def test_edge_cases_on_toy3(golden):
    import pydsm
    names = golden.manifest["sets"]["toy3"]["names"]
    ixs = [pydsm.Index(golden.fmi("toy3", n)) for n in names]
    strs = _naive_strings(golden, names)
    rng = np.random.default_rng(7)
    pats = []
    for _ in range(1500):          # read substrings of length 1..80 (from read + '-' + revcomp: some cross the '-')
        s = strs[rng.integers(3)][rng.integers(1000)]
        L = int(rng.integers(1, 81))
        a = int(rng.integers(0, max(1, len(s) - L + 1)))
        pats.append(s[a:a + L])
    pats += ["".join(rng.choice(list("ACGT"), int(rng.integers(1, 16)))).encode() for _ in range(1500)]
    special = [b"", b"A", b"N", b"-", b"\0", b"AC-G", b"ACGTN", b"NNNN", b"a", b"Z", b"ACGTZ", b"acgt", b"A\0", b"\0A", b"-A", b"C-",
               b"ACGTACGTACGT", b"T" * 200, strs[0][0] + strs[0][1]]
    pats += special
    with pydsm.Counter(ixs) as c0, pydsm.Counter(ixs, kmer=0) as c1:
        cnt, sp = c0.count(pats, with_sp=True)
        cnt1, sp1 = c1.count(pats, with_sp=True)
        st = c0.stats()
    assert cnt.shape == (len(pats), 3) and cnt.dtype == np.uint64
    assert (cnt == cnt1).all()
    pos = cnt > 0
    assert (sp[pos] == sp1[pos]).all()
    assert 0 < st.lane_steps <= 64 * st.wave_steps and st.table_starts > 0 and st.kmer == 10
    for i, ix in enumerate(ixs):
        lc, lsp = chained_lf(ix, pats)
        assert (cnt[:, i] == lc).all(), i
        assert (sp[cnt[:, i] > 0, i] == lsp[cnt[:, i] > 0]).all(), i
        assert cnt[pats.index(b""), i] == ix.n
        for q, p in enumerate(pats):
            if b"\0" in p or not p:
                continue
            assert int(cnt[q, i]) == _naive(strs[i], p), (p, i)
    for b in (b"a", b"Z", b"ACGTZ", b"acgt"):
        assert (cnt[pats.index(b)] == 0).all()
    assert (cnt[pats.index(b"-")] == np.array([len(s) for s in strs], np.uint64)).all()   # one '-' per read
    # count(s) == count(revcomp(s)) for ACGT strings
    acgt = [p for p in pats if p and all(ch in b"ACGT" for ch in p)]
    a = pydsm.count(ixs, acgt)
    b = pydsm.count(ixs, [_revcomp(p) for p in acgt])
    assert (a == b).all()
    # a batch of 1, a batch of 300 000, a single index
    assert (pydsm.count(ixs, [pats[5]]) == cnt[5:6]).all()
    big = [pats[q] for q in rng.integers(0, len(pats), 300000)]
    with pydsm.Counter(ixs) as c:
        got = c.count(big)
    idx = {p: q for q, p in enumerate(pats)}
    assert (got == cnt[[idx[p] for p in big]]).all()
    assert (pydsm.count(ixs[1:2], pats) == cnt[:, 1:2]).all()
    # str input is taken byte for byte
    assert (pydsm.count(ixs, ["ACG", "N"]) == pydsm.count(ixs, [b"ACG", b"N"])).all()
    # the device entry point on torch tensors
    import torch
    data, off = pydsm.pack_patterns(pats)
    d_data = torch.from_numpy(data.copy()).cuda()
    d_off = torch.from_numpy(off.view(np.int64).copy()).cuda()
    d_cnt = torch.zeros((len(pats), 3), dtype=torch.int64, device="cuda")
    with pydsm.Counter(ixs) as c:
        c.count_dev(d_data.data_ptr(), d_off.data_ptr(), len(pats), d_cnt.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert (d_cnt.cpu().numpy().view(np.uint64) == cnt).all()
    # an offloaded index is refused, at creation and at a count
    with pydsm.Counter(ixs) as c:
        ixs[2].offload()
        with pytest.raises(pydsm.DsmError) as e:
            c.count([b"ACGT"])
        assert e.value.code == -22
        with pytest.raises(pydsm.DsmError) as e:
            pydsm.Counter(ixs)
        assert e.value.code == -22
        ixs[2].reload()
        torch.cuda.synchronize()
        assert (c.count(pats[:50]) == cnt[:50]).all()
    for x in ixs:
        x.close()


def test_indexes_on_two_devices_are_refused(golden):
    import torch
    import pydsm
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    a = pydsm.Index(golden.fmi("toy3", "toy-1"), device=0)
    b = pydsm.Index(golden.fmi("toy3", "toy-2"), device=1)
    with pytest.raises(pydsm.DsmError) as e:
        pydsm.Counter([a, b])
    assert e.value.code == -22
    a.close()
    b.close()


def test_cli_round_trip_on_a_golden_server_output(golden, tmp_path):
    names = golden.manifest["sets"]["toy3"]["names"]
    fmis = [golden.fmi("toy3", n) for n in names]
    src = golden.server_out("toy3", "default", "A") + golden.server_out("toy3", "pmax2", "AC")
    r = subprocess.run([EXE, "-f", "2"] + fmis, input=src, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    want = src.splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g, w = g.split(), w.split()
        assert g[0] == w[0]
        assert set(g[1:]) == set(w[2:]), (g, w)
    # --all lists every sample; -k 0 changes nothing
    r2 = subprocess.run([EXE, "--all", "-k", "0", "-f", "2"] + fmis, input=src, capture_output=True, timeout=120)
    assert r2.returncode == 0, r2.stderr
    assert all(len(ln.split()) == 4 for ln in r2.stdout.splitlines())
    assert all(set(x for x in a.split()[1:] if not x.endswith(b":0") and int(x.split(b":")[1]) >= 2) == set(b.split()[1:])
               for a, b in zip(r2.stdout.splitlines(), got))


@pytest.fixture(scope="module")
def big():
    """the configs[1] index: the same seed, file name and directory as test_fullsize_gpu.py's fixture (built once per session)"""
    import torch
    import pydsm
    from pydsm import builder
    reads = int(os.environ.get("DSM_FULLSIZE_READS", "10000000"))
    genome = reads * 5
    d = os.environ.get("DSM_BENCH_DIR", "/tmp/dsm_bench")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "sample-0.s42_r%d_l100_g%d_e0.005.fmi" % (reads, genome))
    if not os.path.exists(path):
        codes = builder.synth_reads(42, reads, 100, genome, 0.005, device="cuda")
        builder.build_from_codes(codes, path + ".tmp")
        del codes
        torch.cuda.empty_cache()
        os.replace(path + ".tmp", path)
    ix = pydsm.Index(path)
    yield pydsm, ix
    ix.close()


def test_full_size_mined_tuples_and_random_patterns(big):
    import ctypes as C
    pydsm, ix = big
    paths, offs, freqs = [], [], []

    def on_batch(b):
        n = int(b.ntuples)
        po = np.ctypeslib.as_array(b.path_off, shape=(n + 1,)).astype(np.uint64)
        paths.append(np.frombuffer(C.string_at(b.path_bytes, int(po[-1])), np.uint8).copy())
        offs.append(po)
        pairs = int(np.ctypeslib.as_array(b.pair_off, shape=(n + 1,))[-1])
        assert pairs == n
        freqs.append(np.ctypeslib.as_array(b.freqs, shape=(pairs,)).copy())

    with pydsm.Miner([ix], pmin=1, emax=2.0) as m:
        m.mine("TG", text=False, on_batch=on_batch)
    data = np.concatenate(paths)
    base = np.cumsum([0] + [int(o[-1]) for o in offs[:-1]]).astype(np.uint64)
    off = np.concatenate([o[:-1] + b for o, b in zip(offs, base)] + [np.array([len(data)], np.uint64)])
    fr = np.concatenate(freqs)
    assert len(fr) > 100000
    with pydsm.Counter([ix]) as c:
        got = c.count_packed(data, off)[:, 0]
        st = c.stats()
    assert (got == fr).all()
    print("configs[1] TG: %d tuples, lane efficiency %.3f, %.3f block loads per step" % (len(fr), st.lane_steps / 64.0 / st.wave_steps,
                                                                                        st.block_loads / max(1, st.lf_steps)))
    _random_vs_chained(pydsm, ix, 2026)


def _random_vs_chained(pydsm, ix, seed):
    rng = np.random.default_rng(seed)
    pats = ["".join(rng.choice(list("ACGT"), int(rng.integers(1, 25)))) for _ in range(4000)]
    pats += ["".join(rng.choice(list("ACGTN-"), int(rng.integers(1, 8)))) for _ in range(96)]
    with pydsm.Counter([ix]) as c:
        got, sp = c.count(pats, with_sp=True)
    lc, lsp = chained_lf(ix, pats)
    assert (got[:, 0] == lc).all()
    assert (sp[got[:, 0] > 0, 0] == lsp[lc > 0]).all()
    assert (got[:, 0] > 0).sum() > 1000


def test_positions_beyond_2_32_against_chained_lf():
    """the pseudo-BWT of test_fullsize_gpu.py::test_positions_beyond_2_32 (same recipe and path): an arbitrary symbol string, so
    counts are compared with chained LF only"""
    import torch
    import pydsm
    from pydsm import builder
    n = int(os.environ.get("DSM_WIDE_N", str((1 << 32) + 300_000_000)))
    d = os.environ.get("DSM_BENCH_DIR", "/tmp/dsm_bench")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "pseudo-%d.fmi" % n)
    if not os.path.exists(path):
        g = torch.Generator(device="cuda").manual_seed(4242)
        syms = torch.tensor([0, ord("-"), ord("A"), ord("C"), ord("G"), ord("N"), ord("T")], dtype=torch.uint8, device="cuda")
        cum = torch.tensor([0.005, 0.010, 0.258, 0.505, 0.750, 0.752], device="cuda")
        bwt = torch.empty(n, dtype=torch.uint8, device="cuda")
        step = 1 << 28
        for o in range(0, n, step):
            m = min(step, n - o)
            bwt[o:o + m] = syms[torch.bucketize(torch.rand(m, device="cuda", generator=g), cum)]
        builder.write_fmi(bwt, path + ".tmp", 1, 0)
        del bwt
        torch.cuda.empty_cache()
        os.replace(path + ".tmp", path)
    with pydsm.Index(path) as ix:
        assert ix.n == n
        _random_vs_chained(pydsm, ix, 99)
