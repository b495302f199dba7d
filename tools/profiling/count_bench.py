#!/usr/bin/env python3
"""Throughput of the pattern counts (dsm_counter_*) on the configs[1] index (d = 1) and on bench.py's eight 1-Gbase samples (d = 8).
  workload A: ~10^6 substrings from mined tuples (a pass over a few prefixes, pmin=1, emax=2.0, fmin=10)
  workload B: 10^6 substrings of length 12..64 of the synthetic reads (seed 42)
Per workload and d: patterns/s, LF steps/s, 64-byte block loads/s and their fraction of the calibrated random-line gather rate
(24.5 G lines/s, profiles/r01_gather_calibration.txt), lane efficiency, k = 0 against the default k, the same counts through chained
dsm_lf_batch_dev calls (what a user had before), and the dsm_count CLI end to end on workload A.  One GPU run; the index files are
shared with bench.py and the tests through DSM_BENCH_DIR.
usage: count_bench.py [--out profiles/count_bench.json] [--quick]   (--quick: d = 1, workload A only, for a kernel-trace run)"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "dsm-framework_amd"))
sys.path.insert(0, ROOT)
GATHER_LINES_PER_S = 24.5e9


def kernel_sha():
    h = hashlib.sha256()
    for f in ("count.hip", "common.h"):
        h.update(open(os.path.join(ROOT, "dsm-framework_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def mined_patterns(pydsm, ix, want):
    import ctypes as C
    paths, offs, total = [], [], 0
    for p in ("TG", "CA", "GA", "AT", "CC", "GT"):
        def on_batch(b):
            n = int(b.ntuples)
            po = np.ctypeslib.as_array(b.path_off, shape=(n + 1,)).astype(np.uint64)
            paths.append(np.frombuffer(C.string_at(b.path_bytes, int(po[-1])), np.uint8).copy())
            offs.append(po)
        with pydsm.Miner([ix], pmin=1, emax=2.0) as m:
            m.mine(p, text=False, on_batch=on_batch)
        total = sum(len(o) - 1 for o in offs)
        if total >= want:
            break
    data = np.concatenate(paths)
    base = np.cumsum([0] + [int(o[-1]) for o in offs[:-1]]).astype(np.uint64)
    off = np.concatenate([o[:-1] + b for o, b in zip(offs, base)] + [np.array([len(data)], np.uint64)])
    npat = min(want, len(off) - 1)
    return data[: int(off[npat])], off[: npat + 1]


def read_patterns(builder, reads, genome, want):
    import torch
    codes = builder.synth_reads(42, reads, 100, genome, 0.005, device="cuda")
    rng = np.random.default_rng(5)
    r = torch.from_numpy(rng.integers(0, reads, want)).cuda()
    L = rng.integers(12, 65, want)
    a = rng.integers(0, 100 - L + 1)
    rows = codes[r].cpu().numpy()
    del codes
    torch.cuda.empty_cache()
    lut = np.frombuffer(b"ACGT", np.uint8)
    off = np.zeros(want + 1, np.uint64)
    off[1:] = np.cumsum(L)
    data = np.empty(int(off[-1]), np.uint8)
    for k in range(want):
        data[off[k]:off[k + 1]] = lut[rows[k, a[k]:a[k] + L[k]]]
    return data, off


def timed_count(pydsm, torch, ixs, data, off, kmer, reps=3):
    """device-resident input; the best of `reps` launches after one warm-up, timed with HIP events"""
    npat = len(off) - 1
    d_data = torch.from_numpy(data).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_cnt = torch.empty((npat, len(ixs)), dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream()
    t0 = time.time()
    c = pydsm.Counter(ixs, kmer=kmer)
    torch.cuda.synchronize()
    create_s = time.time() - t0
    c.count_dev(d_data.data_ptr(), d_off.data_ptr(), npat, d_cnt.data_ptr(), None, s.cuda_stream)
    torch.cuda.synchronize()
    c.stats(reset=True)
    best = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        c.count_dev(d_data.data_ptr(), d_off.data_ptr(), npat, d_cnt.data_ptr(), None, s.cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    st = c.stats(reset=True).as_dict()
    for k in ("lf_steps", "block_loads", "wave_steps", "lane_steps", "table_starts", "rare_blocks", "items", "patterns"):
        st[k] //= reps
    counts = d_cnt.cpu().numpy().view(np.uint64)
    t0 = time.time()
    hc = c.count_packed(data, off)
    host_s = time.time() - t0
    assert (hc == counts).all()
    c.close()
    sec = best / 1e3
    return counts, {
        "kmer": st["kmer"], "ms": best, "patterns_per_s": npat / sec, "items_per_s": npat * len(ixs) / sec,
        "lf_steps": st["lf_steps"], "lf_steps_per_s": st["lf_steps"] / sec, "block_loads": st["block_loads"],
        "block_loads_per_step": st["block_loads"] / max(1, st["lf_steps"]), "block_loads_per_s": st["block_loads"] / sec,
        "frac_of_gather_rate": st["block_loads"] / sec / GATHER_LINES_PER_S, "lane_efficiency": st["lane_efficiency"],
        "table_starts": st["table_starts"], "rare_blocks": st["rare_blocks"], "table_bytes": st["table_bytes"],
        "counter_create_s": create_s, "host_call_s": host_s, "host_call_patterns_per_s": npat / host_s}


def chained_lf_dev(pydsm, torch, ixs, data, off):
    """the counts through dsm_lf_batch_dev, one call per position and sample (each call allocates and synchronises)"""
    npat = len(off) - 1
    lens = torch.from_numpy((off[1:] - off[:-1]).astype(np.int64)).cuda()
    start = torch.from_numpy(off[:-1].astype(np.int64)).cuda()
    d_data = torch.from_numpy(data).cuda()
    out = torch.zeros((npat, len(ixs)), dtype=torch.int64, device="cuda")
    calls = 0
    torch.cuda.synchronize()
    t0 = time.time()
    for i, ix in enumerate(ixs):
        sp = torch.zeros(npat, dtype=torch.int64, device="cuda")
        ep = torch.full((npat,), ix.n - 1, dtype=torch.int64, device="cuda")
        for t in range(int(lens.max())):
            j = torch.nonzero((lens > t) & (ep + 1 > sp)).flatten()
            if j.numel() == 0:
                break
            c = d_data[start[j] + t].contiguous()
            cc = torch.cat([c, c])
            pos = torch.cat([sp[j] - 1, ep[j]]).contiguous()
            res = torch.empty_like(pos)
            ix.lf_batch_dev(cc.data_ptr(), pos.data_ptr(), res.data_ptr(), pos.numel(), 0, torch.cuda.current_stream().cuda_stream)
            calls += 1
            sp[j] = res[: j.numel()]
            ep[j] = res[j.numel():] - 1
        out[:, i] = torch.where(ep + 1 > sp, ep + 1 - sp, torch.zeros_like(sp))
    torch.cuda.synchronize()
    dt = time.time() - t0
    return out.cpu().numpy().view(np.uint64), {"s": dt, "patterns_per_s": npat / dt, "lf_batch_dev_calls": calls}


def cli_run(paths, data, off, workdir):
    exe = os.path.join(ROOT, "dsm-framework_amd", "host", "dsm_count")
    inp = os.path.join(workdir, "count_bench_patterns.txt")
    outp = os.path.join(workdir, "count_bench_counts.txt")
    with open(inp, "wb") as f:
        f.write(b"".join(data[int(off[k]):int(off[k + 1])].tobytes() + b"\n" for k in range(len(off) - 1)))
    t0 = time.time()
    with open(inp, "rb") as fi, open(outp, "wb") as fo:
        r = subprocess.run([exe, "--times", "-f", "1"] + paths, stdin=fi, stdout=fo, stderr=subprocess.PIPE, timeout=600)
    wall = time.time() - t0
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stderr.decode().splitlines() if ln.startswith("dsm_count: parse")][-1]
    parts = line.split()
    lines = sum(1 for _ in open(outp, "rb"))
    assert lines == len(off) - 1
    return {"wall_s": wall, "patterns_per_s": (len(off) - 1) / wall, "parse_s": float(parts[2]), "device_wait_s": float(parts[6]),
            "format_s": float(parts[9]), "output_bytes": os.path.getsize(outp),
            "note": "whole process: index opens, counter (table) creation, read, count, format, write"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "count_bench.json"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--patterns", type=int, default=1000000)
    a = ap.parse_args()
    import argparse as _ap
    import torch
    import bench
    import pydsm
    from pydsm import builder
    reads, genome = 10000000, 50000000
    workdir = os.environ.get("DSM_BENCH_DIR", "/tmp/dsm_bench")
    os.makedirs(workdir, exist_ok=True)
    path1 = os.path.join(workdir, "sample-0.s42_r%d_l100_g%d_e0.005.fmi" % (reads, genome))
    if not os.path.exists(path1):
        codes = builder.synth_reads(42, reads, 100, genome, 0.005, device="cuda")
        builder.build_from_codes(codes, path1 + ".tmp")
        del codes
        torch.cuda.empty_cache()
        os.replace(path1 + ".tmp", path1)
    rec = {"kernel_sha16": kernel_sha(), "kernel": "count_kernel (csrc/count.hip)", "gather_calibration_lines_per_s": GATHER_LINES_PER_S,
           "device": torch.cuda.get_device_name(0), "workloads": {}}
    ix1 = pydsm.Index(path1)
    t0 = time.time()
    wa = mined_patterns(pydsm, ix1, a.patterns)
    rec["workload_A_source"] = {"patterns": len(wa[1]) - 1, "bytes": len(wa[0]), "mine_s": time.time() - t0,
                                "mean_len": len(wa[0]) / (len(wa[1]) - 1)}
    print("workload A: %d patterns" % (len(wa[1]) - 1), flush=True)
    loads = [("A", wa)]
    if not a.quick:
        wb = read_patterns(builder, reads, genome, a.patterns)
        loads.append(("B", wb))
        rec["workload_B_source"] = {"patterns": len(wb[1]) - 1, "bytes": len(wb[0]), "mean_len": len(wb[0]) / (len(wb[1]) - 1)}
    sets = [(1, [ix1], [path1])]
    if not a.quick:
        ns = _ap.Namespace(workdir=workdir, gpus=1, nlocal=8, reads=reads, rlen=100, genome=genome, sub_rate=0.005)
        t0 = time.time()
        paths8 = [bench.build_index(ns, j, "cuda")[0] for j in range(8)]
        rec["d8_index_build_s"] = time.time() - t0
        sets.append((8, [pydsm.Index(p) for p in paths8], paths8))
    for d, ixs, paths in sets:
        for name, (data, off) in loads:
            key = "%s_d%d" % (name, d)
            cnt, r10 = timed_count(pydsm, torch, ixs, data, off, None)
            cnt0, r0 = timed_count(pydsm, torch, ixs, data, off, 0)
            assert (cnt == cnt0).all()
            w = {"default_k": r10, "k0": r0, "speedup_table": r0["ms"] / r10["ms"]}
            if not a.quick:
                lc, rl = chained_lf_dev(pydsm, torch, ixs, data, off)
                assert (lc == cnt).all(), key
                w["chained_lf_batch_dev"] = rl
                w["speedup_vs_chained_lf"] = rl["s"] * 1e3 / r10["ms"]
            if name == "A" and (d == 1 or not a.quick):
                w["cli"] = cli_run(paths, data, off, workdir)
            rec["workloads"][key] = w
            print(key, json.dumps({k: (v if not isinstance(v, dict) else {q: v[q] for q in ("ms", "patterns_per_s", "frac_of_gather_rate", "lane_efficiency", "block_loads_per_step") if q in v}) for k, v in w.items()}), flush=True)
    if not a.quick:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
