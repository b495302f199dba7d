"""bench.py --dump-outputs (CPU only): the capture of the timed path's tuple batches and wire streams, fed synthetic batches through
the library's own batch layout (pydsm.TupleBatch).  The sample and the totals are the same however the batches are cut, the sample is
the tuples of smallest key, every array is float32/float64, and the byte budget holds."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from pydsm import TupleBatch  # noqa: E402

N = 60000


@pytest.fixture(scope="module")
def tuples():
    rng = np.random.default_rng(7)
    plen = rng.integers(1, 40, N)
    npair = rng.integers(1, 6, N)
    return {"plen": plen, "npair": npair, "poff": np.concatenate([[0], np.cumsum(plen)]), "qoff": np.concatenate([[0], np.cumsum(npair)]),
            "letters": rng.choice(np.frombuffer(b"ACGT", np.uint8), plen.sum()), "entropy": rng.random(N),
            "ids": rng.integers(0, 64, npair.sum()).astype(np.uint32), "freqs": rng.integers(1, 1 << 40, npair.sum()).astype(np.uint64)}


class _Stats:
    reported, union_nodes, tuples, pairs = 5, 4, 3, 2


def _dump(t, cuts, tmp_path, name):
    keep = []  # the arrays behind the batches' pointers
    s = bench.TupleSample(0)
    for a, b in zip(cuts[:-1], cuts[1:]):
        p, q = t["poff"], t["qoff"]
        arr = [(p[a:b + 1] - p[a]).astype(np.uint32), (q[a:b + 1] - q[a]).astype(np.uint32), np.ascontiguousarray(t["letters"][p[a]:p[b]]),
               np.ascontiguousarray(t["entropy"][a:b]), np.ascontiguousarray(t["ids"][q[a]:q[b]]), np.ascontiguousarray(t["freqs"][q[a]:q[b]])]
        keep.append(arr)
        tb = TupleBatch()
        tb.ntuples = b - a
        tb.path_off = arr[0].ctypes.data_as(C.POINTER(C.c_uint32))
        tb.pair_off = arr[1].ctypes.data_as(C.POINTER(C.c_uint32))
        tb.path_bytes = arr[2].ctypes.data
        tb.entropy = arr[3].ctypes.data_as(C.POINTER(C.c_double))
        tb.ids = arr[4].ctypes.data_as(C.POINTER(C.c_uint32))
        tb.freqs = arr[5].ctypes.data_as(C.POINTER(C.c_uint64))
        s.add(tb)
    d = str(tmp_path / name)
    nbytes = bench.write_dump(d, [{"dump": (s, _Stats)}], 4, 1, 0)
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}, nbytes


def test_tuple_sample_is_the_smallest_keys_whatever_the_batches(tuples, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 5000)
    a, nbytes = _dump(tuples, [0, 7, 100, 20000, 20001, 45000, N], tmp_path, "a")
    b, _ = _dump(tuples, list(range(0, N, 997)) + [N], tmp_path, "b")
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    keys = bench._mix64(np.arange(N, dtype=np.uint64) ^ np.uint64(bench.DUMP_SEED))
    want = np.sort(np.argsort(keys)[:5000])
    t = tuples
    assert np.array_equal(a["tuple_pos"], want) and not a["tuple_lane"].any()
    assert np.array_equal(a["entropy"], t["entropy"][want])
    p, o = a["path"].astype(np.uint8), a["path_off"].astype(np.int64)
    assert [bytes(p[o[i]:o[i + 1]]) for i in range(len(want))] == [bytes(t["letters"][t["poff"][j]:t["poff"][j + 1]]) for j in want]
    assert np.array_equal(a["pair_off"], np.concatenate([[0], np.cumsum(t["npair"][want])]))
    assert np.array_equal(a["pair_id"], np.concatenate([t["ids"][t["qoff"][j]:t["qoff"][j + 1]] for j in want]))
    assert np.array_equal(a["pair_freq"], np.concatenate([t["freqs"][t["qoff"][j]:t["qoff"][j + 1]] for j in want]).astype(np.float64))
    assert a["totals"].tolist() == [N, t["npair"].sum(), t["plen"].sum(), float(t["freqs"].sum(dtype=np.uint64))]
    assert a["counts"].tolist() == [5, 4, 3, 2]
    assert nbytes == sum(x.nbytes for x in a.values())


def test_tuple_sample_keeps_to_the_byte_budget(tuples, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 5000)
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    a, nbytes = _dump(tuples, [0, 30000, N], tmp_path, "a")
    assert nbytes <= 200_000
    m = len(a["tuple_pos"])
    assert 0 < m < 5000
    keys = bench._mix64(np.arange(N, dtype=np.uint64) ^ np.uint64(bench.DUMP_SEED))
    assert set(a["tuple_pos"].astype(np.int64).tolist()) == set(np.argsort(keys)[:m].tolist())  # the m smallest keys


def test_stream_sample(tmp_path):
    rng = np.random.default_rng(3)
    data = [rng.integers(0, 256, 3_000_000 + g, dtype=np.uint8).tobytes() for g in range(4)]
    lanes = [bench.StreamSample(j, 2) for j in range(2)]
    for g, b in enumerate(data):  # lane j holds prefixes j::2
        for o in range(0, len(b), 700_001):
            lanes[g % 2].add(g // 2, b[o:o + 700_001])
    d = str(tmp_path / "s")
    bench.write_dump(d, [{"dump": (c, _Stats)} for c in lanes], 4, 1, 0)
    a = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert a["stream_bytes"].tolist() == [len(b) for b in data]
    assert a["stream_crc32"].tolist() == [zlib.crc32(b) for b in data]
    h, o = a["stream_head"].astype(np.uint8), a["stream_head_off"].astype(np.int64)
    assert [bytes(h[o[g]:o[g + 1]]) for g in range(4)] == [b[:bench.DUMP_HEAD] for b in data]
