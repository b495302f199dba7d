"""The server's entropy filter restated in Python (metaserver.cpp:357-413), tuple-line parsing, threshold picking, and crafted read
sets whose nodes sit exactly on the frequency limits of the miner (tests/test_entropy_edges.py, tests/test_dist_exchange.py)."""
import collections
import math
import os

LN2 = math.log(2.0)
assert LN2.hex() == "0x1.62e42fefa39efp-1"  # the log(2) entropy_tables.h folds

BIG = 64.0  # an emax above every entropy of at most 273 samples (log2(273) < 8.1)


def exact_entropy(d, freqs):
    """metaserver.cpp:379,389 in the order the readers are printed: sumN starts at d, every reader adds (f+1) log(f+1) / log 2."""
    sumN = d
    s = 0.0
    for f in freqs:
        sumN += f
        s += float(f + 1) * math.log(float(f + 1)) / LN2
    return math.log(float(sumN)) / LN2 - s / float(sumN)


Line = collections.namedtuple("Line", "path printed ids freqs raw")


def parse(text):
    """server stdout bytes -> [Line]: path, printed entropy text, reader ids and frequencies in print order, the raw line."""
    out = []
    for raw in text.splitlines(keepends=True):
        col = raw.split()
        pairs = [c.split(b":") for c in col[2:]]
        out.append(Line(col[0], col[1], [int(a) for a, _ in pairs], [int(b) for _, b in pairs], raw))
    return out


def keep(e, emin, emax):
    """the output test of metaserver.cpp:406"""
    return not (emax > 0 and (e < emin or e > emax))


def restate(lines, d, emin, emax, ents=None):
    """the unfiltered tuple list (emax = 0) filtered by the reference's test -> (bytes, tuples, pairs); ents: the lines' exact
    entropies, when the caller has them already"""
    if ents is None:
        ents = [exact_entropy(d, ln.freqs) for ln in lines]
    kept = [ln for ln, e in zip(lines, ents) if keep(e, emin, emax)]
    return b"".join(ln.raw for ln in kept), len(kept), sum(len(ln.ids) for ln in kept)


def order_sensitive(d, ln):
    """True when summing in id order gives another double than the print order"""
    return exact_entropy(d, [f for _, f in sorted(zip(ln.ids, ln.freqs))]) != exact_entropy(d, ln.freqs)


def pick_thresholds(d, lines, nshared=3, norder=3, drops=3):
    """Entropies of the tuples worth a threshold: smallest, largest, the most shared, some that change with the summation order, and
    the one below the `drops` largest (an emax there drops a handful of tuples).  Sorted, without repeats."""
    ents = [exact_entropy(d, ln.freqs) for ln in lines]
    if not ents:
        return []
    pick = {min(ents), max(ents)}
    pick.update(e for e, _ in collections.Counter(ents).most_common(nshared))
    pick.update([e for e, ln in zip(ents, lines) if order_sensitive(d, ln)][:norder])
    desc = sorted(set(ents), reverse=True)
    if len(desc) > drops:
        pick.add(desc[drops])
    return sorted(pick)


def settings(values):
    """every value, one ulp below and above it, as emin (emax large), as emax (emin 0) and as both -> [(emin, emax)]"""
    out = []
    for t in values:
        for v in (math.nextafter(t, -math.inf), t, math.nextafter(t, math.inf)):
            out += [(v, BIG), (0.0, v), (v, v)]
    return list(dict.fromkeys(out))


# ---------------------------------------------------------------------------------------------------------------------------------
# crafted read sets: runs of A.  A read of L letters A holds the node A^k L - k + 1 times; reads that start with C or G, or end with
# T, make the nodes branch to both sides so their tuples are printed.
# ---------------------------------------------------------------------------------------------------------------------------------
def occ(reads, k):
    """occurrences of A^k in the reads and their reverse complements (what the index holds)"""
    n = 0
    for r in reads:
        for s in (r, r[::-1].translate(str.maketrans("ACGT", "TGCA"))):
            for run in s.replace("C", " ").replace("G", " ").replace("T", " ").split():
                n += max(0, len(run) - k + 1)
    return n


def ladder(k0, target, L, flanks=2):
    """reads whose node A^k0 occurs exactly `target` times: copies of A^L, flank reads CA.., GA.., ..AT, and one shorter run that
    makes up the rest."""
    assert L > k0 + 4
    m = L - 2
    reads = ["C" + "A" * m, "G" + "A" * m, "A" * m + "T"] * flanks
    have = occ(reads, k0)
    assert have <= target, (have, target)
    per = L - k0 + 1
    reads += ["A" * L] * ((target - have) // per)
    rest = target - occ(reads, k0)
    if rest:
        reads.append("A" * (k0 + rest - 1))
    assert occ(reads, k0) == target
    return reads


def write_fasta(path, reads):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write(">r%d\n%s\n" % (i, r))


K0, RUN = 8, 64  # the boundary node is A^8; reads hold runs of 64 letters A (57 occurrences each)
PACK_FMAX, U16, TERM_TAB, LOGN_TAB, KEEP_FREQS = 512, 65535, 1 << 16, 1 << 20, 1 << 22  # lfstep.h, entropy_tables.h
CRAFT_KW = dict(fmin=2, maxdepth=K0 + 3, pmin=1)


def freq_targets(d, f):
    """sample 0 holds A^K0 f times, the others fewer"""
    return [f] + [f - 1 - 3 * s for s in range(1, d)]


def sum_targets(d, total):
    """the tuple of A^K0 has sumN = total"""
    rest = total - d
    t = [rest // d] * d
    t[0] += rest - sum(t)
    return t


def level_max(reads, k):
    """largest frequency of a node of depth k under prefix A (both strands, as the index holds them), and the node"""
    comp = str.maketrans("ACGT", "TGCA")
    c = collections.Counter()
    for r in reads:
        for s in (r, r[::-1].translate(comp)):
            for i in range(len(s) - k + 1):
                if s[i] == "A":
                    c[s[i:i + k]] += 1
    return max(c.values()), max(c, key=c.get)


def build_crafted(tmp, tag, targets, device=None, check_level=True):
    """one sample per target; asserts that every sample's A^K0 occurs exactly its target's number of times and, with check_level,
    is the most frequent node of its depth.  device None: the CPU builder.  -> paths"""
    from pydsm import builder
    paths = []
    for s, t in enumerate(targets):
        reads = ladder(K0, t, RUN)
        assert occ(reads, K0) == t
        if check_level:
            assert level_max(reads, K0) == (t, "A" * K0)
        fa = os.path.join(tmp, "%s_%d.fasta" % (tag, s))
        write_fasta(fa, reads)
        if device is None:
            builder.build_from_fasta(fa, fa + ".fmi")
        else:
            builder.build_fasta_hip(fa, fa + ".fmi", device=device)
        paths.append(fa + ".fmi")
    return paths


def sample_name(path):
    return os.path.basename(path)[:-len(".fasta.fmi")]


def boundary_line(lines, targets):
    """the printed tuple of A^K0; asserts its frequencies are the targets"""
    (ln,) = [ln for ln in lines if ln.path == b"A" * K0]
    assert sorted(zip(ln.ids, ln.freqs)) == list(enumerate(targets)), ln.raw
    return ln
