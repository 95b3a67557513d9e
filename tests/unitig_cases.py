"""The rule of `ploidyfrost build` (K-UNITIG) in plain Python -- sets of strings, nothing tiled or hashed by hand --, the output format,
the comparator against another program's GFA, and the deterministic cases the host restatement (pf_unitig::build_host) and the kernels
(pf_unitig.hip) are held to.

  vertices   S = the canonical k-mers of the reads (windows whose k bytes are all in ACGTacgt, lower case read as upper case).
  link       an oriented k-mer x links to y when succ(x) == [y], pred(y) == [x] and canon(x) != canon(y).  A unitig is a maximal chain of
             links that visits no canonical k-mer twice (a chain that runs into a k-mer equal to its own reverse complement ends there:
             the link that leaves it leads back to where the chain came from).
  simplify   CompactedDBG::removeUnitigs: unitigs of fewer than k k-mers, decided against the graph as it stands, deleted afterwards.
  recompact  the link rule once more over what is left.
"""
import random

_RC = str.maketrans("ACGT", "TGCA")
BASES = "ACGT"
FLAGS = [(False, False), (True, False), (False, True), (True, True)]   # (clip_tips -i, del_isolated -d)
STATS = ("distinct", "unitigs", "removed", "unitigs_out", "longest", "bytes")


def revcomp(s):
    return s.translate(_RC)[::-1]


def canon(s):
    r = revcomp(s)
    return s if s <= r else r


def kmer_set(reads, k):
    """the canonical k-mers of the reads (str or bytes)"""
    S = set()
    for r in reads:
        if isinstance(r, bytes):
            r = r.decode("latin-1")
        r = r.upper()
        for i in range(len(r) - k + 1):
            w = r[i:i + k]
            if all(c in BASES for c in w):
                S.add(canon(w))
    return S


def succ(S, x):
    return [x[1:] + b for b in BASES if canon(x[1:] + b) in S]


def pred(S, x):
    return [b + x[:-1] for b in BASES if canon(b + x[:-1]) in S]


def link(S, x):
    su = succ(S, x)
    if len(su) != 1:
        return None
    y = su[0]
    if canon(y) == canon(x) or pred(S, y) != [x]:
        return None
    return y


def unitigs(S):
    """[(chain of oriented k-mers, closed)]: every canonical k-mer of S in exactly one chain"""
    out, seen = [], set()
    for c in sorted(S):
        if c in seen:
            continue
        chain, inside, closed = [c], {c}, False
        x = c
        while True:
            y = link(S, x)
            if y is None:
                break
            if y == chain[0]:
                closed = True
                break
            if canon(y) in inside:
                break
            chain.append(y)
            inside.add(canon(y))
            x = y
        x = c
        while not closed:
            y = link(S, revcomp(x))
            if y is None or canon(y) in inside:
                break
            x = revcomp(y)
            chain.insert(0, x)
            inside.add(canon(x))
        seen |= inside
        out.append((chain, closed))
    return out


def removed_by(S, chain, closed, k, clip, dele):
    """CompactedDBG::removeUnitigs' predicate on one unitig"""
    if len(chain) >= k:
        return False
    p, s = len(pred(S, chain[0])), len(succ(S, chain[-1]))
    lim = 1 if clip else 0
    if p > lim or s > lim:
        return False
    if clip and dele:
        return p + s <= lim
    if clip or dele:
        return p + s == lim
    return False


def oriented(chain, closed):
    """the reading that is written: (first k-mer as read, sequence)"""
    if closed:
        cs = [canon(x) for x in chain]
        j = cs.index(min(cs))
        if chain[j] != cs[j]:
            chain = [revcomp(x) for x in reversed(chain)]
            j = len(chain) - 1 - j
        chain = chain[j:] + chain[:j]
    elif revcomp(chain[-1]) < chain[0]:
        chain = [revcomp(x) for x in reversed(chain)]
    return chain[0], chain[0] + "".join(x[-1] for x in chain[1:])


def default_g(k):
    return k - 8 if k >= 15 else k - 4 if k >= 7 else k - 2


def header(k, g=None):
    return "H\tVN:Z:1.0\tBV:Z:1.0.6\tKL:Z:%d\tML:Z:%d\n" % (k, default_g(k) if g is None else g)


def build(S, k, clip=False, dele=False, g=None):
    """(text of <out>.gfa as bytes, statistics) from the canonical k-mers S"""
    first = unitigs(S)
    gone = [c for c, closed in first if removed_by(S, c, closed, k, clip, dele)]
    if gone:
        S = S - {canon(x) for c in gone for x in c}
    final = unitigs(S) if gone else first
    lines = sorted(oriented(c, closed) for c, closed in final)
    text = header(k, g) + "".join("S\t%d\t%s\n" % (i + 1, seq) for i, (_, seq) in enumerate(lines))
    stats = dict(distinct=len(S) + sum(len(c) for c in gone), unitigs=len(first), removed=len(gone), unitigs_out=len(lines),
                 longest=max([len(seq) for _, seq in lines] + [0]), bytes=len(text))
    return text.encode(), stats


def build_reads(reads, k, clip=False, dele=False, g=None):
    return build(kmer_set(reads, k), k, clip, dele, g)


# ---- the comparator ----

def gfa_sequences(text):
    """(k, [sequence of every S-line]) of a GFA text (bytes); L-lines are ignored"""
    if isinstance(text, bytes):
        text = text.decode()
    k, seqs = None, []
    for ln in text.split("\n"):
        f = ln.split("\t")
        if f[0] == "H":
            for t in f[1:]:
                if t.startswith("KL:Z:"):
                    k = int(t[5:])
        elif f[0] == "S":
            seqs.append(f[2])
    return k, seqs


def normal_form(seqs, k):
    """the multiset of min(seq, revcomp(seq)) as a sorted list; a unitig whose last k-mer links to its first (a closed cycle, cut where
    the writer happened to start) is rotated to its smallest canonical k-mer first"""
    S = kmer_set(seqs, k)
    out = []
    for s in seqs:
        chain = [s[i:i + k] for i in range(len(s) - k + 1)]
        if len(chain) > 1 and link(S, chain[-1]) == chain[0]:
            s = oriented(chain, True)[1]
        out.append(min(s, revcomp(s)))
    return sorted(out)


def same_graph(text_a, text_b):
    ka, a = gfa_sequences(text_a)
    kb, b = gfa_sequences(text_b)
    return ka == kb and normal_form(a, ka) == normal_form(b, kb)


# ---- the cases ----

def rand_seq(rng, n):
    return "".join(rng.choice(BASES) for _ in range(n))


def _chain_read(rng, n_kmers, k):
    return rand_seq(rng, n_kmers + k - 1)


def _tip_case(rng, k, tip_kmers, backbone=300):
    """a backbone and a read that shares k - 1 bases with its middle and then runs off: a tip of tip_kmers k-mers"""
    b = rand_seq(rng, backbone)
    at = backbone // 2
    other = [c for c in BASES if c != b[at + k - 1]]
    tip = b[at:at + k - 1] + rng.choice(other) + rand_seq(rng, tip_kmers - 1)
    return [b, tip]


def _circle_reads(circle, k, read_len=None):
    n = len(circle)
    read_len = read_len or min(n + k - 1, 3 * k)
    twice = circle * (2 + read_len // n)
    return [twice[i:i + read_len] for i in range(0, n, max(1, read_len - k))] if read_len < n + k - 1 else [twice[:n + k - 1]]


def _isolated(rng, count, k):
    return [rand_seq(rng, k) for _ in range(count)]


def cases():
    """[(name, k, reads)], deterministic; every one runs under the four flag combinations"""
    out = []
    rng = random.Random(20240607)
    for m in (1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025):               # the jumping rounds
        out.append(("chain%d" % m, 25, [_chain_read(rng, m, 25)]))
    for d, name in ((-2, "km2"), (-1, "km1"), (0, "k"), (1, "kp1")):      # clipped, clipped, kept, kept
        out.append(("tip_" + name, 25, _tip_case(rng, 25, 25 + d)))
    b = rand_seq(rng, 200)                                                # two tips on one branch node
    others = [c for c in BASES if c != b[100 + 10]]
    out.append(("two_tips", 11, [b, b[100:110] + others[0] + rand_seq(rng, 4), b[100:110] + others[1] + rand_seq(rng, 6)]))
    circle = rand_seq(rng, 120)                                           # a tip on a closed cycle: clipped, the cycle closes
    other = [c for c in BASES if c != circle[60 + 10]]
    out.append(("cycle_tip", 11, _circle_reads(circle, 11) + [circle[60:70] + other[0] + rand_seq(rng, 3)]))
    out.append(("isolated_km1", 11, [rand_seq(rng, 10 + 11 - 1), rand_seq(rng, 80)]))
    out.append(("isolated_k", 11, [rand_seq(rng, 11 + 11 - 1), rand_seq(rng, 80)]))
    for m in (2, 3, 64, 500):                                             # closed cycles of m k-mers
        k = 25 if m == 500 else 11
        while True:                                                       # a circle whose m windows are one closed unitig
            c = rand_seq(rng, m)
            S = kmer_set([c * (2 + k // m)], k)
            if len(S) == m and [closed for _, closed in unitigs(S)] == [True]:
                break
        out.append(("cycle%d" % m, k, _circle_reads(c, k, None if m > 3 * k else m + k - 1 + 2)))
    out.append(("homopolymer", 25, ["A" * 60]))
    out.append(("at30", 25, ["AT" * 30]))
    out.append(("acgt20", 25, ["ACGT" * 20]))
    out.append(("at30_k8", 8, ["AT" * 30]))
    out.append(("acgt20_k8", 8, ["ACGT" * 20]))
    h = rand_seq(rng, 40)                                                 # a hairpin: the window a + w (w = its own reverse complement,
    out.append(("hairpin", 11, [h + revcomp(h)]))                         # k - 1 bases) is followed by w + comp(a), its reverse complement
    h = rand_seq(rng, 30)
    out.append(("hairpin_tail", 11, [h + revcomp(h)[:14] + rand_seq(rng, 20)]))
    for k in (8, 24):                                                     # even k: a k-mer equal to its own reverse complement inside a read
        half = rand_seq(rng, k // 2)
        pal = half + revcomp(half)
        out.append(("palindrome_k%d" % k, k, [rand_seq(rng, 40) + pal + rand_seq(rng, 40), rand_seq(rng, 3 * k)]))
        out.append(("palindrome_alone_k%d" % k, k, [pal]))
    for k in (3, 5, 25, 31):
        g = rand_seq(rng, 12 if k == 3 else 40 if k == 5 else 400)
        reads = [g[i:i + 60] for i in range(0, len(g) - 30, 20)]
        reads += [revcomp(r) for r in reads[::2]]
        reads.append(g[100:130] + "T" + g[131:160] if len(g) > 160 else g[:6])   # one substitution: a bubble or a tip
        out.append(("k%d" % k, k, reads))
    g = rand_seq(rng, 300)
    out.append(("lower_case", 25, [g[:200].lower(), g[100:], revcomp(g[50:250]).lower()]))
    out.append(("with_n", 25, [g[:120] + "N" + g[121:], g[60:200] + "NN" + g[202:], "N" * 30, g[:24] + "n" + g[25:80]]))
    out.append(("short_reads", 25, [g[:24], g[10:30], "", "ACGT"]))
    out.append(("empty", 25, []))
    for count in (9, 10, 99, 100, 999, 1000, 9999, 10000):               # the id width of the line-length formula
        out.append(("isolated_x%d" % count, 25, _isolated(rng, count, 25)))
    out.append(("isolated_x20500", 25, _isolated(rng, 20500, 25)))
    return out


# ---- a graph made for its size ----
# The cases above are read by the Python rule; this one is too large for it (sets of strings, half a minute at this size) and is held to
# the host's restatement, which the test without a GPU holds to the Python rule on every case above and on a small graph of this
# make.  The kernels stride over their items with one grid of a fixed size (pf::ctx_grid: the device's compute units x 8 blocks of 256
# threads), so the caller asks for more k-mers than one such pass has threads: every kernel over k-mers, over oriented k-mers and
# (without -d) over lines then takes the stride more than once.  Keys are random, so sorting scatters every structure over the array.

def _windows(seqs, k):
    """canonical keys of every window of the rows of seqs (a numpy array of codes 0..3, one read a row), flat"""
    import numpy as np
    w = seqs.shape[1] - k + 1
    fw = np.zeros((seqs.shape[0], w), dtype=np.uint64)
    rc = np.zeros((seqs.shape[0], w), dtype=np.uint64)
    for j in range(k):
        col = seqs[:, j:j + w].astype(np.uint64)
        fw |= col << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - col) << np.uint64(2 * j)
    return np.minimum(fw, rc).ravel()


def grid_case(n_kmers, k=25, seed=20240611):
    """(sorted distinct canonical keys as uint64, at least n_kmers of them; {name: keys of the k-mers of one kind of structure}):
    mostly single k-mers (one line each), chains of 2 to 5 and of k + 16 k-mers, four chains of 3 000 k-mers, backbones with a tip of
    5 k-mers each (clipped with -i, the backbone rejoins), and closed cycles of 120, 500 and 777 k-mers, the first with a tip"""
    import numpy as np
    rng = np.random.default_rng(seed)

    def reads(count, length):
        return rng.integers(0, 4, size=(count, length), dtype=np.uint8)

    def circle(length):
        c = reads(1, length)
        return np.concatenate([c, c[:, :k - 1]], axis=1)

    parts = {}
    short = max(1, n_kmers // 200)
    parts["short"] = np.concatenate([_windows(reads(short, k - 1 + m), k) for m in (2, 3, 4, 5)])
    parts["long"] = _windows(reads(max(1, n_kmers // 1000), 2 * k + 15), k)
    parts["longest"] = _windows(reads(4, 3000 + k - 1), k)
    backbone = reads(max(4, n_kmers // 4000), 100)
    tip = np.concatenate([backbone[:, 30:30 + k - 1], (backbone[:, 30 + k - 1:30 + k] + 1 + reads(len(backbone), 1) % 3) % 4, reads(len(backbone), 4)], axis=1)
    parts["backbone"] = _windows(backbone, k)
    parts["tip"] = _windows(tip, k)
    cyc = circle(120)
    parts["cycle"] = np.concatenate([_windows(cyc, k), _windows(circle(500), k), _windows(circle(777), k)])
    parts["cycle_tip"] = _windows(np.concatenate([cyc[:, 60:60 + k - 1], (cyc[:, 60 + k - 1:60 + k] + 1) % 4, reads(1, 2)], axis=1), k)
    have = sum(len(p) for p in parts.values())
    parts["single"] = _windows(reads(max(1, n_kmers - have) + 64, k), k)
    keys = np.unique(np.concatenate(list(parts.values())))
    assert len(keys) >= n_kmers
    return keys, parts


def _revcomp_keys(x, k):
    """the reverse complement of 2 k-bit keys: the 2-bit groups of the word reversed, complemented, shifted down"""
    import numpy as np
    u = np.uint64
    for bits, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF), (32, 0x00000000FFFFFFFF)):
        x = ((x >> u(bits)) & u(m)) | ((x & u(m)) << u(bits))
    return ~x >> u(64 - 2 * k)


def has_neighbour(keys, k):
    """per key of the sorted distinct canonical keys: some successor or predecessor of it is in the set (itself and its own reverse
    complement count, as in the rule)"""
    import numpy as np
    mask = np.uint64((1 << (2 * k)) - 1)
    some = np.zeros(len(keys), dtype=bool)
    for x in (keys, _revcomp_keys(keys, k)):       # the successors of both readings: all eight neighbours
        for b in range(4):
            y = ((x << np.uint64(2)) | np.uint64(b)) & mask
            y = np.minimum(y, _revcomp_keys(y, k))
            some |= keys[np.minimum(np.searchsorted(keys, y), len(keys) - 1)] == y
    return some


def grid_expected(keys, k, clip, dele, rest_build):
    """(text, statistics) of the graph of `keys` with the rule applied by rest_build(keys, k, clip, dele) to the k-mers that have a
    neighbour only.  A k-mer without a neighbour is in no succ() or pred() of another one, so taking it out changes no link, no p or s
    and no recompaction of the rest; by the rule it is a unitig of one k-mer with p = s = 0, written as its canonical reading (the
    smaller of the two first k-mers), which goes with -d (p + s == 0 == lim, or <= 1 with -i too) and stays otherwise.  The lines of
    the two parts are merged by their first k-mer and numbered."""
    import numpy as np
    lone = ~has_neighbour(keys, k)
    n_lone = int(lone.sum())
    rest_text, rest = rest_build(keys[~lone], k, clip, dele)
    seqs = [s.encode() for s in gfa_sequences(rest_text)[1]]
    first = [encode(s[:k].decode()) for s in seqs]
    if not dele and n_lone:
        lk = keys[lone]
        shifts = np.arange(2 * (k - 1), -1, -2, dtype=np.uint64)
        chars = np.frombuffer(BASES.encode(), dtype=np.uint8)[((lk[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)].tobytes()
        seqs += [chars[i:i + k] for i in range(0, len(chars), k)]
        first += lk.tolist()
    order = np.argsort(np.array(first, dtype=np.uint64), kind="stable").tolist()
    text = header(k).encode() + b"".join(b"S\t%d\t%s\n" % (i + 1, seqs[j]) for i, j in enumerate(order))
    stats = dict(distinct=len(keys), unitigs=rest["unitigs"] + n_lone, removed=rest["removed"] + (n_lone if dele else 0), unitigs_out=len(seqs),
                 longest=max([len(s) for s in seqs] + [0]), bytes=len(text))
    return text, stats


_CACHE = {}


def expected(name, k, reads):
    """{(clip, dele): (text, stats)} of a case, computed once a process"""
    if name not in _CACHE:
        S = kmer_set(reads, k)
        _CACHE[name] = (S, {f: build(S, k, *f) for f in FLAGS})
    return _CACHE[name]


def encode(kmer):
    """pf_count_rule.hpp's key: A0 C1 G2 T3, first base most significant"""
    v = 0
    for c in kmer:
        v = (v << 2) | BASES.index(c)
    return v


def fastq(reads):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, (r if isinstance(r, bytes) else r.encode()), b"I" * len(r)) for i, r in enumerate(reads))


# ---- the hand-worked example: k = 5 ----
# reads AAGACTCCATG (the backbone), ACTCG (shares ACTC with it, then runs off) and GCGTAA (on its own).
#   backbone windows AAGAC AGACT GACTC ACTCC CTCCA TCCAT CCATG; canonical: TCCAT -> ATGGA, CCATG -> CATGG, the others as they read.
#   GACTC has two successors, ACTCC and ACTCG, so no link leaves it: AAGAC -> AGACT -> GACTC is one unitig, AAGACTC (its other
#   reading starts with GAGTC, which is larger); ACTCC -> CTCCA -> TCCAT -> CCATG is the next, ACTCCATG (the other reading starts with
#   CATGG), and it ends there: the only successor of CCATG is CATGG, its own reverse complement.  ACTCG is a unitig of one k-mer,
#   GCGTA -> CGTAA gives GCGTAA (the other reading starts with TTACG).  Four unitigs, all of fewer than 5 k-mers.
#   AAGACTC: p = 0, s = 2: stays under every flag.  ACTCCATG: p = 1 (GACTC), s = 1 (CATGG): stays.  ACTCG: p = 1, s = 0: a tip, goes with
#   -i.  GCGTAA: p = s = 0: isolated, goes with -d, and with -i -d (p + s <= 1), not with -i alone (p + s == 1 is asked).
#   Once ACTCG is gone GACTC has one successor again and the backbone is one unitig: AAGACTCCATG.
HAND_READS = ["AAGACTCCATG", "ACTCG", "GCGTAA"]
HAND_K = 5
HAND = {
    (False, False): (b"S\t1\tAAGACTC\nS\t2\tACTCCATG\nS\t3\tACTCG\nS\t4\tGCGTAA\n", dict(distinct=10, unitigs=4, removed=0, unitigs_out=4, longest=8)),
    (True, False): (b"S\t1\tAAGACTCCATG\nS\t2\tGCGTAA\n", dict(distinct=10, unitigs=4, removed=1, unitigs_out=2, longest=11)),
    (False, True): (b"S\t1\tAAGACTC\nS\t2\tACTCCATG\nS\t3\tACTCG\n", dict(distinct=10, unitigs=4, removed=1, unitigs_out=3, longest=8)),
    (True, True): (b"S\t1\tAAGACTCCATG\n", dict(distinct=10, unitigs=4, removed=2, unitigs_out=1, longest=11)),
}
