"""The colour rule of `ploidyfrost build-multi` (K-COLOR) in plain Python on top of unitig_cases.py -- sets and lists of strings, nothing
tiled or hashed by hand but the placement's hash, which is ploidyfrost_amd/bfg_colors.py's restatement of Bifrost's --, the comparator
against the real Bifrost's dump of a coloured graph, and the deterministic cases the host restatement (pf_color::build_colored_host,
pf_bfg::write) and the kernels (pf_unitig.hip, pf_color.hip) are held to.

  colour     colour c lies on k-mer x of the written graph when some window of some read of file c has x as its canonical form; a window
             is k bytes, all in ACGTacgt.  A window whose k-mer -i / -d removed colours nothing.
  ids        the colour set of a unitig of m k-mers is the sorted ids c * m + p, p the k-mer's position in the S line as written.
  placement  nb_cs = number of lines; round s = 1 .. n_seeds: every unplaced line asks for slot hash(head, seed(s)) % nb_cs, a free slot
             goes to the smallest line that asks; DA = the round; a line left over: DA 0 and slot nb_cs + its rank among those.
"""
import numpy as np

import unitig_cases as uc

from ploidyfrost_amd import bfg_colors

_M64 = (1 << 64) - 1
SEEDS = 31
STATS = ("colors", "windows_colored", "windows_unplaced", "windows_bad", "runs", "overflow")


def seed_of(rnd):
    """splitmix64 of the round number"""
    z = (rnd * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def windows(read, k):
    """(canonical k-mers of the windows of k bases, windows that hold another byte)"""
    if isinstance(read, bytes):
        read = read.decode("latin-1")
    r = read.upper()
    good, bad = [], 0
    for i in range(len(r) - k + 1):
        w = r[i:i + k]
        if all(c in uc.BASES for c in w):
            good.append(uc.canon(w))
        else:
            bad += 1
    return good, bad


def place(seqs, k, n_seeds=SEEDS):
    """(slot, DA) of every line"""
    n = len(seqs)
    heads = [uc.encode(s[:k]) << (64 - 2 * k) for s in seqs]
    slot, da, owner = [None] * n, [0] * n, {}
    for rnd in range(1, n_seeds + 1):
        claim = {}
        for j in range(n):
            if slot[j] is None:
                at = bfg_colors.kmer_hash(heads[j], seed_of(rnd)) % n
                if at not in owner:
                    claim.setdefault(at, j)
        for at, j in claim.items():
            owner[at], slot[j], da[j] = j, at, rnd
    left = [j for j in range(n) if slot[j] is None]
    for r, j in enumerate(left):
        slot[j] = n + r
    return slot, da


def runs_of(ids):
    out = []
    for v in ids:
        if out and out[-1][1] + 1 == v:
            out[-1][1] = v
        else:
            out.append([v, v])
    return out


def build(reads_per_colour, k, clip=False, dele=False, g=None, n_seeds=SEEDS):
    """(text of <out>.gfa with the DA tags as bytes, [bits of every line: uint8 array [colours, k-mers]], statistics: unitig_cases.STATS
    and STATS) from the reads of every colour"""
    every = [r for reads in reads_per_colour for r in reads]
    plain, st = uc.build(uc.kmer_set(every, k), k, clip, dele, g)
    seqs = uc.gfa_sequences(plain)[1]
    where = {}
    for j, s in enumerate(seqs):
        for p in range(len(s) - k + 1):
            where[uc.canon(s[p:p + k])] = (j, p)
    bits = [np.zeros((len(reads_per_colour), len(s) - k + 1), dtype=np.uint8) for s in seqs]
    col = dict(colors=len(reads_per_colour), windows_colored=0, windows_unplaced=0, windows_bad=0)
    for c, reads in enumerate(reads_per_colour):
        for r in reads:
            good, bad = windows(r, k)
            col["windows_bad"] += bad
            for x in good:
                if x in where:
                    j, p = where[x]
                    bits[j][c, p] = 1
                    col["windows_colored"] += 1
                else:
                    col["windows_unplaced"] += 1
    slot, da = place(seqs, k, n_seeds)
    col["runs"] = sum(len(runs_of(np.nonzero(b.ravel())[0].tolist())) for b in bits)
    col["overflow"] = sum(1 for d in da if d == 0)
    text = plain.decode().split("\n", 1)[0] + "\n" + "".join("S\t%d\t%s\tDA:Z:%d\n" % (j + 1, s, da[j]) for j, s in enumerate(seqs))
    st = dict(st, bytes=len(text), **col)
    return text.encode(), bits, st


def colors_file(seqs, bits, k, names, n_seeds=SEEDS):
    """the bytes of <out>.bfg_colors by the layout bfg_colors.py documents, every set in its natural encoding"""
    import struct
    n = len(seqs)
    slot, _ = place(seqs, k, n_seeds)
    sz = max(slot) + 1 if n else 0
    sz = max(sz, n)
    owner = {s: j for j, s in enumerate(slot)}
    out = struct.pack("<7Q", 2, n_seeds, len(names), n, sz, 0, sz - n)
    out += b"".join(struct.pack("<Q", seed_of(r)) for r in range(1, n_seeds + 1)) + struct.pack("<Q", 1024)
    n_pos = (sz + 1023) // 1024
    pos_at = len(out)
    out += b"\0" * (16 * n_pos)
    out += b"".join(nm.encode() + b"\n" for nm in names)
    link = [0] * ((sz + 63) // 64)
    for s in owner:
        link[s >> 6] |= 1 << (s & 63)
    out += struct.pack("<%dQ" % len(link), *link)
    out = bytearray(out)
    for s in range(sz):
        if s % 1024 == 0:
            out[pos_at + 16 * (s // 1024): pos_at + 16 * (s // 1024) + 8] = struct.pack("<q", len(out))
        ids = np.nonzero(bits[owner[s]].ravel())[0].tolist() if s in owner else []
        out += bfg_colors.encode_set(ids, "auto")
    for j in range(n):
        if slot[j] >= n:
            out += struct.pack("<QQQ", uc.encode(seqs[j][:k]) << (64 - 2 * k), len(seqs[j]), slot[j])
    return bytes(out)


# ---- the comparator against a dump of the real Bifrost's reading (oracle/_ref/colors_dump) ----

def read_dump(text):
    """(names, rows) of a dump; a row is (head k-mer, k-mers, size, n_full_enc, bits [colours, k-mers])"""
    names, rows = [], []
    for line in text.split("\n"):
        p = line.split("\t")
        if not line or p[0] == "#colors":
            continue
        if p[0] == "#name":
            names.append(p[1])
            continue
        km = int(p[2])
        b = [np.ones(km, np.uint8) if t == "F" else np.zeros(km, np.uint8) if t == "E" else np.frombuffer(t.encode(), np.uint8) - ord("0")
             for t in p[5].split(",")]
        rows.append((p[1], km, int(p[3]), int(p[4]), np.stack(b)))
    return names, rows


def by_sequence(seqs, bits):
    """{min(sequence, reverse complement): bits in that reading}"""
    out = {}
    for s, b in zip(seqs, bits):
        r = uc.revcomp(s)
        out[min(s, r)] = b if s <= r else b[:, ::-1]
    return out


def dump_by_sequence(gfa_text, dump_text, k):
    """the same from Bifrost's two files: its dump lists the unitigs in its iterator order with their head k-mers, the sequences are
    the GFA's; a unitig is found by its head k-mer (reference orientation: as the S line reads)"""
    seqs = uc.gfa_sequences(gfa_text)[1]
    by_head = {s[:k]: s for s in seqs}
    assert len(by_head) == len(seqs)
    names, rows = read_dump(dump_text)
    out = {}
    for head, km, size, n_full, b in rows:
        s = by_head[head]
        assert len(s) - k + 1 == km and size == int(b.sum())
        r = uc.revcomp(s)
        out[min(s, r)] = b if s <= r else b[:, ::-1]
    return names, out


def dump_text(seqs, bits, k, names):
    """a dump as oracle/_ref/colors_dump prints it, composed from the rule: the unitigs longer than k in line order, then the others"""
    order = reader_order(seqs, k)
    out = ["#colors\t%d\tk\t%d\tunitigs\t%d\n" % (len(names), k, len(seqs))] + ["#name\t%s\n" % n for n in names]
    for i, j in enumerate(order):
        b = bits[j]
        km = b.shape[1]
        toks = ["F" if row.all() else "E" if not row.any() else "".join("01"[v] for v in row) for row in b]
        out.append("%d\t%s\t%d\t%d\t0\t%s\n" % (i + 1, seqs[j][:k], km, int(b.sum()), ",".join(toks)))
    return "".join(out)


def reader_order(seqs, k):
    """the lines in the order the reader numbers unitigs (the reference's): longer than k in line order, then the k-length ones (no
    minimizer is crowded in these graphs, so none is filed as an abundant k-mer)"""
    return [j for j, s in enumerate(seqs) if len(s) > k] + [j for j, s in enumerate(seqs) if len(s) == k]


def colors_bits(colors, gfa_text):
    """[bits of every line, in line order] as hostapi.Colors reads a pair of files, with its sizes and n_full_enc checked"""
    k, seqs = uc.gfa_sequences(gfa_text)
    order = reader_order(seqs, k)
    assert colors.n == len(order)
    out = [None] * len(order)
    for u, j in enumerate(order):
        got, size, n_full = colors.unitig(u)
        assert got.shape[1] == len(seqs[j]) - k + 1 and size == int(got.sum()) and n_full == 0, (u, j)
        out[j] = got
    return out


# ---- reads ----

def table(reads):
    """(text, read_off, read_len) of reads laid end to end"""
    reads = [r if isinstance(r, bytes) else r.encode() for r in reads]
    off = np.cumsum([0] + [len(r) for r in reads[:-1]], dtype=np.uint64) if reads else np.zeros(0, dtype=np.uint64)
    return b"".join(reads), off, np.array([len(r) for r in reads], dtype=np.uint32)


def tiling(seq, k, read_len=None, step=None):
    """reads that cover every k-mer of seq"""
    read_len = read_len or 4 * k
    step = step or read_len - k + 1
    out = [seq[i:i + read_len] for i in range(0, max(len(seq) - k + 1, 1), step)]
    return [r for r in out if len(r) >= k]


def grid_case(n_kmers, n_colors=3, k=25, seed=20240613):
    """a graph of more k-mers than one pass of a grid has threads, and its colours, without the Python rule (too slow at this size):
    n_kmers random k-mers, every one a line of its own (a random 25-mer has no neighbour among a million others; checked), each with the
    colours drawn from the seed -- at least one.  Returns (reads_per_colour as (text, off, len) tables, keys sorted, membership
    [colours, k-mers] in key order)."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, size=(n_kmers + 64, k), dtype=np.uint8)
    keys = uc._windows(codes, k)
    order = np.argsort(keys, kind="stable")
    lone = np.ones(len(keys), dtype=bool)   # (a k-mer whose successor is its own reverse complement counts as its neighbour: dropped)
    lone[order] = ~uc.has_neighbour(keys[order], k)
    lone[order[1:]] &= keys[order[1:]] != keys[order[:-1]]
    codes = codes[lone][:n_kmers]
    keys = uc._windows(codes, k)
    order = np.argsort(keys, kind="stable")
    assert len(np.unique(keys)) == n_kmers and not uc.has_neighbour(keys[order], k).any()
    member = rng.random((n_colors, n_kmers)) < 0.5
    member[rng.integers(0, n_colors, size=n_kmers), np.arange(n_kmers)] = True
    chars = np.frombuffer(uc.BASES.encode(), dtype=np.uint8)[codes]
    tables = []
    for c in range(n_colors):
        rows = chars[member[c]]
        tables.append((rows.tobytes(), np.arange(len(rows), dtype=np.uint64) * np.uint64(k), np.full(len(rows), k, dtype=np.uint32)))
    return tables, keys[order], member[:, order]


def grid_expected(keys, member, k, names, writer, n_seeds=SEEDS):
    """(text, bytes of the colour file, statistics) of grid_case's graph by the rule in numpy: every k-mer is a line of its own (it has
    no neighbour), the lines ascend by key, a line's ids are the colours that hold its k-mer, and the placement is the rule's rounds
    over arrays.  writer(fetched dict, k, names, n_seeds) lays the file out (hostapi.bfg_colors_bytes: the host's writer, which the
    tests without a GPU hold to bfg_colors.py's encodings).  The test without a GPU holds all of this to the host's restatement at a
    small size."""
    n, c_n = len(keys), member.shape[0]
    heads = keys.astype(np.uint64) << np.uint64(64 - 2 * k)
    slot, da, taken = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    for rnd in range(1, n_seeds + 1):
        todo = np.nonzero(slot < 0)[0]
        if not len(todo):
            break
        at = (bfg_colors.kmer_hash_np(heads[todo], seed_of(rnd)) % np.uint64(n)).astype(np.int64)
        claim = np.full(n, n, dtype=np.int64)
        np.minimum.at(claim, at, todo)                  # the smallest line that asks
        win = ~taken[at] & (claim[at] == todo)
        slot[todo[win]], da[todo[win]] = at[win], rnd
        taken[at[win]] = True
    left = np.nonzero(slot < 0)[0]
    slot[left] = n + np.arange(len(left))
    shifts = np.arange(2 * (k - 1), -1, -2, dtype=np.uint64)
    chars = np.frombuffer(uc.BASES.encode(), dtype=np.uint8)[((keys[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)].tobytes()
    text = uc.header(k).encode() + b"".join(b"S\t%d\t%s\tDA:Z:%d\n" % (j + 1, chars[j * k:(j + 1) * k], da[j]) for j in range(n))
    on = member.T                                        # [line, colour]: with one k-mer a line, id = colour
    begins = on & ~np.concatenate([np.zeros((n, 1), dtype=bool), on[:, :-1]], axis=1)
    ends = on & ~np.concatenate([on[:, 1:], np.zeros((n, 1), dtype=bool)], axis=1)
    runs = np.stack([np.nonzero(begins)[1], np.nonzero(ends)[1]], axis=1).astype(np.uint32)
    run_off = np.concatenate([[0], np.cumsum(begins.sum(axis=1))]).astype(np.uint64)
    fetched = dict(heads=keys, m=np.ones(n, dtype=np.uint32), slot=slot.astype(np.uint32), run_off=run_off, runs=runs)
    stats = dict(distinct=n, unitigs=n, removed=0, unitigs_out=n, longest=k if n else 0, bytes=len(text), colors=c_n, windows_colored=int(member.sum()),
                 windows_unplaced=0, windows_bad=0, runs=len(runs), overflow=len(left))
    return text, writer(fetched, k, names, n_seeds), stats


# ---- the cases ----

def _chain(rng, m, k):
    """a sequence of m k-mers that is one unitig (no k-mer twice, none next to another's neighbour: checked by the caller's rule)"""
    return uc.rand_seq(rng, m + k - 1)


def cases():
    """[(name, k, reads_per_colour, (clip, dele), n_seeds)], deterministic: the smallest shapes at which a set takes each form, the colour
    counts round a 64-bit word, strands, removed tips, the edges of the 1024-byte tile, and a placement that overflows"""
    import random
    rng = random.Random(20240612)
    k, out, plain = 25, [], (False, False)
    # set forms: C * m = 60, 61, 62 with the top id set -- the 61-bit vector ends at id 60
    for name, c_n, m in (("top60", 2, 30), ("top61", 1, 61), ("top62", 2, 31)):
        s = _chain(rng, m, k)
        reads = [[s]] + [[s[:k], s[-k:]] for _ in range(c_n - 1)]   # both end k-mers: the top id, whichever reading is written
        out.append((name, k, reads, plain, SEEDS))
    s = _chain(rng, 21846, k)                       # ids cross 2^16: colour 2's last k-mers lie beyond it
    out.append(("cross16", k, [tiling(s, k, 500), tiling(s[3000:9000], k, 500), tiling(s[-200:], k, 100)], plain, SEEDS))
    s = _chain(rng, 60000, k)                       # five containers of a Roaring bitmap: the offset header is present
    full = tiling(s, k, 1000)
    out.append(("five_containers", k, [full] * 5, plain, SEEDS))
    s = _chain(rng, 5000, k)                        # 2 500 runs in one 2^16 block: more than the TinyBitmap holds
    out.append(("alt2500", k, [tiling(s, k, 500), [s[p:p + k] for p in range(0, 5000, 2)]], plain, SEEDS))
    s = _chain(rng, 100, k)                         # two full colours: one merged run
    out.append(("two_full", k, [[s], [uc.revcomp(s)]], plain, SEEDS))
    # colour counts round the words of a mask; the last colour but one has no k-mer at all
    for c_n in (1, 2, 64, 65):
        s = _chain(rng, 40, k)
        reads = [[s]] + [[s[(3 * c) % 30:(3 * c) % 30 + k + c % 9]] for c in range(1, c_n)]
        if c_n > 1:
            reads[-2 if c_n > 2 else -1] = ["ACGT", "N" * 30, ""]
        out.append(("colors%d" % c_n, k, reads, plain, SEEDS))
    s = _chain(rng, 300, k)                         # one colour's reads all reverse-complemented, covering one end only
    out.append(("strand", k, [tiling(s, k, 80), [uc.revcomp(r) for r in tiling(s[-120:], k, 60)]], plain, SEEDS))
    b, tip = uc._tip_case(rng, k, 10)               # -i: colour 1's own k-mers are all a removed tip
    out.append(("tip", k, [[b], [tip, b[:100]]], (True, False), SEEDS))
    out.append(("tip_kept", k, [[b], [tip, b[:100]]], plain, SEEDS))
    s = _chain(rng, 1024 + k + 1, k)                # 1024 + 2 k bases: windows start at bytes 1023 and 1024 of the text
    marred = s[:500] + "N" + s[501:900].lower() + s[900:1100] + "n" + s[1101:]
    out.append(("tile_edges", k, [[s], [marred, s[:k - 1], "", s[1000:1000 + k], "ACGTN"]], plain, SEEDS))
    lone = uc._isolated(rng, 200, k)                # one round alone: lines are left over
    out.append(("overflow", k, [lone, lone[::3] + [lone[1]]], plain, 1))
    return out


_CACHE = {}


def expected(name):
    """(text, bits, statistics, bytes of the colour file, names) of a case by the Python rule, computed once a process"""
    if name not in _CACHE:
        _, k, reads, flags, n_seeds = next(c for c in cases() if c[0] == name)
        text, bits, st = build(reads, k, *flags, n_seeds=n_seeds)
        names = ["c%d" % c for c in range(len(reads))]
        _CACHE[name] = (text, bits, st, colors_file(uc.gfa_sequences(text)[1], bits, k, names, n_seeds), names)
    return _CACHE[name]
