"""The rule of the heterozygous k-mer pairs (K-HETPAIR, `smudge`, `run --smudge`; csrc/pf_hetpair_rule.hpp) restated in plain Python --
dictionaries and loops, nothing shared with the library -- and the generators of the cases the host rule and the kernel are held to.
No device, no library."""
import numpy as np

BASES = "ACGT"
MAX_W = 4096


# ---- keys ----
def enc(s):
    x = 0
    for c in s:
        x = x * 4 + BASES.index(c)
    return x


def dec(x, k):
    return "".join(BASES[(x >> (2 * (k - 1 - p))) & 3] for p in range(k))


def revcomp(x, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def canon(x, k):
    return min(x, revcomp(x, k))


def neighbours(x, k):
    """the 3k neighbours of x, with repeats and possibly x itself"""
    out = []
    for p in range(k):
        s = 2 * (k - 1 - p)
        old = (x >> s) & 3
        for b in range(4):
            if b != old:
                out.append(canon((x & ~(3 << s)) | (b << s), k))
    return out


# ---- the rule ----
def hetpairs(kmers, counts, k, lo, hi):
    """what hipapi.Device.hetpairs and hostapi.hetpairs_host return, from the definitions"""
    assert 1 <= lo <= hi and hi - lo + 1 <= MAX_W
    W = hi - lo + 1
    count_of = {int(x): int(c) for x, c in zip(kmers, counts)}
    assert len(count_of) == len(kmers), "the keys are distinct"
    S = {x for x, c in count_of.items() if lo <= c <= hi}
    partners = {x: {y for y in neighbours(x, k) if y != x and y in S} for x in S}
    table = np.zeros((W, W), dtype=np.uint64)
    px, py, cx, cy = [], [], [], []
    for x in (int(v) for v in kmers):   # the order of x in the key array
        if x not in S or len(partners[x]) != 1:
            continue
        (y,) = partners[x]
        if not (x < y and len(partners[y]) == 1):
            continue
        assert partners[y] == {x}   # the relation is symmetric
        a, b = sorted((count_of[x], count_of[y]))
        table[a - lo, b - lo] += 1
        px.append(x), py.append(y), cx.append(count_of[x]), cy.append(count_of[y])
    stats = {"kmers": len(kmers), "in_range": len(S), "one_partner": sum(len(p) == 1 for p in partners.values()),
             "many_partners": sum(len(p) > 1 for p in partners.values()), "pairs": len(px)}
    return {"table": table, "pair_x": np.array(px, dtype=np.uint64), "pair_y": np.array(py, dtype=np.uint64),
            "cov_x": np.array(cx, dtype=np.uint32), "cov_y": np.array(cy, dtype=np.uint32), "stats": stats}


def smudge_of(a, b, n):
    t = a + b
    p = min(max((2 * t + n) // (2 * n), 2), 16)
    m = min(max((2 * a * p + t) // (2 * t), 1), p // 2)
    return p, m, "A" * (p - m) + "B" * m


def summary(table, lo, n):
    """({(p, m): pairs}, the proposed (p, m) or None)"""
    sm = {}
    for i, j in np.argwhere(table):
        p, m, _ = smudge_of(lo + int(i), lo + int(j), n)
        sm[(p, m)] = sm.get((p, m), 0) + int(table[i, j])
    best = None
    for key in sorted(sm):   # ascending p, then m: a later label wins only with more pairs
        if best is None or sm[key] > sm[best]:
            best = key
    return sm, best


def report(table, stats, k, lo, hi, n=0):
    o = ["# ploidyfrost smudge 1", "# k %d lower %d upper %d n %d" % (k, lo, hi, n), ">>totals", "kmers\tin_range\tone_partner\tmany_partners\tpairs",
         "\t".join(str(stats[f]) for f in ("kmers", "in_range", "one_partner", "many_partners", "pairs")), ">>table", "cov_a\tcov_b\tpairs"]
    total = {}
    for i, j in np.argwhere(table):   # row-major: ascending cov_a, then cov_b
        o.append("%d\t%d\t%d" % (lo + i, lo + j, table[i, j]))
        total[2 * lo + int(i) + int(j)] = total.get(2 * lo + int(i) + int(j), 0) + int(table[i, j])
    o += [">>total", "cov_a+cov_b\tpairs"] + ["%d\t%d" % (t, total[t]) for t in sorted(total)]
    if n:
        sm, best = summary(table, lo, n)
        o += [">>smudges", "label\tp\tm\tpairs"] + ["%s\t%d\t%d\t%d" % ("A" * (p - m) + "B" * m, p, m, sm[(p, m)]) for p, m in sorted(sm)]
        o += [">>proposed", "p\tlabel\tpairs", "0\tnone\t0" if best is None else "%d\t%s\t%d" % (best[0], "A" * (best[0] - best[1]) + "B" * best[1], sm[best])]
    return ("\n".join(o) + "\n").encode()


def pairs_text(r, k):
    return "".join("%s\t%s\t%d\t%d\n" % (dec(int(x), k), dec(int(y), k), a, b) for x, y, a, b in zip(r["pair_x"], r["pair_y"], r["cov_x"], r["cov_y"])).encode()


# ---- cases: (kmers u64 sorted, counts u32, k, lo, hi) ----
def arrays(count_of):
    keys = sorted(count_of)
    return np.array(keys, dtype=np.uint64), np.array([count_of[x] for x in keys], dtype=np.uint32)


def all_canonical(k):
    return sorted({canon(x, k) for x in range(4 ** k)})


def genome(n, seed):
    return "".join(BASES[b] for b in np.random.default_rng(seed).integers(0, 4, size=n))


def substituted(s, positions):
    t = list(s)
    for p in positions:
        t[p] = BASES[(BASES.index(t[p]) + 1 + p % 3) % 4]
    return "".join(t)


def count_strings(strings, k, depth=20):
    """every string sequenced `depth` times: canonical k-mer -> depth x occurrences"""
    count_of = {}
    for s in strings:
        x = enc(s[:k - 1]) if k > 1 else 0
        for c in s[k - 1:]:
            x = ((x << 2) | BASES.index(c)) & (4 ** k - 1)
            y = canon(x, k)
            count_of[y] = count_of.get(y, 0) + depth
    return count_of


HAP_LEN, HAP_STEP, HAP_SEED = 3000, 97, 7
HAP_SITES = list(range(HAP_STEP, 2900, HAP_STEP))   # 29 substitutions


def haplotypes(k, seed=HAP_SEED):
    """two haplotypes of 3000 bases with a substitution every 97 bases, each sequenced 20 times: shared k-mers count 40, the k-mers
    over a substitution 20 on either side"""
    a = genome(HAP_LEN, seed)
    return arrays(count_strings([a, substituted(a, HAP_SITES)], k))


def small_cases():
    """name -> (kmers, counts, k, lo, hi): every case the Python restatement above can afford"""
    out = {}
    k5 = all_canonical(5)
    out["k5_all"] = arrays({x: 7 for x in k5}) + (5, 1, 10)                                   # 32 self-neighbours, doubled neighbours, 0 pairs
    out["k5_every_second_out"] = arrays({x: (7 if i % 2 == 0 else 50) for i, x in enumerate(k5)}) + (5, 1, 10)
    k4 = all_canonical(4)
    rng = np.random.default_rng(11)
    for j, frac in enumerate((0.08, 0.15, 0.3)):   # doubled neighbours with degree 1
        pick = [x for x in k4 if rng.random() < frac]
        out["k4_subset%d" % j] = arrays({x: int(rng.integers(1, 13)) for x in pick}) + (4, 2, 9)
    out["k4_aatt"] = arrays({enc("AAAT"): 5, enc("AATT"): 6}) + (4, 1, 10)
    for k in (17, 18, 25, 31):   # 17 / 18: the two sides of HOME_M + 2; 31: the top bits of the word
        out["hap_k%d" % k] = haplotypes(k) + (k, 10, 100)
    a = genome(400, 3)
    # a triallelic site: three keys mutually at distance 1 over every window, 0 pairs there
    tri = [a, a[:200] + BASES[(BASES.index(a[200]) + 1) % 4] + a[201:], a[:200] + BASES[(BASES.index(a[200]) + 2) % 4] + a[201:]]
    out["triallelic"] = arrays(count_strings(tri, 21)) + (21, 10, 100)
    # two substitutions fewer than k apart: the windows over both have no partner, those over one alone pair up
    out["two_close"] = arrays(count_strings([a, substituted(a, [200, 210])], 21)) + (21, 10, 100)
    # counters at lo - 1, lo, hi, hi + 1 on one side of a pair
    base = count_strings([a, substituted(a, [100, 200, 300])], 21)
    b = substituted(a, [100, 200, 300])
    for site, c in ((100, 14), (200, 15), (300, 30)):
        x = canon(enc(b[site - 10: site + 11]), 21)
        base[x] = c
    x = canon(enc(b[291: 312]), 21)
    base[x] = 31
    out["edges"] = arrays(base) + (21, 15, 30)
    one = arrays(count_strings([a, substituted(a, [200])], 21))
    out["w1"] = one + (21, 20, 20)
    out["w4096"] = one + (21, 5, 4100)
    for n in (0, 1, 63, 64, 65):   # n keys given
        km, ct = haplotypes(25)
        out["n%d" % n] = (km[:n], ct[:n], 25, 10, 100)
    for r in (15, 16, 17):   # keys in range: the edges of a 16-lane row
        km, ct = haplotypes(25)
        ct = ct.copy()
        ct[r:] = 5
        out["in_range%d" % r] = (km, ct, 25, 10, 100)
    return out


def one_cell_case(n_pairs=100000, k=25, seed=5):
    """2 n_pairs keys, all of its pairs in one cell (the contention path of the table kernel): random k-mers and the same with the
    middle base changed, every counter 20.  Too large for the restatement above: the kernel is held to the host rule."""
    rng = np.random.default_rng(seed)
    fw = rng.integers(0, 1 << 62, size=n_pairs, dtype=np.uint64) >> np.uint64(62 - 2 * k)
    s = np.uint64(2 * (k // 2))
    other = fw ^ (np.uint64(1) << s)
    both = np.concatenate([fw, other])
    rc = np.zeros_like(both)
    x = ~both & np.uint64(4 ** k - 1)
    for _ in range(k):
        rc = (rc << np.uint64(2)) | (x & np.uint64(3))
        x = x >> np.uint64(2)
    keys = np.unique(np.minimum(both, rc))
    return keys, np.full(len(keys), 20, dtype=np.uint32), k, 20, 20 + 63
