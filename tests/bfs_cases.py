"""Graphs on which K-BFS's wavefront tier gives traversals up, for the tests of its tiers and entry points."""
import numpy as np


def lattice_gfa(path, k=25, depth=7, seed=3):
    """A superbubble wider than the LDS tables of K-BFS: a binary tree of `depth` levels fanning out
    from one entrance and its mirror image collapsing into one exit (2^depth unitigs in the middle)."""
    rng = np.random.default_rng(seed)

    def rnd(n):
        return bytes(rng.choice(list(b"ACGT"), size=n).tolist())

    segs = [rnd(60)]
    level = [0]  # indices into segs
    # expanding half: node -> two children that start with the node's last k-1 bases + a distinct base
    for _ in range(depth):
        nxt = []
        for i in level:
            for b in (b"A", b"C"):
                segs.append(segs[i][-(k - 1):] + b + rnd(30))
                nxt.append(len(segs) - 1)
        level = nxt
    # collapsing half: two parents are extended so that both end with the same k-1 bases after distinct bases
    while len(level) > 1:
        nxt = []
        for i in range(0, len(level), 2):
            join = rnd(k - 1)
            segs[level[i]] += b"G" + join
            segs[level[i + 1]] += b"T" + join
            segs.append(join + rnd(30))
            nxt.append(len(segs) - 1)
        level = nxt
    with open(path, "wb") as f:
        f.write(b"H\tVN:Z:1.0\tKL:Z:%d\tML:Z:17\n" % k)
        for i, s in enumerate(segs):
            f.write(b"S\t%d\t%s\n" % (i + 1, s))
    return len(segs)
