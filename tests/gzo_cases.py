"""Texts for the K-DEFLATE tests (blocked-gzip output), all made here from seeds: the edges of the encoder -- one-symbol alphabets, no or
one distance code, match lengths about 258, distances about 32 768, code lengths past 15 bits, member cuts about 65 280 -- and FASTQ as
sequencers write it."""
import random

import gz_cases as gz

CUT = 65280


def binned_fastq(n_bytes: int = CUT, seed: int = 31) -> bytes:
    """instrument-style headers, binned qualities: runs of F with a few ':', ',' and '#'"""
    rnd = random.Random(seed)
    out, size, i = [], 0, 0
    while size < n_bytes:
        seq = bytes(rnd.choice(b"ACGT") for _ in range(151))
        qual = bytearray(b"F" * 151)
        for _ in range(rnd.randrange(0, 12)):
            qual[rnd.randrange(151)] = rnd.choice(b":,#")
        rec = b"@A00123:45:HXXXXDSXX:%d:%d:%d:%d 1:N:0:ACGTACGT\n%s\n+\n%s\n" % (rnd.randrange(1, 5), 1101 + i // 50, rnd.randrange(1000, 30000),
                                                                               rnd.randrange(1000, 30000), seq, bytes(qual))
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)[:n_bytes]


def fibonacci(seed: int = 32) -> bytes:
    """symbol i occurring F(i) times over 23 symbols, shuffled: Huffman's code for it is 22 bits deep.  The 75 024 bytes are cut to a
    member's 65 280 behind the shuffle, which leaves the code deeper than 15 bits (huffman_depth below; the test asserts it)"""
    fib = [1, 1]
    while len(fib) < 23:
        fib.append(fib[-1] + fib[-2])
    text = bytearray()
    for i, f in enumerate(fib):
        text += bytes([65 + i]) * f
    random.Random(seed).shuffle(text)
    return bytes(text[:CUT])


def huffman_depth(freqs) -> int:
    """the longest code of Huffman's construction without a limit"""
    import heapq
    heap = [(f, 0) for f in freqs if f]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def far(distance: int, seed: int = 33) -> bytes:
    """100 random bytes, a filler of ACGTN, and the same 100 bytes `distance` behind the first"""
    rnd = random.Random(seed)
    head = bytes(rnd.randrange(128, 256) for _ in range(100))   # (no byte of the filler: the match starts and ends where the copy does)
    filler = bytes(rnd.choice(b"ACGTN") for _ in range(distance - 100))
    return head + filler + head


def texts():
    """(name, text): the texts of the issue's list; every one fits a member but the last"""
    rnd = random.Random(30)
    fq = gz.fastq(700)
    out = [("empty", b""), ("one_byte", b"A"), ("two_bytes", b"AC"), ("three_bytes", b"ACG")]
    out += [("i_%d" % n, b"I" * n) for n in (4, 257, 258, 259, 260, 261, 262, CUT)]
    out += [("acgt", b"ACGT" * 4000), ("literal_and_match", b"B" + b"ACGTA" + b"ACGTA"), ("far_32768", far(32768)), ("far_32769", far(32769)),
            ("random_65280", bytes(rnd.randrange(256) for _ in range(CUT))), ("fastq_65280", gz.fastq(400)[:CUT]), ("binned_fastq", binned_fastq()),
            ("fibonacci", fibonacci()), ("fastq_65279", fq[:CUT - 1]), ("fastq_cut", fq[100:100 + CUT]), ("fastq_65281", fq[:CUT + 1])]
    return out


def member_texts():
    return [(name, text) for name, text in texts() if len(text) <= CUT]
