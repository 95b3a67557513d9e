"""Shared by test_fasta_cpu.py and test_gpu_fasta.py: the rule of `--fasta` (K-FASTA, csrc/pf_fasta_rule.hpp) restated in Python, the
rewriting Q(F) that defines what every sub-command makes of a FASTA file, writers of FASTA text and the edge texts both suites run.

The rule: lines end at '\\n' and a '\\r' directly in front of it is no content; a line that starts with '>' is a header and opens a
record; every other line is a sequence line of the record opened last; a record's sequence is its sequence lines joined.  In a chunk
that is not final the record the last header opens is carried: bytes_used is that header's first byte."""
import numpy as np

TILE = 4096   # PF_FASTA_TILE: bytes of the chunk one block of the compaction kernel takes at a time


def ref_index(text: bytes, final: bool = True):
    """{"text", "read_off", "read_len", "bytes_used", "records", "bases", "headers"} by splitting lines and joining"""
    assert not text or text[:1] == b">"
    recs, starts, pos = [], [], 0
    for line in text.split(b"\n") if text else []:
        end = pos + len(line)                       # the line's '\n', or the end of the text
        if line[:1] == b">":
            recs.append([line[1:], b""])
            starts.append(pos)
        elif pos < len(text):                       # (behind a last '\n' split() gives one empty piece that is no line)
            recs[-1][1] += line[:-1] if line[-1:] == b"\r" and end < len(text) else line
        pos = end + 1
    used = len(text)
    if not final:
        used = starts[-1] if len(recs) > 1 else 0
        recs = recs[:-1]
    seqs = [s for _, s in recs]
    off = np.cumsum([0] + [len(s) for s in seqs[:-1]], dtype=np.uint64) if seqs else np.zeros(0, dtype=np.uint64)
    return {"text": b"".join(seqs), "read_off": off, "read_len": np.array([len(s) for s in seqs], dtype=np.uint32), "bytes_used": used,
            "records": len(seqs), "bases": sum(len(s) for s in seqs), "headers": [h for h, _ in recs]}


def q_of(text: bytes) -> bytes:
    """Q(F): every record as "@" + header without its '>', the joined sequence, "+", and 'I' once per base"""
    r = ref_index(text, True)
    out = []
    for h, o, n in zip(r["headers"], r["read_off"], r["read_len"]):
        h = h[:-1] if h[-1:] == b"\r" else h
        out.append(b"@" + h + b"\n" + r["text"][int(o):int(o) + int(n)] + b"\n+\n" + b"I" * int(n) + b"\n")
    return b"".join(out)


def fasta(reads, width: int = 60, names=None, crlf: bool = False, last_newline: bool = True) -> bytes:
    """the reads as FASTA records r0, r1, ... with sequence lines of `width`"""
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for i, r in enumerate(reads):
        r = r if isinstance(r, bytes) else r.encode()
        out.append(b">" + (names[i] if names else b"r%d" % i) + nl)
        out += [r[a:a + width] + nl for a in range(0, len(r), width)]
    text = b"".join(out)
    return text if last_newline or not text.endswith(nl) else text[: -len(nl)]


def random_seq(rng, n: int) -> bytes:
    return bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=n))


def edge_texts():
    """(name, text): every text starts with '>'.  Widths put line ends before, on and behind a 64-byte word edge; CRLF lines, one with
    '\\r' as the last byte of a word and '\\n' as the first of the next; headers of one byte, of more than 200 bytes over four words and
    with '>' inside; '>' inside a sequence line; empty lines; records without sequence; a last record without '\\n'; texts of TILE - 1,
    TILE and TILE + 1 bytes and a record whose sequence crosses a tile edge."""
    rng = np.random.default_rng(11)
    out = [("empty", b""), ("two_lines", b">a\nACGTA\nCGTAC\n"), ("header_alone", b">"), ("header_alone_nl", b">x\n")]
    for w in (1, 59, 63, 64, 65, 127):
        out.append(("width_%d" % w, fasta([random_seq(rng, n) for n in (200, 0, 64, 63, 65, 129, 1)], width=w)))
    out.append(("crlf", fasta([random_seq(rng, n) for n in (150, 61, 0, 62)], width=60, crlf=True)))
    head = b">ab\r\n"                                    # 5 bytes: a line of 58 bases puts its '\r' at byte 63 and its '\n' at byte 64
    out.append(("crlf_on_word_edge", head + random_seq(rng, 58) + b"\r\n" + random_seq(rng, 70) + b"\r\nAC\r\n"))
    assert out[-1][1][63:65] == b"\r\n"
    out.append(("cr_alone_is_content", b">a\nAC\rGT\r\r\nTT\r"))
    out.append(("headers", b">\nACGT\n>" + b"h" * 230 + b"\nTTGA\nCC\n>x>y >z\nGATTACA\n"))
    out.append(("gt_in_sequence", b">a\nACG>TAC\nA>\n>b\nTT\n"))
    out.append(("empty_lines", b">a\nACGT\n\n\nTTAA\n\n>b\n\nGG\n\n\n"))
    out.append(("no_sequence", b">a\n>b\n>c\nACGT\n>d\n>e"))
    out.append(("no_last_newline", b">a\nACGTACGT\nTTT"))
    out.append(("no_last_newline_cr", b">a\r\nACGT\r\nTT\r"))
    for n in (TILE - 1, TILE, TILE + 1):
        body = fasta([random_seq(rng, 3 * TILE)], width=60)
        out.append(("bytes_%d" % n, body[:n]))
    out.append(("sequence_over_tile_edges", fasta([random_seq(rng, 100), random_seq(rng, 2 * TILE + 500), random_seq(rng, 7)], width=60)))
    return out


def cuts_of(text: bytes):
    """the cuts the issue names for chunks that are not final: inside a sequence line, inside a header, directly behind a '\\n',
    directly in front of a '>' -- and a chunk with a single header"""
    cuts = set()
    heads = [i for i in range(len(text)) if text[i:i + 1] == b">" and (i == 0 or text[i - 1:i] == b"\n")]
    for h in heads[1:3] + heads[-1:]:
        cuts.update((h, h + 1, h + 2, h - 1, h - 3))
    nls = [i for i in range(len(text)) if text[i:i + 1] == b"\n"]
    for i in nls[:3] + nls[-2:]:
        cuts.update((i, i + 1))
    cuts.update((1, 2, len(text) // 2, len(text) - 1))
    return sorted(c for c in cuts if 0 < c <= len(text))


def big_text(seed: int = 5, n_records: int = 2000, width: int = 60) -> bytes:
    """about 300 KB: records of random length 0 to 400"""
    rng = np.random.default_rng(seed)
    return fasta([random_seq(rng, int(n)) for n in rng.integers(0, 401, size=n_records)], width=width)
